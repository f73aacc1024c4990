// test_gemm_routes: the MFMA GEMMs (gemm.hip rtx_gemm_nt, gemm_dma.hip rtx_gemm_dma, gemm_f32.hip rtx_gemm_f32_km, dw_adam.hip rtx_dw_tn) on every
// tile map, split-K partition and epilogue edge, against an INTEGER reference, on the harness of check.h.
//
// Exact data.  Operand entries are k / 8 with k in [-8, 8] (exact in bf16 and float32); in the `lse` and `edges` sections B is j / 64 with |j| <= 8
// and the bias a multiple of 1 / 64 in [-1, 1]; in `dw` the deltas are k / 128.  Every product is a multiple of one power of two, K <= 2048, so a
// partial sum in ANY order is an integer of at most 17 bits times that power: accumulators, slabs and acc + bias are exact in float32 whatever the
// kernel's summation order.  The reference is an int64 count of units (product()); every product, slab, bias sum, gradient, half logit and strip
// maximum is compared bit for bit, every element of every output, and everything outside the valid block must still hold the poison.
//
// The one bound.  A strip partial's .y = sum exp(x - max) goes through __expf.  Its worst relative error against the float64 sum, measured on
// the MI355X over every launch of the `lse` section (profiles/gemm_routes_lse.txt): LSE_MEASURED = 4.158e-7.  The bound LSE_REL = 1.6632e-6 is
// four times that (room for other inputs: the error is a few roundings and not input-sensitive at these magnitudes; the `edges` launches, other
// data, reach 3.68e-7) and must stay <= 1e-5 (static_assert below).  The
// inputs are such that the smallest valid term of every strip is >= 1e-4 of the strip's sum (--host checks it): one column too many or too few
// moves .y by at least ten bounds.  (`dw` holds the Adam outputs to the absolute 2e-6 test_gemm's run_dw_case uses, computed from the exact gradient.)
//
// Sections (argument; none = all) and what each launch reaches.  Grids are m_tiles x n_tiles of the configuration's own tile.
//   map    K = 128.
//          rtx_gemm_dma, all six RtxDmaCfg x NT / NN x STORE / BIAS_ROWS:
//            xcd_block = 1   8 x 4 (one block), 9 x 5 (ragged both ways), 17 x 9 (three block rows, ragged; kept on the 512-row and 256 x 256
//                            tiles as well: the whole section takes under two seconds)                                -> the 8 x 4 block map
//            xcd_block = 1   10 x 2, 2 x 10: the launcher falls back to the strips; equal to the xcd_block = 0 launch, bit for bit
//            xcd_block = 0   10 x 2 (m > n, a second round of groups), 2 x 10 (m <= n, second round), 3 x 3       -> both strip maps
//          rtx_gemm_nt, every (RtxTileShape, dtype, epilogue) kTile serves, and rtx_gemm_f32_km NN / TN x STORE / GRAD: the three strip grids
//   slabs  split-K, RTX_EPI_STORE, grid 2 x 3: every slab alone equals the product over ITS slices [s per, min((s + 1) per, k_slices)).
//            7 slices / 3 splits (3, 3, 1: the short last split), 22 / 11 (splits 8 .. 10: the second XCD round), 2 / 2
//          on rtx_gemm_dma (all configurations, both forms), rtx_gemm_nt (every shape serving STORE: the depth-2 loop at nk = 1, 2, 3 and the
//          depth-3 loop's clamped prefetch) and rtx_gemm_f32_km.  11 slices / 5 splits: rtx_gemm_nt's fifth slab is empty and holds +0;
//          rtx_gemm_dma_launch refuses the request (also under --host).
//   lse    BIAS_ROWS with lse_part, (M_real, N_real, K) = (410, 701, 128), (77, 131, 64), (250, 2300, 192), (130, 192, 128: N_real a multiple
//          of 64) in tile-padded buffers, on rtx_gemm_nt (every shape, bf16 and float32) and rtx_gemm_dma (every configuration, NT / NN): C
//          bit for bit; per (row, strip) .x bit for bit and .y within LSE_REL; strips without a valid column hold (-inf, 0); rows >= M_real and
//          strips the grid does not have keep the poison.  A strip is the wave's column block: 64 columns, 128 on RTX_DMA_256x256_W4.
//          rtx_gemm_nt, bf16: the same launch with C16 (the step's logits): half(clamp(exact)) bit for bit, the float32 C untouched, the
//          same partials; and the first case with A and the bias scaled by 2^18 (products pass +-65504, still exact): the clamp bit for bit.
//   edges  every operand has junk rows beyond the valid ones and NaN between its extent and its leading dimension (lda = K + 64, ldb = K + 64,
//          K-major ld = extent + 128).  BIAS_ROWS with ldc > N_real, ldc % 4 == 0 (vector stores) and odd (scalar stores) with lse_part; GRAD
//          (gW, gbias) on rtx_gemm_nt and rtx_gemm_f32_km; hop_word (rtx_gemm_dma) and wait_word already at its number (both kernels).
//   dw     rtx_dw_launch on all nine RtxDwCfg: RTX_DW_GRAD (gW, gbias, g16, gbias16) at 300 x 200 K 250, 77 x 301 K 190, 2 x 1 K 3,
//          1000 x 27 K 128; RTX_DW_ADAM with gkeep (aligned and N % 4 != 0 rows); rtx_dw_launch_group with three matrices.
// --host makes no HIP call: the generator's exactness in two other summation orders, the lse input condition, the launchers' refusals, and that
// the judging reports a reference off by one unit, two swapped tiles, a slab over the neighbouring slices, a strip that takes in column N_real
// and a guard with one byte written.
//
// Not reached by anything in rectorch_amd/ and not tested here: rtx_gemm_launch's syrk_lower map, its fp8 operands, and the K-blocked
// a_slice_stride / b_slice_stride layout.
#include "../../rectorch_amd/csrc/rtx_gemm.h"
#include "check.h"

#include <omp.h>

static constexpr double LSE_MEASURED = 4.158e-7;        // MI355X, every launch of the lse section (see above)
static constexpr double LSE_REL = 4 * LSE_MEASURED;
static_assert(LSE_REL <= 1e-5, "a strip sum that needs more than 1e-5 is a finding to explain, not a bound to raise");
static double g_lse_worst = 0;                          // worst relative error of a strip sum seen in this run

static const char* const FORM_NAME[] = {"NT", "NN", "TN"};
static const char* const EPI_NAME[] = {"store", "bias", "grad"};
static const char* const DT_NAME[] = {"f32", "bf16"};
static const uint32_t NEG_INF_BITS = 0xff800000u;

// ---- exact operands and their product --------------------------------------------------------------------------------------------------------
struct Exact {
    int M = 0, N = 0, K = 0;
    std::vector<int16_t> a, b;     // numerators: A[m][k] = a[m K + k] sa, B[n][k] = b[n K + k] sb
    std::vector<int> bias;         // [N] numerators of the bias
    std::vector<int64_t> c;        // [M][N] = sum_k a b, over the whole K
    double sa = 0.125, sb = 0.125, sbias = 1.0 / 64;
    float prod(const std::vector<int64_t>& units, int m, int n) const { return (float)((double)units[(size_t)m * N + n] * sa * sb); }
    float prod(int m, int n) const { return prod(c, m, n); }
    float logit(int m, int n) const { return (float)((double)c[(size_t)m * N + n] * sa * sb + bias[n] * sbias); }
};
// the int64 count of units over k in [k0, k1), every (m, n)
static void product(const Exact& E, int k0, int k1, std::vector<int64_t>& out)
{
    out.assign((size_t)E.M * E.N, 0);
#pragma omp parallel for schedule(static)
    for (int m = 0; m < E.M; ++m) {
        const int16_t* am = &E.a[(size_t)m * E.K];
        for (int n = 0; n < E.N; ++n) {
            const int16_t* bn = &E.b[(size_t)n * E.K];
            int s = 0;                                       // |s| <= 2048 * 64
            for (int k = k0; k < k1; ++k) s += am[k] * bn[k];
            out[(size_t)m * E.N + n] = s;
        }
    }
}
// rows are drawn one after the other, so the first rows of a larger Exact with the same K and seed are a smaller one: a section draws one
// and every grid is a corner of it
static Exact make_exact(int M, int N, int K, uint32_t seed, bool with_product = true)
{
    Exact E;
    E.M = M; E.N = N; E.K = K;
    Rng r{seed};
    E.a.resize((size_t)M * K); E.b.resize((size_t)N * K); E.bias.resize(N);
    for (auto& v : E.a) v = (int16_t)r.i(-8, 8);
    for (auto& v : E.b) v = (int16_t)r.i(-8, 8);
    for (auto& v : E.bias) v = r.i(-64, 64);
    if (with_product) product(E, 0, K, E.c);
    return E;
}

template <typename T> static T enc(float v);
template <> bf16_t enc<bf16_t>(float v) { return f32_to_bf16(v); }
template <> float enc<float>(float v) { return v; }
template <typename T> static T nan_of();
template <> bf16_t nan_of<bf16_t>() { return 0xffff; }
template <> float nan_of<float>() { return poison_f32(); }

// a rows x K matrix of numerators as an operand image.  K-contiguous: [rows][ld], ld >= K; K-major: [K][ld], ld >= rows.  Rows >= valid
// hold junk when a generator is given; what lies between the extent and ld holds NaN
template <typename T>
static std::vector<T> image(const std::vector<int16_t>& u, int rows, int K, double scale, bool kmajor, long ld, int valid = 1 << 30, Rng* junk = nullptr)
{
    std::vector<T> out((size_t)(kmajor ? K : rows) * ld, nan_of<T>());
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < K; ++k) {
            float v = (float)(u[(size_t)r * K + k] * scale);
            if (junk && r >= valid) v = junk->junk();
            out[kmajor ? (size_t)k * ld + r : (size_t)r * ld + k] = enc<T>(v);
        }
    return out;
}

// the images of one Exact on the device
struct DevOps {
    int M, N, K;
    const bf16_t *a16, *b16, *b16_kn;       // A [M][lda], B [N][ldb] (NT), B [K][ld_kn] (NN)
    const float *a32, *b32, *b32_kn, *a32_km;   // the same in float32, and A [K][ld_km] (TN)
    const float* bias;
    long lda, ldb, ld_kn, ld_km;
};
static DevOps upload(const Exact& E, bool gaps = false, int validM = 1 << 30, int validN = 1 << 30, Rng* junk = nullptr)
{
    DevOps D;
    D.M = E.M; D.N = E.N; D.K = E.K;
    D.lda = D.ldb = E.K + (gaps ? 64 : 0);
    D.ld_kn = E.N + (gaps ? 128 : 0);
    D.ld_km = E.M + (gaps ? 128 : 0);
    D.a16 = to_dev(image<bf16_t>(E.a, E.M, E.K, E.sa, false, D.lda, validM, junk));
    D.b16 = to_dev(image<bf16_t>(E.b, E.N, E.K, E.sb, false, D.ldb, validN, junk));
    D.b16_kn = to_dev(image<bf16_t>(E.b, E.N, E.K, E.sb, true, D.ld_kn, validN, junk));
    D.a32 = to_dev(image<float>(E.a, E.M, E.K, E.sa, false, D.lda, validM, junk));
    D.b32 = to_dev(image<float>(E.b, E.N, E.K, E.sb, false, D.ldb, validN, junk));
    D.b32_kn = to_dev(image<float>(E.b, E.N, E.K, E.sb, true, D.ld_kn, validN, junk));
    D.a32_km = to_dev(image<float>(E.a, E.M, E.K, E.sa, true, D.ld_km, validM, junk));
    std::vector<float> hb(E.N);
    for (int n = 0; n < E.N; ++n) hb[n] = (float)(E.bias[n] * E.sbias);
    D.bias = to_dev(hb);
    return D;
}

// ---- one launch -----------------------------------------------------------------------------------------------------------------------------
enum Kern { KERN_DMA = 0, KERN_RTX = 1, KERN_KM = 2 };
static const char* const KERN_NAME[] = {"gemm_dma", "gemm", "gemm_f32"};
struct Run {
    int kern = KERN_DMA, cfg = 0, form = RTX_FORM_NT, dtype = RTX_DT_BF16, epi = RTX_EPI_STORE;
    int mt = 1, nt = 1, K = 128, splits = 1, xcd = 0;
    int M_real = 0, N_real = 0;
    long ldc = 0;                   // 0: N
    bool lse = false, c16 = false;
    const unsigned* wait_word = nullptr;
    unsigned wait_seq = 0, hop_seq = 0;
    unsigned* hop_word = nullptr;
};
struct Out {
    int M = 0, N = 0, lse_ld = 0, strip = 64, n_strips = 0;
    long ldc = 0;
    std::vector<float> C, gbias;         // C: splits slabs of [M][ldc] (GRAD: [M][N_real])
    std::vector<float2> part;            // [M][lse_ld]
    std::vector<_Float16> c16;           // [M][N]
};
static void tile_of(const Run& r, int* bm, int* bn)
{
    if (r.kern == KERN_DMA) rtx_gemm_dma_tile_dims(r.cfg, bm, bn);
    else if (r.kern == KERN_RTX) rtx_gemm_tile_dims(r.cfg, bm, bn);
    else *bm = *bn = 128;
}
// the slices of K the kernel counts: 64 bf16 (gemm_dma), 128 bytes (gemm.hip), 32 floats (gemm_f32)
static int slice_len(const Run& r) { return r.kern == KERN_DMA ? 64 : r.kern == KERN_KM ? 32 : (r.dtype == RTX_DT_BF16 ? 64 : 32); }
static std::string tag_of(const Run& r)
{
    int bm, bn;
    tile_of(r, &bm, &bn);
    char s[200];
    snprintf(s, sizeof s, "%s cfg%d (%dx%d) %s %s %s %dx%d tiles K=%d splits=%d%s", KERN_NAME[r.kern], r.cfg, bm, bn, FORM_NAME[r.form], DT_NAME[r.dtype],
             EPI_NAME[r.epi], r.mt, r.nt, r.K, r.splits, r.xcd ? " xcd" : "");
    return s;
}
// fills the launch structure; the outputs are null
static RtxGemm describe(const DevOps& D, const Run& r, int M, int N)
{
    RtxGemm g = {};
    g.form = r.form;
    if (r.kern == KERN_KM) {
        g.A = r.form == RTX_FORM_TN ? D.a32_km : D.a32; g.lda = r.form == RTX_FORM_TN ? D.ld_km : D.lda;
        g.B = D.b32_kn; g.ldb = D.ld_kn;
    } else if (r.dtype == RTX_DT_BF16) {
        g.A = D.a16; g.lda = D.lda;
        g.B = r.form == RTX_FORM_NN ? D.b16_kn : D.b16; g.ldb = r.form == RTX_FORM_NN ? D.ld_kn : D.ldb;
    } else {
        g.A = D.a32; g.lda = D.lda; g.B = D.b32; g.ldb = D.ldb;
    }
    g.tile_shape = r.cfg; g.m_tiles = r.mt; g.n_tiles = r.nt; g.k_slices = r.K / slice_len(r); g.splits = r.splits;
    g.xcd_block = r.xcd;
    g.M_real = r.M_real; g.N_real = r.N_real; g.bias = D.bias;
    g.slab_stride = (long)M * N;
    g.wait_word = r.wait_word; g.wait_seq = r.wait_seq; g.hop_word = r.hop_word; g.hop_seq = r.hop_seq;
    return g;
}
static int call(const RtxGemm& g, const Run& r)
{
    if (r.kern == KERN_DMA) return rtx_gemm_dma_launch(g, r.epi, 0);
    if (r.kern == KERN_RTX) return rtx_gemm_launch(g, r.dtype, r.epi, 0);
    return rtx_gemm_f32_km_launch(g, r.epi, 0);
}
// launches, waits, fetches every output with its guard checked, frees
static Out launch(const DevOps& D, const Run& r, Line& L)
{
    int bm, bn;
    tile_of(r, &bm, &bn);
    Out o;
    o.M = r.mt * bm; o.N = r.nt * bn;
    g_tag = tag_of(r);
    if (o.M > D.M || o.N > D.N || r.K != D.K || r.K % slice_len(r)) { printf("%s: the operands are %d x %d x %d\n", g_tag.c_str(), D.M, D.N, D.K); exit(2); }
    const size_t mark = pool_size();
    RtxGemm g = describe(D, r, o.M, o.N);
    o.ldc = r.epi == RTX_EPI_GRAD ? r.N_real : (r.ldc ? r.ldc : o.N);
    g.ldc = o.ldc;
    const size_t csz = (size_t)r.splits * o.M * o.ldc;
    g.C = dev_out<float>(csz);
    if (r.epi == RTX_EPI_GRAD) g.gbias = dev_out<float>(o.M);
    if (r.lse) {
        o.strip = (r.kern == KERN_DMA && r.cfg == RTX_DMA_256x256_W4) ? 128 : 64;
        o.n_strips = o.N / o.strip;
        o.lse_ld = o.N / 64 + 1;          // one strip more than any kernel has: it keeps the poison
        g.lse_ld = o.lse_ld;
        g.lse_part = dev_out<float2>((size_t)o.M * o.lse_ld);
    }
    if (r.c16) { g.C16 = dev_out<_Float16>((size_t)o.M * o.N); g.ldc16 = o.N; }
    RT(call(g, r));
    CK(hipDeviceSynchronize());
    o.C = fetch<float>(g.C, csz, L, "C");
    if (g.gbias) o.gbias = fetch<float>(g.gbias, o.M, L, "gbias");
    if (g.lse_part) o.part = fetch<float2>(g.lse_part, (size_t)o.M * o.lse_ld, L, "lse_part");
    if (g.C16) o.c16 = fetch<_Float16>(g.C16, (size_t)o.M * o.N, L, "C16");
    free_from(mark);
    return o;
}

// ---- judging --------------------------------------------------------------------------------------------------------------------------------
// rows x ld floats: (m < Mv, n < Nv) must hold want(m, n) bit for bit, every other element the poison
template <typename F>
static void judge_block(const float* got, long rows, long ld, int Mv, int Nv, F&& want, Line& L, const char* what)
{
    for (long m = 0; m < rows; ++m)
        for (long n = 0; n < ld; ++n)
            judge_bits(f_bits(got[m * ld + n]), (m < Mv && n < Nv) ? f_bits(want((int)m, (int)n)) : ~0u, L, what, m, n);
}
static void judge_output(const Exact& E, const Run& r, const Out& o, Line& L)
{
    if (r.epi == RTX_EPI_STORE) judge_block(o.C.data(), o.M, o.ldc, o.M, o.N, [&](int m, int n) { return E.prod(m, n); }, L, "C");
    else if (r.epi == RTX_EPI_BIAS_ROWS) judge_block(o.C.data(), o.M, o.ldc, r.M_real, r.N_real, [&](int m, int n) { return E.logit(m, n); }, L, "C");
    else {
        judge_block(o.C.data(), o.M, o.ldc, r.M_real, r.N_real, [&](int m, int n) { return E.prod(m, n); }, L, "gW");
        judge_block(o.gbias.data(), o.M, 1, r.M_real, 1, [&](int m, int) { return E.prod(m, r.N_real); }, L, "gbias");
    }
}

// the strip partials of the logits of E's first M_real rows and N_real columns, strips W columns wide
struct LseRef {
    int W, n_strips, M_real, N_real;
    std::vector<float> mx;       // [M_real][n_strips]; -inf where the strip has no valid column
    std::vector<double> sum;     // sum exp(x - max) in float64; 0 there
    double min_share = 1;        // the smallest term / its strip's sum
};
static LseRef lse_reference(const Exact& E, int M_real, int N_real, int W, int extra_cols = 0)   // extra_cols: a deliberately wrong reference (--host)
{
    LseRef R;
    R.W = W; R.M_real = M_real; R.N_real = N_real; R.n_strips = (E.N + W - 1) / W;
    R.mx.assign((size_t)M_real * R.n_strips, -INFINITY);
    R.sum.assign((size_t)M_real * R.n_strips, 0.0);
    for (int m = 0; m < M_real; ++m)
        for (int q = 0; q < R.n_strips; ++q) {
            const int c0 = q * W, c1 = std::min({(q + 1) * W, N_real + extra_cols, E.N});
            if (c1 <= c0) continue;
            float mx = -INFINITY;
            for (int n = c0; n < c1; ++n) mx = std::max(mx, E.logit(m, n));
            double s = 0, least = 1e300;
            for (int n = c0; n < c1; ++n) { const double t = exp((double)E.logit(m, n) - (double)mx); s += t; least = std::min(least, t); }
            R.mx[(size_t)m * R.n_strips + q] = mx;
            R.sum[(size_t)m * R.n_strips + q] = s;
            R.min_share = std::min(R.min_share, least / s);
        }
    return R;
}
// part: rows x lse_ld.  Rows >= M_real and strips >= n_strips keep the poison; a strip without a valid column holds (-inf, +0)
static void judge_partials(const float2* part, int rows, int lse_ld, int n_strips, const LseRef& R, Line& L, bool bounded = true)
{
    for (int m = 0; m < rows; ++m)
        for (int q = 0; q < lse_ld; ++q) {
            const float2 p = part[(size_t)m * lse_ld + q];
            if (m >= R.M_real || q >= n_strips) {
                judge_bits(f_bits(p.x), ~0u, L, "lse.x", m, q);
                judge_bits(f_bits(p.y), ~0u, L, "lse.y", m, q);
                continue;
            }
            const float mx = R.mx[(size_t)m * R.n_strips + q];
            const double s = R.sum[(size_t)m * R.n_strips + q];
            judge_bits(f_bits(p.x), f_bits(mx), L, "lse.x", m, q);
            if (s == 0) { judge_bits(f_bits(p.y), 0u, L, "lse.y", m, q); continue; }
            if (bounded) {
                judge((double)p.y, s, LSE_REL * s, L, "lse.y", m, q);
                if (p.y == p.y) g_lse_worst = std::max(g_lse_worst, fabs((double)p.y - s) / s);
            } else if (!(p.y >= 1.f && p.y - p.y == 0.f && p.x - p.x == 0.f)) {     // the large-range case: finite, and the maximum's own term is 1
                host_fail(L, "lse partial (%.0f, ...) is not finite with a sum >= 1", m, q);
            }
        }
}
static void judge_c16(const Exact& E, const Run& r, const Out& o, Line& L)
{
    for (int m = 0; m < o.M; ++m)
        for (int n = 0; n < o.N; ++n) {
            uint16_t got;
            memcpy(&got, &o.c16[(size_t)m * o.N + n], 2);
            if (m >= r.M_real) { judge_bits(got, 0xffffu, L, "C16", m, n); continue; }
            if (n >= r.N_real) continue;     // padding columns of valid rows: don't-care values (rtx_gemm.h)
            const float c = std::min(std::max(E.logit(m, n), -65504.f), 65504.f);
            const _Float16 h = (_Float16)c;
            uint16_t want;
            memcpy(&want, &h, 2);
            judge_bits(got, want, L, "C16", m, n);
        }
}

// which (shape, dtype, epilogue) rtx_gemm_launch serves: gemm.hip kTile, restated (refusals() checks the complement)
static bool served(int shape, int dtype, int epi)
{
    if (shape <= RTX_TILE_128x256) return true;
    if (dtype != RTX_DT_BF16) return false;
    return shape == RTX_TILE_128x128_K32 ? epi == RTX_EPI_BIAS_ROWS : (epi == RTX_EPI_STORE || epi == RTX_EPI_BIAS_ROWS);
}
static const int DMA_CFGS = 6;

// ---- map ----------------------------------------------------------------------------------------------------------------------------------------
static void section_map()
{
    const Exact E = make_exact(8704, 2560, 128, 101);
    const DevOps D = upload(E);
    struct Grid { int mt, nt, xcd; };
    const Grid dma_grids[] = {{8, 4, 1}, {9, 5, 1}, {17, 9, 1}, {10, 2, 1}, {2, 10, 1}, {10, 2, 0}, {2, 10, 0}, {3, 3, 0}};
    const Grid strip_grids[] = {{10, 2, 0}, {2, 10, 0}, {3, 3, 0}};
    auto set_real = [](Run& r) {
        int bm, bn;
        tile_of(r, &bm, &bn);
        r.M_real = r.epi == RTX_EPI_STORE ? 0 : r.mt * bm - 3;
        r.N_real = r.epi == RTX_EPI_STORE ? 0 : r.nt * bn - 5;
    };
    for (int cfg = 0; cfg < DMA_CFGS; ++cfg)
        for (int form : {RTX_FORM_NT, RTX_FORM_NN}) {
            Line L;
            int launches = 0;
            for (int epi : {RTX_EPI_STORE, RTX_EPI_BIAS_ROWS}) {
                std::vector<float> thin[2];     // the xcd_block = 1 launches of 10 x 2 and 2 x 10
                for (const Grid& G : dma_grids) {
                    Run r;
                    r.kern = KERN_DMA; r.cfg = cfg; r.form = form; r.epi = epi; r.mt = G.mt; r.nt = G.nt; r.xcd = G.xcd;
                    set_real(r);
                    const Out o = launch(D, r, L);
                    judge_output(E, r, o, L);
                    ++launches;
                    const bool is_thin = G.mt < 8 || G.nt < 4;
                    if (G.xcd && is_thin) thin[G.mt < G.nt] = o.C;
                    else if (!G.xcd && (G.mt == 10 || G.nt == 10) &&
                             (thin[G.mt < G.nt].size() != o.C.size() || memcmp(thin[G.mt < G.nt].data(), o.C.data(), o.C.size() * 4)))
                        host_fail(L, "the xcd_block launch of the thin %.0f x %.0f grid differs from the strip launch", G.mt, G.nt);
                }
            }
            char name[160];
            snprintf(name, sizeof name, "map  gemm_dma cfg%d %s: block map 8x4 9x5 17x9, fall-back 10x2 2x10, strips 10x2 2x10 3x3 (%d launches)", cfg,
                     FORM_NAME[form], launches);
            report(name, L);
        }
    for (int shape = 0; shape < RTX_TILE_COUNT; ++shape)
        for (int dtype : {RTX_DT_BF16, RTX_DT_F32}) {
            Line L;
            int launches = 0;
            for (int epi : {RTX_EPI_STORE, RTX_EPI_BIAS_ROWS, RTX_EPI_GRAD}) {
                if (!served(shape, dtype, epi)) continue;
                for (const Grid& G : strip_grids) {
                    Run r;
                    r.kern = KERN_RTX; r.cfg = shape; r.dtype = dtype; r.epi = epi; r.mt = G.mt; r.nt = G.nt;
                    set_real(r);
                    judge_output(E, r, launch(D, r, L), L);
                    ++launches;
                }
            }
            if (!launches) continue;
            char name[160];
            snprintf(name, sizeof name, "map  gemm tile%d %s: strips 10x2 2x10 3x3, every epilogue it serves (%d launches)", shape, DT_NAME[dtype], launches);
            report(name, L);
        }
    for (int form : {RTX_FORM_NN, RTX_FORM_TN}) {
        Line L;
        for (int epi : {RTX_EPI_STORE, RTX_EPI_GRAD})
            for (const Grid& G : strip_grids) {
                Run r;
                r.kern = KERN_KM; r.form = form; r.dtype = RTX_DT_F32; r.epi = epi; r.mt = G.mt; r.nt = G.nt;
                set_real(r);
                judge_output(E, r, launch(D, r, L), L);
            }
        report(std::string("map  gemm_f32 ") + FORM_NAME[form] + ": strips 10x2 2x10 3x3, store and grad (6 launches)", L);
    }
}

// ---- slabs --------------------------------------------------------------------------------------------------------------------------------------
// slab s of `splits` over `slices` slices of `len` elements: the product over [s per, min((s + 1) per, slices)) -- shifted by `shift` slices for the
// deliberately wrong reference of --host
static std::vector<std::vector<int64_t>> slab_reference(const Exact& E, int slices, int splits, int len, int shift = 0)
{
    const int per = (slices + splits - 1) / splits;
    std::vector<std::vector<int64_t>> S(splits);
    for (int s = 0; s < splits; ++s) {
        const int s0 = std::min(std::max(s * per + shift, 0), slices), s1 = std::min(std::max((s + 1) * per + shift, 0), slices);
        product(E, s0 * len, std::max(s1, s0) * len, S[s]);
    }
    return S;
}
static void judge_slabs(const Exact& E, const std::vector<std::vector<int64_t>>& S, const float* C, int M, int N, Line& L)
{
    for (size_t s = 0; s < S.size(); ++s) {
        char what[32];
        snprintf(what, sizeof what, "slab %zu", s);
        judge_block(C + s * (size_t)M * N, M, N, M, N, [&](int m, int n) { return E.prod(S[s], m, n); }, L, what);
    }
}
static void section_slabs()
{
    struct Split { int slices, splits; };
    const Split cases[] = {{7, 3}, {22, 11}, {2, 2}, {11, 5}};   // the last: an empty fifth split (rtx_gemm_nt only)
    for (const Split& c : cases)
        for (int len : {64, 32}) {      // 64: the bf16 kernels; 32: the float32 ones
            const size_t mark = pool_size();
            const Exact E = make_exact(len == 64 ? 1024 : 512, 768, c.slices * len, 202 + c.slices, false);
            const auto S = slab_reference(E, c.slices, c.splits, len);
            const DevOps D = upload(E);
            const bool empty = (c.splits - 1) * ((c.slices + c.splits - 1) / c.splits) >= c.slices;
            Line L;
            int launches = 0;
            auto go = [&](Run r) {
                r.mt = 2; r.nt = 3; r.K = E.K; r.splits = c.splits; r.epi = RTX_EPI_STORE;
                const Out o = launch(D, r, L);
                judge_slabs(E, S, o.C.data(), o.M, o.N, L);
                ++launches;
            };
            for (int cfg = 0; len == 64 && !empty && cfg < DMA_CFGS; ++cfg)
                for (int form : {RTX_FORM_NT, RTX_FORM_NN}) { Run r; r.kern = KERN_DMA; r.cfg = cfg; r.form = form; go(r); }
            for (int shape = 0; shape < RTX_TILE_COUNT; ++shape) {
                const int dtype = len == 64 ? RTX_DT_BF16 : RTX_DT_F32;
                if (!served(shape, dtype, RTX_EPI_STORE)) continue;
                Run r; r.kern = KERN_RTX; r.cfg = shape; r.dtype = dtype; go(r);
            }
            for (int form : {RTX_FORM_NN, RTX_FORM_TN}) {
                if (len != 32 || empty) continue;
                Run r; r.kern = KERN_KM; r.form = form; r.dtype = RTX_DT_F32; go(r);
            }
            char name[160];
            snprintf(name, sizeof name, "slabs %d slices / %d splits%s, %s kernels: every slab over its own slices (%d launches)", c.slices, c.splits,
                     empty ? " (the last one empty: +0)" : "", len == 64 ? "bf16" : "float32", launches);
            report(name, L);
            free_from(mark);
        }
}

// ---- lse ----------------------------------------------------------------------------------------------------------------------------------------
struct LseCase { int M_real, N_real, K; };
static const LseCase LSE_CASES[] = {{410, 701, 128}, {77, 131, 64}, {250, 2300, 192}, {130, 192, 128}};
// the recipe of the lse data: B = j / 64, bias multiples of 1 / 64; drawn for the largest padding any tile gives the case
static Exact make_lse_exact(const LseCase& c, uint32_t seed)
{
    Exact E = make_exact((c.M_real + 511) / 512 * 512, (c.N_real + 255) / 256 * 256, c.K, seed, false);
    E.sb = 1.0 / 64;
    product(E, 0, E.K, E.c);
    return E;
}
static void section_lse()
{
    uint32_t seed = 300;
    for (const LseCase& c : LSE_CASES) {
        const size_t mark = pool_size();
        const Exact E = make_lse_exact(c, ++seed);
        const LseRef R64 = lse_reference(E, c.M_real, c.N_real, 64), R128 = lse_reference(E, c.M_real, c.N_real, 128);
        const DevOps D = upload(E);
        auto go = [&](Run r, Line& L) {
            int bm, bn;
            tile_of(r, &bm, &bn);
            r.epi = RTX_EPI_BIAS_ROWS; r.K = c.K; r.M_real = c.M_real; r.N_real = c.N_real; r.lse = true;
            r.mt = (c.M_real + bm - 1) / bm; r.nt = (c.N_real + bn - 1) / bn;
            const Out o = launch(D, r, L);
            judge_output(E, r, o, L);
            judge_partials(o.part.data(), o.M, o.lse_ld, o.n_strips, o.strip == 64 ? R64 : R128, L);
            if (r.kern == KERN_RTX && r.dtype == RTX_DT_BF16) {      // the step's launch: half logits instead of C, the same partials
                r.c16 = true;
                const Out h = launch(D, r, L);
                g_tag += " C16";
                judge_block(h.C.data(), h.M, h.ldc, 0, 0, [](int, int) { return 0.f; }, L, "C beside C16");
                judge_c16(E, r, h, L);
                judge_partials(h.part.data(), h.M, h.lse_ld, h.n_strips, R64, L);
            }
        };
        char name[160];
        for (int shape = 0; shape < RTX_TILE_COUNT; ++shape)
            for (int dtype : {RTX_DT_BF16, RTX_DT_F32}) {
                if (!served(shape, dtype, RTX_EPI_BIAS_ROWS)) continue;
                Line L;
                Run r; r.kern = KERN_RTX; r.cfg = shape; r.dtype = dtype;
                go(r, L);
                snprintf(name, sizeof name, "lse  %d x %d K %d  gemm tile%d %s%s", c.M_real, c.N_real, c.K, shape, DT_NAME[dtype], dtype == RTX_DT_BF16 ? " (+ C16)" : "");
                report(name, L);
            }
        for (int cfg = 0; cfg < DMA_CFGS; ++cfg)
            for (int form : {RTX_FORM_NT, RTX_FORM_NN}) {
                Line L;
                Run r; r.kern = KERN_DMA; r.cfg = cfg; r.form = form;
                go(r, L);
                snprintf(name, sizeof name, "lse  %d x %d K %d  gemm_dma cfg%d %s", c.M_real, c.N_real, c.K, cfg, FORM_NAME[form]);
                report(name, L);
            }
        free_from(mark);
    }
    {   // the large range: A and the bias times 2^18 -- still exact, and most logits beyond the half range
        const LseCase& c = LSE_CASES[0];
        Exact E = make_lse_exact(c, 399);
        E.sa *= 262144.0; E.sbias *= 262144.0;
        const LseRef R = lse_reference(E, c.M_real, c.N_real, 64);
        const DevOps D = upload(E);
        long beyond = 0;
        for (int m = 0; m < c.M_real; ++m)
            for (int n = 0; n < c.N_real; ++n) beyond += fabsf(E.logit(m, n)) > 65504.f;
        for (int shape = 0; shape < RTX_TILE_COUNT; ++shape) {
            Line L;
            if (beyond * 4 < (long)c.M_real * c.N_real) host_fail(L, "only %.0f of %.0f logits are beyond the half range", (double)beyond, (double)c.M_real * c.N_real);
            Run r;
            r.kern = KERN_RTX; r.cfg = shape; r.epi = RTX_EPI_BIAS_ROWS; r.K = c.K; r.M_real = c.M_real; r.N_real = c.N_real; r.lse = true;
            int bm, bn;
            tile_of(r, &bm, &bn);
            r.mt = (c.M_real + bm - 1) / bm; r.nt = (c.N_real + bn - 1) / bn;
            Out o = launch(D, r, L);
            judge_output(E, r, o, L);
            judge_partials(o.part.data(), o.M, o.lse_ld, o.n_strips, R, L, false);
            r.c16 = true;
            o = launch(D, r, L);
            judge_c16(E, r, o, L);
            judge_partials(o.part.data(), o.M, o.lse_ld, o.n_strips, R, L, false);
            char name[160];
            snprintf(name, sizeof name, "lse  %d x %d K %d times 2^18 (%ld logits clamped)  gemm tile%d bf16, C and C16", c.M_real, c.N_real, c.K, beyond, shape);
            report(name, L);
        }
    }
    printf("lse: worst relative error of a strip sum against float64: %.3e (LSE_MEASURED %.3e, bound LSE_REL %.3e)\n", g_lse_worst, LSE_MEASURED, LSE_REL);
}

// ---- edges --------------------------------------------------------------------------------------------------------------------------------------
// valid rows; valid columns of the bias launches (N_real % 4 == 2: with 701, 131, 2300 and 192 of the lse cases every one of the four column masks of a
// float4 has its boundary case) and of the grad launches (column 333: gbias)
static const int EDGE_M = 300, EDGE_NB = 334, EDGE_NG = 333;
static Exact make_edges_exact()
{
    Exact E = make_exact(512, 512, 128, 404, false);
    E.sb = 1.0 / 64;       // (the recipe of the lse data: the same bound holds the strip sums here)
    product(E, 0, E.K, E.c);
    return E;
}
static void section_edges()
{
    const Exact E = make_edges_exact();
    Rng junk{405};
    const DevOps D = upload(E, true, EDGE_M, EDGE_NB, &junk);       // junk rows, NaN gaps
    const LseRef R64 = lse_reference(E, EDGE_M, EDGE_NB, 64), R128 = lse_reference(E, EDGE_M, EDGE_NB, 128);
    auto grid = [&](Run& r) {
        int bm, bn;
        tile_of(r, &bm, &bn);
        r.mt = (EDGE_M + bm - 1) / bm; r.nt = (EDGE_NB + bn - 1) / bn; r.M_real = EDGE_M;
    };
    auto bias_runs = [&](Run r, Line& L) {
        for (long ldc : {336L, 335L}) {      // ldc % 4 == 0: the vector stores; odd: the scalar ones.  Both below the padded width
            r.epi = RTX_EPI_BIAS_ROWS; r.N_real = EDGE_NB; r.ldc = ldc; r.lse = true;
            grid(r);
            const Out o = launch(D, r, L);
            g_tag += ldc & 3 ? " odd ldc" : " ldc % 4 == 0";
            judge_output(E, r, o, L);
            judge_partials(o.part.data(), o.M, o.lse_ld, o.n_strips, o.strip == 64 ? R64 : R128, L);
        }
    };
    auto grad_run = [&](Run r, Line& L) {
        r.epi = RTX_EPI_GRAD; r.N_real = EDGE_NG;
        grid(r);
        judge_output(E, r, launch(D, r, L), L);
    };
    char name[160];
    for (int cfg = 0; cfg < DMA_CFGS; ++cfg)
        for (int form : {RTX_FORM_NT, RTX_FORM_NN}) {
            Line L;
            Run r; r.kern = KERN_DMA; r.cfg = cfg; r.form = form;
            bias_runs(r, L);
            snprintf(name, sizeof name, "edges gemm_dma cfg%d %s: bias + lse at ldc 336 / 335, junk rows, NaN gaps", cfg, FORM_NAME[form]);
            report(name, L);
        }
    for (int shape = 0; shape < RTX_TILE_COUNT; ++shape)
        for (int dtype : {RTX_DT_BF16, RTX_DT_F32}) {
            if (!served(shape, dtype, RTX_EPI_BIAS_ROWS)) continue;
            Line L;
            Run r; r.kern = KERN_RTX; r.cfg = shape; r.dtype = dtype;
            bias_runs(r, L);
            if (served(shape, dtype, RTX_EPI_GRAD)) grad_run(r, L);
            snprintf(name, sizeof name, "edges gemm tile%d %s: bias + lse at ldc 336 / 335%s, junk rows, NaN gaps", shape, DT_NAME[dtype],
                     served(shape, dtype, RTX_EPI_GRAD) ? ", grad" : "");
            report(name, L);
        }
    for (int form : {RTX_FORM_NN, RTX_FORM_TN}) {
        Line L;
        Run r; r.kern = KERN_KM; r.form = form; r.dtype = RTX_DT_F32;
        grad_run(r, L);
        report(std::string("edges gemm_f32 ") + FORM_NAME[form] + ": grad, junk rows, NaN gaps", L);
    }
    // the folded hop and wait words.  The wait word ALREADY holds its number: a launch that had to wait would be a deliberate hang
    {
        Line L;
        const unsigned seq = 0x1234567u;
        const std::vector<unsigned> reached(1, seq);
        const unsigned* wait_word = to_dev(reached);
        unsigned* hop_word = dev_out<unsigned>(1);
        for (int kern : {KERN_DMA, KERN_RTX})
            for (int epi : {RTX_EPI_STORE, RTX_EPI_BIAS_ROWS}) {
                Run r; r.kern = kern; r.epi = epi; r.mt = 2; r.nt = 2; r.M_real = epi ? 250 : 0; r.N_real = epi ? 251 : 0;     // (256 x 256: no junk row in it)
                const Out plain = launch(D, r, L);
                judge_output(E, r, plain, L);
                r.wait_word = wait_word; r.wait_seq = seq;
                if (kern == KERN_DMA) { r.hop_word = hop_word; r.hop_seq = 77u + epi; }
                const Out folded = launch(D, r, L);
                g_tag += " wait_word";
                judge_output(E, r, folded, L);
                if (plain.C.size() != folded.C.size() || memcmp(plain.C.data(), folded.C.data(), plain.C.size() * 4)) host_fail(L, "the launch with a wait word differs from the one without");
                if (kern == KERN_DMA) judge_bits(fetch<unsigned>(hop_word, 1, L, "hop_word")[0], r.hop_seq, L, "hop_word", 0);
            }
        report("edges hop_word takes hop_seq (gemm_dma); wait_word at its number changes nothing (gemm_dma, gemm)", L);
    }
    printf("edges: worst relative error of a strip sum against float64: %.3e (bound LSE_REL %.3e)\n", g_lse_worst, LSE_REL);
}

// ---- dw -----------------------------------------------------------------------------------------------------------------------------------------
// D [Kp][Mp] deltas k / 128 (columns >= M_real junk), X [Kp][Np] activations k / 8 with ones in column N_real; rows >= K_real zero (the contract)
struct DwProblem {
    int M_real, N_real, K_real, Mp, Np, Kp;
    std::vector<int16_t> d, x;          // [K_real][M_real], [K_real][N_real + 1] (the ones column: 8)
    std::vector<int64_t> g;             // [M_real][N_real + 1], units of 2^-10
    const bf16_t *D, *X;
    float grad(int m, int n) const { return (float)((double)g[(size_t)m * (N_real + 1) + n] * (1.0 / 1024)); }
};
static DwProblem make_dw(int M_real, int N_real, int K_real, uint32_t seed, bool device)
{
    DwProblem P;
    P.M_real = M_real; P.N_real = N_real; P.K_real = K_real;
    P.Mp = rtx_pad(M_real); P.Np = rtx_pad(N_real); P.Kp = rtx_pad_batch(K_real);
    Rng r{seed};
    P.d.resize((size_t)K_real * M_real); P.x.resize((size_t)K_real * (N_real + 1));
    for (auto& v : P.d) v = (int16_t)r.i(-8, 8);
    for (int k = 0; k < K_real; ++k)
        for (int n = 0; n <= N_real; ++n) P.x[(size_t)k * (N_real + 1) + n] = n == N_real ? 8 : (int16_t)r.i(-8, 8);
    P.g.assign((size_t)M_real * (N_real + 1), 0);
#pragma omp parallel for schedule(static)
    for (int m = 0; m < M_real; ++m)
        for (int k = 0; k < K_real; ++k) {
            const int dk = P.d[(size_t)k * M_real + m];
            for (int n = 0; n <= N_real; ++n) P.g[(size_t)m * (N_real + 1) + n] += dk * P.x[(size_t)k * (N_real + 1) + n];
        }
    P.D = P.X = nullptr;
    if (device) {
        std::vector<bf16_t> hD((size_t)P.Kp * P.Mp, 0), hX((size_t)P.Kp * P.Np, 0);
        for (int k = 0; k < K_real; ++k) {
            for (int m = 0; m < P.Mp; ++m) hD[(size_t)k * P.Mp + m] = f32_to_bf16(m < M_real ? P.d[(size_t)k * M_real + m] * (1.f / 128) : r.junk());
            for (int n = 0; n <= N_real; ++n) hX[(size_t)k * P.Np + n] = f32_to_bf16(P.x[(size_t)k * (N_real + 1) + n] * 0.125f);
        }
        P.D = to_dev(hD); P.X = to_dev(hX);
    }
    return P;
}
static RtxDw describe_dw(const DwProblem& P, int cfg)
{
    RtxDw d = {};
    d.A = P.D; d.lda = P.Mp; d.B = P.X; d.ldb = P.Np;
    d.m_tiles = P.Mp / rtx_dw_tile_rows(cfg); d.n_tiles = (P.Np + rtx_dw_tile_cols(cfg) - 1) / rtx_dw_tile_cols(cfg); d.k_slices = P.Kp / 64;
    d.M_real = P.M_real; d.N_real = P.N_real;
    return d;
}
struct DwGradOut { float *gW, *gbias; bf16_t *g16, *gbias16; };
static DwGradOut dw_grad_outputs(const DwProblem& P, RtxDw& d)
{
    const size_t n = (size_t)P.M_real * P.N_real;
    DwGradOut o = {dev_out<float>(n), dev_out<float>(P.M_real), dev_out<bf16_t>(n), dev_out<bf16_t>(P.M_real)};
    d.gW = o.gW; d.gbias = o.gbias; d.g16 = o.g16; d.gbias16 = o.gbias16;
    return o;
}
static void judge_dw_grad(const DwProblem& P, const DwGradOut& o, Line& L)
{
    const size_t n = (size_t)P.M_real * P.N_real;
    const std::vector<float> gW = fetch<float>(o.gW, n, L, "gW"), gb = fetch<float>(o.gbias, P.M_real, L, "gbias");
    const std::vector<bf16_t> g16 = fetch<bf16_t>(o.g16, n, L, "g16"), gb16 = fetch<bf16_t>(o.gbias16, P.M_real, L, "gbias16");
    for (int m = 0; m < P.M_real; ++m) {
        for (int c = 0; c < P.N_real; ++c) {
            judge_bits(f_bits(gW[(size_t)m * P.N_real + c]), f_bits(P.grad(m, c)), L, "gW", m, c);
            judge_bits(g16[(size_t)m * P.N_real + c], f32_to_bf16(P.grad(m, c)), L, "g16", m, c);
        }
        judge_bits(f_bits(gb[m]), f_bits(P.grad(m, P.N_real)), L, "gbias", m);
        judge_bits(gb16[m], f32_to_bf16(P.grad(m, P.N_real)), L, "gbias16", m);
    }
}
static void section_dw()
{
    const int grad_shapes[][3] = {{300, 200, 250}, {77, 301, 190}, {2, 1, 3}, {1000, 27, 128}};
    const int group_shapes[][2] = {{70, 132}, {300, 200}, {130, 600}};
    std::vector<DwProblem> P, G;
    for (auto& s : grad_shapes) P.push_back(make_dw(s[0], s[1], s[2], 500 + s[0], true));
    for (auto& s : group_shapes) G.push_back(make_dw(s[0], s[1], 250, 600 + s[0], true));
    char name[160];
    for (int cfg = 0; cfg < RTX_DW_CFG_COUNT; ++cfg) {
        {
            Line L;
            for (const DwProblem& p : P) {
                const size_t mark = pool_size();
                snprintf(name, sizeof name, "dw cfg%d grad %d x %d K %d", cfg, p.M_real, p.N_real, p.K_real);
                g_tag = name;
                RtxDw d = describe_dw(p, cfg);
                const DwGradOut o = dw_grad_outputs(p, d);
                RT(rtx_dw_launch(d, RTX_DW_GRAD, cfg, 0));
                CK(hipDeviceSynchronize());
                judge_dw_grad(p, o, L);
                free_from(mark);
            }
            snprintf(name, sizeof name, "dw   cfg%d (%d x %d) RTX_DW_GRAD: gW, gbias, g16, gbias16 at the four shapes", cfg, rtx_dw_tile_rows(cfg), rtx_dw_tile_cols(cfg));
            report(name, L);
        }
        {
            Line L;
            const size_t mark = pool_size();
            g_tag = "dw group";
            RtxDw d[3];
            DwGradOut o[3];
            for (int k = 0; k < 3; ++k) { d[k] = describe_dw(G[k], cfg); o[k] = dw_grad_outputs(G[k], d[k]); }
            RT(rtx_dw_launch_group(d, 3, RTX_DW_GRAD, cfg, 0));
            CK(hipDeviceSynchronize());
            for (int k = 0; k < 3; ++k) {
                snprintf(name, sizeof name, "dw cfg%d group matrix %d (%d x %d)", cfg, k, G[k].M_real, G[k].N_real);
                g_tag = name;
                judge_dw_grad(G[k], o[k], L);
            }
            free_from(mark);
            snprintf(name, sizeof name, "dw   cfg%d rtx_dw_launch_group, three matrices, RTX_DW_GRAD", cfg);
            report(name, L);
        }
        {   // the fused Adam step, the gradient kept: gkeep exact; p, m, v within run_dw_case's 2e-6 of the float32 formulas on the EXACT gradient
            Line L;
            for (const DwProblem& p : P) {
                if (p.N_real < 4) continue;      // (the fused epilogue needs rows of four floats)
                const size_t mark = pool_size();
                snprintf(name, sizeof name, "dw cfg%d adam %d x %d K %d", cfg, p.M_real, p.N_real, p.K_real);
                g_tag = name;
                const size_t n = (size_t)p.M_real * p.N_real;
                Rng r{700u + cfg};
                std::vector<float> hp(n), hm(n), hv(n), hbp(p.M_real), hbm(p.M_real), hbv(p.M_real);
                for (size_t i = 0; i < n; ++i) { hp[i] = r.f(); hm[i] = r.f() * 0.01f; hv[i] = fabsf(r.f()) * 1e-4f; }
                for (int i = 0; i < p.M_real; ++i) { hbp[i] = r.f(); hbm[i] = r.f() * 0.01f; hbv[i] = fabsf(r.f()) * 1e-4f; }
                auto out_of = [&](const std::vector<float>& h) {
                    float* dptr = dev_out<float>(h.size());
                    CK(hipMemcpy(dptr, h.data(), h.size() * 4, hipMemcpyHostToDevice));
                    return dptr;
                };
                RtxDw d = describe_dw(p, cfg);
                const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
                const float step_size = (float)(1e-3 / (1.0 - pow((double)b1, 3))), bc2 = (float)sqrt(1.0 - pow((double)b2, 3));
                d.adam.p = out_of(hp); d.adam.m = out_of(hm); d.adam.v = out_of(hv); d.adam.gkeep = dev_out<float>(n);
                d.adam.sh = dev_bytes((size_t)p.Mp * p.Np * 2, 0); d.adam.ld_sh = p.Np;
                d.adam.step_size = step_size; d.adam.bc2_sqrt = bc2; d.adam.beta1 = b1; d.adam.beta2 = b2; d.adam.eps = eps;
                d.bias_p = out_of(hbp); d.bias_m = out_of(hbm); d.bias_v = out_of(hbv);
                d.gbias = dev_out<float>(p.M_real);
                RT(rtx_dw_launch(d, RTX_DW_ADAM, cfg, 0));
                CK(hipDeviceSynchronize());
                const std::vector<float> gp = fetch<float>(d.adam.p, n, L, "p"), gm = fetch<float>(d.adam.m, n, L, "m"), gv = fetch<float>(d.adam.v, n, L, "v"),
                                         gk = fetch<float>(d.adam.gkeep, n, L, "gkeep"), gb = fetch<float>(d.gbias, p.M_real, L, "gbias"),
                                         bp = fetch<float>(d.bias_p, p.M_real, L, "bias_p"), bm = fetch<float>(d.bias_m, p.M_real, L, "bias_m"),
                                         bv = fetch<float>(d.bias_v, p.M_real, L, "bias_v");
                const std::vector<bf16_t> sh = to_host((const bf16_t*)d.adam.sh, (size_t)p.Mp * p.Np);
                auto adam = [&](float g, float p0, float m0, float v0, float* p1, float* m1, float* v1) {
                    *m1 = m0 + (g - m0) * (1.f - b1);
                    *v1 = v0 * b2 + (1.f - b2) * g * g;
                    *p1 = p0 - step_size * (*m1 / (sqrtf(*v1) / bc2 + eps));
                };
                for (int m = 0; m < p.M_real; ++m) {
                    float p1, m1, v1;
                    for (int c = 0; c < p.N_real; ++c) {
                        const size_t i = (size_t)m * p.N_real + c;
                        judge_bits(f_bits(gk[i]), f_bits(p.grad(m, c)), L, "gkeep", m, c);
                        adam(p.grad(m, c), hp[i], hm[i], hv[i], &p1, &m1, &v1);
                        judge(gp[i], p1, 2e-6, L, "p", m, c); judge(gm[i], m1, 2e-6, L, "m", m, c); judge(gv[i], v1, 2e-6, L, "v", m, c);
                        judge_bits(sh[(size_t)m * p.Np + c], f32_to_bf16(gp[i]), L, "compute copy", m, c);
                    }
                    judge_bits(f_bits(gb[m]), f_bits(p.grad(m, p.N_real)), L, "gbias", m);
                    adam(p.grad(m, p.N_real), hbp[m], hbm[m], hbv[m], &p1, &m1, &v1);
                    judge(bp[m], p1, 2e-6, L, "bias_p", m); judge(bm[m], m1, 2e-6, L, "bias_m", m); judge(bv[m], v1, 2e-6, L, "bias_v", m);
                }
                for (int m = 0; m < p.Mp; ++m)       // the padding of the compute copy stays zero
                    for (int c = 0; c < p.Np; ++c)
                        if (m >= p.M_real || c >= p.N_real) judge_bits(sh[(size_t)m * p.Np + c], 0, L, "compute-copy padding", m, c);
                free_from(mark);
            }
            snprintf(name, sizeof name, "dw   cfg%d RTX_DW_ADAM with gkeep: gkeep and gbias exact; p, m, v, bias within 2e-6; compute copy = bf16(p)", cfg);
            report(name, L);
        }
    }
}

// ---- --host -------------------------------------------------------------------------------------------------------------------------------------
static int refused(int rc, const char* word)
{
    return rc == RTX_EINVAL && strstr(rtx_last_error_str(), word) != nullptr;
}
static void host_refusals()
{
    Line L;
    static float buf[64];     // never read or written: every request below is refused before anything is launched
    RtxGemm g = {};
    g.A = g.B = buf; g.C = buf; g.lda = g.ldb = 128; g.ldc = 128; g.m_tiles = g.n_tiles = 1; g.k_slices = 11; g.splits = 5; g.slab_stride = 128 * 128;
    if (!refused(rtx_gemm_dma_launch(g, RTX_EPI_STORE, 0), "empty split")) host_fail(L, "gemm_dma takes 11 slices in 5 splits");
    g.form = RTX_FORM_NN;
    if (!refused(rtx_gemm_f32_km_launch(g, RTX_EPI_STORE, 0), "empty split")) host_fail(L, "gemm_f32 takes 11 slices in 5 splits");
    g.form = RTX_FORM_NT; g.k_slices = 2; g.splits = 1;
    g.tile_shape = 6;
    if (!refused(rtx_gemm_dma_launch(g, RTX_EPI_STORE, 0), "bad tile configuration")) host_fail(L, "gemm_dma takes configuration 6");
    g.tile_shape = -1;
    if (!refused(rtx_gemm_dma_launch(g, RTX_EPI_STORE, 0), "bad tile configuration")) host_fail(L, "gemm_dma takes configuration -1");
    g.tile_shape = 0; g.form = RTX_FORM_TN;
    if (!refused(rtx_gemm_dma_launch(g, RTX_EPI_STORE, 0), "form")) host_fail(L, "gemm_dma takes the TN form");
    g.form = RTX_FORM_NT;
    if (!refused(rtx_gemm_dma_launch(g, RTX_EPI_GRAD, 0), "bad epilogue")) host_fail(L, "gemm_dma takes the grad epilogue");
    g.splits = 2;
    if (!refused(rtx_gemm_dma_launch(g, RTX_EPI_BIAS_ROWS, 0), "split-K only")) host_fail(L, "gemm_dma takes split-K with the bias epilogue");
    if (!refused(rtx_gemm_launch(g, RTX_DT_BF16, RTX_EPI_BIAS_ROWS, 0), "split-K only")) host_fail(L, "gemm takes split-K with the bias epilogue");
    g.splits = 1;
    if (!refused(rtx_gemm_f32_km_launch(g, RTX_EPI_STORE, 0), "form")) host_fail(L, "gemm_f32 takes the NT form");
    // the half logits: bias epilogue, bf16, 8-byte aligned, ldc16 a multiple of 4 and >= N_pad
    g.M_real = g.N_real = 100; g.bias = buf;
    g.C16 = (char*)buf + 2; g.ldc16 = 128;
    if (!refused(rtx_gemm_launch(g, RTX_DT_BF16, RTX_EPI_BIAS_ROWS, 0), "half-precision")) host_fail(L, "gemm takes a misaligned C16");
    g.C16 = buf; g.ldc16 = 130;
    if (!refused(rtx_gemm_launch(g, RTX_DT_BF16, RTX_EPI_BIAS_ROWS, 0), "half-precision")) host_fail(L, "gemm takes ldc16 = 130");
    g.ldc16 = 64;
    if (!refused(rtx_gemm_launch(g, RTX_DT_BF16, RTX_EPI_BIAS_ROWS, 0), "half-precision")) host_fail(L, "gemm takes ldc16 below the padded width");
    g.ldc16 = 128;
    if (!refused(rtx_gemm_launch(g, RTX_DT_F32, RTX_EPI_BIAS_ROWS, 0), "half-precision")) host_fail(L, "gemm takes C16 with float32 operands");
    if (!refused(rtx_gemm_launch(g, RTX_DT_BF16, RTX_EPI_STORE, 0), "half-precision")) host_fail(L, "gemm takes C16 with the store epilogue");
    g.C16 = nullptr;
    // every (shape, dtype, epilogue) kTile does not serve
    int unserved = 0;
    for (int shape = 0; shape < RTX_TILE_COUNT; ++shape)
        for (int dtype : {RTX_DT_F32, RTX_DT_BF16})
            for (int epi : {RTX_EPI_STORE, RTX_EPI_BIAS_ROWS, RTX_EPI_GRAD}) {
                if (served(shape, dtype, epi)) continue;
                ++unserved;
                g.tile_shape = shape;
                if (!refused(rtx_gemm_launch(g, dtype, epi, 0), "tile exists for")) host_fail(L, "gemm takes tile %.0f with a combination kTile does not serve", shape);
            }
    if (unserved != 9) host_fail(L, "%.0f unserved combinations, expected 9", unserved);
    g.tile_shape = RTX_TILE_COUNT;
    if (!refused(rtx_gemm_launch(g, RTX_DT_BF16, RTX_EPI_STORE, 0), "bad tile shape")) host_fail(L, "gemm takes an unknown tile shape");
    report("host refusals: empty split, configuration, form, epilogue, C16 alignment and pitch, unserved kTile combinations", L);
}
// a scratch line that counts mismatches without printing them
static Line quiet() { Line L; L.bad = 4; return L; }
static long caught(const Line& L) { return L.bad - 4; }
static void host_checks()
{
    {   // the generator: float32 sums of the longest K in two other orders equal the int64 count
        Line L;
        const int K = 22 * 64;
        const Exact E = make_exact(24, 24, K, 202 + 22);
        for (int m = 0; m < E.M; ++m)
            for (int n = 0; n < E.N; ++n) {
                float rev = 0.f, strided = 0.f;
                auto term = [&](int k) { return (float)(E.a[(size_t)m * K + k] * E.sa) * (float)(E.b[(size_t)n * K + k] * E.sb); };
                for (int k = K - 1; k >= 0; --k) rev += term(k);
                for (int s = 0; s < 7; ++s)
                    for (int k = s; k < K; k += 7) strided += term(k);
                judge_bits(f_bits(rev), f_bits(E.prod(m, n)), L, "reversed sum", m, n);
                judge_bits(f_bits(strided), f_bits(E.prod(m, n)), L, "strided sum", m, n);
                const bf16_t a0 = f32_to_bf16((float)(E.a[(size_t)m * K + n] * E.sa));
                if (bf16_to_f32(a0) != (float)(E.a[(size_t)m * K + n] * E.sa)) host_fail(L, "an operand entry is not exact in bf16");
            }
        report("host generator: float32 sums over K = 1408 reversed and strided equal the integer reference; entries exact in bf16", L);
    }
    {   // the lse inputs: the smallest valid term of every strip is at least 1e-4 of the strip's sum, at both strip widths
        Line L;
        uint32_t seed = 300;
        for (const LseCase& c : LSE_CASES) {
            const Exact E = make_lse_exact(c, ++seed);
            for (int W : {64, 128}) {
                const double share = lse_reference(E, c.M_real, c.N_real, W).min_share;
                printf("    lse inputs %d x %d K %d, strips of %d: smallest share %.3e\n", c.M_real, c.N_real, c.K, W, share);
                if (!(share >= 1e-4)) host_fail(L, "a term is %.3e of its strip's sum: below 1e-4", share);
            }
            // a strip that takes in column N_real is reported, in every row of the boundary strip
            const LseRef R = lse_reference(E, c.M_real, c.N_real, 64), wrong = lse_reference(E, c.M_real, c.N_real, 64, 1);
            std::vector<float2> perfect((size_t)c.M_real * R.n_strips);
            for (size_t i = 0; i < perfect.size(); ++i) perfect[i] = make_float2(R.mx[i], (float)R.sum[i]);
            Line ok, bad = quiet();
            judge_partials(perfect.data(), c.M_real, R.n_strips, R.n_strips, R, ok);
            judge_partials(perfect.data(), c.M_real, R.n_strips, R.n_strips, wrong, bad);
            if (ok.bad) host_fail(L, "the reference's own partials are judged bad");
            if (caught(bad) < c.M_real) host_fail(L, "a strip including column N_real is judged bad in %.0f rows of %.0f", (double)caught(bad), c.M_real);
        }
        const Exact E = make_edges_exact();
        for (int W : {64, 128}) {
            const double share = lse_reference(E, EDGE_M, EDGE_NB, W).min_share;
            printf("    edges inputs %d x %d K %d, strips of %d: smallest share %.3e\n", EDGE_M, EDGE_NB, E.K, W, share);
            if (!(share >= 1e-4)) host_fail(L, "a term is %.3e of its strip's sum: below 1e-4", share);
        }
        report("host lse inputs: smallest share >= 1e-4; a strip that includes column N_real is judged bad in every row", L);
    }
    {   // map: one element off by one unit; two tiles swapped
        Line L;
        Exact E = make_exact(256, 384, 128, 101);
        std::vector<float> perfect((size_t)E.M * E.N);
        for (int m = 0; m < E.M; ++m)
            for (int n = 0; n < E.N; ++n) perfect[(size_t)m * E.N + n] = E.prod(m, n);
        Line ok, off = quiet(), swapped = quiet();
        judge_block(perfect.data(), E.M, E.N, E.M, E.N, [&](int m, int n) { return E.prod(m, n); }, ok, "C");
        judge_block(perfect.data(), E.M, E.N, E.M, E.N, [&](int m, int n) { return E.prod(m ^ 128, n); }, swapped, "C");      // tile rows 0 and 1 exchanged
        E.c[(size_t)77 * E.N + 131] += 1;
        judge_block(perfect.data(), E.M, E.N, E.M, E.N, [&](int m, int n) { return E.prod(m, n); }, off, "C");
        E.c[(size_t)77 * E.N + 131] -= 1;
        if (ok.bad || caught(off) != 1) host_fail(L, "one unit off in one element: %.0f mismatches", (double)caught(off));
        if (caught(swapped) < (long)E.M * E.N / 2) host_fail(L, "two swapped tile rows: %.0f mismatches", (double)caught(swapped));
        // edges: a written padding column, a written row beyond M_real
        Line pad = quiet();
        judge_block(perfect.data(), E.M, E.N, E.M - 1, E.N - 1, [&](int m, int n) { return E.prod(m, n); }, pad, "C");
        if (caught(pad) != E.M + E.N - 1) host_fail(L, "a written last row and column: %.0f mismatches", (double)caught(pad));
        report("host judging (map, edges): one unit, swapped tiles, written padding are all reported", L);
    }
    {   // slabs: a slab over the neighbouring slices
        Line L;
        const Exact E = make_exact(64, 64, 7 * 64, 209, false);
        const auto S = slab_reference(E, 7, 3, 64), shifted = slab_reference(E, 7, 3, 64, 1);
        std::vector<float> perfect((size_t)3 * E.M * E.N);
        for (int s = 0; s < 3; ++s)
            for (int m = 0; m < E.M; ++m)
                for (int n = 0; n < E.N; ++n) perfect[((size_t)s * E.M + m) * E.N + n] = E.prod(S[s], m, n);
        Line ok, bad = quiet();
        judge_slabs(E, S, perfect.data(), E.M, E.N, ok);
        judge_slabs(E, shifted, perfect.data(), E.M, E.N, bad);
        std::vector<int64_t> whole;
        product(E, 0, E.K, whole);
        for (size_t i = 0; i < whole.size(); ++i)
            if (S[0][i] + S[1][i] + S[2][i] != whole[i]) { host_fail(L, "the slabs do not add up to the product"); break; }
        if (ok.bad || caught(bad) < (long)3 * E.M * E.N / 2) host_fail(L, "slabs over the neighbouring slices: %.0f mismatches", (double)caught(bad));
        report("host judging (slabs): slabs over slices shifted by one are reported; the slabs add up to the product", L);
    }
    {   // dw: one unit; and the guard
        Line L;
        DwProblem P = make_dw(5, 9, 70, 1, false);
        Line off = quiet();
        const float before = P.grad(3, 4);
        P.g[(size_t)3 * 10 + 4] += 1;
        judge_bits(f_bits(before), f_bits(P.grad(3, 4)), off, "gW", 3, 4);
        if (caught(off) != 1) host_fail(L, "a gradient off by one unit passes");
        std::vector<unsigned char> guard(GUARD * sizeof(float), 0xff);
        size_t at = 0;
        if (!guard_intact(guard.data(), guard.size(), &at)) host_fail(L, "an untouched guard is reported");
        guard[100] = 0xfe;
        if (guard_intact(guard.data(), guard.size(), &at) || at != 100) host_fail(L, "one written guard byte passes");
        report("host judging (dw, guards): one unit in a gradient and one written guard byte are reported", L);
    }
    host_refusals();
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    g_name_width = 118;
    omp_set_num_threads(std::min(16, omp_get_max_threads()));
    if (g_host) {
        if (argc > 1) { printf("usage: test_gemm_routes [--host | map | slabs | lse | edges | dw]\n"); return 2; }
        host_checks();
        return finish("GEMM ROUTES");
    }
    const struct { const char* name; void (*run)(); } sections[] = {{"map", section_map}, {"slabs", section_slabs}, {"lse", section_lse}, {"edges", section_edges}, {"dw", section_dw}};
    int ran = 0;
    for (const auto& s : sections)
        if (argc < 2 || !strcmp(argv[1], s.name)) { s.run(); free_all(); ++ran; }
    if (!ran || argc > 2) { printf("usage: test_gemm_routes [--host | map | slabs | lse | edges | dw]\n"); return 2; }
    {   // what the launchers refuse holds on the device as well (nothing is launched)
        Line L;
        RtxGemm g = {};
        static float buf[64];
        g.A = g.B = buf; g.C = buf; g.lda = g.ldb = g.ldc = 128; g.m_tiles = g.n_tiles = 1; g.k_slices = 11; g.splits = 5;
        if (!refused(rtx_gemm_dma_launch(g, RTX_EPI_STORE, 0), "empty split")) host_fail(L, "gemm_dma takes 11 slices in 5 splits");
        report("gemm_dma refuses 11 slices in 5 splits before any launch", L);
    }
    return finish((std::string("GEMM ROUTES") + (argc > 1 ? std::string(" ") + argv[1] : "")).c_str());
}
