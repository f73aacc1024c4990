// Native (no Python) check of loss.hip -- the kernels every backward pass starts with -- against plain float64 host code, one launcher
// at a time and on every route of rtx_launch_dlogits:
//   A  k_dlogits_row<5>: half-precision logits in place, one workgroup per row (S = 1) or two (S = 2), at its capacity limits
//   B  the chunked k_dlogits<bf16 | float>: half logits in place, float32 logits with and without the log-sum-exp partials
//   C  rtx_launch_bce_dlogits and rtx_launch_mse_dlogits, float32 and bf16 deltas
//   D  the dense loss functions, the loss sum, predict()'s -inf mask and the sigmoid of VAE_net's predict()
// Every output buffer is poisoned (all bits set: a NaN in every format used) before the launch, so an element nobody wrote is seen;
// the padding of D (rows >= B, columns >= I) and the row-loss partials a route declares zero are compared bit for bit.
// Each element is judged against ITS OWN scale (the bounds and where they come from: DESIGN.md section 6), and every line prints
// the worst error as a fraction of its bound.
//   test_loss          the device run
//   test_loss --host   no HIP call: the case generator and the float64 reference, checked against a second, independent formulation
//                      (a direct softmax in long double, a searched dense target image) and against the conditions the bounds assume
#include "../../rectorch_amd/csrc/rtx_kernels.h"

#include "check.h"

static const int B = 5, Bp = 8;       // real rows, padded rows of every case
static const float INV_B = 1.f / B;   // (an input of the kernels: the reference reads this float)
static const float BETA = 0.3f;
// the two bounds that were tightened to the measurements (derived: 4e-6 and 1e-5):
static const double LSE_TOL = 5e-7;    // |lse - lse64| <= LSE_TOL max(1, |lse64|): 4.6 x the worst measured (1.08e-7)
static const double SUM_TOL = 1e-6;    // a row loss / loss sum, of the sum of the absolute values of its terms: 8 x the worst (1.2e-7)

static uint16_t f2h(float f) { const _Float16 h = (_Float16)f; uint16_t b; memcpy(&b, &h, 2); return b; }
static double h2d(uint16_t b) { _Float16 h; memcpy(&h, &b, 2); return (double)(float)h; }
static double ulp32(double x) { return x == 0 ? 0 : ldexp(1.0, ilogb(x) - 23); }
static double ulp_bf16(double x) { return x == 0 ? 0 : ldexp(1.0, ilogb(x) - 7); }

// ---- the target: a CSR matrix and the batch rows taken from it ---------------------------------------------------------------------
enum { F_COL0 = 1, F_LAST = 2, F_SPLO = 4, F_SPHI = 8, F_PAD = 16, F_EXT = 32 };
struct RowSpec {
    int len;          // stored entries, the one in the padding included
    unsigned flags;   // columns the row must hold: 0, I - 1, the last column of workgroup 0 / the first of workgroup 1 of a shared
};                    // row, one index in [I, ldd) (ignored by every kernel), columns 3 and 5 (where C puts extreme logits)

struct Csr {
    std::vector<int64_t> indptr;
    std::vector<int32_t> idx;
    std::vector<float> val;
    std::vector<int32_t> ids;
    bool has_val = false, has_ids = false;
    int longest = 0;
    int64_t row(int b) const { return has_ids ? ids[b] : b; }
    float value(int64_t k) const { return has_val ? val[k] : 1.f; }
};

// the first column of the second workgroup of a row two workgroups share (16-byte groups [0, n8 / 2) and [n8 / 2, n8))
static int split_col(int ldd) { return ldd > 10240 ? (ldd / 8 / 2) * 8 : -1; }

static std::vector<int32_t> gen_row(int I, int ldd, RowSpec s, Rng& r)
{
    const int npad = ((s.flags & F_PAD) && ldd > I && s.len > 0) ? 1 : 0;
    const int real = std::min(s.len - npad, I);
    std::vector<int32_t> out;
    std::vector<char> used(I, 0);
    auto add = [&](int c) {
        if (c >= 0 && c < I && !used[c] && (int)out.size() < real) { used[c] = 1; out.push_back(c); }
    };
    if (s.flags & F_LAST) add(I - 1);
    if (s.flags & F_COL0) add(0);
    if (s.flags & F_SPLO) add(split_col(ldd) - 1);
    if (s.flags & F_SPHI) add(split_col(ldd));
    if (s.flags & F_EXT) { add(3); add(5); }
    std::vector<int32_t> rest;
    for (int c = 0; c < I; ++c) if (!used[c]) rest.push_back(c);
    for (int k = 0; (int)out.size() < real; ++k) {    // distinct columns: a partial shuffle
        std::swap(rest[k], rest[k + r.below((int)rest.size() - k)]);
        out.push_back(rest[k]);
    }
    std::sort(out.begin(), out.end());
    if (npad) out.push_back(I + (ldd - I) / 2);
    return out;
}

// val_kind 0: ratings 0.5 .. 5 in steps of 0.5;  1: the values 0, 1 and 0.5 (a stored zero included)
static Csr build_csr(int I, int ldd, const std::vector<RowSpec>& rows, bool has_val, int val_kind, bool has_ids, Rng& r)
{
    Csr c;
    c.has_val = has_val;
    c.has_ids = has_ids;
    c.indptr.push_back(0);
    for (const RowSpec& s : rows) {
        const std::vector<int32_t> row = gen_row(I, ldd, s, r);
        for (int32_t i : row) {
            c.idx.push_back(i);
            const int q = r.below(val_kind ? 3 : 10);
            if (has_val) c.val.push_back(val_kind ? (q == 0 ? 0.f : q == 1 ? 1.f : 0.5f) : 0.5f * (1 + q));
        }
        c.indptr.push_back((int64_t)c.idx.size());
        c.longest = std::max(c.longest, (int)row.size());
    }
    if (has_ids) c.ids = {4, 2, 4, 6, 0};     // permuted, row 4 twice; rows 1, 3 and 5 of the matrix are not in the batch
    return c;
}

static RtxCsrView dev_view(const Csr& c, int max_row_len)
{
    RtxCsrView v = {};
    v.indptr = to_dev(c.indptr);
    v.indices = to_dev(c.idx);
    v.values = c.has_val ? to_dev(c.val) : nullptr;
    v.row_ids = c.has_ids ? to_dev(c.ids) : nullptr;
    v.max_row_len = max_row_len;
    v.avg_row_len = std::max<int>(1, (int)(c.idx.size() / (c.indptr.size() - 1)));
    return v;
}

// dense image of batch row b by scatter (the reference) ...
static void dense_row(const Csr& c, int b, int I, std::vector<double>& t)
{
    std::fill(t.begin(), t.end(), 0.0);
    const int64_t u = c.row(b);
    for (int64_t k = c.indptr[u]; k < c.indptr[u + 1]; ++k)
        if (c.idx[k] < I) t[c.idx[k]] = c.value(k);
}
// ... and by looking every column up in the row's sorted entries (--host: the second formulation); also the generator's conditions
static int check_dense_image(const Csr& c, int b, int I, int ldd, const std::vector<double>& t)
{
    const int64_t u = c.row(b);
    std::vector<std::pair<int32_t, float>> e;
    for (int64_t k = c.indptr[u]; k < c.indptr[u + 1]; ++k) e.push_back({c.idx[k], c.value(k)});
    std::sort(e.begin(), e.end());
    int bad = 0;
    for (size_t k = 0; k < e.size(); ++k) {
        if (e[k].first < 0 || e[k].first >= ldd) ++bad;           // an index outside the padded row
        if (k && e[k].first == e[k - 1].first) ++bad;             // a duplicate
    }
    if ((int)e.size() > c.longest) ++bad;
    for (int i = 0; i < I; ++i) {
        auto it = std::lower_bound(e.begin(), e.end(), std::make_pair((int32_t)i, -INFINITY));
        const double want = (it != e.end() && it->first == i) ? (double)it->second : 0.0;
        if (want != t[i]) ++bad;
    }
    return bad;
}

// ---- judging ------------------------------------------------------------------------------------------------------------------------
// the three ratios of a line (worst error / bound of D, of the log-sum-exp, of the loss); a failure that belongs to no ratio (a padding
// element, a partial that must be exact, a --host condition) is counted with D
struct Worst {
    Line d, lse, loss;
    long bad() const { return d.bad + lse.bad + loss.bad; }
};
static double kl_terms(const std::vector<float>& mu, const std::vector<float>& lv, int b, int Z, double* abs_sum)
{
    double kl = 0, a = 0;
    for (int j = 0; j < Z; ++j) {
        const double m = mu[(size_t)b * Z + j], l = lv[(size_t)b * Z + j];
        kl += 1.0 + l - m * m - exp(l);
        a += 1.0 + fabs(l) + m * m + exp(l);
    }
    *abs_sum = 0.5 * a;
    return -0.5 * kl;
}
static void gen_latent(int Z, Rng& r, std::vector<float>& mu, std::vector<float>& lv)
{
    mu.resize((size_t)B * Z);
    lv.resize((size_t)B * Z);
    for (auto& x : mu) x = r.f();
    for (auto& x : lv) x = r.f();
}
static void report(const std::string& name, const char* route, const Worst& w, const char* extra = "")
{
    printf("%-46s %-34s D %.3f  lse %.3f  loss %.3f of bound  bad=%ld%s  %s\n", name.c_str(), route, w.d.worst, w.lse.worst, w.loss.worst, w.bad(), extra,
           w.bad() ? "FAIL" : "ok");
    ++g_cases;
    if (w.bad()) ++g_failed;
}

// =====================================================================================================================================
// A, B: the multinomial likelihood
// =====================================================================================================================================
struct MCase {
    std::string name;
    int I, ldd, ldy;          // ldy: leading dimension of the float32 logits (the half logits live in D: ldd)
    int Z;
    bool half_inplace, use_part, bf16_out;
    bool mrl_zero;            // the view says max_row_len == 0 (a densified batch)
    bool has_val, has_ids;
    std::vector<RowSpec> rows;
    int extra_strips;         // further strips of partials behind the padded row, all (-inf, 0)
    uint32_t seed;
};
struct MInput {
    std::vector<float> Yf;            // [B][ldy]; columns >= I are NaN
    std::vector<uint16_t> img;        // half in place: [Bp][ldd], all bits set except the real logits
    std::vector<float2> part;         // [B][part_ld]
    int n_strips = 0, part_ld = 0;
    Csr t;
    std::vector<float> tsum, mu, lv;
};
struct MRef {
    std::vector<double> D, T, SP;     // [B][I]: d loss / d logit, the dense target, s_b p_i
    std::vector<double> lse, loss, loss_abs;
};

static void gen_logit_row(float* y, int I, int kind, Rng& r)
{
    for (int i = 0; i < I; ++i) y[i] = kind == 1 ? 1.25f : (kind == 2 ? 30.f : 3.f) * r.f();
    if (kind == 2) { y[I / 3] = 30.f; y[2 * I / 3] = -30.f; }     // a spread of 60
    if (kind == 3) y[I / 2] = 65504.f;                            // the largest half
}

static MInput gen_mult(const MCase& c)
{
    Rng r = {c.seed};
    MInput in;
    in.t = build_csr(c.I, c.ldd, c.rows, c.has_val, 0, c.has_ids, r);
    in.Yf.assign((size_t)B * c.ldy, NAN);
    static const int kinds[B] = {0, 1, 2, 3, 0};      // plain, constant, spread of 60, holds +65504, plain
    for (int b = 0; b < B; ++b) gen_logit_row(&in.Yf[(size_t)b * c.ldy], c.I, kinds[b], r);
    if (c.half_inplace) {
        in.img.assign((size_t)Bp * c.ldd, 0xffff);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < c.I; ++i) in.img[(size_t)b * c.ldd + i] = f2h(in.Yf[(size_t)b * c.ldy + i]);
    }
    if (c.use_part) {     // what the logits product leaves: (max, sum exp(y - max)) of every 64-column strip of the float32 logits
        in.n_strips = (c.ldd + 63) / 64 + c.extra_strips;
        in.part_ld = in.n_strips + 1;
        in.part.assign((size_t)B * in.part_ld, make_float2(NAN, NAN));
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < in.n_strips; ++k) {
                const int lo = 64 * k, hi = std::min(c.I, lo + 64);
                double m = -INFINITY, s = 0;
                for (int i = lo; i < hi; ++i) m = std::max(m, (double)in.Yf[(size_t)b * c.ldy + i]);
                for (int i = lo; i < hi; ++i) s += exp((double)in.Yf[(size_t)b * c.ldy + i] - m);
                in.part[(size_t)b * in.part_ld + k] = make_float2((float)m, (float)s);
            }
    }
    in.tsum.resize(B);
    for (int b = 0; b < B; ++b) {     // the row's value sum over the item columns, as the gather kernel forms it
        const int64_t u = in.t.row(b);
        double s = 0;
        for (int64_t k = in.t.indptr[u]; k < in.t.indptr[u + 1]; ++k)
            if (in.t.idx[k] < c.I) s += in.t.value(k);
        in.tsum[b] = (float)s;
    }
    gen_latent(c.Z, r, in.mu, in.lv);
    return in;
}

static double logit(const MCase& c, const MInput& in, int b, int i)
{
    return c.half_inplace ? h2d(in.img[(size_t)b * c.ldd + i]) : (double)in.Yf[(size_t)b * c.ldy + i];
}

static MRef ref_mult(const MCase& c, const MInput& in)
{
    MRef R;
    const int I = c.I;
    R.D.assign((size_t)B * I, 0);
    R.T.assign((size_t)B * I, 0);
    R.SP.assign((size_t)B * I, 0);
    R.lse.resize(B); R.loss.resize(B); R.loss_abs.resize(B);
    const double inv = INV_B;
    std::vector<double> t(I);
    for (int b = 0; b < B; ++b) {
        double M = -INFINITY, S = 0;
        if (c.use_part) {     // the partials define the log-sum-exp
            for (int k = 0; k < in.n_strips; ++k) M = std::max(M, (double)in.part[(size_t)b * in.part_ld + k].x);
            for (int k = 0; k < in.n_strips; ++k) {
                const float2 p = in.part[(size_t)b * in.part_ld + k];
                if (p.x != -INFINITY) S += (double)p.y * exp((double)p.x - M);
            }
        } else {
            for (int i = 0; i < I; ++i) M = std::max(M, (double)in.Yf[(size_t)b * c.ldy + i]);
            for (int i = 0; i < I; ++i) S += exp((double)in.Yf[(size_t)b * c.ldy + i] - M);
        }
        const double lse = M + log(S), s = in.tsum[b];
        R.lse[b] = lse;
        dense_row(in.t, b, I, t);
        double dot = 0, dot_abs = 0;
        for (int i = 0; i < I; ++i) {
            const double y = logit(c, in, b, i), sp = s * exp(y - lse);
            R.SP[(size_t)b * I + i] = sp;
            R.T[(size_t)b * I + i] = t[i];
            R.D[(size_t)b * I + i] = (sp - t[i]) * inv;
            dot += t[i] * y;
            dot_abs += fabs(t[i] * y);
        }
        double kl_abs = 0;
        const double kl = c.Z ? kl_terms(in.mu, in.lv, b, c.Z, &kl_abs) : 0.0;
        R.loss[b] = (s * lse - dot) * inv + BETA * kl * inv;
        R.loss_abs[b] = (fabs(s * lse) + dot_abs) * inv + BETA * kl_abs * inv;
    }
    return R;
}

// --host: the reference against a direct softmax in long double over the searched dense image, and the conditions of the bounds
static long host_check_mult(const MCase& c, const MInput& in, const MRef& R)
{
    long bad = 0;
    const int I = c.I;
    std::vector<double> t(I);
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < I; ++i) t[i] = R.T[(size_t)b * I + i];
        bad += check_dense_image(in.t, b, I, c.ldd, t);
        long double mx = -INFINITY, mn = INFINITY, sum = 0;
        for (int i = 0; i < I; ++i) {
            const long double y = in.Yf[(size_t)b * c.ldy + i];
            mx = std::max(mx, y); mn = std::min(mn, y);
        }
        for (int i = 0; i < I; ++i) sum += expl((long double)in.Yf[(size_t)b * c.ldy + i] - mx);
        const long double direct = mx + logl(sum);
        // partials rounded to float: a relative 2^-24 of each strip's sum, so 2^-24 in the log-sum-exp (and exact without partials)
        if (!(fabsl(direct - (long double)R.lse[b]) <= (c.use_part ? 2e-7L : 1e-12L) * std::max(1.0L, fabsl(direct)))) {
            printf("    lse[%d] = %.17g, direct %.17Lg\n", b, R.lse[b], direct); ++bad;
        }
        if (mx < 65504.0L && mx - mn > 60.0L) { printf("    row %d: spread %.3Lg > 60\n", b, mx - mn); ++bad; }
        long double psum = 0, dsum = 0, tsum = 0;
        for (int i = 0; i < I; ++i) {
            const long double lse = c.use_part ? (long double)R.lse[b] : direct;
            const long double p = expl((long double)logit(c, in, b, i) - lse);
            const long double d = ((long double)in.tsum[b] * p - (long double)t[i]) * (long double)INV_B;
            if (!(fabsl(d - (long double)R.D[(size_t)b * I + i]) <= 1e-12L * ((long double)in.tsum[b] * p + (long double)t[i]) + 1e-300L)) ++bad;
            if (!std::isfinite(R.D[(size_t)b * I + i])) ++bad;
            psum += p; dsum += d; tsum += t[i];
        }
        // softmax of the float32 logits sums to one (the half logits differ from them by a relative 2^-11 at most: p by 65504 * 2^-11
        // at the very worst, which only the row that holds 65504 could reach, and there p is 0 or 1)
        if (!c.half_inplace && fabsl(psum - 1.0L) > 1e-6L) { printf("    row %d: probabilities sum to %.9Lg\n", b, psum); ++bad; }
        if (fabsl(tsum - (long double)in.tsum[b]) > 1e-6L * std::max(1.0L, tsum)) { printf("    row %d: tsum\n", b); ++bad; }
        if (!std::isfinite(R.loss[b]) || !std::isfinite(R.lse[b])) ++bad;
    }
    return bad;
}

static const char* route_of(const MCase& c, int mrl, int* S)
{
    const int chunks = (c.ldd + RTX_GATHER_CHUNK - 1) / RTX_GATHER_CHUNK;
    *S = 0;
    if (c.bf16_out && c.half_inplace && c.use_part && c.ldd <= 20480 && mrl > 0 && mrl <= 4096) {
        *S = std::min(chunks, (c.ldd + 10239) / 10240);
        return *S == 1 ? "row kernel, S = 1" : "row kernel, S = 2";
    }
    if (c.half_inplace) return "chunked, half logits in place";
    if (c.bf16_out) return c.use_part ? "chunked bf16, f32 logits, partials" : "chunked bf16, f32 logits, k_row_lse";
    return c.use_part ? "chunked f32, partials" : "chunked f32, k_row_lse";
}

// runs one case; `image` receives the raw D image (bf16 cases) for the A / B comparison
static void run_mult(const MCase& c, std::vector<uint16_t>* image = nullptr)
{
    const MInput in = gen_mult(c);
    const MRef R = ref_mult(c, in);
    const int I = c.I, ldd = c.ldd, chunks = (ldd + RTX_GATHER_CHUNK - 1) / RTX_GATHER_CHUNK;
    const int mrl = c.mrl_zero ? 0 : in.t.longest;
    int S;
    const char* route = route_of(c, mrl, &S);
    Worst w;
    char extra[96];
    snprintf(extra, sizeof extra, "  [I=%d ldd=%d Z=%d longest=%d strips=%d]", I, ldd, c.Z, in.t.longest, in.n_strips);
    if (g_host) {
        w.d.bad = host_check_mult(c, in, R);
        report(c.name, route, w, extra);
        return;
    }
    RtxDlogitsArgs a = {};
    a.loss.Y = c.half_inplace ? nullptr : to_dev(in.Yf);
    a.loss.ldy = c.half_inplace ? ldd : c.ldy;
    a.loss.B = B; a.loss.I = I;
    a.loss.part = c.use_part ? to_dev(in.part) : nullptr;
    a.loss.n_strips = in.n_strips; a.loss.part_ld = in.part_ld;
    a.loss.target = dev_view(in.t, mrl);
    a.loss.tsum = to_dev(in.tsum);
    a.loss.lse = dev_poison<float>(Bp);
    a.loss.row_loss = dev_poison<float>((size_t)Bp * chunks);
    a.loss.inv_batch = INV_B;
    a.loss.mu32 = c.Z ? to_dev(in.mu) : nullptr;
    a.loss.lv32 = c.Z ? to_dev(in.lv) : nullptr;
    a.loss.Z = c.Z; a.loss.beta = BETA;
    a.Bp = Bp; a.ldd = ldd;
    if (c.half_inplace) { a.D = to_dev(in.img); a.Y16 = a.D; }
    else a.D = c.bf16_out ? (void*)dev_poison<uint16_t>((size_t)Bp * ldd) : (void*)dev_poison<float>((size_t)Bp * ldd);
    RT(rtx_launch_dlogits(a, c.bf16_out ? 1 : 0, 0));
    CK(hipDeviceSynchronize());

    std::vector<uint16_t> d16;
    std::vector<float> d32;
    if (c.bf16_out) d16 = to_host((const uint16_t*)a.D, (size_t)Bp * ldd);
    else d32 = to_host((const float*)a.D, (size_t)Bp * ldd);
    const std::vector<float> lse = to_host(a.loss.lse, Bp), rl = to_host(a.loss.row_loss, (size_t)Bp * chunks);
    for (int b = 0; b < Bp; ++b)
        for (int i = 0; i < ldd; ++i) {
            const size_t at = (size_t)b * ldd + i;
            if (b >= B || i >= I) {
                judge_bits(c.bf16_out ? d16[at] : f_bits(d32[at]), 0, w.d, "pad D", b, i);
                continue;
            }
            const double want = R.D[(size_t)b * I + i];
            double bound = 2e-5 * (R.SP[(size_t)b * I + i] + R.T[(size_t)b * I + i]) / B;
            if (c.bf16_out) bound += fabs(want) / 256.0;
            judge(c.bf16_out ? (double)bf16_to_f32(d16[at]) : (double)d32[at], want, bound, w.d, "D", b, i);
        }
    for (int b = 0; b < B; ++b) {
        judge(lse[b], R.lse[b], LSE_TOL * std::max(1.0, fabs(R.lse[b])), w.lse, "lse", b, 0);
        double sum = 0;
        for (int k = 0; k < chunks; ++k) {
            sum += rl[(size_t)b * chunks + k];
            if (S && k >= S) judge_bits(f_bits(rl[(size_t)b * chunks + k]), 0, w.d, "row-loss partial", b, k);
        }
        judge(sum, R.loss[b], SUM_TOL * R.loss_abs[b], w.loss, "row loss", b, 0);
    }
    report(c.name, route, w, extra);
    if (image) *image = d16;
    free_all();
}

static void multinomial_cases()
{
    const RowSpec U = {40, 0};     // rows of the matrix that the batch does not take
    // A: the shapes of the row kernel, each run again as a densified batch (max_row_len == 0: the chunked kernel on identical inputs)
    std::vector<MCase> A;
    A.push_back({"A 5/8 every load clamped", 5, 8, 8, 0, true, true, true, false, false, false,
                 {{0, 0}, {1, F_LAST}, {6, F_COL0 | F_LAST | F_PAD}, {2, F_COL0 | F_LAST}, {3, 0}}, 0, 11});
    A.push_back({"A 1000/1024 one chunk, ratings, row_ids", 1000, 1024, 1024, 3, true, true, true, false, true, true,
                 {{256, F_COL0 | F_LAST}, U, {257, F_PAD | F_LAST}, U, {1, F_COL0}, U, {0, 0}}, 0, 12});
    A.push_back({"A 4100/4224 lane zeroes partial 1", 4100, 4224, 4224, 256, true, true, true, false, false, false,
                 {{4096, F_COL0 | F_LAST}, {1, F_LAST}, {257, F_PAD}, {0, 0}, {256, F_LAST}}, 1, 13});
    A.push_back({"A 10233/10240 S=1 at capacity, ratings", 10233, 10240, 10240, 257, true, true, true, false, true, false,
                 {{4096, F_COL0 | F_LAST | F_PAD}, {256, F_PAD}, {0, 0}, {1, F_COL0}, {257, F_LAST}}, 0, 14});
    A.push_back({"A 10241/10248 S=2 split 640+641, row_ids", 10241, 10248, 10248, 600, true, true, true, false, false, true,
                 {{257, F_SPLO | F_SPHI | F_LAST}, U, {4096, F_COL0 | F_LAST | F_SPLO | F_SPHI | F_PAD}, U, {1, F_SPHI}, U, {1, F_SPLO}}, 0, 15});
    A.push_back({"A 20479/20480 both workgroups full, ratings", 20479, 20480, 20480, 3, true, true, true, false, true, false,
                 {{4096, F_COL0 | F_LAST | F_SPLO | F_SPHI | F_PAD}, {257, F_SPLO | F_SPHI}, {1, F_SPHI}, {1, F_SPLO}, {0, 0}}, 0, 16});
    for (const MCase& c : A) {
        std::vector<uint16_t> row_img, chunk_img;
        run_mult(c, &row_img);
        MCase d = c;
        d.name = "B" + c.name.substr(1) + " (max_row_len 0)";
        d.mrl_zero = true;
        run_mult(d, &chunk_img);
        if (!g_host) {
            size_t differ = 0;
            for (size_t k = 0; k < row_img.size(); ++k) differ += row_img[k] != chunk_img[k];
            if (differ) printf("    row kernel vs chunked kernel, same inputs: %zu of %zu elements of D differ\n", differ, row_img.size());
            else printf("    row kernel vs chunked kernel, same inputs: D bit-identical\n");
        }
    }
    // B: what only the chunked kernel takes
    run_mult({"B 4100/4224 a row of 4097 entries", 4100, 4224, 4224, 3, true, true, true, false, false, false,
              {{4097, F_COL0 | F_LAST}, {1, F_LAST}, {257, F_PAD}, {0, 0}, {256, 0}}, 0, 21});
    run_mult({"B 20485/20488 wider than the row kernel", 20485, 20488, 20488, 257, true, true, true, false, true, true,
              {{300, F_COL0 | F_LAST | F_PAD}, U, {257, F_LAST}, U, {1, F_LAST}, U, {0, 0}}, 0, 22});
    struct Shape { const char* what; int I, ldd, ldy; };
    const Shape shapes[] = {{"5/8", 5, 8, 8}, {"1000/1024", 1000, 1024, 1024}, {"4097/4104 ldy 4100", 4097, 4104, 4100}, {"4100/4224", 4100, 4224, 4224}};
    uint32_t seed = 30;
    for (const Shape& s : shapes)
        for (int v = 0; v < 4; ++v) {
            const bool bf16 = v < 2, part = v & 1;
            const bool val = (v == 1 || v == 2), ids = (v == 0 || v == 3);
            std::vector<RowSpec> rows;
            const int big = std::min(s.I, 300);
            if (ids) rows = {{big, F_COL0 | F_LAST | F_PAD}, U, {std::min(s.I, 257), F_LAST}, U, {1, F_COL0}, U, {0, 0}};
            else rows = {{big, F_COL0 | F_LAST | F_PAD}, {1, F_LAST}, {0, 0}, {std::min(s.I, 256), 0}, {2, F_COL0 | F_LAST}};
            if (s.I < 40) for (auto& q : rows) q.len = std::min(q.len, s.I);
            run_mult({std::string("B f32 logits ") + s.what, s.I, s.ldd, s.ldy, v == 0 ? 0 : v == 1 ? 3 : v == 2 ? 256 : 600, false, part, bf16,
                      (v & 2) != 0, val, ids, rows, 0, ++seed});
        }
}

// =====================================================================================================================================
// C: binary cross-entropy on the sigmoid (VAE_net) and the mean squared error (AETrainer), one chunked kernel each
// =====================================================================================================================================
struct ECase {
    std::string name;
    bool bce;
    int I, ldd, ldy, Z;
    bool bf16_out, has_val, has_ids;
    std::vector<RowSpec> rows;
    uint32_t seed;
};

static bool extreme(float y) { return fabsf(y) >= 18.f; }

static void run_elem(const ECase& c)
{
    Rng r = {c.seed};
    const int I = c.I, ldd = c.ldd, ldy = c.ldy, chunks = (ldd + RTX_GATHER_CHUNK - 1) / RTX_GATHER_CHUNK;
    const Csr t = build_csr(I, ldd, c.rows, c.has_val, 1, c.has_ids, r);
    std::vector<float> Y((size_t)B * ldy, NAN), mu, lv;
    static const float ext[3] = {20.f, 90.f, -90.f};
    for (int b = 0; b < B; ++b) {
        float* y = &Y[(size_t)b * ldy];
        for (int i = 0; i < I; ++i) y[i] = (c.bce ? 10.f : 3.f) * r.f();
        if (c.bce && b == B - 1) for (int i = 0; i < I; ++i) y[i] = ext[i % 3];     // a row of extreme logits only: an exact loss
        else if (c.bce) for (int k = 0; k < 3 && k < I; ++k) { y[(3 + k) % I] = ext[k]; y[I - 1 - k] = ext[(k + b) % 3]; }
    }
    gen_latent(c.bce ? c.Z : 0, r, mu, lv);
    const int Z = c.bce ? c.Z : 0;
    const float inv_elems = 1.f / ((float)B * (float)I);
    const double inv = inv_elems;

    // float64 reference: D [B][I] with its bound, and per (row, chunk) the loss partial with its bound
    std::vector<double> D((size_t)B * I), Dbound((size_t)B * I), part((size_t)B * chunks, 0), pbound((size_t)B * chunks, 0), tt(I);
    std::vector<char> exact((size_t)B * chunks, 1);
    std::vector<double> raw((size_t)B * chunks, 0);      // the plain sum of the element losses (exact where `exact`)
    long host_bad = 0;
    for (int b = 0; b < B; ++b) {
        dense_row(t, b, I, tt);
        if (g_host) host_bad += check_dense_image(t, b, I, ldd, tt);
        for (int i = 0; i < I; ++i) {
            const float yf = Y[(size_t)b * ldy + i];
            const double y = yf, x = tt[i];
            const int k = i / RTX_GATHER_CHUNK;
            double term, tb, d, db;
            if (c.bce) {
                if (g_host && !(fabs(y) <= 10.0 || yf == 20.f || yf == 90.f || yf == -90.f)) ++host_bad;
                if (g_host && !(x == 0 || x == 1 || x == 0.5)) ++host_bad;
                if (extreme(yf)) {    // float32 p is exactly 1 (or 0): the -100 clamp of the logarithm, a zero gradient
                    term = y > 0 ? 100.0 * (1.0 - x) : 100.0 * x;
                    tb = 1e-6 * fabs(term);
                    d = 0; db = 0;
                } else {
                    const double p = 1.0 / (1.0 + exp(-y));
                    term = -(x * log(p) + (1.0 - x) * log1p(-p));
                    tb = 4 * E24 * (1.0 / (1.0 - p) + x / p) + 1e-6 * fabs(term);
                    d = (p - x) * inv;
                    // p to 3 float32 ulps (expf, an addition, a division), then one subtraction, one division and two products on
                    // p - x: (3 p + 4 |p - x|) 2^-24 <= 8 (p + x) 2^-24
                    db = 8 * E24 * (p + x) * inv;
                    exact[(size_t)b * chunks + k] = 0;
                }
            } else {
                const double e = y - x;
                term = e * e;
                tb = SUM_TOL * term;
                d = 2.0 * inv * e;
                db = 4 * ulp32(d);
                exact[(size_t)b * chunks + k] = 0;
            }
            if (c.bf16_out) db = c.bce ? db + fabs(d) / 256.0 : std::max(db, ulp_bf16(d));
            D[(size_t)b * I + i] = d; Dbound[(size_t)b * I + i] = db;
            part[(size_t)b * chunks + k] += term * inv;
            raw[(size_t)b * chunks + k] += term;
            pbound[(size_t)b * chunks + k] += tb * inv;
            if (g_host && (!std::isfinite(term) || !std::isfinite(d))) ++host_bad;
        }
        if (Z) {
            double kl_abs;
            part[(size_t)b * chunks] += BETA * kl_terms(mu, lv, b, Z, &kl_abs) * INV_B;
            pbound[(size_t)b * chunks] += SUM_TOL * BETA * kl_abs * INV_B;
            exact[(size_t)b * chunks] = 0;
        }
    }
    Worst w;
    char extra[64];
    snprintf(extra, sizeof extra, "  [I=%d ldd=%d ldy=%d Z=%d]", I, ldd, ldy, Z);
    const char* route = c.bce ? (c.bf16_out ? "k_elem_dlogits<bf16, BceKlLoss>" : "k_elem_dlogits<float, BceKlLoss>")
                              : (c.bf16_out ? "k_elem_dlogits<bf16, MseLoss>" : "k_elem_dlogits<float, MseLoss>");
    if (g_host) { w.d.bad = host_bad; report(c.name, route, w, extra); return; }

    RtxDlogitsArgs a = {};
    a.loss.Y = to_dev(Y); a.loss.ldy = ldy; a.loss.B = B; a.loss.I = I;
    a.loss.target = dev_view(t, t.longest);
    a.loss.lse = dev_poison<float>(Bp);
    a.loss.row_loss = dev_poison<float>((size_t)Bp * chunks);
    a.loss.inv_batch = INV_B;
    a.loss.mu32 = Z ? to_dev(mu) : nullptr; a.loss.lv32 = Z ? to_dev(lv) : nullptr; a.loss.Z = Z; a.loss.beta = BETA;
    a.Bp = Bp; a.ldd = ldd;
    a.D = c.bf16_out ? (void*)dev_poison<uint16_t>((size_t)Bp * ldd) : (void*)dev_poison<float>((size_t)Bp * ldd);
    if (c.bce) RT(rtx_launch_bce_dlogits(a, inv_elems, c.bf16_out ? 1 : 0, 0));
    else RT(rtx_launch_mse_dlogits(a, inv_elems, c.bf16_out ? 1 : 0, 0));
    CK(hipDeviceSynchronize());
    std::vector<uint16_t> d16;
    std::vector<float> d32;
    if (c.bf16_out) d16 = to_host((const uint16_t*)a.D, (size_t)Bp * ldd);
    else d32 = to_host((const float*)a.D, (size_t)Bp * ldd);
    const std::vector<float> rl = to_host(a.loss.row_loss, (size_t)Bp * chunks);
    for (int b = 0; b < Bp; ++b)
        for (int i = 0; i < ldd; ++i) {
            const size_t at = (size_t)b * ldd + i;
            if (b >= B || i >= I) { judge_bits(c.bf16_out ? d16[at] : f_bits(d32[at]), 0, w.d, "pad D", b, i); continue; }
            const double got = c.bf16_out ? (double)bf16_to_f32(d16[at]) : (double)d32[at];
            judge(got, D[(size_t)b * I + i], Dbound[(size_t)b * I + i], w.d, "D", b, i);
        }
    for (int b = 0; b < B; ++b) {
        double sum = 0, want = 0, bound = 0;
        for (int k = 0; k < chunks; ++k) {
            const size_t at = (size_t)b * chunks + k;
            sum += rl[at]; want += part[at]; bound += pbound[at];
            if (exact[at]) {      // extreme logits only: multiples of 50 summed in float32, one product with inv_elems
                const float e = (float)raw[at] * inv_elems;
                if (!(rl[at] == e)) { if (w.d.bad < 4) printf("    exact partial[%d][%d] = %.9g, expected %.9g\n", b, k, rl[at], e); ++w.d.bad; }
            }
        }
        judge(sum, want, bound, w.loss, "row loss", b, 0);
    }
    report(c.name, route, w, extra);
    free_all();
}

static void elementwise_cases()
{
    const RowSpec U = {3, 0};
    struct Shape { const char* what; int I, ldd, ldy; };
    const Shape shapes[] = {{"5/8", 5, 8, 8}, {"4095/4096", 4095, 4096, 4096}, {"4097/4104 ldy 4100", 4097, 4104, 4100}};
    uint32_t seed = 50;
    for (int bce = 1; bce >= 0; --bce)
        for (const Shape& s : shapes)
            for (int bf16 = 0; bf16 < 2; ++bf16) {
                const bool val = bf16 == 0, ids = (s.I == 4095) == (bf16 == 1);
                const int big = std::min(s.I, 300), two = std::min(s.I, 257);
                std::vector<RowSpec> rows;
                if (ids) rows = {{big, F_COL0 | F_LAST | F_EXT | F_PAD}, U, {two, F_LAST | F_EXT}, U, {std::min(s.I, 40), F_COL0 | F_EXT}, U, {0, 0}};
                else rows = {{big, F_COL0 | F_LAST | F_EXT | F_PAD}, {1, F_LAST}, {0, 0}, {two, F_EXT}, {std::min(s.I, 40), F_COL0 | F_LAST | F_EXT}};
                run_elem({std::string(bce ? "C bce " : "C mse ") + s.what + (val ? ", values 0 / 1 / 0.5" : ", values NULL") + (ids ? ", row_ids" : ""),
                          bce != 0, s.I, s.ldd, s.ldy, bf16 ? (s.I == 5 ? 3 : 257) : 0, bf16 != 0, val, ids, rows, ++seed});
            }
}

// =====================================================================================================================================
// D: the smaller launchers
// =====================================================================================================================================
static void dense_cases()
{
    const int Is[] = {7, 257, 4099};
    uint32_t seed = 70;
    for (int kind = 0; kind < 3; ++kind)          // 0: rtx_launch_dense_loss, 1: rtx_launch_dense_bce_kl, 2: rtx_launch_dense_mse
        for (int I : Is)
            for (int with_kl = 0; with_kl < 2; ++with_kl) {
                if (kind == 2 && with_kl) continue;
                Rng r = {++seed};
                const int Z = with_kl ? (I == 257 ? 257 : 20) : 0;
                std::vector<float> Y((size_t)B * I), X((size_t)B * I), mu, lv;
                static const int kinds[B] = {0, 1, 2, 3, 0};
                for (int b = 0; b < B; ++b)
                    for (int i = 0; i < I; ++i) {
                        const int q = r.below(8);
                        X[(size_t)b * I + i] = b == 1 ? 0.f : q == 0 ? 1.f : q == 1 ? 0.5f : q == 2 ? 2.f : 0.f;     // (row 1: an empty row)
                    }
                for (int b = 0; b < B; ++b) {
                    float* y = &Y[(size_t)b * I];
                    if (kind == 0) gen_logit_row(y, I, kinds[b], r);
                    else if (kind == 2) for (int i = 0; i < I; ++i) y[i] = 3.f * r.f();
                    else for (int i = 0; i < I; ++i) {      // probabilities, the ends of the interval included (the -100 clamp)
                        const int q = r.below(16);
                        y[i] = q == 0 ? 0.f : q == 1 ? 1.f : 1e-4f + (1.f - 2e-4f) * (0.5f + 0.5f * r.f());
                        if (kind == 1 && X[(size_t)b * I + i] == 2.f) X[(size_t)b * I + i] = 1.f;
                    }
                }
                gen_latent(Z, r, mu, lv);
                const float inv_elems = 1.f / ((float)B * (float)I);
                std::vector<double> want(B), bound(B);
                long host_bad = 0;
                for (int b = 0; b < B; ++b) {
                    double sum = 0, abs_sum = 0, kl_abs = 0;
                    const double kl = Z ? kl_terms(mu, lv, b, Z, &kl_abs) : 0.0;
                    if (kind == 0) {
                        double M = -INFINITY, S = 0, sx = 0, dot = 0, dabs = 0;
                        for (int i = 0; i < I; ++i) M = std::max(M, (double)Y[(size_t)b * I + i]);
                        for (int i = 0; i < I; ++i) {
                            const double y = Y[(size_t)b * I + i], x = X[(size_t)b * I + i];
                            S += exp(y - M); sx += x; dot += x * y; dabs += fabs(x * y);
                        }
                        const double lse = M + log(S);
                        sum = (sx * lse - dot) * INV_B + BETA * kl * INV_B;
                        abs_sum = (fabs(sx * lse) + dabs) * INV_B + BETA * kl_abs * INV_B;
                    } else if (kind == 1) {
                        for (int i = 0; i < I; ++i) {
                            const double p = Y[(size_t)b * I + i], x = X[(size_t)b * I + i];
                            const double a = (x - 1.0) * std::max(log1p(-p), -100.0), c2 = x == 0 ? 0.0 : -x * std::max(log(p), -100.0);
                            sum += (a + c2) * inv_elems; abs_sum += (fabs(a) + fabs(c2)) * inv_elems;
                        }
                        sum += kl * INV_B; abs_sum += kl_abs * INV_B;       // (this loss function has no beta)
                    } else {
                        for (int i = 0; i < I; ++i) {
                            const double e = (double)X[(size_t)b * I + i] - (double)Y[(size_t)b * I + i];
                            sum += e * e * inv_elems;
                        }
                        abs_sum = sum;
                    }
                    want[b] = sum; bound[b] = SUM_TOL * abs_sum;
                    if (!std::isfinite(sum)) ++host_bad;
                }
                Worst w;
                char name[96];
                snprintf(name, sizeof name, "D %s I=%d%s", kind == 0 ? "dense_loss" : kind == 1 ? "dense_bce_kl" : "dense_mse", I, Z ? ", mu / lv" : "");
                const char* route = kind == 0 ? "k_dense_loss" : kind == 1 ? "k_dense_bce_kl" : "k_dense_mse";
                if (g_host) { w.d.bad = host_bad; report(name, route, w); continue; }
                const float *dY = to_dev(Y), *dX = to_dev(X), *dmu = Z ? to_dev(mu) : nullptr, *dlv = Z ? to_dev(lv) : nullptr;
                float* rl = dev_poison<float>(Bp);
                if (kind == 0) RT(rtx_launch_dense_loss(dY, dX, B, I, dmu, dlv, Z, BETA, INV_B, rl, 0));
                else if (kind == 1) RT(rtx_launch_dense_bce_kl(dY, dX, B, I, dmu, dlv, Z, inv_elems, INV_B, rl, 0));
                else RT(rtx_launch_dense_mse(dY, dX, B, I, inv_elems, rl, 0));
                CK(hipDeviceSynchronize());
                const std::vector<float> got = to_host(rl, Bp);
                for (int b = 0; b < B; ++b) judge(got[b], want[b], bound[b], w.loss, "row loss", b, 0);
                for (int b = B; b < Bp; ++b)
                    if (f_bits(got[b]) != 0xffffffffu) { printf("    row_loss[%d] was written\n", b); ++w.d.bad; }
                report(name, route, w);
                free_all();
            }
}

static void reduce_cases()
{
    const int ns[] = {1, 255, 256, 257, 2560};
    uint32_t seed = 90;
    for (int n : ns)
        for (int with_norms = 0; with_norms < 2; ++with_norms) {
            Rng r = {++seed};
            std::vector<float> rl(n), sumsq = {2.25f, 1e-3f, 777.f};
            for (auto& x : rl) x = 2.f + 3.f * r.f();
            const float lam = 0.1f, acc0 = 1.5f;
            double s = 0, a = 0;
            for (float x : rl) { s += x; a += fabs(x); }
            if (with_norms) for (float q : sumsq) { s += (double)lam * sqrt((double)q); a += (double)lam * sqrt((double)q); }
            Worst w;
            char name[96];
            snprintf(name, sizeof name, "D reduce_loss n=%d%s", n, with_norms ? ", lam 0.1 x 3 norms" : "");
            if (g_host) { w.d.bad = !std::isfinite(s); report(name, "k_reduce_loss", w); continue; }
            const float *drl = to_dev(rl), *dsq = to_dev(sumsq);
            float* out = dev_poison<float>(1);
            float* acc = to_dev(std::vector<float>{acc0});
            for (int call = 0; call < 2; ++call)
                RT(rtx_launch_reduce_loss(drl, n, lam, with_norms ? dsq : nullptr, with_norms ? 3 : 0, out, acc, 0));
            CK(hipDeviceSynchronize());
            judge(to_host(out, 1)[0], s, SUM_TOL * a, w.loss, "loss_out", 0, 0);
            judge(to_host(acc, 1)[0], acc0 + 2 * s, SUM_TOL * (acc0 + 2 * a), w.loss, "loss_accum", 0, 0);
            report(name, "k_reduce_loss", w);
            free_all();
        }
}

static void mask_cases()
{
    for (int variant = 0; variant < 2; ++variant) {
        Rng r = {100u + variant};
        const int n_items = 1500, ldd = 1536;
        const long ld = 1531;           // (rows of the logits need no alignment here)
        const bool ids = variant == 1;
        const RowSpec U = {9, 0};
        std::vector<RowSpec> rows;
        if (ids) rows = {{300, F_COL0 | F_LAST}, U, {257, F_LAST}, U, {40, F_COL0}, U, {0, 0}};
        else rows = {{300, F_COL0 | F_LAST}, {1, F_LAST}, {0, 0}, {257, 0}, {40, F_COL0 | F_LAST}};
        // condition columns behind the items: stored indices in [n_items, ld) that must stay
        Csr t = build_csr(n_items, ldd, rows, true, 1, ids, r);
        for (size_t rr = 0; rr + 1 < t.indptr.size(); ++rr)      // the last entry of every row becomes a condition column
            if (t.indptr[rr + 1] - t.indptr[rr] >= 2) { t.idx[t.indptr[rr + 1] - 1] = n_items + 7 + (int)rr; t.val[t.indptr[rr + 1] - 1] = 1.f; }
        std::vector<float> L((size_t)Bp * ld);
        for (auto& x : L) x = 5.f * r.f();
        std::vector<float> want = L;
        long zeros = 0, masked = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t u = t.row(b);
            for (int64_t k = t.indptr[u]; k < t.indptr[u + 1]; ++k) {
                if (t.val[k] == 0.f) ++zeros;
                if (t.val[k] != 0.f && t.idx[k] < n_items) { want[(size_t)b * ld + t.idx[k]] = -INFINITY; ++masked; }
            }
        }
        Worst w;
        const char* name = ids ? "D neg_inf stored zeros, condition columns, row_ids" : "D neg_inf stored zeros, condition columns";
        if (g_host) { w.d.bad = (zeros == 0) + (masked == 0); report(name, "k_neg_inf", w); continue; }
        float* dL = to_dev(L);
        RT(rtx_launch_neg_inf(dev_view(t, t.longest), B, dL, ld, n_items, 0));
        CK(hipDeviceSynchronize());
        const std::vector<float> got = to_host(dL, L.size());
        for (size_t k = 0; k < got.size(); ++k)
            if (f_bits(got[k]) != f_bits(want[k])) { if (w.d.bad < 4) printf("    logits[%zu][%zu] = %g, expected %g\n", k / ld, k % ld, got[k], want[k]); ++w.d.bad; }
        report(name, "k_neg_inf", w);
        free_all();
    }
    const int shapes[][2] = {{7, 12}, {1500, 1531}, {4099, 4104}, {20000, 20003}};      // n_items, ld: 1 .. 16 workgroups per row
    for (const auto& sh : shapes) {
        Rng r = {110u + (uint32_t)sh[0]};
        const int n_items = sh[0];
        const long ld = sh[1];
        std::vector<float> L((size_t)Bp * ld);
        for (auto& x : L) x = 10.f * r.f();
        for (int b = 0; b < B; ++b) { L[(size_t)b * ld] = 90.f; L[(size_t)b * ld + n_items - 1] = -90.f; L[(size_t)b * ld + n_items / 2] = 20.f; }
        Worst w;
        char name[96];
        snprintf(name, sizeof name, "D sigmoid_rows n_items=%d ld=%ld", n_items, ld);
        if (g_host) { report(name, "k_sigmoid_rows", w); continue; }
        float* dL = to_dev(L);
        RT(rtx_launch_sigmoid_rows(dL, B, ld, n_items, 0));
        CK(hipDeviceSynchronize());
        const std::vector<float> got = to_host(dL, L.size());
        for (int b = 0; b < Bp; ++b)
            for (int i = 0; i < ld; ++i) {
                const size_t at = (size_t)b * ld + i;
                if (b >= B || i >= n_items) {
                    if (f_bits(got[at]) != f_bits(L[at])) { if (w.d.bad < 4) printf("    logits[%d][%d] was touched\n", b, i); ++w.d.bad; }
                    continue;
                }
                const double p = 1.0 / (1.0 + exp(-(double)L[at]));
                // expf to 2 ulps, an addition, a division: 4 float32 ulps of p (and p == 1 / p == 0 exactly at +-90, where the bound is generous)
                judge(got[at], p, 4 * E24 * p + 1e-38, w.d, "p", b, i);
            }
        report(name, "k_sigmoid_rows", w);
        free_all();
    }
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    multinomial_cases();
    elementwise_cases();
    dense_cases();
    reduce_cases();
    mask_cases();
    return finish("LOSS");
}
