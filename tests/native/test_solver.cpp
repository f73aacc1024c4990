// Native (no Python) check of the float64 solver stack behind EASE and ADMM SLIM, one launcher at a time, against exact host references:
//   A  rtx_dgemm_launch (dgemm.hip), both tile sizes on the same problems: integer-valued operands in [-8, 8], K <= 640, so every partial
//      sum is exact in float64 in any order and the result is BIT FOR BIT the host sum over the tile's K range (no tolerance).  Every
//      (k_lo, k_hi) pair, lower_only on / off, (alpha, beta) in {(1, 0), (-1, 1), (-1, 0)}, CT null / not, k_slices 0 / 8 / 16 / 24, on
//      3x3, 2x5 and 5x2 128-tiles; the launches of ease_factor, of the float64 Gram matrix and of P = W^T W by name with the solver's
//      flags; one real-valued case per tile size against a long double product under (K + 2) 2^-53 sum |a||b| per element.
//   B  rtx_dgemm_admm_launch: the same integer operands (exact accumulator), real e_add / e_gamma / e_pdiag, rho dyadic and not; e_gamma,
//      e_mnext and CT BIT FOR BIT against the same expressions in the same order on the host without contraction.  All variants, e_n in
//      {384, 300, 257, 1} of np = 384, CT null, k_slices = 0 with a NaN A, the launcher's refusals.  Each case counts the three branches
//      of the soft threshold and asserts all occur (e_n = 1 has ONE element, the diagonal one: its three branches are spread over the
//      e_n = 1 cases, and asserted over them together).
//   C  rtx_syrk_lower_launch (syrk.hip), fp8 and bf16: integers |v| <= 4 encoded as the callers encode them (fp8 by the hardware
//      conversion in a kernel of this file); every element of the lower 256-tiles is bit for bit the integer Gram.  rows256 in {1, 2, 9}
//      (9 reaches the second patch row of the tile map), cols128 even and odd, k_slices 1 / 2 / 3.
//   D  rtx_gram_inverse (ease.hip) on every Gram route (binary, fp8, bf16, scaled fp8 by 4 and by 8, float64 for 0.3 steps and for
//      |v| > 256, the mx^2 U >= 2^24 switch on both sides), n in {129, 300, 520}, each with (want_G, bias, full_P) in
//      {(0, -, 0), (1, -, 1), (1, b, 1), (0, b, 0)}: G bit for bit the exact Gram + rank-1 term where the data are integers or dyadic,
//      under the derived summation bound on the 0.3 route, bitwise symmetric, zero in the pad; P against a long double Cholesky
//      inverse, within 10x the error of the same inverse in plain double on the host (the floor, printed per case); identity pad;
//      a not-positive-definite case.
//   E  rtx_dense_scores_launch against a long double loop under (row length + 2) 2^-53 sum |v||B|; the -inf pattern exactly.
// Every output is filled with NaNs (all bits set) before the launch and whatever a launch must leave alone is compared bit for bit with
// that poison; every operand region a launch must not read (outside a tile's K range, A with k_slices = 0, rows behind the declared
// tiles, row pads) holds NaNs too, which would surface in the result.
//
// The reference of A and B takes a tile's sum from prefix sums over 64-wide K blocks of a plain integer triple loop (all K ranges are
// multiples of 64); --host checks that table against a direct triple loop over explicitly zeroed operands.
//
// The floor of D.  max|P - P_ld| / max|P_ld| of the host's plain double inverse depends tenfold on the order in which the Cholesky
// factor's sums run once the rank-1 item-bias term (bias_scale b b^T, ~1e4 against a shift of 50) is in the matrix: subtracting the
// terms from A one after the other cancels the large term first and keeps every later rounding small, while accumulating the sum
// first and subtracting it from A -- the order of any blocked update A22 -= L21 L21^T, the device's included -- rounds every partial
// sum at the large term's scale.  Both are plain Cholesky factorisations, so the driver runs both and the floor is the larger error.
// Measured on the MI355X (device | term by term | sum first), worst over the routes:
//   no bias, n = 129 / 300 / 520:  1.6e-15 | 1.6e-15 | 1.3e-15,   2.4e-15 | 3.6e-15 | 3.1e-15,   4.3e-14 | 2.3e-14 | 4.2e-14
//   bias,    n = 129 / 300 / 520:  6.7e-14 | 1.3e-14 | 1.4e-13,   3.0e-13 | 1.4e-14 | 3.9e-13,   4.7e-13 | 1.6e-14 | 5.7e-13
//   (bf16 17..256 and |v| > 256, whose Gram entries reach 1e6..1e8 against the same shift: up to 1.4e-11 | 5.8e-12 | 1.2e-11 and
//   1.6e-10 | 9.1e-11 | 1.4e-10)
// The device stayed between 0.4x and 1.3x the sum-first error in every case (0.04 .. 0.16 of the 10x allowed); against the
// term-by-term error alone it reaches 29x with a bias (4.7e-13 against 1.6e-14, binary n = 520) and would fail there: LAPACK's
// blocked potrf measured 2.9e-13 on a matrix of the same kind (n = 300) where term by term gives 2.0e-14.
//
//   test_solver            the device run
//   test_solver --host     no HIP call: the long double Cholesky inverse against P (G + shift I) = I, the K-range reference against a dense
//                          product of zeroed operands, the epilogue reference against a second formulation, the launchers' refusals
//   test_solver --mutate N the device run with ONE reference deliberately wrong (1: k_lo TM and TN swapped, 2: no diagonal correction in the
//                          epilogue, 3: SYRK reference one K block short): must FAIL -- the check that the comparisons can fail
#include "../../rectorch_amd/csrc/rtx_dgemm.h"
#include "../../rectorch_amd/csrc/rtx_gemm.h"
#include "../../rectorch_amd/csrc/rtx_kernels.h"

#include "check.h"

#include <stdarg.h>
#include <cmath>

static int g_mutate = 0;

// this driver's line: [name] what -> ok; it counts failures only
static void report(const std::string& name, bool ok, const std::string& what)
{
    printf("[%s] %s -> %s\n", name.c_str(), what.c_str(), ok ? "ok" : "FAIL");
    if (!ok) ++g_failed;
}
static std::string fmt(const char* f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// =================================================================================================================================
// A / B: integer operands and the K-range reference
// =================================================================================================================================
static const int DMAX = 640;                        // rows of A0 / B0 and the largest K
static std::vector<int> g_A0, g_B0, g_C0;           // [DMAX][DMAX] each, integers in [-8, 8]

static void make_int_operands()
{
    Rng r{12345u};
    g_A0.resize((size_t)DMAX * DMAX); g_B0.resize(g_A0.size()); g_C0.resize(g_A0.size());
    for (auto& v : g_A0) v = r.i(-8, 8);
    for (auto& v : g_B0) v = r.i(-8, 8);
    for (auto& v : g_C0) v = r.i(-8, 8);
}

// pre[(kb * M + m) * N + n] = sum_{k < 64 kb} A[m][k] B[n][k], kb = 0 .. K / 64: a plain triple loop per 64-wide K block, in int32 (exact)
static std::vector<int> prefix_table(const int* A, const int* B, int M, int N, int K)
{
    const int nb = K / 64;
    std::vector<int> pre((size_t)(nb + 1) * M * N, 0);
    for (int kb = 0; kb < nb; ++kb)
#pragma omp parallel for
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) {
                const int* a = A + (size_t)m * DMAX + kb * 64;
                const int* b = B + (size_t)n * DMAX + kb * 64;
                int s = 0;
                for (int k = 0; k < 64; ++k) s += a[k] * b[k];
                pre[((size_t)(kb + 1) * M + m) * N + n] = pre[((size_t)kb * M + m) * N + n] + s;
            }
    return pre;
}

// the K range of tile (tm, tn) as rtx_dgemm.h states it: from tile * {0, tm, tn, max(tm, tn)} to tile * ({tm, tn} + 1), capped at K
static void k_range(int k_lo, int k_hi, int K, int tile, int tm, int tn, int* k0, int* k1)
{
    if (g_mutate == 1) { if (k_lo == RTX_DK_TM) k_lo = RTX_DK_TN; else if (k_lo == RTX_DK_TN) k_lo = RTX_DK_TM; }
    int lo = 0, hi = K;
    if (k_lo == RTX_DK_TM) lo = tile * tm;
    else if (k_lo == RTX_DK_TN) lo = tile * tn;
    else if (k_lo == RTX_DK_MAX) lo = tile * std::max(tm, tn);
    if (k_hi == RTX_DK_TM) hi = std::min(hi, tile * (tm + 1));
    else if (k_hi == RTX_DK_TN) hi = std::min(hi, tile * (tn + 1));
    *k0 = lo; *k1 = hi;   // empty when hi <= lo
}

struct DgProb {
    int Mt, Nt;        // 128-tiles
    int ks;            // K / 16
    int k_lo, k_hi, lower, small;
    bool same;         // B is A (the update, the Gram matrix, P)
};
struct DgDev {
    DgProb p;
    int M, N, K, tile;
    long lda, ldb, ldc, ldct;
    double *A, *B, *C, *CT;
    const std::vector<int>* pre;
};
static const char* kname(int k) { return k == RTX_DK_ALL ? "ALL" : k == RTX_DK_TM ? "TM" : k == RTX_DK_TN ? "TN" : "MAX"; }

// operand image [rows + 8][ld]: NaN everywhere but the 16-wide K slices that some tile of this row tile reads
static std::vector<double> operand_image(const std::vector<int>& src, int rows, long ld, int tile, const std::vector<char>& need, int slices)
{
    std::vector<double> h((size_t)(rows + 8) * ld, poison_f64());
    for (int m = 0; m < rows; ++m)
        for (int s = 0; s < slices; ++s)
            if (need[(size_t)(m / tile) * slices + s])
                for (int k = 16 * s; k < 16 * s + 16; ++k) h[(size_t)m * ld + k] = (double)src[(size_t)m * DMAX + k];
    return h;
}

static DgDev dg_prepare(const DgProb& p, const std::vector<int>& pre)
{
    DgDev d;
    d.p = p; d.pre = &pre;
    d.M = 128 * p.Mt; d.N = 128 * p.Nt; d.K = 16 * p.ks; d.tile = p.small ? 64 : 128;
    d.lda = 648; d.ldb = p.same ? 648 : 672; d.ldc = d.N + 24; d.ldct = d.M + 40;
    const int mt = d.M / d.tile, nt = d.N / d.tile, slices = DMAX / 16;
    std::vector<char> needA((size_t)std::max(mt, nt) * slices, 0), needB(needA.size(), 0);
    const int save = g_mutate;
    g_mutate = 0;   // the operand image follows the true ranges
    for (int tm = 0; tm < mt; ++tm)
        for (int tn = 0; tn < nt; ++tn) {
            if (p.lower && tn > tm) continue;
            int k0, k1;
            k_range(p.k_lo, p.k_hi, d.K, d.tile, tm, tn, &k0, &k1);
            for (int s = k0 / 16; s < k1 / 16; ++s) needA[(size_t)tm * slices + s] = needB[(size_t)tn * slices + s] = 1;
        }
    g_mutate = save;
    if (p.same) {
        for (size_t i = 0; i < needA.size(); ++i) needA[i] = needA[i] | needB[i];
        d.A = to_dev(operand_image(g_A0, std::max(d.M, d.N), d.lda, d.tile, needA, slices));
        d.B = d.A;
    } else {
        d.A = to_dev(operand_image(g_A0, d.M, d.lda, d.tile, needA, slices));
        d.B = to_dev(operand_image(g_B0, d.N, d.ldb, d.tile, needB, slices));
    }
    d.C = (double*)dev_bytes(sizeof(double) * (size_t)(d.M + 2) * d.ldc, 0xff);
    d.CT = (double*)dev_bytes(sizeof(double) * (size_t)(d.N + 2) * d.ldct, 0xff);
    return d;
}

// one launch; returns "" or the first difference
static std::string dg_run(const DgDev& d, double alpha, double beta, bool want_ct)
{
    const DgProb& p = d.p;
    std::vector<double> c0((size_t)(d.M + 2) * d.ldc, poison_f64());
    if (beta != 0.0)
        for (int m = 0; m < d.M; ++m)
            for (int n = 0; n < d.N; ++n) c0[(size_t)m * d.ldc + n] = (double)g_C0[(size_t)m * DMAX + n];
    if (beta != 0.0) CK(hipMemcpy(d.C, c0.data(), c0.size() * 8, hipMemcpyHostToDevice));
    else CK(hipMemset(d.C, 0xff, c0.size() * 8));
    if (want_ct) CK(hipMemset(d.CT, 0xff, sizeof(double) * (size_t)(d.N + 2) * d.ldct));
    RtxDgemm g = {};
    g.A = d.A; g.B = d.B; g.lda = d.lda; g.ldb = d.ldb; g.m_tiles = d.M / d.tile; g.n_tiles = d.N / d.tile; g.k_slices = p.ks;
    g.C = d.C; g.ldc = d.ldc; g.CT = want_ct ? d.CT : nullptr; g.ldct = d.ldct; g.alpha = alpha; g.beta = beta; g.lower_only = p.lower;
    g.k_lo = p.k_lo; g.k_hi = p.k_hi; g.small_tile = p.small;
    RT(rtx_dgemm_launch(g, 0));
    CK(hipDeviceSynchronize());
    const std::vector<double> c = to_host(d.C, c0.size());
    std::vector<double> ct;   // never handed to the kernel when CT is null
    if (want_ct) ct = to_host(d.CT, (size_t)(d.N + 2) * d.ldct);
    const std::vector<int>& pre = *d.pre;
    std::vector<double> want_t((size_t)(d.N + 2) * d.ldct, poison_f64());
    for (int m = 0; m < d.M + 2; ++m)
        for (int n = 0; n < d.ldc; ++n) {
            double want = c0[(size_t)m * d.ldc + n];
            if (m < d.M && n < d.N) {
                const int tm = m / d.tile, tn = n / d.tile;
                if (!(p.lower && tn > tm)) {
                    int k0, k1;
                    k_range(p.k_lo, p.k_hi, d.K, d.tile, tm, tn, &k0, &k1);
                    int acc = 0;
                    if (k1 > k0) acc = pre[((size_t)(k1 / 64) * d.M + m) * d.N + n] - pre[((size_t)(k0 / 64) * d.M + m) * d.N + n];
                    double v = alpha * (double)acc;
                    if (beta != 0.0) v += beta * want;
                    want = v;
                    if (want_ct) want_t[(size_t)n * d.ldct + m] = v;
                }
            }
            const double got = c[(size_t)m * d.ldc + n];
            if (d_bits(got) != d_bits(want)) return fmt("C[%d][%d] = %.17g (bits %016llx), expected %.17g (%016llx)", m, n, got, (unsigned long long)d_bits(got), want, (unsigned long long)d_bits(want));
        }
    for (size_t i = 0; i < ct.size(); ++i)
        if (d_bits(ct[i]) != d_bits(want_t[i]))
            return fmt("CT[%d][%d] = %.17g, expected %.17g", (int)(i / d.ldct), (int)(i % d.ldct), ct[i], want_t[i]);
    return "";
}

static void dgemm_cross_product()
{
    static const double AB[3][2] = {{1.0, 0.0}, {-1.0, 1.0}, {-1.0, 0.0}};
    static const int SHAPES[3][2] = {{3, 3}, {2, 5}, {5, 2}};
    for (const auto& sh : SHAPES) {
        const std::vector<int> pre = prefix_table(g_A0.data(), g_B0.data(), 128 * sh[0], 128 * sh[1], 384);
        for (int small = 0; small < 2; ++small)
            for (int k_lo = 0; k_lo < 4; ++k_lo)
                for (int k_hi = 0; k_hi < 3; ++k_hi)
                    for (int lower = 0; lower < 2; ++lower) {
                        int launches = 0, empty_tiles = 0;
                        std::string bad;
                        for (int ks : {0, 8, 16, 24}) {
                            const DgProb p = {sh[0], sh[1], ks, k_lo, k_hi, lower, small, false};
                            const DgDev d = dg_prepare(p, pre);
                            for (int tm = 0; tm < d.M / d.tile; ++tm)
                                for (int tn = 0; tn < d.N / d.tile; ++tn) {
                                    int k0, k1;
                                    k_range(k_lo, k_hi, d.K, d.tile, tm, tn, &k0, &k1);
                                    if (!(lower && tn > tm) && k1 <= k0) ++empty_tiles;
                                }
                            for (const auto& ab : AB)
                                for (int ct = 0; ct < 2; ++ct) {
                                    const std::string r = dg_run(d, ab[0], ab[1], ct != 0);
                                    ++launches;
                                    if (!r.empty() && bad.empty()) bad = fmt("k_slices %d alpha %g beta %g CT %d: ", ks, ab[0], ab[1], ct) + r;
                                }
                            free_all();
                        }
                        report(fmt("dgemm %dx%d tile %d k_lo %s k_hi %s lower %d", sh[0], sh[1], small ? 64 : 128, kname(k_lo), kname(k_hi), lower), bad.empty(),
                               bad.empty() ? fmt("%d launches (k_slices 0/8/16/24 x 3 alpha,beta x CT), %d tiles with an empty K range: all bitwise", launches, empty_tiles) : bad);
                    }
    }
}

// the solver's own launches (ease.hip: ease_factor(lo, hi) with n1 = 3, n2 = 2 blocks; the float64 Gram matrix; P = W^T W with KB = 5)
static void dgemm_named()
{
    struct Named { const char* name; DgProb p; double alpha, beta; bool ct; };
    const std::vector<int> preAA = prefix_table(g_A0.data(), g_A0.data(), 640, 640, 640);
    for (int small = 0; small < 2; ++small) {
        const Named cases[] = {
            {"panel  L21 = A21 W11^T", {2, 3, 24, RTX_DK_ALL, RTX_DK_TN, 0, small, false}, 1.0, 0.0, false},
            {"update A22 -= L21 L21^T", {2, 2, 24, RTX_DK_ALL, RTX_DK_ALL, 1, small, true}, -1.0, 1.0, false},
            {"T^T = W11^T L21^T", {3, 2, 24, RTX_DK_TM, RTX_DK_ALL, 0, small, false}, 1.0, 0.0, false},
            {"W21 = -W22 T (+ W^T)", {2, 3, 16, RTX_DK_ALL, RTX_DK_TM, 0, small, false}, -1.0, 0.0, true},
            {"Gram G = X^T X (float64 route, 320 users)", {5, 5, 20, RTX_DK_ALL, RTX_DK_ALL, 1, small, true}, 1.0, 0.0, false},
            {"P = W^T W", {5, 5, 40, RTX_DK_MAX, RTX_DK_ALL, 1, small, true}, 1.0, 0.0, false},
        };
        for (const Named& c : cases) {
            std::vector<int> own;   // the table is [M][N] of its problem
            if (c.p.Mt != 5) own = prefix_table(g_A0.data(), c.p.same ? g_A0.data() : g_B0.data(), 128 * c.p.Mt, 128 * c.p.Nt, 640);
            const DgDev d = dg_prepare(c.p, c.p.Mt != 5 ? own : preAA);
            const std::string r = dg_run(d, c.alpha, c.beta, c.ct);
            report(fmt("dgemm tile %d %s", small ? 64 : 128, c.name), r.empty(),
                   r.empty() ? fmt("%dx%d tiles, K = %d, k_lo %s k_hi %s lower %d alpha %g beta %g CT %d: bitwise", c.p.Mt, c.p.Nt, 16 * c.p.ks, kname(c.p.k_lo), kname(c.p.k_hi), c.p.lower, c.alpha, c.beta, (int)c.ct) : r);
            free_all();
        }
    }
}

static void dgemm_real()
{
    const int M = 384, N = 384, K = 384;
    const long lda = 392, ldb = 408, ldc = 424;
    Rng r{777u};
    std::vector<double> A((size_t)(M + 8) * lda, poison_f64()), B((size_t)(N + 8) * ldb, poison_f64());
    for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) A[(size_t)m * lda + k] = r.f48();
    for (int n = 0; n < N; ++n) for (int k = 0; k < K; ++k) B[(size_t)n * ldb + k] = r.f48();
    std::vector<long double> ref((size_t)M * N), mag((size_t)M * N);
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            long double s = 0, a = 0;
            for (int k = 0; k < K; ++k) { const long double t = (long double)A[(size_t)m * lda + k] * B[(size_t)n * ldb + k]; s += t; a += fabsl(t); }
            ref[(size_t)m * N + n] = s; mag[(size_t)m * N + n] = a;
        }
    double* dA = to_dev(A); double* dB = to_dev(B);
    for (int small = 0; small < 2; ++small) {
        double* dC = (double*)dev_bytes(sizeof(double) * (size_t)M * ldc, 0xff);
        RtxDgemm g = {};
        const int tile = small ? 64 : 128;
        g.A = dA; g.B = dB; g.lda = lda; g.ldb = ldb; g.m_tiles = M / tile; g.n_tiles = N / tile; g.k_slices = K / 16; g.C = dC; g.ldc = ldc;
        g.alpha = 1.0; g.small_tile = small;
        RT(rtx_dgemm_launch(g, 0));
        CK(hipDeviceSynchronize());
        const std::vector<double> c = to_host(dC, (size_t)M * ldc);
        double worst = 0;
        bool pad_ok = true;
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < ldc; ++n) {
                if (n >= N) { pad_ok = pad_ok && is_poison(c[(size_t)m * ldc + n]); continue; }
                const double bound = (K + 2) * U53 * (double)mag[(size_t)m * N + n];
                const double err = (double)fabsl((long double)c[(size_t)m * ldc + n] - ref[(size_t)m * N + n]);
                const double ratio = std::isfinite(c[(size_t)m * ldc + n]) ? err / bound : INFINITY;
                worst = std::max(worst, ratio);
            }
        report(fmt("dgemm tile %d real-valued 384^3", tile), worst <= 1.0 && pad_ok, fmt("worst error %.2e of (K + 2) 2^-53 sum|a||b|, pad %s", worst, pad_ok ? "kept" : "OVERWRITTEN"));
    }
    free_all();
}

// =================================================================================================================================
// B: the fused ADMM SLIM epilogue
// =================================================================================================================================
struct EpiOut { double c, gamma, mnext; int branch; };   // branch: 0 above, 1 below, 2 inside the dead zone

// the reference's element-wise steps, one IEEE operation per line of arithmetic, no contraction
static EpiOut epi_ref(double acc, double add, double pd, bool diag, double g, double rho, double thr, int variant)
{
#pragma clang fp contract(off)
    const double bt = add + acc;
    double b = bt;
    if (diag && g_mutate != 2) {
        const double q = bt / pd;
        const double t = pd * q;
        b = bt - t;
    }
    const double gr = g / rho;
    const double a = b + gr;
    const double s1 = a - thr, s2 = -a - thr;
    const double p1 = s1 > 0.0 ? s1 : 0.0, p2 = s2 > 0.0 ? s2 : 0.0;
    EpiOut o;
    o.branch = s1 > 0.0 ? 0 : (s2 > 0.0 ? 1 : 2);
    double cv = p1 - p2;
    if (variant == RTX_ADMM_SOFT_NN) cv = cv >= 0.0 ? cv : 0.0;
    else if (variant == RTX_ADMM_B_NN) cv = b >= 0.0 ? b : 0.0;
    const double dlt = b - cv;
    const double rd = rho * dlt;
    o.gamma = g + rd;
    const double rc = rho * cv;
    o.mnext = rc - o.gamma;
    o.c = cv;
    return o;
}
// a second formulation: the soft threshold as sign(a) max(|a| - k, 0), the projections as fmax
static EpiOut epi_ref2(double acc, double add, double pd, bool diag, double g, double rho, double thr, int variant)
{
#pragma clang fp contract(off)
    double b = add + acc;
    if (diag) b = b - pd * (b / pd);
    const double a = b + g / rho;
    const double sh = fabs(a) - thr;
    double cv = sh > 0.0 ? copysign(sh, a) : 0.0;
    EpiOut o;
    o.branch = a > thr ? 0 : (a < -thr ? 1 : 2);
    if (variant == RTX_ADMM_SOFT_NN) cv = fmax(cv, 0.0);
    else if (variant == RTX_ADMM_B_NN) cv = fmax(b, 0.0);
    o.gamma = g + rho * (b - cv);
    o.mnext = rho * cv - o.gamma;
    o.c = cv;
    return o;
}

static const int ENP = 384;
static const double ETHR = 0.75;
struct EpiData { std::vector<double> add, gamma, pdiag; };   // [ENP][ENP], [ENP]: the clean values
static EpiData epi_data(const std::vector<int>& pre, double rho, bool with_acc)
{
    EpiData e;
    Rng r{4242u};
    e.add.resize((size_t)ENP * ENP); e.gamma.resize(e.add.size()); e.pdiag.resize(ENP);
    for (int i = 0; i < ENP; ++i) e.pdiag[i] = 0.5 + r.u01();
    for (int i = 0; i < ENP; ++i)
        for (int j = 0; j < ENP; ++j) {
            const size_t o = (size_t)i * ENP + j;
            const double acc = with_acc ? (double)pre[((size_t)6 * ENP + i) * ENP + j] : 0.0;
            // a third of the elements land around the dead zone, the rest far on either side
            e.add[o] = ((i + j) % 3 == 0) ? -acc + 3.0 * ETHR * r.f48() : 300.0 * r.f48();
            e.gamma[o] = rho * ETHR * 0.5 * r.f48();
        }
    return e;
}

static int g_en1_branches[3] = {0, 0, 0};

static void admm_case(const std::vector<int>& pre, const double* dA_int, const double* dA_nan, const double* dB, int variant, int e_n, double rho, bool want_ct,
                      bool k0, int index)
{
    const long lda = 648, ldb = 672, ldc = ENP + 24, ldct = ENP + 40;
    EpiData e = epi_data(pre, rho, !k0);
    static const double G0[3] = {2.0, -2.0, 0.3};
    e.gamma[0] = rho * ETHR * G0[index % 3];   // the diagonal element (0, 0): b ~ 0 there, so gamma alone picks the branch
    std::vector<double> add((size_t)(ENP + 2) * ldc, poison_f64()), gam(add.size(), poison_f64());
    std::vector<double> pd(ENP + 8, poison_f64());
    for (int i = 0; i < e_n; ++i) {
        pd[i] = e.pdiag[i];
        for (int j = 0; j < e_n; ++j) { add[(size_t)i * ldc + j] = e.add[(size_t)i * ENP + j]; gam[(size_t)i * ldc + j] = e.gamma[(size_t)i * ENP + j]; }
    }
    double* d_add = to_dev(add); double* d_gam = to_dev(gam); double* d_pd = to_dev(pd);
    double* d_mn = (double*)dev_bytes(add.size() * 8, 0xff);
    double* d_C = (double*)dev_bytes(add.size() * 8, 0xff);
    double* d_CT = (double*)dev_bytes(sizeof(double) * (size_t)(ENP + 2) * ldct, 0xff);
    RtxDgemm g = {};
    g.A = k0 ? dA_nan : dA_int; g.B = dB; g.lda = lda; g.ldb = ldb; g.m_tiles = g.n_tiles = ENP / 128; g.k_slices = k0 ? 0 : ENP / 16;
    g.C = d_C; g.ldc = ldc; g.CT = want_ct ? d_CT : nullptr; g.ldct = ldct;
    g.e_add = d_add; g.e_pdiag = d_pd; g.e_gamma = d_gam; g.e_mnext = d_mn; g.e_rho = rho; g.e_thr = ETHR; g.e_n = e_n; g.e_variant = variant;
    RT(rtx_dgemm_admm_launch(g, 0));
    CK(hipDeviceSynchronize());
    const std::vector<double> o_gam = to_host(d_gam, add.size()), o_mn = to_host(d_mn, add.size()), o_C = to_host(d_C, add.size());
    const std::vector<double> o_CT = to_host(d_CT, (size_t)(ENP + 2) * ldct);
    std::vector<double> want_ct_img((size_t)(ENP + 2) * ldct, poison_f64());
    int branches[3] = {0, 0, 0};
    std::string bad;
    for (int i = 0; i < ENP + 2 && bad.empty(); ++i)
        for (int j = 0; j < ldc; ++j) {
            const size_t o = (size_t)i * ldc + j;
            double wg = poison_f64(), wm = poison_f64();
            if (i < ENP && j < ENP) {
                EpiOut r = {0.0, 0.0, 0.0, 2};
                if (i < e_n && j < e_n) {
                    const double acc = k0 ? 0.0 : (double)pre[((size_t)6 * ENP + i) * ENP + j];
                    r = epi_ref(acc, add[o], pd[i], i == j, gam[o], rho, ETHR, variant);
                    ++branches[r.branch];
                }
                wg = r.gamma; wm = r.mnext;
                if (want_ct) want_ct_img[(size_t)j * ldct + i] = r.c;
            }
            if (d_bits(o_gam[o]) != d_bits(wg)) { bad = fmt("e_gamma[%d][%d] = %.17g, expected %.17g", i, j, o_gam[o], wg); break; }
            if (d_bits(o_mn[o]) != d_bits(wm)) { bad = fmt("e_mnext[%d][%d] = %.17g, expected %.17g", i, j, o_mn[o], wm); break; }
            if (!is_poison(o_C[o])) { bad = fmt("C[%d][%d] written (%.17g)", i, j, o_C[o]); break; }
        }
    for (size_t i = 0; i < o_CT.size() && bad.empty(); ++i)
        if (d_bits(o_CT[i]) != d_bits(want_ct_img[i])) bad = fmt("CT[%d][%d] = %.17g, expected %.17g", (int)(i / ldct), (int)(i % ldct), o_CT[i], want_ct_img[i]);
    bool counted = true;
    if (e_n > 1) counted = branches[0] > 0 && branches[1] > 0 && branches[2] > 0;
    else for (int b = 0; b < 3; ++b) g_en1_branches[b] += branches[b];
    if (bad.empty() && !counted) bad = "a branch of the soft threshold did not occur";
    report(fmt("admm variant %d e_n %d rho %g CT %d k_slices %d", variant, e_n, rho, (int)want_ct, k0 ? 0 : ENP / 16), bad.empty(),
           bad.empty() ? fmt("gamma, mnext, CT bitwise; pad exact zeros; branches above %d below %d inside %d", branches[0], branches[1], branches[2]) : bad);
}

static int admm_refusals()
{
    int bad = 0;
    double x = 0;
    RtxDgemm g = {};
    g.A = g.B = &x; g.m_tiles = g.n_tiles = 1; g.k_slices = 1; g.e_add = g.e_pdiag = &x; g.e_gamma = g.e_mnext = &x; g.C = &x;
    { RtxDgemm h = g; h.small_tile = 1; bad += rtx_dgemm_admm_launch(h, 0) != RTX_EINVAL; }
    { RtxDgemm h = g; h.e_add = nullptr; bad += rtx_dgemm_admm_launch(h, 0) != RTX_EINVAL; }
    { RtxDgemm h = g; h.e_pdiag = nullptr; bad += rtx_dgemm_admm_launch(h, 0) != RTX_EINVAL; }
    { RtxDgemm h = g; h.e_gamma = nullptr; bad += rtx_dgemm_admm_launch(h, 0) != RTX_EINVAL; }
    { RtxDgemm h = g; h.e_mnext = nullptr; bad += rtx_dgemm_admm_launch(h, 0) != RTX_EINVAL; }
    { RtxDgemm h = g; h.m_tiles = 0; bad += rtx_dgemm_admm_launch(h, 0) != RTX_EINVAL; bad += rtx_dgemm_launch(h, 0) != RTX_EINVAL; }
    { RtxDgemm h = g; h.k_slices = -1; bad += rtx_dgemm_launch(h, 0) != RTX_EINVAL; }
    float c = 0;
    bad += rtx_syrk_lower_launch(nullptr, 128, 128, 1, 2, 1, 1, &c, 256, 0) != RTX_EINVAL;
    bad += rtx_syrk_lower_launch(&x, 128, 128, 1, 2, 1, 1, nullptr, 256, 0) != RTX_EINVAL;
    bad += rtx_syrk_lower_launch(&x, 128, 128, 0, 2, 1, 1, &c, 256, 0) != RTX_EINVAL;
    bad += rtx_syrk_lower_launch(&x, 128, 128, 1, 2, 0, 1, &c, 256, 0) != RTX_EINVAL;
    report("refusals", bad == 0, fmt("dgemm_admm: small_tile, each null e_* pointer, no tiles; dgemm: no tiles, negative K; syrk: null operand / result, no rows, no K: %d wrong returns", bad));
    return bad;
}

static void admm_all()
{
    const std::vector<int> pre = prefix_table(g_A0.data(), g_B0.data(), ENP, ENP, 384);
    const int slices = DMAX / 16;
    std::vector<char> need((size_t)3 * slices, 0), none(need.size(), 0);
    for (int t = 0; t < 3; ++t) for (int s = 0; s < ENP / 16; ++s) need[(size_t)t * slices + s] = 1;
    double* dA = to_dev(operand_image(g_A0, ENP, 648, 128, need, slices));
    double* dAn = to_dev(operand_image(g_A0, ENP, 648, 128, none, slices));
    double* dB = to_dev(operand_image(g_B0, ENP, 672, 128, need, slices));
    double* dBn = to_dev(operand_image(g_B0, ENP, 672, 128, none, slices));
    const size_t keep = pool_size();
    int index = 0;
    for (int variant : {RTX_ADMM_SOFT, RTX_ADMM_SOFT_NN, RTX_ADMM_B_NN})
        for (int e_n : {384, 300, 257, 1})
            for (double rho : {4.0, 1e5 / 3.0})
                for (int ct = 0; ct < 2; ++ct)
                    for (int k0 = 0; k0 < 2; ++k0) {
                        admm_case(pre, dA, dAn, k0 ? dBn : dB, variant, e_n, rho, ct != 0, k0 != 0, index++);
                        free_from(keep);
                    }
    report("admm e_n 1, all cases together", g_en1_branches[0] > 0 && g_en1_branches[1] > 0 && g_en1_branches[2] > 0,
           fmt("branches of the one element: above %d below %d inside %d", g_en1_branches[0], g_en1_branches[1], g_en1_branches[2]));
    admm_refusals();
    free_all();
}

// =================================================================================================================================
// C: the SYRK
// =================================================================================================================================
__global__ void k_test_to_fp8(const float* src, uint8_t* dst, long total)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float v = src[i];
    // the conversion k_ease_scatter_T8 uses; a NaN becomes e4m3's NaN code
    dst[i] = (v != v) ? (uint8_t)0x7f : (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false) & 0xff);
}

static const int SROWS = 2304, SK = 384;

static void syrk_all()
{
    Rng r{99u};
    std::vector<int8_t> V((size_t)SROWS * SK);
    for (auto& v : V) v = (int8_t)r.i(-4, 4);
    // Q[kb][i][j] = sum_{k < 64 (kb + 1)} V[i][k] V[j][k] for the lower 256-tiles (whole diagonal tiles), int32 sums kept as int16 (<= 6144)
    const int NB = SK / 64;
    std::vector<int16_t> Q((size_t)NB * SROWS * SROWS, 0);
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < SROWS; ++i) {
        const int jend = (i / 256 + 1) * 256;
        for (int j = 0; j < jend; ++j) {
            int s = 0;
            for (int kb = 0; kb < NB; ++kb) {
                const int8_t* a = &V[(size_t)i * SK + kb * 64];
                const int8_t* b = &V[(size_t)j * SK + kb * 64];
                int t = 0;
                for (int k = 0; k < 64; ++k) t += (int)a[k] * (int)b[k];
                s += t;
                Q[((size_t)kb * SROWS + i) * SROWS + j] = (int16_t)s;
            }
        }
    }
    for (int fp8 = 1; fp8 >= 0; --fp8)
        for (int ks : {1, 2, 3}) {
            const int esz = fp8 ? 1 : 2, K = 128 * ks / esz;
            const long row_bytes = 128 * ks + 64, row_elems = row_bytes / esz;
            void* dA = nullptr;
            if (fp8) {
                std::vector<float> h((size_t)(SROWS + 8) * row_elems, NAN);
                for (int i = 0; i < SROWS; ++i) for (int k = 0; k < K; ++k) h[(size_t)i * row_elems + k] = (float)V[(size_t)i * SK + k];
                float* dsrc = to_dev(h);
                dA = dev_bytes(h.size(), 0);
                hipLaunchKernelGGL(k_test_to_fp8, dim3((unsigned)((h.size() + 255) / 256)), dim3(256), 0, 0, dsrc, (uint8_t*)dA, (long)h.size());
                CK(hipGetLastError());
                CK(hipDeviceSynchronize());
            } else {
                std::vector<bf16_t> h((size_t)(SROWS + 8) * row_elems, (bf16_t)0xffff);
                for (int i = 0; i < SROWS; ++i) for (int k = 0; k < K; ++k) h[(size_t)i * row_elems + k] = f32_to_bf16((float)V[(size_t)i * SK + k]);
                dA = to_dev(h);
            }
            int kb = K / 64 - 1;
            if (g_mutate == 3 && kb > 0) --kb;
            for (int rows256 : {1, 2, 9})
                for (int odd = 0; odd < 2; ++odd) {
                    const int cols128 = 2 * rows256 - odd, ncols = 128 * cols128, rows = 256 * rows256;
                    const long ldc = ncols + 8 + (odd ? 128 : 0);   // the overhang columns exist in the buffer and must keep the poison
                    float* dC = (float*)dev_bytes(sizeof(float) * (size_t)(rows + 2) * ldc, 0xff);
                    RT(rtx_syrk_lower_launch(dA, row_bytes, 128, rows256, cols128, ks, fp8, dC, ldc, 0));
                    CK(hipDeviceSynchronize());
                    const std::vector<float> c = to_host(dC, (size_t)(rows + 2) * ldc);
                    free_from(pool_size() - 1);      // dC
                    std::string bad;
                    long written = 0;
                    for (int i = 0; i < rows + 2 && bad.empty(); ++i)
                        for (int j = 0; j < ldc; ++j) {
                            uint32_t want = 0xffffffffu;
                            if (i < rows && j < ncols && j / 256 <= i / 256) { want = f_bits((float)Q[((size_t)kb * SROWS + i) * SROWS + j]); ++written; }
                            if (f_bits(c[(size_t)i * ldc + j]) != want) {
                                bad = fmt("C[%d][%d] (tile %d, %d) = %g (bits %08x), expected bits %08x", i, j, i / 256, j / 256, c[(size_t)i * ldc + j], f_bits(c[(size_t)i * ldc + j]), want);
                                break;
                            }
                        }
                    report(fmt("syrk %s rows256 %d cols128 %d k_slices %d", fp8 ? "fp8" : "bf16", rows256, cols128, ks), bad.empty(),
                           bad.empty() ? fmt("%ld elements of the lower tiles bitwise the integer Gram (K = %d), upper tiles, columns >= %d and guard rows keep the poison", written, K, ncols) : bad);
                }
            free_all();
        }
}

// =================================================================================================================================
// D: rtx_gram_inverse
// =================================================================================================================================
// lower Cholesky, the inverse of the factor (kept transposed: WT[j][k] = W[k][j]) and P = W^T W, all in T; false if not positive definite
// sum_first: each element's sum over k is accumulated from zero and then subtracted from A (the order of a blocked update
// A22 -= L21 L21^T); otherwise the terms are subtracted from A one after the other.  Both are plain Cholesky factorisations
template <typename T>
static bool chol_inverse(const std::vector<T>& A, int n, std::vector<T>& P, bool sum_first = false)
{
    std::vector<T> L((size_t)n * n, 0), WT((size_t)n * n, 0);
    for (int j = 0; j < n; ++j) {
        T d = sum_first ? (T)0 : A[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (sum_first) d += A[(size_t)j * n + j];
        if (!(d > 0)) return false;
        L[(size_t)j * n + j] = std::sqrt(d);
#pragma omp parallel for if (n - j > 64)
        for (int i = j + 1; i < n; ++i) {
            T s = sum_first ? (T)0 : A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            if (sum_first) s += A[(size_t)i * n + j];
            L[(size_t)i * n + j] = s / L[(size_t)j * n + j];
        }
    }
#pragma omp parallel for schedule(dynamic, 8)
    for (int j = 0; j < n; ++j) {
        WT[(size_t)j * n + j] = (T)1 / L[(size_t)j * n + j];
        for (int i = j + 1; i < n; ++i) {
            T s = 0;
            for (int k = j; k < i; ++k) s -= L[(size_t)i * n + k] * WT[(size_t)j * n + k];
            WT[(size_t)j * n + i] = s / L[(size_t)i * n + i];
        }
    }
    P.assign((size_t)n * n, 0);
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            T s = 0;
            for (int k = i; k < n; ++k) s += WT[(size_t)i * n + k] * WT[(size_t)j * n + k];
            P[(size_t)i * n + j] = P[(size_t)j * n + i] = s;
        }
    return true;
}

struct HostCsr {
    int n = 0;
    long U = 0;
    bool binary = false;
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<float> values;
};
enum { R_BINARY, R_FP8, R_BF16, R_QUARTER, R_EIGHTH, R_STEP03, R_BIG, R_ALL16 };
static const char* RNAME[] = {"binary", "fp8 1..16", "bf16 17..256", "quarters (fp8 x4)", "eighths (fp8 x8)", "0.3 steps (f64)", "|v| > 256 (f64)", "all 16"};

static HostCsr make_csr(int route, int n, long U, double density, int empty_col, uint32_t seed)
{
    HostCsr x;
    Rng r{seed};
    x.n = n; x.U = U; x.binary = route == R_BINARY;
    x.indptr.push_back(0);
    for (long u = 0; u < U; ++u) {
        for (int j = 0; j < n; ++j) {
            if (j == empty_col || r.u01() >= density) continue;
            float v = 1.f;
            switch (route) {
            case R_FP8: v = (float)r.i(1, 16); break;
            case R_BF16: v = (float)r.i(17, 256); break;
            case R_QUARTER: v = 0.25f * (float)r.i(1, 16); break;
            case R_EIGHTH: v = 0.125f * (float)r.i(1, 16); break;
            case R_STEP03: v = (float)(0.3 * r.i(1, 16)); break;
            case R_BIG: v = (float)r.i(1, 1000) * ((r.u() & 1) ? 1.f : -1.f); break;
            case R_ALL16: v = 16.f; break;
            }
            x.indices.push_back(j);
            x.values.push_back(v);
        }
        x.indptr.push_back((int64_t)x.indices.size());
    }
    if (route == R_BF16) x.values[0] = 256.f;
    if (route == R_BIG) x.values[0] = 1000.f;
    return x;
}

struct GramRef {
    std::vector<long double> G, mag;   // X^T X of the float32 values in long double (exact for integers and dyadic values) and sum |x||x|
    std::vector<double> Gd;            // the same sum in plain double, row by row
};
static GramRef gram_ref(const HostCsr& x)
{
    GramRef g;
    const int n = x.n;
    g.G.assign((size_t)n * n, 0); g.mag.assign((size_t)n * n, 0); g.Gd.assign((size_t)n * n, 0);
    for (long u = 0; u < x.U; ++u)
        for (int64_t a = x.indptr[u]; a < x.indptr[u + 1]; ++a)
            for (int64_t b = x.indptr[u]; b < x.indptr[u + 1]; ++b) {
                const float va = x.binary ? 1.f : x.values[a], vb = x.binary ? 1.f : x.values[b];
                const size_t o = (size_t)x.indices[a] * n + x.indices[b];
                const long double t = (long double)va * vb;
                g.G[o] += t; g.mag[o] += fabsl(t); g.Gd[o] += (double)va * (double)vb;
            }
    return g;
}

struct PRef { bool pd; std::vector<long double> P; double floor, floor_seq, floor_sum; };
// P_ld = (G + bs b b^T + shift I)^-1 in long double, and the error of the same inverse in plain double against it: the floor.  The
// double inverse is run in both plain orders of chol_inverse and the floor is the larger error: with the rank-1 item-bias term the
// two differ tenfold (see the header), and the device's blocked updates sum first
static PRef p_ref(const GramRef& g, int n, const std::vector<double>* bias, double bs, double shift)
{
    std::vector<long double> A((size_t)n * n);
    std::vector<double> Ad((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const size_t o = (size_t)i * n + j;
            A[o] = g.G[o] + (bias ? (long double)bs * (*bias)[i] * (*bias)[j] : 0.0L) + (i == j ? (long double)shift : 0.0L);
            double v = g.Gd[o];
            if (bias) v += (bs * (*bias)[i]) * (*bias)[j];
            Ad[o] = v + (i == j ? shift : 0.0);
        }
    PRef r;
    std::vector<double> Pd;
    r.pd = chol_inverse(A, n, r.P);
    r.floor = r.floor_seq = r.floor_sum = 0;
    for (int sum_first = 0; sum_first < 2 && r.pd; ++sum_first)
        if (chol_inverse(Ad, n, Pd, sum_first != 0)) {
            long double e = 0, s = 0;
            for (size_t o = 0; o < Pd.size(); ++o) { e = std::max(e, fabsl((long double)Pd[o] - r.P[o])); s = std::max(s, fabsl(r.P[o])); }
            (sum_first ? r.floor_sum : r.floor_seq) = (double)(e / s);
        }
    r.floor = std::max(r.floor_seq, r.floor_sum);
    return r;
}

struct DevCsr { rtx_csr x; };
static DevCsr csr_to_dev(const HostCsr& h)
{
    DevCsr d;
    d.x.indptr = to_dev(h.indptr);
    d.x.indices = to_dev(h.indices);
    d.x.values = h.binary ? nullptr : to_dev(h.values);
    d.x.n_rows = h.U; d.x.nnz = (int64_t)h.indices.size(); d.x.n_cols = h.n;
    int mx = 0;
    for (long u = 0; u < h.U; ++u) mx = std::max(mx, (int)(h.indptr[u + 1] - h.indptr[u]));
    d.x.max_row_len = mx;
    return d;
}

// freed device memory is handed out again: leave NaNs in it, so that a kernel reading what no launch wrote reads NaNs and not the
// zeros of a fresh page
static void dirty_the_heap(size_t bytes)
{
    void* p = nullptr;
    CK(hipMalloc(&p, bytes));
    CK(hipMemset(p, 0xff, bytes));
    CK(hipDeviceSynchronize());
    CK(hipFree(p));
}

static void gi_run(const char* tag, int route, const HostCsr& hx, const rtx_csr* dx, const GramRef& gr, const PRef& pr, const std::vector<double>* bias, double bs,
                   const double* d_bias, double shift, int want_G, int full_P, bool exact, hipEvent_t* ev)
{
    const int n = hx.n;
    std::vector<void*> keep, work;
    RtxGramInverse out;
    dirty_the_heap((size_t)48 << 20);
    RT(rtx_gram_inverse(dx, shift, d_bias, bs, want_G, full_P, &out, keep, work, ev, 0));
    CK(hipDeviceSynchronize());
    const int np = out.np;
    int status = -1;
    CK(hipMemcpy(&status, out.status, 4, hipMemcpyDeviceToHost));
    const std::vector<double> P = to_host(out.P, (size_t)np * np);
    std::vector<double> G;
    if (want_G) G = to_host(out.G, (size_t)np * np);
    for (void* p : keep) (void)hipFree(p);
    for (void* p : work) (void)hipFree(p);
    std::string bad;
    if (np != (n + 127) / 128 * 128) bad = fmt("np = %d", np);
    if ((out.G != nullptr) != (want_G != 0)) bad = "G pointer does not follow want_G";
    double g_worst = 0;
    if (want_G && bad.empty()) {
        for (int i = 0; i < np && bad.empty(); ++i)
            for (int j = 0; j < np; ++j) {
                const double got = G[(size_t)i * np + j];
                if (d_bits(got) != d_bits(G[(size_t)j * np + i])) { bad = fmt("G[%d][%d] = %.17g but G[%d][%d] = %.17g", i, j, got, j, i, G[(size_t)j * np + i]); break; }
                if (i >= n || j >= n) {
                    if (got != 0.0) { bad = fmt("G pad [%d][%d] = %.17g", i, j, got); break; }
                    continue;
                }
                const size_t o = (size_t)i * n + j;
                const long double term = bias ? (long double)bs * (*bias)[i] * (*bias)[j] : 0.0L;
                const long double ref = gr.G[o] + term;
                if (exact) {
                    if (!(got == (double)ref) || (long double)(double)ref != ref) { bad = fmt("G[%d][%d] = %.17g, exact value %.17Lg", i, j, got, ref); break; }
                } else {
                    // U products, each rounded once at most (float32 x float32 is exact in float64), summed in any order; the rank-1 term adds two
                    // roundings of its own and one of the final sum
                    const double bound = (double)(hx.U + 2) * U53 * (double)gr.mag[o] + 3.0 * U53 * (double)fabsl(term) + U53 * (double)fabsl(ref);
                    const double err = (double)fabsl((long double)got - ref);
                    const double ratio = std::isfinite(got) ? (bound > 0 ? err / bound : (err == 0 ? 0.0 : INFINITY)) : INFINITY;
                    g_worst = std::max(g_worst, ratio);
                    if (!(ratio <= 1.0)) { bad = fmt("G[%d][%d] = %.17g, long double %.17Lg, bound %.3g", i, j, got, ref, bound); break; }
                }
            }
    }
    double err = 0;
    if (bad.empty()) {
        if (status != 0) bad = fmt("status %d", status);
        long double e = 0, s = 0;
        for (int i = 0; i < np && bad.empty(); ++i)
            for (int j = 0; j < (full_P ? np : i + 1); ++j) {
                const double got = P[(size_t)i * np + j];
                if (full_P && d_bits(got) != d_bits(P[(size_t)j * np + i])) { bad = fmt("P[%d][%d] != P[%d][%d] bitwise", i, j, j, i); break; }
                if (i >= n || j >= n) {
                    if (got != (i == j ? 1.0 : 0.0)) { bad = fmt("P pad [%d][%d] = %.17g", i, j, got); break; }
                    continue;
                }
                if (!std::isfinite(got)) { bad = fmt("P[%d][%d] = %g", i, j, got); break; }
                e = std::max(e, fabsl((long double)got - pr.P[(size_t)i * n + j]));
                s = std::max(s, fabsl(pr.P[(size_t)i * n + j]));
            }
        err = (double)(e / s);
        if (bad.empty() && !(err <= 10.0 * pr.floor)) bad = fmt("P error %.3g above 10x the floor %.3g (term by term %.3g, sum first %.3g)", err, pr.floor, pr.floor_seq, pr.floor_sum);
    }
    report(fmt("gram-inverse %s%s n %d U %ld want_G %d bias %d full_P %d", tag, RNAME[route], n, hx.U, want_G, bias ? 1 : 0, full_P), bad.empty(),
           bad.empty() ? fmt("G %s; P max error %.2e, host double floor %.2e (term by term %.2e, sum first %.2e): %.2f of the 10x allowed, status %d, pad identity",
                             want_G ? (exact ? "bitwise exact" : fmt("within %.3f of its bound", g_worst).c_str()) : "not asked", err, pr.floor, pr.floor_seq, pr.floor_sum,
                             err / (10.0 * pr.floor), status) : bad);
}

static void gi_route(const char* tag, int route, int n, long U, double density, double shift, hipEvent_t* ev)
{
    const HostCsr hx = make_csr(route, n, U, density, -1, 1000u * route + n);
    const GramRef gr = gram_ref(hx);
    Rng r{(uint32_t)(31 * n + route)};
    std::vector<double> bias(n);
    for (auto& b : bias) b = (double)r.i(-6, 6);
    const double bs = (double)(U % 1000 + 3);   // integer-valued
    const DevCsr dx = csr_to_dev(hx);
    double* d_bias = to_dev(bias);
    const bool exact = route != R_STEP03;
    const PRef plain = p_ref(gr, n, nullptr, 0.0, shift), biased = p_ref(gr, n, &bias, bs, shift);
    if (!plain.pd || !biased.pd) { report(fmt("gram-inverse %s n %d", RNAME[route], n), false, "the host reference is not positive definite"); free_all(); return; }
    gi_run(tag, route, hx, &dx.x, gr, plain, nullptr, 0.0, nullptr, shift, 0, 0, exact, ev);
    gi_run(tag, route, hx, &dx.x, gr, plain, nullptr, 0.0, nullptr, shift, 1, 1, exact, ev);
    gi_run(tag, route, hx, &dx.x, gr, biased, &bias, bs, d_bias, shift, 1, 1, exact, ev);
    gi_run(tag, route, hx, &dx.x, gr, biased, &bias, bs, d_bias, shift, 0, 0, exact, ev);
    free_all();
}

static void gram_inverse_all()
{
    hipEvent_t ev[4];
    for (auto& evt : ev) CK(hipEventCreate(&evt));
    static const int NS[3] = {129, 300, 520};
    static const long US[3] = {211, 333, 257};
    for (int route : {R_BINARY, R_FP8, R_BF16, R_QUARTER, R_EIGHTH, R_STEP03, R_BIG})
        for (int s = 0; s < 3; ++s) gi_route("", route, NS[s], route == R_BF16 ? 250 : US[s], 0.1, 50.0, ev);   // 256^2 * 250 < 2^24: stays on bf16
    // 16^2 * 65536 = 2^24: the float32 accumulators could no longer hold every sum -> float64; one row fewer stays on fp8
    gi_route("switch at 2^24, f64 side: ", R_ALL16, 129, 65536, 0.06, 50.0, ev);
    gi_route("switch at 2^24, fp8 side: ", R_ALL16, 129, 65535, 0.06, 50.0, ev);
    {   // not positive definite: an empty column and no shift
        const HostCsr hx = make_csr(R_BINARY, 129, 211, 0.1, 40, 5u);
        const DevCsr dx = csr_to_dev(hx);
        std::vector<void*> keep, work;
        RtxGramInverse out;
        RT(rtx_gram_inverse(&dx.x, 0.0, nullptr, 0.0, 0, 0, &out, keep, work, ev, 0));
        CK(hipDeviceSynchronize());
        int status = 0;
        CK(hipMemcpy(&status, out.status, 4, hipMemcpyDeviceToHost));
        for (void* p : keep) (void)hipFree(p);
        for (void* p : work) (void)hipFree(p);
        report("gram-inverse not positive definite (empty column 40, shift 0)", status != 0, fmt("status %d", status));
        free_all();
    }
    for (auto& evt : ev) (void)hipEventDestroy(evt);
}

// =================================================================================================================================
// E: dense scores
// =================================================================================================================================
static void scores_all()
{
    for (int n : {1, 2, 511, 513, 515, 1025}) {   // (515: one workgroup's 512 columns plus three, the edge of the shared -inf tail)
        const int rows = 7, batch = 5;
        const long ldb = n + 6;
        Rng r{(uint32_t)(500 + n)};
        std::vector<double> B((size_t)n * ldb, poison_f64()), bias(n);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) B[(size_t)i * ldb + j] = r.f48();
        for (auto& b : bias) b = 3.0 * r.f48();
        // x: 7 rows, row 2 empty; mask: 7 rows with entries at the workgroup boundary (columns 511, 512) and stored zeros
        HostCsr x, m;
        x.indptr.push_back(0); m.indptr.push_back(0);
        for (int u = 0; u < rows; ++u) {
            for (int j = 0; j < n; ++j) {
                if (u != 2 && (n <= 2 || r.u01() < 0.05)) { x.indices.push_back(j); x.values.push_back((float)(0.3 * r.i(-9, 9))); }
                const bool edge = j == 0 || j == 511 || j == 512 || j == n - 1;
                if (edge || r.u01() < 0.03) { m.indices.push_back(j); m.values.push_back(((u + j) % 3 == 0) ? 0.f : (float)r.i(1, 5)); }
            }
            x.indptr.push_back((int64_t)x.indices.size()); m.indptr.push_back((int64_t)m.indices.size());
        }
        const std::vector<int32_t> ids = {6, 2, 0, 5, 5};
        double* dB = to_dev(B); double* dbias = to_dev(bias);
        int64_t* xp = to_dev(x.indptr); int32_t* xi = to_dev(x.indices); float* xv = to_dev(x.values);
        int64_t* mp = to_dev(m.indptr); int32_t* mi = to_dev(m.indices); float* mv = to_dev(m.values);
        int32_t* dids = to_dev(ids);
        for (int with_bias = 0; with_bias < 2; ++with_bias)
            for (int mode = 0; mode < 5; ++mode) {   // 0 no mask, 1 mask, 2 row_ids on x, 3 row_ids on the mask, 4 mask without values (all ones)
                RtxCsrView xv_ = {xp, xi, xv, mode == 2 ? dids : nullptr, 0, 0};
                RtxCsrView mv_ = {nullptr, nullptr, nullptr, nullptr, 0, 0};
                if (mode) mv_ = RtxCsrView{mp, mi, mode == 4 ? nullptr : mv, mode == 3 ? dids : nullptr, 0, 0};
                double* dout = (double*)dev_bytes(sizeof(double) * ((size_t)batch * n + 16), 0xff);
                RT(rtx_dense_scores_launch(xv_, mv_, dB, ldb, with_bias ? dbias : nullptr, n, batch, dout, 0));
                CK(hipDeviceSynchronize());
                const std::vector<double> out = to_host(dout, (size_t)batch * n + 16);
                free_from(pool_size() - 1);      // dout
                std::string bad;
                double worst = 0;
                long ninf = 0;
                for (int b = 0; b < batch && bad.empty(); ++b) {
                    const int xu = mode == 2 ? ids[b] : b, mu = mode == 3 ? ids[b] : b;
                    std::vector<char> inf(n, 0);
                    if (mode)
                        for (int64_t k = m.indptr[mu]; k < m.indptr[mu + 1]; ++k)
                            if (mode == 4 || m.values[k] != 0.f) inf[m.indices[k]] = 1;
                    for (int j = 0; j < n; ++j) {
                        const double got = out[(size_t)b * n + j];
                        if (inf[j]) { ++ninf; if (!(got == -INFINITY)) { bad = fmt("out[%d][%d] = %g, expected -inf", b, j, got); break; } continue; }
                        long double s = 0, a = 0;
                        for (int64_t k = x.indptr[xu]; k < x.indptr[xu + 1]; ++k) {
                            const long double t = (long double)x.values[k] * B[(size_t)x.indices[k] * ldb + j];
                            s += t; a += fabsl(t);
                        }
                        if (with_bias) { s += bias[j]; a += fabsl(bias[j]); }
                        const double bound = (double)(x.indptr[xu + 1] - x.indptr[xu] + 2) * U53 * (double)a;
                        const double err = (double)fabsl((long double)got - s);
                        if (!std::isfinite(got) || err > bound) { bad = fmt("out[%d][%d] = %.17g, long double %.17Lg, bound %.3g", b, j, got, s, bound); break; }
                        if (bound > 0) worst = std::max(worst, err / bound);
                    }
                }
                for (size_t i = (size_t)batch * n; i < out.size() && bad.empty(); ++i)
                    if (!is_poison(out[i])) bad = "wrote behind the end of out";
                report(fmt("scores n %d bias %d mode %d", n, with_bias, mode), bad.empty(),
                       bad.empty() ? fmt("worst error %.2e of (len + 2) 2^-53 sum|v||B|, %ld -inf exactly where the mask is non-zero", worst, ninf) : bad);
            }
        free_all();
    }
}

// =================================================================================================================================
// --host
// =================================================================================================================================
static void host_checks()
{
    // 1. the long double Cholesky inverse: P (G + shift I) = I
    {
        const HostCsr hx = make_csr(R_STEP03, 129, 211, 0.1, -1, 77u);
        const GramRef gr = gram_ref(hx);
        const PRef pr = p_ref(gr, 129, nullptr, 0.0, 50.0);
        long double worst = 0;
        const int n = 129;
        for (int i = 0; i < n && pr.pd; ++i)
            for (int j = 0; j < n; ++j) {
                long double s = 0;
                for (int k = 0; k < n; ++k) s += pr.P[(size_t)i * n + k] * (gr.G[(size_t)k * n + j] + (k == j ? 50.0L : 0.0L));
                worst = std::max(worst, fabsl(s - (i == j ? 1.0L : 0.0L)));
            }
        report("host: long double Cholesky inverse", pr.pd && worst < 1e-15L && pr.floor > 0 && pr.floor < 1e-12,
               fmt("max|P (G + 50 I) - I| %.2Le, plain double against it %.2e", worst, pr.floor));
        const HostCsr he = make_csr(R_BINARY, 129, 211, 0.1, 40, 5u);
        const PRef pe = p_ref(gram_ref(he), 129, nullptr, 0.0, 0.0);
        report("host: an empty column without a shift", !pe.pd, "the host Cholesky refuses it too");
    }
    // 2. the prefix-sum reference over the triangular K ranges against a dense product of explicitly zeroed operands
    for (int tile : {64, 128}) {
        const int Mt = tile == 64 ? 3 : 2, Nt = 2, M = Mt * tile, N = Nt * tile, K = tile == 64 ? 256 : 384;
        const std::vector<int> pre = prefix_table(g_A0.data(), g_B0.data(), M, N, K);
        long bad = 0, empty = 0;
        for (int k_lo = 0; k_lo < 4; ++k_lo)
            for (int k_hi = 0; k_hi < 3; ++k_hi)
                for (int m = 0; m < M; ++m)
                    for (int n = 0; n < N; ++n) {
                        const int tm = m / tile, tn = n / tile;
                        int k0, k1;
                        k_range(k_lo, k_hi, K, tile, tm, tn, &k0, &k1);
                        const int fast = k1 > k0 ? pre[((size_t)(k1 / 64) * M + m) * N + n] - pre[((size_t)(k0 / 64) * M + m) * N + n] : 0;
                        // the triangular operand written out: W11 lower (k_hi TN): B[n][k] = 0 for k >= tile (tn + 1), and so on
                        int s = 0;
                        for (int k = 0; k < K; ++k) {
                            int a = g_A0[(size_t)m * DMAX + k], b = g_B0[(size_t)n * DMAX + k];
                            if (k_lo == RTX_DK_TM && k < tile * tm) a = 0;
                            if (k_lo == RTX_DK_TN && k < tile * tn) b = 0;
                            if (k_lo == RTX_DK_MAX && (k < tile * tm || k < tile * tn)) a = b = 0;
                            if (k_hi == RTX_DK_TM && k >= tile * (tm + 1)) a = 0;
                            if (k_hi == RTX_DK_TN && k >= tile * (tn + 1)) b = 0;
                            s += a * b;
                        }
                        bad += s != fast;
                        empty += (m % tile == 0 && n % tile == 0 && k1 <= k0);
                    }
        report(fmt("host: K-range reference, tile %d", tile), bad == 0 && empty > 0, fmt("12 (k_lo, k_hi) pairs on %dx%d tiles, K = %d: %ld differences, %ld empty ranges met", Mt, Nt, K, bad, empty));
    }
    // 3. the epilogue reference against the second formulation
    {
        Rng r{9u};
        long bad = 0, n = 0, br[3] = {0, 0, 0};
        for (int variant = 0; variant < 3; ++variant)
            for (double rho : {4.0, 1e5 / 3.0})
                for (int t = 0; t < 20000; ++t) {
                    const double acc = (double)r.i(-400, 400), add = (t % 3 == 0) ? -acc + 3.0 * ETHR * r.f48() : 300.0 * r.f48();
                    const double pd = 0.5 + r.u01(), g = rho * ETHR * 0.5 * r.f48();
                    const bool diag = t % 7 == 0;
                    const EpiOut a = epi_ref(acc, add, pd, diag, g, rho, ETHR, variant), b = epi_ref2(acc, add, pd, diag, g, rho, ETHR, variant);
                    bad += !(a.c == b.c && a.gamma == b.gamma && a.mnext == b.mnext && a.branch == b.branch);
                    ++br[a.branch]; ++n;
                }
        report("host: epilogue reference", bad == 0 && br[0] && br[1] && br[2], fmt("%ld elements, %ld differences from the second formulation; branches %ld / %ld / %ld", n, bad, br[0], br[1], br[2]));
    }
    // 4. the launchers' refusals come before any HIP call
    admm_refusals();
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--mutate") && i + 1 < argc) g_mutate = atoi(argv[++i]);
        else { printf("usage: test_solver [--host] [--mutate 1|2|3]\n"); return 2; }
    }
    make_int_operands();
    if (g_host) {
        host_checks();
    } else {
        if (g_mutate) printf("reference %d deliberately wrong: this run must fail\n", g_mutate);
        if (!g_mutate || g_mutate == 1) { dgemm_named(); dgemm_cross_product(); dgemm_real(); }
        if (!g_mutate || g_mutate == 2) admm_all();
        if (!g_mutate || g_mutate == 3) syrk_all();
        if (!g_mutate) { gram_inverse_all(); scores_all(); }
    }
    return finish("SOLVER");
}
