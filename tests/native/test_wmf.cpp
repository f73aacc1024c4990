// test_wmf -- the WMF stack of wmf.hip (rtx_wmf_systems, rtx_wmf_solve_rows, rtx_wmf_fit / load / copy, rtx_wmf_scores) through the C ABI
// of the built library, on the harness of check.h.  include/rectorch_hip.h has the definition and the operation order.
//
// Host formulations, float64 unless said:
//   mirror   the device's order: G as partial Gram matrices of RTX_WMF_GRAM_ROWS rows added in ascending order; per row the entries in
//            stored order, S[r][c] = fma(w y[r], y[c], S[r][c]), b[c] = fma(1 + w, y[c], b[c]); rows longer than RTX_WMF_SEGMENT as
//            segments added in ascending order; A = (G + S) + lam on the diagonal, mirrored; a column Cholesky and two substitutions.
//   second   the definition, literal: A = Y^T Y + Y_u^T diag(w) Y_u + lam I and b = Y_u^T (1 + w) summed in long double, entries in
//            REVERSE order, rounded once; the solve by a long-double Cholesky.
// EXACT DATA: ratings are integers 1 .. 5, alpha = 0.5, lam = 1, factor entries multiples of 1/4 in [-2, 2]: every term of G, A and b is
// a small dyadic rational, every partial sum is exact, so every summation order gives the same bits -- mirror, second and the MFMA.
// `test_wmf --host` checks mirror against second on every case (systems bit for bit; the float64 solve by its residual against the
// textbook backward-error bound of a Cholesky solve) and makes no HIP call.  Without an argument:
//   A  rtx_wmf_systems bit for bit against the mirror, on every row and on both sides (users against item factors, items -- through the
//      transposed matrix -- against user factors), all rows and a row_ids subset; symmetric to the bit; guards behind both outputs.
//   B  rtx_wmf_solve_rows on the same systems against the long-double solve, by |x^ - x|_inf / |x|_inf per system.  The bound of a case
//      is 4 x the largest such error of the float64 column-Cholesky mirror over the case's systems, floored at f 2^-52 (the margin is for
//      the blocked factorisation's other summation order).  Both columns are printed (lines "wmf_ulp:").  Empty rows: exact zeros.
//   C  rtx_wmf_scores (a loaded model: fold-in + scores) bit for bit against fma(x[k], y[k], acc) over the device's own fold-in vector,
//      on exact and on generic factors; on generic factors also within gamma_f sum |x_k y_k| of the long-double dot product
//      (gamma_f = f u / (1 - f u), u = 2^-53); -inf exactly at the mask's non-zero entries, with mask_row_ids; ld > n_items.
//      The kernel's -inf tail at its edge: 256 + 3 items, nine users, a mask of its own with entries at columns 0, 255, 256, 258 and a
//      stored zero, its rows permuted.
//   D  one iteration of rtx_wmf_fit = the two half-sweeps of rtx_wmf_solve_rows, bit for bit; rtx_wmf_copy / shape / timings.
//   E  every refusal returns RTX_EINVAL with its documented message.
#include "../../include/rectorch_hip.h"
#include "../../rectorch_amd/csrc/rtx_common.h"
#include "check.h"

#include <cmath>

static const double ALPHA = 0.5, LAM = 1.0;
static const int SEG = RTX_WMF_SEGMENT;

struct HostCsr {
    int64_t n_rows = 0;
    int n_cols = 0;
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<float> values;
};

// users x items at the given density, ratings 1 .. 5; long_item0: item 0 is rated by everybody
static HostCsr make_ratings(int64_t U, int I, double density, bool long_item0, uint32_t seed)
{
    HostCsr x;
    Rng r{seed};
    x.n_rows = U; x.n_cols = I;
    x.indptr.push_back(0);
    const uint32_t thr = (uint32_t)(density * 16777216.0);
    for (int64_t u = 0; u < U; ++u) {
        for (int i = 0; i < I; ++i)
            if ((long_item0 && i == 0) || r.u() < thr) { x.indices.push_back(i); x.values.push_back((float)r.i(1, 5)); }
        x.indptr.push_back((int64_t)x.indices.size());
    }
    return x;
}

static HostCsr transpose(const HostCsr& x)
{
    HostCsr t;
    t.n_rows = x.n_cols; t.n_cols = (int)x.n_rows;
    t.indptr.assign((size_t)x.n_cols + 1, 0);
    for (int32_t i : x.indices) ++t.indptr[(size_t)i + 1];
    for (int i = 0; i < x.n_cols; ++i) t.indptr[(size_t)i + 1] += t.indptr[(size_t)i];
    t.indices.resize(x.indices.size()); t.values.resize(x.values.size());
    std::vector<int64_t> at(t.indptr.begin(), t.indptr.end() - 1);
    for (int64_t u = 0; u < x.n_rows; ++u)
        for (int64_t p = x.indptr[(size_t)u]; p < x.indptr[(size_t)u + 1]; ++p) {
            const int64_t q = at[(size_t)x.indices[(size_t)p]]++;
            t.indices[(size_t)q] = (int32_t)u; t.values[(size_t)q] = x.values[(size_t)p];
        }
    return t;
}

static std::vector<double> exact_factors(int64_t n, int f, uint32_t seed)
{
    Rng r{seed};
    std::vector<double> y((size_t)n * f);
    for (double& v : y) v = 0.25 * r.i(-8, 8);
    return y;
}
static std::vector<double> generic_factors(int64_t n, int f, uint32_t seed)
{
    Rng r{seed};
    std::vector<double> y((size_t)n * f);
    for (double& v : y) v = 0.3 * r.f48();
    return y;
}

// ---- mirror ---------------------------------------------------------------------------------------------------------------------------
static std::vector<double> gram_mirror(const std::vector<double>& Y, int64_t n, int f)
{
    std::vector<double> G((size_t)f * f, 0.0), S((size_t)f * f);
    bool first = true;
    for (int64_t n0 = 0; n0 < n; n0 += RTX_WMF_GRAM_ROWS) {
        std::fill(S.begin(), S.end(), 0.0);
        for (int64_t k = n0; k < std::min<int64_t>(n, n0 + RTX_WMF_GRAM_ROWS); ++k)
            for (int r = 0; r < f; ++r)
                for (int c = 0; c <= r; ++c) S[(size_t)r * f + c] = std::fma(Y[(size_t)k * f + r], Y[(size_t)k * f + c], S[(size_t)r * f + c]);
        for (size_t t = 0; t < S.size(); ++t) G[t] = first ? S[t] : G[t] + S[t];
        first = false;
    }
    for (int r = 0; r < f; ++r)
        for (int c = r + 1; c < f; ++c) G[(size_t)r * f + c] = G[(size_t)c * f + r];
    return G;
}

// A [f][f] and b [f] of row u
static void system_mirror(const HostCsr& x, int64_t u, const std::vector<double>& Y, int f, const std::vector<double>& G, double* A, double* b)
{
    const int64_t beg = x.indptr[(size_t)u], end = x.indptr[(size_t)u + 1];
    std::vector<double> S((size_t)f * f, 0.0), P((size_t)f * f), bs((size_t)f);
    std::fill(b, b + f, 0.0);
    bool first = true;
    for (int64_t s0 = beg; s0 < end || first; s0 += SEG) {
        std::fill(P.begin(), P.end(), 0.0);
        std::fill(bs.begin(), bs.end(), 0.0);
        for (int64_t p = s0; p < std::min(end, s0 + SEG); ++p) {
            const double* y = &Y[(size_t)x.indices[(size_t)p] * f];
            const double w = ALPHA * (double)x.values[(size_t)p];
            volatile double c1 = 1.0 + w;
            for (int r = 0; r < f; ++r) {
                volatile double a = w * y[r];
                for (int c = 0; c <= r; ++c) P[(size_t)r * f + c] = std::fma(a, y[c], P[(size_t)r * f + c]);
                bs[(size_t)r] = std::fma(c1, y[r], bs[(size_t)r]);
            }
        }
        for (size_t t = 0; t < S.size(); ++t) S[t] = first ? P[t] : S[t] + P[t];
        for (int c = 0; c < f; ++c) b[c] = first ? bs[(size_t)c] : b[c] + bs[(size_t)c];
        first = false;
    }
    for (int r = 0; r < f; ++r)
        for (int c = 0; c <= r; ++c) {
            volatile double v = G[(size_t)r * f + c] + S[(size_t)r * f + c];
            if (r == c) v = v + LAM;
            A[(size_t)r * f + c] = v;
            A[(size_t)c * f + r] = v;
        }
}

// float64 column Cholesky + two substitutions; false: a pivot is not positive
static bool solve_f64(const double* A, const double* b, int f, double* x)
{
    std::vector<double> L((size_t)f * f, 0.0);
    for (int j = 0; j < f; ++j) {
        double d = A[(size_t)j * f + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * f + k] * L[(size_t)j * f + k];
        if (!(d > 0.0)) return false;
        const double ljj = sqrt(d);
        L[(size_t)j * f + j] = ljj;
        for (int i = j + 1; i < f; ++i) {
            double s = A[(size_t)i * f + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * f + k] * L[(size_t)j * f + k];
            L[(size_t)i * f + j] = s / ljj;
        }
    }
    std::vector<double> z((size_t)f);
    for (int i = 0; i < f; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[(size_t)i * f + k] * z[(size_t)k];
        z[(size_t)i] = s / L[(size_t)i * f + i];
    }
    for (int i = f - 1; i >= 0; --i) {
        double s = z[(size_t)i];
        for (int k = i + 1; k < f; ++k) s -= L[(size_t)k * f + i] * x[k];
        x[i] = s / L[(size_t)i * f + i];
    }
    return true;
}

// ---- second formulation ---------------------------------------------------------------------------------------------------------------
static std::vector<double> gram_second(const std::vector<double>& Y, int64_t n, int f)
{
    std::vector<double> G((size_t)f * f);
    for (int r = 0; r < f; ++r)
        for (int c = 0; c < f; ++c) {
            long double s = 0.0L;
            for (int64_t k = n - 1; k >= 0; --k) s += (long double)Y[(size_t)k * f + r] * (long double)Y[(size_t)k * f + c];
            G[(size_t)r * f + c] = (double)s;
        }
    return G;
}

static void system_second(const HostCsr& x, int64_t u, const std::vector<double>& Y, int f, double* A, double* b, int64_t n_src)
{
    const int64_t beg = x.indptr[(size_t)u], end = x.indptr[(size_t)u + 1];
    for (int r = 0; r < f; ++r) {
        for (int c = 0; c < f; ++c) {
            long double s = 0.0L;
            for (int64_t k = n_src - 1; k >= 0; --k) s += (long double)Y[(size_t)k * f + r] * (long double)Y[(size_t)k * f + c];
            for (int64_t p = end - 1; p >= beg; --p) {
                const double* y = &Y[(size_t)x.indices[(size_t)p] * f];
                s += (long double)ALPHA * (long double)x.values[(size_t)p] * (long double)y[r] * (long double)y[c];
            }
            if (r == c) s += (long double)LAM;
            A[(size_t)r * f + c] = (double)s;
        }
        long double t = 0.0L;
        for (int64_t p = end - 1; p >= beg; --p)
            t += (1.0L + (long double)ALPHA * (long double)x.values[(size_t)p]) * (long double)Y[(size_t)x.indices[(size_t)p] * f + r];
        b[r] = (double)t;
    }
}

static bool solve_ld(const double* A, const double* b, int f, long double* x)
{
    std::vector<long double> L((size_t)f * f, 0.0L), z((size_t)f);
    for (int j = 0; j < f; ++j) {
        long double d = A[(size_t)j * f + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * f + k] * L[(size_t)j * f + k];
        if (!(d > 0.0L)) return false;
        const long double ljj = sqrtl(d);
        L[(size_t)j * f + j] = ljj;
        for (int i = j + 1; i < f; ++i) {
            long double s = A[(size_t)i * f + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * f + k] * L[(size_t)j * f + k];
            L[(size_t)i * f + j] = s / ljj;
        }
    }
    for (int i = 0; i < f; ++i) {
        long double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[(size_t)i * f + k] * z[(size_t)k];
        z[(size_t)i] = s / L[(size_t)i * f + i];
    }
    for (int i = f - 1; i >= 0; --i) {
        long double s = z[(size_t)i];
        for (int k = i + 1; k < f; ++k) s -= L[(size_t)k * f + i] * x[k];
        x[i] = s / L[(size_t)i * f + i];
    }
    return true;
}

// |got - want|_inf / |want|_inf
static double rel_inf(const double* got, const long double* want, int f)
{
    long double e = 0.0L, m = 0.0L;
    for (int i = 0; i < f; ++i) {
        e = std::max(e, fabsl((long double)got[i] - want[i]));
        m = std::max(m, fabsl(want[i]));
    }
    return m > 0.0L ? (double)(e / m) : (double)e;
}

// ---- cases ----------------------------------------------------------------------------------------------------------------------------
struct Case {
    const char* name;
    int64_t U;
    int I, f;
    double density;
    bool long_row;
    uint32_t seed;
};
static std::vector<Case> make_cases()
{
    return {
        {"67 x 45 x 24", 67, 45, 24, 0.15, false, 101u},
        {"130 x 77 x 128", 130, 77, 128, 0.15, false, 102u},
        {"40 x 300 x 17 (density 0.05: items without a user)", 40, 300, 17, 0.05, false, 103u},
        {"67 x 45 x 1", 67, 45, 1, 0.15, false, 101u},
        {"67 x 45 x 16", 67, 45, 16, 0.15, false, 101u},
        {"long row: (3 SEG + 5) x 8 x 24, item 0 rated by everybody", 3 * (int64_t)SEG + 5, 8, 24, 0.2, true, 104u},
    };
}

// one side of a case: the rows of x against the factor table Y (x.n_cols rows)
struct Side {
    std::string name;
    const HostCsr* x;
    const std::vector<double>* Y;
};

static bool same_bits(const double* a, const double* b, size_t n) { return memcmp(a, b, 8 * n) == 0; }

// --host
static void host_side(const Side& s, int f)
{
    const HostCsr& x = *s.x;
    const std::vector<double>& Y = *s.Y;
    Line LG, LS, LX;
    g_tag = s.name;
    const std::vector<double> G = gram_mirror(Y, x.n_cols, f), G2 = gram_second(Y, x.n_cols, f);
    if (!same_bits(G.data(), G2.data(), G.size())) host_fail(LG, "the chunked fma Gram matrix and the long-double one differ");
    report("host: Gram matrix, mirror = second: " + s.name, LG);
    std::vector<double> A((size_t)f * f), b((size_t)f), A2((size_t)f * f), b2((size_t)f), xm((size_t)f);
    const int64_t step = x.n_rows > 400 ? 97 : 1;   // (the long case: every 97th row, and its transposed side is 8 rows)
    for (int64_t u = 0; u < x.n_rows; u += step) {
        system_mirror(x, u, Y, f, G, A.data(), b.data());
        system_second(x, u, Y, f, A2.data(), b2.data(), x.n_cols);
        if (!same_bits(A.data(), A2.data(), A.size())) host_fail(LS, "A of row %.0f: mirror and second differ", (double)u);
        if (!same_bits(b.data(), b2.data(), b.size())) host_fail(LS, "b of row %.0f: mirror and second differ", (double)u);
        for (int r = 0; r < f; ++r)
            for (int c = 0; c < r; ++c)
                if (d_bits(A[(size_t)r * f + c]) != d_bits(A[(size_t)c * f + r])) host_fail(LS, "A of row %.0f is not symmetric", (double)u);
        if (!solve_f64(A.data(), b.data(), f, xm.data())) { host_fail(LX, "row %.0f: not positive definite", (double)u); continue; }
        // residual in long double against (3 f + 1) u (|A|_inf |x|_inf + |b|_inf), u = 2^-53 (Higham, Cholesky solve, first order), doubled
        long double res = 0.0L, an = 0.0L, xn = 0.0L, bn = 0.0L;
        for (int r = 0; r < f; ++r) {
            long double t = -(long double)b[(size_t)r], row = 0.0L;
            for (int c = 0; c < f; ++c) { t += (long double)A[(size_t)r * f + c] * xm[(size_t)c]; row += fabsl(A[(size_t)r * f + c]); }
            res = std::max(res, fabsl(t)); an = std::max(an, row);
            xn = std::max(xn, fabsl((long double)xm[(size_t)r])); bn = std::max(bn, fabsl((long double)b[(size_t)r]));
        }
        judge((double)res, 0.0, 2.0 * (3 * f + 1) * U53 * (double)(an * xn + bn), LX, "residual", (long)u);
    }
    report("host: systems, mirror = second, bit for bit: " + s.name, LS);
    report("host: float64 Cholesky solve, residual: " + s.name, LX);
}

static rtx_csr* upload(const HostCsr& x)
{
    rtx_csr* d = nullptr;
    RT(rtx_csr_upload(x.indptr.data(), x.indices.data(), x.values.data(), x.n_rows, x.n_cols, &d));
    return d;
}

static double g_worst_dev = 0, g_worst_mirror = 0;

// A, B on one side; returns the device's solve of every row (for D)
static std::vector<double> device_side(const Side& s, int f, rtx_csr* dx)
{
    const HostCsr& x = *s.x;
    const std::vector<double>& Y = *s.Y;
    const int64_t n = x.n_rows;
    const size_t mark = pool_size();
    g_tag = s.name;
    const std::vector<double> G = gram_mirror(Y, x.n_cols, f);
    std::vector<double> A((size_t)n * f * f), b((size_t)n * f);
    for (int64_t u = 0; u < n; ++u) system_mirror(x, u, Y, f, G, &A[(size_t)u * f * f], &b[(size_t)u * f]);
    double* dY = to_dev(Y);
    // ---- A: all rows
    {
        Line L;
        double* dA = dev_out<double>((size_t)n * f * f);
        double* db = dev_out<double>((size_t)n * f);
        RT(rtx_wmf_systems(dx, nullptr, (int32_t)n, dY, f, ALPHA, LAM, dA, db, 0));
        const std::vector<double> gA = fetch<double>(dA, (size_t)n * f * f, L, "A"), gb = fetch<double>(db, (size_t)n * f, L, "b");
        for (int64_t u = 0; u < n; ++u) {
            const double* ga = &gA[(size_t)u * f * f];
            if (!same_bits(ga, &A[(size_t)u * f * f], (size_t)f * f)) {
                for (int t = 0; t < f * f; ++t)
                    if (d_bits(ga[t]) != d_bits(A[(size_t)u * f * f + t])) { judge(ga[t], A[(size_t)u * f * f + t], 0.0, L, "A", (long)u, t); break; }
            }
            if (!same_bits(&gb[(size_t)u * f], &b[(size_t)u * f], (size_t)f)) host_fail(L, "b of row %.0f differs from the mirror", (double)u);
            for (int r = 0; r < f; ++r)
                for (int c = 0; c < r; ++c)
                    if (d_bits(ga[(size_t)r * f + c]) != d_bits(ga[(size_t)c * f + r])) host_fail(L, "A of row %.0f is not symmetric", (double)u);
        }
        report("systems, all rows, bit for bit: " + s.name, L);
    }
    // ---- A: a subset through row_ids, in descending order
    {
        Line L;
        std::vector<int32_t> ids;
        for (int64_t u = n - 1; u >= 0; u -= (n > 400 ? 501 : 3)) ids.push_back((int32_t)u);
        const int nb = (int)ids.size();
        int32_t* dids = to_dev(ids);
        double* dA = dev_out<double>((size_t)nb * f * f);
        double* db = dev_out<double>((size_t)nb * f);
        RT(rtx_wmf_systems(dx, dids, nb, dY, f, ALPHA, LAM, dA, db, 0));
        const std::vector<double> gA = fetch<double>(dA, (size_t)nb * f * f, L, "A"), gb = fetch<double>(db, (size_t)nb * f, L, "b");
        for (int q = 0; q < nb; ++q) {
            if (!same_bits(&gA[(size_t)q * f * f], &A[(size_t)ids[(size_t)q] * f * f], (size_t)f * f)) host_fail(L, "A at position %.0f differs", q);
            if (!same_bits(&gb[(size_t)q * f], &b[(size_t)ids[(size_t)q] * f], (size_t)f)) host_fail(L, "b at position %.0f differs", q);
        }
        report("systems, row_ids subset, bit for bit: " + s.name, L);
    }
    // ---- B: the solves
    std::vector<double> X;
    {
        Line L;
        double* dX = dev_out<double>((size_t)n * f);
        RT(rtx_wmf_solve_rows(dx, nullptr, (int32_t)n, dY, x.n_cols, f, ALPHA, LAM, dX, 0));
        X = fetch<double>(dX, (size_t)n * f, L, "x");
        std::vector<long double> xl((size_t)f);
        std::vector<double> xm((size_t)f), err((size_t)n, 0.0);
        double mirror_worst = 0, dev_worst = 0;
        long empty = 0;
        for (int64_t u = 0; u < n; ++u) {
            if (x.indptr[(size_t)u + 1] == x.indptr[(size_t)u]) {
                ++empty;
                for (int c = 0; c < f; ++c)
                    if (d_bits(X[(size_t)u * f + c]) != 0) host_fail(L, "the empty row %.0f did not get exact zeros", (double)u);
                continue;
            }
            if (!solve_ld(&A[(size_t)u * f * f], &b[(size_t)u * f], f, xl.data()) || !solve_f64(&A[(size_t)u * f * f], &b[(size_t)u * f], f, xm.data())) {
                host_fail(L, "row %.0f: the host's factorisation failed", (double)u);
                continue;
            }
            mirror_worst = std::max(mirror_worst, rel_inf(xm.data(), xl.data(), f));
            err[(size_t)u] = rel_inf(&X[(size_t)u * f], xl.data(), f);
            if (!(err[(size_t)u] == err[(size_t)u])) err[(size_t)u] = INFINITY;
            dev_worst = std::max(dev_worst, err[(size_t)u]);
        }
        const double bound = std::max(4.0 * mirror_worst, f * 2.0 * U53);
        for (int64_t u = 0; u < n; ++u) judge(err[(size_t)u], 0.0, bound, L, "relative error of x", (long)u);
        if (strstr(s.name.c_str(), "items without a user") && strstr(s.name.c_str(), "item side") && empty == 0)
            host_fail(L, "the case was built to hold empty rows and holds none");
        printf("wmf_ulp: %-78s device %.3e  mirror %.3e  bound %.3e  (empty rows: %ld)\n", s.name.c_str(), dev_worst, mirror_worst, bound, empty);
        g_worst_dev = std::max(g_worst_dev, dev_worst);
        g_worst_mirror = std::max(g_worst_mirror, mirror_worst);
        report("solve_rows against the long-double solve: " + s.name, L);
    }
    free_from(mark);
    return X;
}

// C.  Without `mask` the rows of x themselves mask, random rows of it for random users; with one, its row (4 q + 1) mod n_rows masks user q
// -- a permutation where n_rows is odd -- and its stored zeros must not mask.
static void scores_case(const char* name, const HostCsr& x, rtx_csr* dx, const std::vector<double>& Y, int f, bool generic, uint32_t seed,
                        const HostCsr* mask = nullptr)
{
    const size_t mark = pool_size();
    g_tag = name;
    Line L;
    const int I = x.n_cols;
    rtx_wmf* h = nullptr;
    RT(rtx_wmf_load(I, f, ALPHA, LAM, Y.data(), &h));
    int32_t nu = -1, ni = 0, ff = 0;
    RT(rtx_wmf_shape(h, &nu, &ni, &ff));
    if (nu != 0 || ni != I || ff != f) host_fail(L, "shape of a loaded model");
    Rng r{seed};
    const HostCsr& m = mask ? *mask : x;
    rtx_csr* dm = mask ? upload(m) : dx;
    const int nb = (int)(mask ? m.n_rows : std::min<int64_t>(x.n_rows, 21));
    std::vector<int32_t> ids((size_t)nb), mids((size_t)nb);
    for (int q = 0; q < nb; ++q) { ids[(size_t)q] = r.below((int)x.n_rows); mids[(size_t)q] = mask ? (4 * q + 1) % nb : r.below((int)x.n_rows); }
    int32_t *dids = to_dev(ids), *dmids = to_dev(mids);
    double* dY = to_dev(Y);
    double* dX = dev_out<double>((size_t)nb * f);
    RT(rtx_wmf_solve_rows(dx, dids, nb, dY, I, f, ALPHA, LAM, dX, 0));
    const std::vector<double> X = fetch<double>(dX, (size_t)nb * f, L, "x");
    const int64_t ld = I + 3;
    double* dS = dev_out<double>((size_t)nb * ld);
    RT(rtx_wmf_scores(h, dx, dids, nb, dm, dmids, dS, ld, 0));
    CK(hipDeviceSynchronize());
    const std::vector<double> S = fetch<double>(dS, (size_t)nb * ld, L, "scores");
    const double gam = f * U53 / (1.0 - f * U53);
    for (int q = 0; q < nb; ++q) {
        std::vector<char> masked((size_t)I, 0);
        for (int64_t p = m.indptr[(size_t)mids[(size_t)q]]; p < m.indptr[(size_t)mids[(size_t)q] + 1]; ++p)
            if (m.values[(size_t)p] != 0.f) masked[(size_t)m.indices[(size_t)p]] = 1;
        for (int j = 0; j < I; ++j) {
            const double got = S[(size_t)q * ld + j];
            if (masked[(size_t)j]) {
                if (!(got == -INFINITY)) host_fail(L, "a masked entry is not -inf (user %.0f, item %.0f)", q, j);
                continue;
            }
            double acc = 0.0;
            long double exact = 0.0L, mag = 0.0L;
            for (int k = 0; k < f; ++k) {
                acc = std::fma(X[(size_t)q * f + k], Y[(size_t)j * f + k], acc);
                const long double t = (long double)X[(size_t)q * f + k] * (long double)Y[(size_t)j * f + k];
                exact += t; mag += fabsl(t);
            }
            if (d_bits(got) != d_bits(acc)) judge(got, acc, 0.0, L, "score", q, j);
            if (generic) judge(got, (double)exact, gam * (double)mag + 1e-300, L, "score against the long-double dot product", q, j);
        }
        for (int j = I; j < ld; ++j)
            if (!is_poison(S[(size_t)q * ld + j])) host_fail(L, "the columns beyond n_items were written (user %.0f)", q);
    }
    RT(rtx_wmf_destroy(h));
    if (mask) RT(rtx_csr_destroy(dm));
    report(std::string("scores: ") + name, L);
    free_from(mark);
}

// C at the edge of the -inf tail: one block of 256 columns plus three, nine users (one more than a workgroup scores), a mask with stored
// entries in the first and the last column of the first block, the first column of the second block and the last column, and a stored zero
static void mask_tail_case()
{
    const int I = 256 + 3, f = 17;
    const HostCsr x = make_ratings(12, I, 0.1, false, 105u);
    HostCsr m;
    m.n_rows = 9; m.n_cols = I;
    m.indptr.push_back(0);
    for (int u = 0; u < 9; ++u) {
        for (int j : {0, 7, 255, 256, I - 1}) { m.indices.push_back(j); m.values.push_back(j == 7 ? 0.f : (float)(1 + u)); }
        m.indptr.push_back((int64_t)m.indices.size());
    }
    rtx_csr* dx = upload(x);
    scores_case("mask tail: 259 items, 9 users, mask at columns 0, 255, 256, 258, a stored zero, permuted mask rows", x, dx,
                generic_factors(I, f, 106u), f, true, 107u, &m);
    RT(rtx_csr_destroy(dx));
}

// D
static void fit_case(const char* name, const HostCsr& x, const HostCsr& xt, rtx_csr* dx, rtx_csr* dxt, const std::vector<double>& Y0, int f)
{
    const size_t mark = pool_size();
    g_tag = name;
    Line L;
    const int64_t U = x.n_rows;
    const int I = x.n_cols;
    double* dY0 = to_dev(Y0);
    double* dU = dev_out<double>((size_t)U * f);
    double* dY1 = dev_out<double>((size_t)I * f);
    RT(rtx_wmf_solve_rows(dx, nullptr, (int32_t)U, dY0, I, f, ALPHA, LAM, dU, 0));
    RT(rtx_wmf_solve_rows(dxt, nullptr, I, dU, (int32_t)U, f, ALPHA, LAM, dY1, 0));
    const std::vector<double> Uw = fetch<double>(dU, (size_t)U * f, L, "U"), Yw = fetch<double>(dY1, (size_t)I * f, L, "Y");
    rtx_wmf* h = nullptr;
    RT(rtx_wmf_fit(dx, dxt, f, ALPHA, LAM, 1, Y0.data(), &h, 0));
    int32_t nu = 0, ni = 0, ff = 0;
    RT(rtx_wmf_shape(h, &nu, &ni, &ff));
    if (nu != U || ni != I || ff != f) host_fail(L, "shape of a fitted model");
    double* gU = dev_out<double>((size_t)U * f);
    double* gY = dev_out<double>((size_t)I * f);
    RT(rtx_wmf_copy(h, RTX_WMF_USERS, gU, 0));
    RT(rtx_wmf_copy(h, RTX_WMF_ITEMS, gY, 0));
    CK(hipDeviceSynchronize());
    const std::vector<double> Ug = fetch<double>(gU, (size_t)U * f, L, "user factors"), Yg = fetch<double>(gY, (size_t)I * f, L, "item factors");
    if (!same_bits(Ug.data(), Uw.data(), Ug.size())) host_fail(L, "the user factors of one iteration differ from the user half-sweep");
    if (!same_bits(Yg.data(), Yw.data(), Yg.size())) host_fail(L, "the item factors of one iteration differ from the item half-sweep");
    double t[4] = {-1, -1, -1, -1};
    RT(rtx_wmf_timings(h, &t[0], &t[1], &t[2], &t[3]));
    if (!(t[0] > 0 && t[1] > 0 && t[2] > 0 && t[3] > 0 && t[1] + t[2] + t[3] <= t[0] * 1.001 + 1e-3)) host_fail(L, "timings: fit %.3f ms, Gram %.3f ms", t[0], t[1]);
    RT(rtx_wmf_destroy(h));
    (void)xt;
    report(std::string("one iteration of the fit = two half-sweeps: ") + name, L);
    free_from(mark);
}

// E
static void refusal(const char* name, int rc, const char* needle, const void* handle_after)
{
    Line L;
    const char* msg = rtx_last_error_str();
    if (rc != RTX_EINVAL) host_fail(L, "returned %.0f, expected RTX_EINVAL", rc);
    if (!msg || !strstr(msg, needle)) host_fail(L, "the message does not hold the documented words");
    if (handle_after) host_fail(L, "the output handle was written");
    report(std::string("refusal: ") + name, L, (std::string("  [") + (msg ? msg : "") + "]").c_str());
}
static void refusals()
{
    const size_t mark = pool_size();
    g_tag = "refusals";
    const HostCsr x = make_ratings(30, 20, 0.2, false, 9u), xt = transpose(x);
    HostCsr xz = x;
    xz.values[3] = 0.f;
    HostCsr xn = x;
    xn.values[5] = -1.f;
    rtx_csr *dx = upload(x), *dxt = upload(xt), *dz = upload(xz), *dn = upload(xn);
    const int f = 8;
    const std::vector<double> Y = exact_factors(20, f, 5u);
    double* dY = to_dev(Y);
    double* dO = dev_out<double>(30 * f);
    double* dA = dev_out<double>(30 * f * f);
    rtx_wmf* h = nullptr;
    refusal("fit: lam = 0", rtx_wmf_fit(dx, dxt, f, ALPHA, 0.0, 2, Y.data(), &h, 0), "lam must be finite and > 0", h);
    refusal("fit: lam < 0", rtx_wmf_fit(dx, dxt, f, ALPHA, -1.0, 2, Y.data(), &h, 0), "lam must be finite and > 0", h);
    refusal("fit: alpha < 0", rtx_wmf_fit(dx, dxt, f, -0.5, LAM, 2, Y.data(), &h, 0), "alpha must be finite and >= 0", h);
    refusal("fit: f = 0", rtx_wmf_fit(dx, dxt, 0, ALPHA, LAM, 2, Y.data(), &h, 0), "f must be in [1, 128]", h);
    refusal("fit: f = 129", rtx_wmf_fit(dx, dxt, 129, ALPHA, LAM, 2, Y.data(), &h, 0), "f must be in [1, 128]", h);
    refusal("fit: a stored value of 0", rtx_wmf_fit(dz, dxt, f, ALPHA, LAM, 2, Y.data(), &h, 0), "stores a value <= 0", h);
    refusal("fit: the second matrix is not the transpose", rtx_wmf_fit(dx, dx, f, ALPHA, LAM, 2, Y.data(), &h, 0), "not the transpose", h);
    refusal("solve_rows: lam = 0", rtx_wmf_solve_rows(dx, nullptr, 30, dY, 20, f, ALPHA, 0.0, dO, 0), "lam must be finite and > 0", nullptr);
    refusal("solve_rows: f = 129", rtx_wmf_solve_rows(dx, nullptr, 30, dY, 20, 129, ALPHA, LAM, dO, 0), "f must be in [1, 128]", nullptr);
    refusal("solve_rows: a stored value of 0", rtx_wmf_solve_rows(dz, nullptr, 30, dY, 20, f, ALPHA, LAM, dO, 0), "stores a value <= 0", nullptr);
    refusal("solve_rows: a negative stored value", rtx_wmf_solve_rows(dn, nullptr, 30, dY, 20, f, ALPHA, LAM, dO, 0), "stores a value <= 0", nullptr);
    refusal("solve_rows: a factor table of another height", rtx_wmf_solve_rows(dx, nullptr, 30, dY, 19, f, ALPHA, LAM, dO, 0), "factor table has 19 rows", nullptr);
    refusal("systems: f = 0", rtx_wmf_systems(dx, nullptr, 30, dY, 0, ALPHA, LAM, dA, dO, 0), "f must be in [1, 128]", nullptr);
    refusal("systems: a stored value of 0", rtx_wmf_systems(dz, nullptr, 30, dY, f, ALPHA, LAM, dA, dO, 0), "stores a value <= 0", nullptr);
    refusal("load: lam = 0", rtx_wmf_load(20, f, ALPHA, 0.0, Y.data(), &h), "lam must be finite and > 0", h);
    {
        CK(hipDeviceSynchronize());
        Line L;
        const std::vector<double> o = fetch<double>(dO, 30 * f, L, "out"), a = fetch<double>(dA, 30 * f * f, L, "A");
        for (double v : o)
            if (!is_poison(v)) { host_fail(L, "a refused call wrote its output"); break; }
        for (double v : a)
            if (!is_poison(v)) { host_fail(L, "a refused call wrote A"); break; }
        report("refusal: the refused calls wrote nothing", L);
    }
    // the status word: factors that are not finite leave no positive pivot
    std::vector<double> Yn = Y;
    Yn[(size_t)x.indices[0] * f + 2] = NAN;
    double* dYn = to_dev(Yn);
    refusal("solve_rows: not positive definite (a NaN factor)", rtx_wmf_solve_rows(dx, nullptr, 30, dYn, 20, f, ALPHA, LAM, dO, 0), "not positive definite", nullptr);
    refusal("fit: not positive definite (a NaN factor)", rtx_wmf_fit(dx, dxt, f, ALPHA, LAM, 1, Yn.data(), &h, 0), "not positive definite", h);
    RT(rtx_csr_destroy(dx)); RT(rtx_csr_destroy(dxt)); RT(rtx_csr_destroy(dz)); RT(rtx_csr_destroy(dn));
    free_from(mark);
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    if (argc > 1) { printf("usage: test_wmf [--host]\n"); return 2; }
    g_name_width = 100;
    for (const Case& c : make_cases()) {
        const HostCsr x = make_ratings(c.U, c.I, c.density, c.long_row, c.seed), xt = transpose(x);
        const std::vector<double> Yi = exact_factors(c.I, c.f, c.seed * 7u + 1u), Yu = exact_factors(c.U, c.f, c.seed * 7u + 2u);
        const Side user{std::string(c.name) + ", user side", &x, &Yi}, item{std::string(c.name) + ", item side", &xt, &Yu};
        int64_t longest_u = 0, longest_i = 0, long_rows = 0, empty_items = 0;
        for (int64_t u = 0; u < x.n_rows; ++u) longest_u = std::max(longest_u, x.indptr[(size_t)u + 1] - x.indptr[(size_t)u]);
        for (int64_t i = 0; i < xt.n_rows; ++i) {
            const int64_t len = xt.indptr[(size_t)i + 1] - xt.indptr[(size_t)i];
            longest_i = std::max(longest_i, len);
            long_rows += len > SEG;
            empty_items += len == 0;
        }
        {
            Line L;
            g_tag = c.name;
            if (c.long_row && !(long_rows == 1 && longest_i == 3 * (int64_t)SEG + 5 && longest_u <= SEG))
                host_fail(L, "the long-row case must hold exactly one segmented row (found %.0f) with a ragged last segment", (double)long_rows);
            if (!c.long_row && (longest_i > SEG || longest_u > SEG)) host_fail(L, "an unexpected long row");
            if (c.I == 300 && empty_items < 12) host_fail(L, "the sparse case holds %.0f items without a user, expected dozens", (double)empty_items);
            report(std::string("shape of the case: ") + c.name, L);
        }
        if (g_host) {
            host_side(user, c.f);
            host_side(item, c.f);
            continue;
        }
        rtx_csr *dx = upload(x), *dxt = upload(xt);
        device_side(user, c.f, dx);
        device_side(item, c.f, dxt);
        scores_case((std::string(c.name) + ", exact factors").c_str(), x, dx, Yi, c.f, false, c.seed + 11u);
        scores_case((std::string(c.name) + ", generic factors").c_str(), x, dx, generic_factors(c.I, c.f, c.seed + 5u), c.f, true, c.seed + 12u);
        fit_case(c.name, x, xt, dx, dxt, Yi, c.f);
        RT(rtx_csr_destroy(dx));
        RT(rtx_csr_destroy(dxt));
    }
    if (!g_host) {
        mask_tail_case();
        refusals();
        printf("largest relative error of a solve against the long-double solve: device %.3e, float64 column Cholesky %.3e\n", g_worst_dev, g_worst_mirror);
        free_all();
    }
    return finish("WMF");
}
