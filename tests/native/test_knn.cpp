// test_knn -- the item-kNN stack of knn.hip (rtx_knn_similarity, rtx_knn_fit, rtx_knn_load / copy, rtx_knn_scores) through the C ABI of the
// built library, on the harness of check.h.
//
// Two host formulations of the model (include/rectorch_hip.h has the definition), both float64:
//   mirror   what the device does: S as a matrix; per row j the ranked list -> threshold (tau.value, tau.id) and d_j; W by source item
//            from the threshold rule on S_ij; scores by std::fma over the user's stored entries in stored order.
//   brute    the definition, dense and literal: per j the candidates i != j with G_ij > 0, S_ij computed scalar by scalar, a stable sort
//            by (similarity descending, id ascending), the first k are N_k(j); a dense W with a presence matrix; scores by a triple loop.
// `test_knn --host` checks mirror against brute on every generated case and makes no HIP call.  Without an argument:
//   A  rtx_knn_similarity against the mirror's S from the host's G.  jaccard: bit for bit (integers, one division).  cosine: within
//      COS_ULPS units in the last place, derived -- not measured: with u = 2^-53, the device's double sqrt is documented to 1 ulp
//      (relative 2u), the host's is correctly rounded (u): 2 (2u + u) = 6u on the product of the two roots, + 2u for the product's two
//      roundings (device, host), + 2u for the two sums with shrink (an exact non-negative addend does not raise a relative error),
//      + 2u for the two divisions: 12u relative; a relative error r is at most r / u ulps: 12, and 1 for the second-order terms: 13.
//      On the float64 Gram route (non-dyadic ratings) G itself is a sum of U exactly representable products rounded once per term in
//      the device's order, and the host's G (summed in long double, rounded once) is within u: (U + 1) u on the numerator and
//      (U + 1) u / 2 on each root: 2 (U + 1) more ulps there.  The largest observed distance is printed.  S must be symmetric to the bit.
//   B  the fit: indptr, indices and values bit-equal to the mirror run on the DEVICE's own S (so a last-ulp difference in a cosine
//      excuses nothing and no case is left out); normalised values bit-equal to the division by the list-order sum.
//   C  rtx_knn_scores bit for bit against the std::fma loop: without row_ids, with them, with mask + mask_row_ids (zero-valued mask
//      entries do not mask); an empty user gives zeros; -inf exactly at the mask entries; guard scan around every output.
//      The kernel's -inf tail at its edge: n = one column block + 3, mask entries at the block's first and last column, the next block's
//      first and the last column, permuted row numbers.
//   D  rtx_knn_copy -> rtx_knn_load -> the same score bits; loaded models at the scoring kernel's column-block edges.
//   E  every refusal returns RTX_EINVAL with a message and leaves its output alone.
#include "../../include/rectorch_hip.h"
#include "../../rectorch_amd/csrc/rtx_common.h"
#include "check.h"

#include <limits.h>
#include <cmath>

static const int COS_ULPS = 13;
static const int BLOCK_COLS = 4096;   // RTX_KNN_BLOCK_COLS of knn.hip

enum { R_BINARY = 0, R_HALF = 1, R_STEP03 = 2 };
static const char* route_name(int r) { return r == R_BINARY ? "binary" : r == R_HALF ? "half-star" : "0.3-step"; }

struct HostCsr {
    int n = 0;
    long U = 0;
    bool binary = true;
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<float> values;
    double val(int64_t p) const { return binary ? 1.0 : (double)values[p]; }
};

// users x n items.  Every 7th user is empty; item 1 is an empty column (n >= 6); item n - 2 co-occurs with nothing (user 0 holds it
// alone, n >= 6); items n / 2 and n - 1 are copies of item 0 (n >= 6): exact ties across ids.
static HostCsr make_csr(int route, int n, long U, uint32_t seed)
{
    HostCsr x;
    Rng r{seed};
    x.n = n; x.U = U; x.binary = route == R_BINARY;
    const bool special = n >= 6;
    const int emp = 1, iso = n - 2, d1 = n / 2, d2 = n - 1;
    const int dens = std::max(2, std::min(n, 6 + n / 16));   // expected entries per user
    x.indptr.push_back(0);
    for (long u = 0; u < U; ++u) {
        std::vector<float> row(n, 0.f);
        if (u % 7 != 3) {
            for (int i = 0; i < n; ++i)
                if (r.below(n) < dens) row[i] = route == R_BINARY ? 1.f : route == R_HALF ? 0.5f * r.i(1, 10) : 0.3f * r.i(1, 10);
            if (special) {
                row[emp] = 0.f; row[iso] = 0.f;
                row[d1] = row[0]; row[d2] = row[0];
                if (u == 0 && U > 1) { std::fill(row.begin(), row.end(), 0.f); row[iso] = route == R_BINARY ? 1.f : 1.5f; }
            }
        }
        for (int i = 0; i < n; ++i)
            if (row[i] != 0.f) { x.indices.push_back(i); x.values.push_back(row[i]); }
        x.indptr.push_back((int64_t)x.indices.size());
    }
    return x;
}

static std::vector<double> gram_host(const HostCsr& x)
{
    const int n = x.n;
    std::vector<long double> g((size_t)n * n, 0.0L);
    for (long u = 0; u < x.U; ++u)
        for (int64_t p = x.indptr[u]; p < x.indptr[u + 1]; ++p)
            for (int64_t q = x.indptr[u]; q < x.indptr[u + 1]; ++q)
                g[(size_t)x.indices[p] * n + x.indices[q]] += (long double)x.val(p) * (long double)x.val(q);
    std::vector<double> G((size_t)n * n);
    for (size_t t = 0; t < G.size(); ++t) G[t] = (double)g[t];
    return G;
}

static const double NEG_INF = -INFINITY;

// ---- mirror ---------------------------------------------------------------------------------------------------------------------------
static std::vector<double> sim_mirror(const std::vector<double>& G, int n, int sim, double shrink)
{
    std::vector<double> d(n), S((size_t)n * n);
    for (int i = 0; i < n; ++i) d[i] = sim == RTX_KNN_COSINE ? sqrt(G[(size_t)i * n + i]) : G[(size_t)i * n + i];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double g = G[(size_t)i * n + j];
            double s = NEG_INF;
            if (i != j && g > 0.0) {
                volatile double den;   // (volatile: every step rounded to double, no contraction)
                if (sim == RTX_KNN_COSINE) { den = d[i] * d[j]; den = den + shrink; }
                else { den = d[i] + d[j]; den = den - g; den = den + shrink; }
                s = g / den;
            }
            S[(size_t)i * n + j] = s;
        }
    return S;
}

struct HostW {
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<double> values;
};

static HostW fit_mirror(const std::vector<double>& S, int n, int k, int normalize)
{
    const int K = std::min(k, n);
    std::vector<double> tau_v(n), dsum(n);
    std::vector<int32_t> tau_id(n);
    std::vector<std::pair<double, int>> list;
    for (int j = 0; j < n; ++j) {
        list.clear();
        for (int i = 0; i < n; ++i) list.push_back({S[(size_t)j * n + i], i});
        std::partial_sort(list.begin(), list.begin() + K, list.end(),
                          [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first > b.first || (a.first == b.first && a.second < b.second); });
        const bool full = list[K - 1].first > NEG_INF;
        tau_v[j] = full ? list[K - 1].first : NEG_INF;
        tau_id[j] = full ? list[K - 1].second : INT_MAX;
        double d = 0.0;
        for (int t = 0; t < K && list[t].first > NEG_INF; ++t) d += list[t].first;
        dsum[j] = d;
    }
    HostW w;
    w.indptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            const double s = S[(size_t)i * n + j];
            if (s > NEG_INF && (s > tau_v[j] || (s == tau_v[j] && i <= tau_id[j]))) {
                w.indices.push_back(j);
                w.values.push_back(normalize ? s / dsum[j] : s);
            }
        }
        w.indptr.push_back((int64_t)w.indices.size());
    }
    return w;
}

// rows: the batch's user rows (empty: 0 .. U); mask rows = the same rows of `mask` (nullable)
static std::vector<double> scores_mirror(const HostW& w, const HostCsr& x, const std::vector<int32_t>& rows, const HostCsr* mask)
{
    const int n = x.n;
    const long B = rows.empty() ? x.U : (long)rows.size();
    std::vector<double> out((size_t)B * n, 0.0);
    for (long b = 0; b < B; ++b) {
        const long u = rows.empty() ? b : rows[b];
        double* o = out.data() + (size_t)b * n;
        for (int64_t e = x.indptr[u]; e < x.indptr[u + 1]; ++e) {
            const int i = x.indices[e];
            const double v = x.val(e);
            for (int64_t p = w.indptr[i]; p < w.indptr[i + 1]; ++p) o[w.indices[p]] = std::fma(v, w.values[p], o[w.indices[p]]);
        }
        if (mask)
            for (int64_t e = mask->indptr[u]; e < mask->indptr[u + 1]; ++e)
                if (mask->val(e) != 0.0) o[mask->indices[e]] = NEG_INF;
    }
    return out;
}

// ---- brute force ----------------------------------------------------------------------------------------------------------------------
struct Brute {
    std::vector<double> W;       // dense [n][n]
    std::vector<char> present;   // dense [n][n]
};
static Brute fit_brute(const std::vector<double>& G, int n, int sim, double shrink, int k, int normalize)
{
    Brute b;
    b.W.assign((size_t)n * n, 0.0);
    b.present.assign((size_t)n * n, 0);
    for (int j = 0; j < n; ++j) {
        std::vector<std::pair<double, int>> cand;
        for (int i = 0; i < n; ++i) {
            if (i == j || !(G[(size_t)i * n + j] > 0.0)) continue;
            const double gij = G[(size_t)i * n + j], gii = G[(size_t)i * n + i], gjj = G[(size_t)j * n + j];
            volatile double den;
            if (sim == RTX_KNN_COSINE) { den = sqrt(gii) * sqrt(gjj); den = den + shrink; }
            else { den = gii + gjj; den = den - gij; den = den + shrink; }
            cand.push_back({gij / den, i});
        }
        std::stable_sort(cand.begin(), cand.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& c) { return a.first > c.first; });
        if ((int)cand.size() > k) cand.resize(k);
        double d = 0.0;
        for (auto& c : cand) d += c.first;
        for (auto& c : cand) {
            b.W[(size_t)c.second * n + j] = normalize ? c.first / d : c.first;
            b.present[(size_t)c.second * n + j] = 1;
        }
    }
    return b;
}
static std::vector<double> scores_brute(const Brute& w, const HostCsr& x)
{
    const int n = x.n;
    std::vector<double> out((size_t)x.U * n, 0.0);
    for (long u = 0; u < x.U; ++u)
        for (int j = 0; j < n; ++j) {
            double acc = 0.0;
            for (int64_t e = x.indptr[u]; e < x.indptr[u + 1]; ++e) {
                const int i = x.indices[e];
                if (w.present[(size_t)i * n + j]) acc = std::fma(x.val(e), w.W[(size_t)i * n + j], acc);
            }
            out[(size_t)u * n + j] = acc;
        }
    return out;
}

static inline void judge_bits64(double got, double want, Line& L, const char* what, long i, long j = -1)
{
    if (d_bits(got) != d_bits(want)) {
        if (L.bad < 4) printf("    %s holds %.17g (%016llx), expected %.17g (%016llx)\n", where(what, i, j).c_str(), got,
                              (unsigned long long)d_bits(got), want, (unsigned long long)d_bits(want));
        ++L.bad;
    }
}
// distance in units in the last place between two finite doubles of one sign (the key of a monotone integer order)
static inline int64_t ulp_key(double v) { const int64_t b = (int64_t)d_bits(v); return b < 0 ? INT64_MIN - b : b; }
static inline double ulp_dist(double a, double b) { return fabs((double)(ulp_key(a) - ulp_key(b))); }

// ---- the cases ------------------------------------------------------------------------------------------------------------------------
struct Case {
    int n; long U; int k; int route; int sim; int normalize; double shrink;
};
static std::vector<Case> make_cases()
{
    std::vector<Case> cs;
    const int ns[] = {1, 2, 127, 128, 129, 257, 300};
    const long Us[] = {1, 127, 129, 1000};
    int t = 0;
    for (int n : ns) {
        std::vector<int> ks = {1, 3, n - 1, n, n + 5};
        std::sort(ks.begin(), ks.end());
        ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
        for (int k : ks) {
            if (k < 1) continue;
            for (int variant = 0; variant < 4; ++variant, ++t) {
                // variants: binary cosine, binary jaccard, half-star cosine, 0.3-step cosine; users, normalize and shrink rotate
                Case c;
                c.n = n; c.k = k; c.U = Us[(t / 4 + variant) % 4];
                c.route = variant <= 1 ? R_BINARY : variant == 2 ? R_HALF : R_STEP03;
                c.sim = variant == 1 ? RTX_KNN_JACCARD : RTX_KNN_COSINE;
                c.normalize = (t / 2) & 1;
                c.shrink = (t % 3 == 0) ? 0.0 : (t % 3 == 1) ? 10.0 : 0.3;
                cs.push_back(c);
            }
        }
    }
    // every user count on every route at one size
    for (long U : Us)
        for (int route : {R_BINARY, R_HALF, R_STEP03})
            for (int sim : {RTX_KNN_COSINE, RTX_KNN_JACCARD}) {
                if (sim == RTX_KNN_JACCARD && route != R_BINARY) continue;
                cs.push_back(Case{129, U, 3, route, sim, (int)(U & 1), 0.0});
            }
    cs.push_back(Case{1100, 129, 1024, R_BINARY, RTX_KNN_COSINE, 1, 0.0});   // the selection's largest k
    return cs;
}
static std::string case_name(const Case& c)
{
    char buf[160];
    snprintf(buf, sizeof buf, "n=%d U=%ld k=%d %s %s%s shrink=%g", c.n, c.U, c.k, route_name(c.route), c.sim == RTX_KNN_COSINE ? "cosine" : "jaccard",
             c.normalize ? " normalized" : "", c.shrink);
    return buf;
}

static void host_case(const Case& c, uint32_t seed)
{
    const HostCsr x = make_csr(c.route, c.n, c.U, seed);
    const std::vector<double> G = gram_host(x);
    const std::vector<double> S = sim_mirror(G, c.n, c.sim, c.shrink);
    const HostW w = fit_mirror(S, c.n, c.k, c.normalize);
    const Brute b = fit_brute(G, c.n, c.sim, c.shrink, c.k, c.normalize);
    Line L;
    g_tag = case_name(c);
    // S symmetric to the bit
    for (int i = 0; i < c.n; ++i)
        for (int j = 0; j < i; ++j) judge_bits64(S[(size_t)i * c.n + j], S[(size_t)j * c.n + i], L, "S", i, j);
    // W: the same entries, the same bits
    long nnz_b = 0;
    for (char p : b.present) nnz_b += p;
    if (nnz_b != (long)w.indices.size()) host_fail(L, "the mirror's W holds %.0f entries, the brute force %.0f", (double)w.indices.size(), (double)nnz_b);
    for (int i = 0; i < c.n; ++i)
        for (int64_t p = w.indptr[i]; p < w.indptr[i + 1]; ++p) {
            const int j = w.indices[p];
            if (p > w.indptr[i] && w.indices[p - 1] >= j) host_fail(L, "row %.0f of the mirror's W is not ascending", i);
            if (!b.present[(size_t)i * c.n + j]) host_fail(L, "the mirror keeps W[%.0f][%.0f], the brute force does not", i, j);
            else judge_bits64(w.values[p], b.W[(size_t)i * c.n + j], L, "W", i, j);
        }
    const std::vector<double> sm = scores_mirror(w, x, {}, nullptr), sb = scores_brute(b, x);
    for (size_t t = 0; t < sm.size(); ++t) judge_bits64(sm[t], sb[t], L, "scores", (long)(t / c.n), (long)(t % c.n));
    report("host: " + case_name(c), L);
}

// ---- device side ----------------------------------------------------------------------------------------------------------------------
static rtx_csr* upload(const HostCsr& x)
{
    rtx_csr* h = nullptr;
    RT(rtx_csr_upload(x.indptr.data(), x.indices.data(), x.binary ? nullptr : x.values.data(), x.U, x.n, &h));
    return h;
}

static HostW copy_w(const rtx_knn* h, Line& L)
{
    int32_t n = 0;
    int64_t nnz = 0;
    RT(rtx_knn_shape(h, &n, &nnz));
    int64_t* dp = dev_out<int64_t>((size_t)n + 1);
    int32_t* di = dev_out<int32_t>((size_t)nnz);
    double* dv = dev_out<double>((size_t)nnz);
    RT(rtx_knn_copy(h, dp, di, dv, 0));
    CK(hipDeviceSynchronize());
    HostW w;
    w.indptr = fetch<int64_t>(dp, (size_t)n + 1, L, "indptr");
    w.indices = fetch<int32_t>(di, (size_t)nnz, L, "indices");
    w.values = fetch<double>(dv, (size_t)nnz, L, "values");
    return w;
}

// the three calls of C on one model; returns the raw score bytes (for the load round trip)
static std::vector<unsigned char> check_scores(const rtx_knn* h, const HostW& w, const HostCsr& x, rtx_csr* dx, uint32_t seed, Line& L)
{
    const int n = x.n;
    std::vector<unsigned char> raw;
    // without row_ids
    {
        double* out = dev_out<double>((size_t)x.U * n);
        RT(rtx_knn_scores(h, dx, nullptr, (int32_t)x.U, nullptr, nullptr, out, 0));
        CK(hipDeviceSynchronize());
        const std::vector<double> got = fetch<double>(out, (size_t)x.U * n, L, "scores", &raw), want = scores_mirror(w, x, {}, nullptr);
        for (size_t t = 0; t < got.size(); ++t) judge_bits64(got[t], want[t], L, "scores", (long)(t / n), (long)(t % n));
    }
    // with row_ids (repeats, any order), then with a mask whose every third entry stores 0
    Rng r{seed};
    const int B = (int)std::min<long>(x.U + 3, 200);
    std::vector<int32_t> rows(B);
    for (auto& u : rows) u = r.below((int)x.U);
    if (x.U > 3) rows[0] = 3;   // an empty user
    HostCsr m = x;
    m.binary = false;
    m.values.resize(m.indices.size());
    for (size_t p = 0; p < m.values.size(); ++p) m.values[p] = (p % 3 == 2) ? 0.f : (float)x.val((int64_t)p);
    rtx_csr* dm = upload(m);
    int32_t* drows = to_dev(rows);
    for (int with_mask = 0; with_mask < 2; ++with_mask) {
        double* out = dev_out<double>((size_t)B * n);
        RT(rtx_knn_scores(h, dx, drows, B, with_mask ? dm : nullptr, with_mask ? drows : nullptr, out, 0));
        CK(hipDeviceSynchronize());
        const std::vector<double> got = fetch<double>(out, (size_t)B * n, L, with_mask ? "masked scores" : "row scores", &raw);
        const std::vector<double> want = scores_mirror(w, x, rows, with_mask ? &m : nullptr);
        for (size_t t = 0; t < got.size(); ++t) judge_bits64(got[t], want[t], L, with_mask ? "masked scores" : "row scores", (long)(t / n), (long)(t % n));
    }
    RT(rtx_csr_destroy(dm));
    return raw;
}

static double g_worst_ulp = 0, g_worst_ulp_f64route = 0;

static void device_case(const Case& c, uint32_t seed)
{
    const size_t mark = pool_size();
    const int n = c.n;
    const HostCsr x = make_csr(c.route, n, c.U, seed);
    rtx_csr* dx = upload(x);
    g_tag = case_name(c);
    // ---- A: the similarity
    Line LA;
    double* dS = dev_out<double>((size_t)n * n);
    RT(rtx_knn_similarity(dx, c.shrink, c.sim, dS, 0));
    CK(hipDeviceSynchronize());
    const std::vector<double> S = fetch<double>(dS, (size_t)n * n, LA, "S");
    const std::vector<double> Sh = sim_mirror(gram_host(x), n, c.sim, c.shrink);
    const double bound = c.sim == RTX_KNN_JACCARD ? 0.0 : COS_ULPS + (c.route == R_STEP03 ? 2.0 * (double)(c.U + 1) : 0.0);
    double worst = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double got = S[(size_t)i * n + j], want = Sh[(size_t)i * n + j];
            if (got != got || (got > NEG_INF) != (want > NEG_INF) || got == INFINITY) { judge_bits64(got, want, LA, "S", i, j); continue; }
            if (j < i) judge_bits64(got, S[(size_t)j * n + i], LA, "S against its mirror element", i, j);
            if (!(want > NEG_INF)) continue;
            const double dist = ulp_dist(got, want);
            worst = std::max(worst, dist);
            if (!(dist <= bound)) {
                if (LA.bad < 4) printf("    %s = %.17g, expected %.17g: %.0f ulps apart (bound %.0f)\n", where("S", i, j).c_str(), got, want, dist, bound);
                ++LA.bad;
            }
            if (bound > 0 && dist / bound > LA.worst) LA.worst = dist / bound;
        }
    double& slot = c.route == R_STEP03 ? g_worst_ulp_f64route : g_worst_ulp;
    if (c.sim == RTX_KNN_COSINE) slot = std::max(slot, worst);
    char extra[64];
    snprintf(extra, sizeof extra, "  [%.0f ulps of %.0f]", worst, bound);
    report("similarity: " + case_name(c), LA, extra);
    // ---- B: the fit against the mirror on the device's own S
    Line LB;
    rtx_knn* h = nullptr;
    RT(rtx_knn_fit(dx, c.k, c.shrink, c.sim, c.normalize, &h, 0));
    const HostW got = copy_w(h, LB), want = fit_mirror(S, n, c.k, c.normalize);
    if (got.indptr.size() != want.indptr.size() || got.indices.size() != want.indices.size())
        host_fail(LB, "W holds %.0f entries, expected %.0f", (double)got.indices.size(), (double)want.indices.size());
    else {
        for (size_t t = 0; t < got.indptr.size(); ++t)
            if (got.indptr[t] != want.indptr[t]) host_fail(LB, "indptr[%.0f] = %.0f", (double)t, (double)got.indptr[t]);
        for (size_t t = 0; t < got.indices.size(); ++t) {
            if (got.indices[t] != want.indices[t]) host_fail(LB, "indices[%.0f] = %.0f", (double)t, (double)got.indices[t]);
            judge_bits64(got.values[t], want.values[t], LB, "values", (long)t);
        }
    }
    double ms[4] = {-1, -1, -1, -1};
    RT(rtx_knn_timings(h, &ms[0], &ms[1], &ms[2], &ms[3]));
    if (!(ms[0] > 0 && ms[1] >= 0 && ms[2] >= 0 && ms[3] >= 0 && ms[1] + ms[2] + ms[3] <= ms[0] * 1.001 + 1e-3)) host_fail(LB, "timings: fit %.4f ms, Gram %.4f ms", ms[0], ms[1]);
    report("fit: " + case_name(c), LB);
    // ---- C, D: scores of the fitted model, then of its copy loaded back
    if (!LB.bad) {
        Line LC;
        const std::vector<unsigned char> raw = check_scores(h, got, x, dx, seed ^ 0x5bd1u, LC);
        report("scores: " + case_name(c), LC);
        Line LD;
        rtx_knn* h2 = nullptr;
        RT(rtx_knn_load(n, got.indptr.data(), got.indices.data(), got.values.data(), &h2));
        const HostW again = copy_w(h2, LD);
        if (again.indptr != got.indptr || again.indices != got.indices || memcmp(again.values.data(), got.values.data(), 8 * got.values.size()))
            host_fail(LD, "the loaded model's arrays differ from the ones it was loaded from");
        Line scratch;
        const std::vector<unsigned char> raw2 = check_scores(h2, got, x, dx, seed ^ 0x5bd1u, scratch);
        if (raw2 != raw) host_fail(LD, "the loaded model scores other bits than the fitted one");
        RT(rtx_knn_destroy(h2));
        report("load round trip: " + case_name(c), LD);
    }
    RT(rtx_knn_destroy(h));
    RT(rtx_csr_destroy(dx));
    free_from(mark);
}

// D: loaded models at the scoring kernel's column-block edges: a random W of ~24 entries per row (one long row, one empty row)
static void block_edge_case(int n, uint32_t seed)
{
    const size_t mark = pool_size();
    Rng r{seed};
    HostW w;
    w.indptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        const int want = i == 2 ? n : i == 3 ? 0 : 24;
        for (int j = 0; j < n; ++j)
            if (want == n || r.below(n) < want) { w.indices.push_back(j); w.values.push_back(r.f48()); }
        w.indptr.push_back((int64_t)w.indices.size());
    }
    const long U = 37;
    HostCsr x;
    x.n = n; x.U = U; x.binary = false;
    x.indptr.push_back(0);
    for (long u = 0; u < U; ++u) {
        if (u != 3)
            for (int i = 0; i < n; ++i)
                if (i == (int)u % 5 || r.below(n) < (u == 5 ? 150 : 40)) { x.indices.push_back(i); x.values.push_back(0.5f * r.i(1, 10)); }
        x.indptr.push_back((int64_t)x.indices.size());
    }
    char name[96];
    snprintf(name, sizeof name, "block edge: loaded W, n=%d (block width %d)", n, BLOCK_COLS);
    g_tag = name;
    Line L;
    rtx_csr* dx = upload(x);
    rtx_knn* h = nullptr;
    RT(rtx_knn_load(n, w.indptr.data(), w.indices.data(), w.values.data(), &h));
    check_scores(h, w, x, dx, seed, L);
    RT(rtx_knn_destroy(h));
    RT(rtx_csr_destroy(dx));
    report(name, L);
    free_from(mark);
}

// C at the edge of the -inf tail: one block of columns plus three, nine users, a mask with stored entries in the first and the last column
// of the first block, the first column of the second block and the last column, a stored zero (which must not mask), and a permutation
// as the row numbers of both matrices
static void mask_tail_case()
{
    const size_t mark = pool_size();
    const int n = BLOCK_COLS + 3, U = 9;
    Rng r{4099u};
    HostW w;
    w.indptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j)
            if (r.below(n) < 24) { w.indices.push_back(j); w.values.push_back(r.f48()); }
        w.indptr.push_back((int64_t)w.indices.size());
    }
    HostCsr x, m;
    x.n = m.n = n; x.U = m.U = U; x.binary = m.binary = false;
    x.indptr.push_back(0); m.indptr.push_back(0);
    for (int u = 0; u < U; ++u) {
        for (int i = 0; i < n; ++i)
            if (r.below(n) < 40) { x.indices.push_back(i); x.values.push_back(0.5f * r.i(1, 10)); }
        x.indptr.push_back((int64_t)x.indices.size());
        for (int j : {0, 7, BLOCK_COLS - 1, BLOCK_COLS, n - 1}) { m.indices.push_back(j); m.values.push_back(j == 7 ? 0.f : (float)(1 + u)); }
        m.indptr.push_back((int64_t)m.indices.size());
    }
    const std::vector<int32_t> rows = {4, 8, 3, 7, 2, 6, 1, 5, 0};
    g_tag = "mask tail";
    Line L;
    rtx_csr *dx = upload(x), *dm = upload(m);
    rtx_knn* h = nullptr;
    RT(rtx_knn_load(n, w.indptr.data(), w.indices.data(), w.values.data(), &h));
    int32_t* drows = to_dev(rows);
    double* out = dev_out<double>((size_t)U * n);
    RT(rtx_knn_scores(h, dx, drows, U, dm, drows, out, 0));
    CK(hipDeviceSynchronize());
    const std::vector<double> got = fetch<double>(out, (size_t)U * n, L, "masked scores"), want = scores_mirror(w, x, rows, &m);
    long ninf = 0;
    for (size_t t = 0; t < got.size(); ++t) {
        judge_bits64(got[t], want[t], L, "masked scores", (long)(t / n), (long)(t % n));
        ninf += want[t] == NEG_INF;
    }
    if (ninf != 4L * U) host_fail(L, "the mirror masks %.0f entries, expected four a user", (double)ninf);
    RT(rtx_knn_destroy(h));
    RT(rtx_csr_destroy(dx));
    RT(rtx_csr_destroy(dm));
    report("mask tail: n = block + 3, 9 users, mask at columns 0, block - 1, block, n - 1, a stored zero, permuted rows", L);
    free_from(mark);
}

// E
static void refusal(const char* name, int rc, const void* handle_after)
{
    Line L;
    const char* msg = rtx_last_error_str();
    if (rc != RTX_EINVAL) host_fail(L, "returned %.0f, expected RTX_EINVAL", rc);
    if (!msg || !msg[0]) host_fail(L, "no message");
    if (handle_after) host_fail(L, "the output handle was written");
    report(std::string("refusal: ") + name, L, rc == RTX_EINVAL ? (std::string("  [") + msg + "]").c_str() : "");
}
static void refusals()
{
    const size_t mark = pool_size();
    const HostCsr xb = make_csr(R_BINARY, 40, 30, 9u), xr = make_csr(R_HALF, 40, 30, 9u);
    rtx_csr *db = upload(xb), *dr = upload(xr);
    rtx_knn* h = nullptr;
    refusal("k = 0", rtx_knn_fit(db, 0, 0.0, RTX_KNN_COSINE, 0, &h, 0), h);
    refusal("k = 1025", rtx_knn_fit(db, 1025, 0.0, RTX_KNN_COSINE, 0, &h, 0), h);
    refusal("shrink < 0", rtx_knn_fit(db, 3, -1.0, RTX_KNN_COSINE, 0, &h, 0), h);
    refusal("shrink NaN", rtx_knn_fit(db, 3, NAN, RTX_KNN_COSINE, 0, &h, 0), h);
    refusal("shrink inf", rtx_knn_fit(db, 3, INFINITY, RTX_KNN_COSINE, 0, &h, 0), h);
    refusal("unknown similarity", rtx_knn_fit(db, 3, 0.0, 7, 0, &h, 0), h);
    refusal("jaccard on ratings", rtx_knn_fit(dr, 3, 0.0, RTX_KNN_JACCARD, 0, &h, 0), h);
    // the stand-alone operator: the same refusals, S untouched
    {
        double* dS = dev_out<double>(40 * 40);
        const int rc1 = rtx_knn_similarity(db, -2.0, RTX_KNN_COSINE, dS, 0);
        refusal("similarity: shrink < 0", rc1, nullptr);
        const int rc2 = rtx_knn_similarity(dr, 0.0, RTX_KNN_JACCARD, dS, 0);
        refusal("similarity: jaccard on ratings", rc2, nullptr);
        const int rc3 = rtx_knn_similarity(db, 0.0, 2, dS, 0);
        refusal("similarity: unknown similarity", rc3, nullptr);
        CK(hipDeviceSynchronize());
        Line L;
        const std::vector<double> s = fetch<double>(dS, 40 * 40, L, "S");
        for (size_t t = 0; t < s.size(); ++t)
            if (!is_poison(s[t])) { host_fail(L, "S[%.0f] was written by a refused call", (double)t); break; }
        report("refusal: the refused calls wrote nothing", L);
    }
    const int64_t ip[4] = {0, 2, 2, 3};
    const int32_t unsorted[3] = {2, 0, 1}, range[3] = {0, 3, 1}, dup[3] = {1, 1, 0}, neg[3] = {-1, 1, 0};
    const double vals[3] = {1, 2, 3};
    refusal("load: unsorted indices", rtx_knn_load(3, ip, unsorted, vals, &h), h);
    refusal("load: index out of range", rtx_knn_load(3, ip, range, vals, &h), h);
    refusal("load: repeated index", rtx_knn_load(3, ip, dup, vals, &h), h);
    refusal("load: negative index", rtx_knn_load(3, ip, neg, vals, &h), h);
    const int64_t ip_bad[4] = {0, 2, 1, 3};
    refusal("load: indptr decreases", rtx_knn_load(3, ip_bad, unsorted, vals, &h), h);
    RT(rtx_csr_destroy(db));
    RT(rtx_csr_destroy(dr));
    free_from(mark);
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    if (argc > 1) { printf("usage: test_knn [--host]\n"); return 2; }
    g_name_width = 86;
    const std::vector<Case> cases = make_cases();
    uint32_t seed = 1;
    for (const Case& c : cases) {
        seed = seed * 2654435761u + 12345u;
        if (g_host) {
            if (c.n <= 300) host_case(c, seed);   // (the brute force is cubic: the k = 1024 case runs against the mirror on the device only)
        } else device_case(c, seed);
    }
    if (!g_host) {
        for (int n : {BLOCK_COLS - 1, BLOCK_COLS, BLOCK_COLS + 1, 2 * BLOCK_COLS + 1}) block_edge_case(n, 77u + n);
        mask_tail_case();
        refusals();
        printf("largest cosine distance from the host: %.0f ulps on the exact Gram routes (bound %d), %.0f ulps on the float64 route (bound %d + 2 (U + 1))\n",
               g_worst_ulp, COS_ULPS, g_worst_ulp_f64route, COS_ULPS);
        free_all();
    }
    return finish("KNN");
}
