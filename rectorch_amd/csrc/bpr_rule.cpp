// BPRMF's batch rule and fold-in, host half: the float64 definition operation by operation, in plain host code (no HIP call), beside
// the integer definition of the triples in bpr_draw.cpp.  The contract is text in include/rectorch_hip.h ("BPRMF rule"); a device
// trainer has to give rtx_bpr_update_host's tables bit for bit when both are fed the same s_t.  Every product and sum below is rounded
// on its own: the pragma keeps the compiler from fusing any of them.
#include <math.h>
#include <stdint.h>
#include <vector>

#include "../../include/rectorch_hip.h"
#include "rtx_common.h"

#pragma clang fp contract(off)

namespace {

// c stored in the sorted indices [beg, end)?
bool stored(const int32_t* idx, int64_t beg, int64_t end, int32_t c)
{
    int64_t lo = beg, hi = end;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && idx[lo] == c;
}

// 1 / (1 + exp(a . (p - q))), the products added in ascending k from 0.0
double coefficient(const double* a, const double* p, const double* q, int f)
{
    double x = 0.0;
    for (int k = 0; k < f; ++k) x = x + a[k] * (p[k] - q[k]);
    return 1.0 / (1.0 + exp(x));
}

int check_rates(const char* who, int f, double lr, double reg)
{
    RTX_CHECK(f >= 1 && f <= RTX_BPR_MAX_FACTORS, RTX_EINVAL, "%s: f must be in [1, %d], got %d", who, RTX_BPR_MAX_FACTORS, f);
    RTX_CHECK(isfinite(lr) && lr > 0.0, RTX_EINVAL, "%s: lr must be finite and > 0, got %g", who, lr);
    RTX_CHECK(isfinite(reg) && reg >= 0.0, RTX_EINVAL, "%s: reg must be finite and >= 0, got %g", who, reg);
    return RTX_OK;
}

// theta + lr * (acc - (c * reg) * theta): five roundings
inline double moved(double theta, double acc, int64_t c, double lr, double reg)
{
    const double cr = (double)c * reg;
    const double p = cr * theta;
    const double q = acc - p;
    const double w = lr * q;
    return theta + w;
}

}  // namespace

int rtx_bpr_update_host(double* U, double* Y, int32_t n_users, int32_t n_items, int32_t f, const int32_t* u, const int32_t* i, const int32_t* j,
                        int64_t count, double lr, double reg, const double* s_in, double* s_out)
{
    RTX_CHECK(U && Y && (count == 0 || (u && i && j)), RTX_EINVAL, "bpr_update_host: NULL argument");
    RTX_TRY(check_rates("bpr_update_host", f, lr, reg));
    RTX_CHECK(n_users > 0 && n_items > 0, RTX_EINVAL, "bpr_update_host: tables of %d users and %d items: both must be >= 1", n_users, n_items);
    RTX_CHECK(count >= 0, RTX_EINVAL, "bpr_update_host: count must be >= 0, got %lld", (long long)count);
    for (int64_t t = 0; t < count; ++t)   // before anything is written
        RTX_CHECK(u[t] >= 0 && u[t] < n_users && i[t] >= 0 && i[t] < n_items && j[t] >= -1 && j[t] < n_items, RTX_EINVAL,
                  "bpr_update_host: sample %lld names a row outside the tables (u = %d, i = %d, j = %d): supported: 0 <= u < %d, 0 <= i < %d, "
                  "-1 <= j < %d (-1: skipped); nothing was written",
                  (long long)t, u[t], i[t], j[t], n_users, n_items, n_items);
    // one pass over the samples in ascending order, an accumulator and a count per row: a row's sum is in ascending sample order, and
    // sample t's positive role comes before its negative role
    std::vector<double> aU((size_t)n_users * f, 0.0), aY((size_t)n_items * f, 0.0);
    std::vector<int64_t> cU((size_t)n_users, 0), cY((size_t)n_items, 0);
    for (int64_t t = 0; t < count; ++t) {
        if (j[t] < 0) {
            if (s_out) s_out[t] = 0.0;
            continue;
        }
        const double* ur = U + (size_t)u[t] * f;
        const double* yi = Y + (size_t)i[t] * f;
        const double* yj = Y + (size_t)j[t] * f;
        const double s = s_in ? s_in[t] : coefficient(ur, yi, yj, f);
        if (s_out) s_out[t] = s;
        double* au = aU.data() + (size_t)u[t] * f;
        double* ai = aY.data() + (size_t)i[t] * f;
        double* aj = aY.data() + (size_t)j[t] * f;
        for (int k = 0; k < f; ++k) {
            const double d = yi[k] - yj[k];
            const double gu = s * d;
            const double gi = s * ur[k];
            au[k] = au[k] + gu;
            ai[k] = ai[k] + gi;
            aj[k] = aj[k] + (-gi);     // (i = j: the two roles of one row, in this order)
        }
        ++cU[u[t]]; ++cY[i[t]]; ++cY[j[t]];
    }
    // every gradient above was taken at the tables of the batch's start; now every touched row moves, once
    for (int32_t r = 0; r < n_users; ++r)
        if (cU[r])
            for (int k = 0; k < f; ++k) U[(size_t)r * f + k] = moved(U[(size_t)r * f + k], aU[(size_t)r * f + k], cU[r], lr, reg);
    for (int32_t r = 0; r < n_items; ++r)
        if (cY[r])
            for (int k = 0; k < f; ++k) Y[(size_t)r * f + k] = moved(Y[(size_t)r * f + k], aY[(size_t)r * f + k], cY[r], lr, reg);
    return RTX_OK;
}

int rtx_bpr_fold_in_host(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int32_t n_items, const double* Y, int32_t f, double lr,
                         double reg, int32_t fold_in_epochs, uint64_t seed, double* out)
{
    RTX_CHECK(indptr && Y && out, RTX_EINVAL, "bpr_fold_in_host: NULL argument");
    RTX_TRY(check_rates("bpr_fold_in_host", f, lr, reg));
    RTX_CHECK(fold_in_epochs >= 0, RTX_EINVAL, "bpr_fold_in_host: fold_in_epochs must be >= 0, got %d", fold_in_epochs);
    RTX_CHECK(n_rows >= 0 && n_rows <= INT32_MAX && n_items > 0, RTX_EINVAL, "bpr_fold_in_host: %lld rows and %d items: supported: rows in [0, 2^31), items in [1, 2^31)",
              (long long)n_rows, n_items);
    if (n_rows > 0 && indptr[n_rows] != 0) {   // the draws' rule
        RTX_CHECK(indices, RTX_EINVAL, "bpr_fold_in_host: NULL argument");
        RTX_TRY(rtx_bpr_check_rows_host(indptr, indices, n_rows, n_items));
    } else {                                   // a matrix without entries, which that check refuses as nothing to sample, folds in to zeros
        for (int64_t r = 0; r < n_rows; ++r)
            RTX_CHECK(indptr[r] == 0, RTX_EINVAL, "bpr_fold_in_host: indptr must be ascending from 0 to nnz = 0, got %lld at row %lld", (long long)indptr[r],
                      (long long)r);
    }
    for (int64_t r = 0; r < n_rows; ++r) {
        double* x = out + (size_t)r * f;
        for (int k = 0; k < f; ++k) x[k] = 0.0;
        const int64_t beg = indptr[r], end = indptr[r + 1], n = end - beg;
        if (n <= 0 || n >= n_items) continue;   // nothing to draw from, or no negative to find
        for (int64_t t = 0; t < (int64_t)fold_in_epochs * n; ++t) {
            const Philox4 r0 = philox4x32_10(seed, RTX_BPR_FOLD_STREAM, 2 * (uint64_t)t);
            const int32_t it = indices[beg + (int64_t)rtx_mulhi32(r0.x, (uint32_t)n)];
            uint32_t w[RTX_BPR_NEG_TRIES] = {r0.y, r0.z, r0.w, 0, 0, 0, 0};
            int32_t jt = -1;
            for (int k = 0; k < RTX_BPR_NEG_TRIES && jt < 0; ++k) {
                if (k == 3) {   // the second call, only when the first one's words are used up
                    const Philox4 r1 = philox4x32_10(seed, RTX_BPR_FOLD_STREAM, 2 * (uint64_t)t + 1);
                    w[3] = r1.x; w[4] = r1.y; w[5] = r1.z; w[6] = r1.w;
                }
                const int32_t c = (int32_t)rtx_mulhi32(w[k], (uint32_t)n_items);
                if (!stored(indices, beg, end, c)) jt = c;
            }
            if (jt < 0) continue;
            const double* yi = Y + (size_t)it * f;
            const double* yj = Y + (size_t)jt * f;
            const double s = coefficient(x, yi, yj, f);
            for (int k = 0; k < f; ++k) {
                const double d = yi[k] - yj[k];
                const double a = s * d;
                const double b = reg * x[k];
                const double c = a - b;
                const double e = lr * c;
                x[k] = x[k] + e;
            }
        }
    }
    return RTX_OK;
}
