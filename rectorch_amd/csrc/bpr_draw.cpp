// The sampled triples of pairwise-ranking matrix factorisation (BPR), host half: (user, positive, negative) per sample as a pure function
// of (seed, epoch, sample), in integer arithmetic over the engine's Philox4x32-10.  Plain host code: no HIP call.  The contract is
// text in include/rectorch_hip.h ("BPR triples"); a device sampler has to give the same numbers.  rtx_bpr_check_rows_host checks a
// matrix once; rtx_bpr_draw_host, called once per batch, costs its samples alone.
#include <stdint.h>

#include "../../include/rectorch_hip.h"
#include "rtx_common.h"

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

}  // namespace

// the shape checks both entries share
static int bpr_host_shape(const char* who, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int32_t n_items)
{
    RTX_CHECK(indptr && indices, RTX_EINVAL, "%s: NULL argument", who);
    RTX_CHECK(n_rows > 0 && n_rows <= INT32_MAX && n_items > 0, RTX_EINVAL, "%s: %lld rows and %d items: both must be in [1, 2^31)", who,
              (long long)n_rows, n_items);
    const int64_t nnz = indptr[n_rows];
    RTX_CHECK(indptr[0] == 0, RTX_EINVAL, "%s: indptr must start at 0, got %lld", who, (long long)indptr[0]);
    RTX_CHECK(nnz > 0, RTX_EINVAL, "%s: the matrix holds no entries (nnz = %lld): there is nothing to sample", who, (long long)nnz);
    RTX_CHECK(nnz <= INT32_MAX, RTX_EINVAL, "%s: nnz = %lld must be below 2^31", who, (long long)nnz);
    return RTX_OK;
}

int rtx_bpr_check_rows_host(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int32_t n_items)
{
    RTX_TRY(bpr_host_shape("bpr_check_rows_host", indptr, indices, n_rows, n_items));
    const int64_t nnz = indptr[n_rows];
    // ascending row ends inside the matrix (checked before a row's entries are read), column ids strictly ascending and below n_items
    for (int64_t r = 0; r < n_rows; ++r) {
        RTX_CHECK(indptr[r] <= indptr[r + 1] && indptr[r + 1] <= nnz, RTX_EINVAL, "bpr_check_rows_host: indptr decreases or passes nnz at row %lld",
                  (long long)r);
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e)
            RTX_CHECK(indices[e] >= 0 && indices[e] < n_items && (e == indptr[r] || indices[e - 1] < indices[e]), RTX_EINVAL,
                      "bpr_check_rows_host: row %lld: column ids must be sorted, unique and below %d (entry %lld holds %d)", (long long)r, n_items,
                      (long long)e, indices[e]);
    }
    return RTX_OK;
}

int rtx_bpr_draw_host(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int32_t n_items, uint64_t seed, int32_t epoch, int64_t lo,
                      int64_t count, int32_t* u_out, int32_t* i_out, int32_t* j_out)
{
    RTX_CHECK(u_out && i_out && j_out, RTX_EINVAL, "bpr_draw_host: NULL argument");
    RTX_TRY(bpr_host_shape("bpr_draw_host", indptr, indices, n_rows, n_items));
    const int64_t nnz = indptr[n_rows];
    RTX_CHECK(epoch >= 0, RTX_EINVAL, "bpr_draw_host: epoch must be >= 0, got %d", epoch);
    RTX_CHECK(lo >= 0 && lo <= nnz && count >= 0 && count <= nnz - lo, RTX_EINVAL, "bpr_draw_host: %lld samples from sample %lld on are outside the epoch's %lld",
              (long long)count, (long long)lo, (long long)nnz);
    const uint64_t offset = RTX_BPR_FIT_STREAM + (uint64_t)epoch;
    for (int64_t t = 0; t < count; ++t) {
        const uint64_t s = (uint64_t)(lo + t);
        const Philox4 r0 = philox4x32_10(seed, offset, 2 * s);
        const int64_t p = (int64_t)rtx_mulhi32(r0.x, (uint32_t)nnz);
        int64_t a = 0, b = n_rows - 1;   // the first row whose end lies beyond p (indptr[n_rows] = nnz > p): empty rows are passed over
        while (a < b) {
            const int64_t mid = a + ((b - a) >> 1);
            if (indptr[mid + 1] > p) b = mid;
            else a = mid + 1;
        }
        const int64_t beg = indptr[a], end = indptr[a + 1];
        // the rows are the caller's promise (rtx_bpr_check_rows_host); what is read stays inside the arrays whatever they hold
        RTX_CHECK(beg >= 0 && beg <= p && p < end && end <= nnz, RTX_EINVAL, "bpr_draw_host: indptr is not ascending at row %lld (sample %lld)", (long long)a,
                  (long long)(lo + t));
        uint32_t w[RTX_BPR_NEG_TRIES] = {r0.y, r0.z, r0.w, 0, 0, 0, 0};
        int32_t j = -1;
        for (int k = 0; k < RTX_BPR_NEG_TRIES && j < 0; ++k) {
            if (k == 3) {   // the second call, only when the first one's words are used up
                const Philox4 r1 = philox4x32_10(seed, offset, 2 * s + 1);
                w[3] = r1.x; w[4] = r1.y; w[5] = r1.z; w[6] = r1.w;
            }
            const int32_t c = (int32_t)rtx_mulhi32(w[k], (uint32_t)n_items);
            if (!stored(indices, beg, end, c)) j = c;
        }
        u_out[t] = (int32_t)a;
        i_out[t] = indices[p];
        j_out[t] = j;
    }
    return RTX_OK;
}
