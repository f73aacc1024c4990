// solver_common.h -- what the resident fold-in solvers (ease.hip, admm.hip, knn.hip, wmf.hip) share: each is fitted once, keeps its
// model in HBM and scores users' sparse rows against it.
//   host    rtx_elapsed_ms, rtx_dev_alloc / rtx_pool_alloc / rtx_free_all, RtxFitScope (what a fit holds only while it runs),
//           rtx_scores_args (the argument checks and the two row views of every rtx_*_scores)
//   device  rtx_mask_neg_inf (the -inf tail of the three score kernels)
#pragma once
#include "../../include/rectorch_hip.h"
#include "rtx_kernels.h"

#include <math.h>
#include <vector>

static inline double rtx_elapsed_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

// hipMalloc with the caller's prefix (`who`: "ease", "knn", ...) in the message; an empty request still gets a valid pointer
static inline int rtx_dev_alloc(const char* who, void** p, size_t bytes)
{
    hipError_t rc = hipMalloc(p, bytes ? bytes : 16);
    if (rc != hipSuccess) {
        *p = nullptr;
        rtx_set_error("%s: hipMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(rc));
        return RTX_ENOMEM;
    }
    return RTX_OK;
}

// ... into a pool that rtx_free_all releases
static inline int rtx_pool_alloc(const char* who, void** p, size_t bytes, std::vector<void*>& pool)
{
    RTX_TRY(rtx_dev_alloc(who, p, bytes));
    pool.push_back(*p);
    return RTX_OK;
}

static inline void rtx_free_all(std::vector<void*>& pool)
{
    for (void* p : pool) (void)hipFree(p);
    pool.clear();
}

// Work memory released when its owner returns -- on every path.  It frees and does not synchronise: whoever queued launches that use
// the pool synchronises the stream before this object goes out of scope.
struct RtxDevPool {
    std::vector<void*> pool;

    RtxDevPool() = default;
    RtxDevPool(const RtxDevPool&) = delete;
    RtxDevPool& operator=(const RtxDevPool&) = delete;
    ~RtxDevPool() { rtx_free_all(pool); }
};

// ... and the NEV timing events of one fit with it
template <int NEV>
struct RtxFitScope : RtxDevPool {
    hipEvent_t ev[NEV] = {};

    int create_events()
    {
        for (hipEvent_t& e : ev) RTX_HIP(hipEventCreate(&e));
        return RTX_OK;
    }
    ~RtxFitScope()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// The checks every rtx_*_scores makes on its rows and its mask (after its own NULL check: n_items comes out of the handle), and the
// views of both: batch row b is row row_ids[b] of X (row b without row_ids), and likewise for the mask.  *mv has a NULL indptr
// without a mask.
static inline int rtx_scores_args(const char* who, int n_items, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const rtx_csr* mask,
                                  const int32_t* mask_row_ids, RtxCsrView* xv, RtxCsrView* mv)
{
    RTX_CHECK(X->n_cols == n_items, RTX_EINVAL, "%s: matrix has %d columns, model has %d items", who, X->n_cols, n_items);
    RTX_CHECK(batch >= 0 && (row_ids || batch <= X->n_rows), RTX_EINVAL, "%s: bad batch %d", who, batch);
    RTX_CHECK(!mask || (mask->n_cols == n_items && (mask_row_ids || batch <= mask->n_rows)), RTX_EINVAL,
              "%s: mask matrix does not match (%d columns, %lld rows)", who, mask ? mask->n_cols : 0, mask ? (long long)mask->n_rows : 0LL);
    *xv = RtxCsrView{X->indptr, X->indices, X->values, row_ids};
    *mv = RtxCsrView{nullptr, nullptr, nullptr, nullptr};
    if (mask) *mv = RtxCsrView{mask->indptr, mask->indices, mask->values, mask_row_ids};
    return RTX_OK;
}

// out_row[i] = -inf for the stored NON-ZERO entries i of the mask's row of batch row b that fall into lo <= i < hi: the columns the
// calling workgroup has written, so hi <= n_items and the workgroup's __syncthreads() goes before the call.  256 threads.
__device__ __forceinline__ void rtx_mask_neg_inf(const RtxCsrView& mask, int b, int lo, int hi, double* out_row, int tid)
{
    const int64_t mu = mask.row_ids ? (int64_t)mask.row_ids[b] : (int64_t)b;
    for (int64_t k = mask.indptr[mu] + tid; k < mask.indptr[mu + 1]; k += 256) {
        const int i = mask.indices[k];
        const float v = mask.values ? mask.values[k] : 1.f;
        if (v != 0.f && i >= lo && i < hi) out_row[i] = -INFINITY;
    }
}
