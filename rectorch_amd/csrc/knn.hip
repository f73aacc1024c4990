// knn.hip -- item-based k-nearest-neighbour model (ItemKNN) on MI355X, in float64.
//
// Definition (include/rectorch_hip.h has the full text):
//     G = X^T X;  for i != j with G_ij > 0:  cosine  S_ij = G_ij / (sqrt(G_ii) sqrt(G_jj) + shrink)
//                                            jaccard S_ij = G_ij / (G_ii + G_jj - G_ij + shrink)       (binary data)
//     every other entry is "no neighbour" = -inf.  N_k(j) = the k best i of row j of S (similarity descending, id ascending among
//     equal ones, finite entries only);  W_ij = S_ij [/ d_j] for i in N_k(j), d_j = the list's sum best first;  scores = X W.
// Here:
//   1. G by step 1 of the EASE pipeline (rtx_gram_full, ease.hip): exact on fp8 / bf16 MFMA where the data allow, f64 MFMA otherwise.
//   2. k_knn_diag reads the diagonal FIRST (sqrt for cosine), k_knn_sim writes S beside G.  The operation order is fixed and
//      commutative in (i, j), so S_ij and S_ji are the same bits.
//   3. Selection: the float64 list kernel of recommend() (k_topk_items, topk_select.h) on the rows of S, in chunks of rows; per row j
//      only the threshold (tau_j.value, tau_j.id) = the K-th entry of the list (or "every finite entry") and d_j are kept.
//   4. W as CSR BY SOURCE ITEM i (the rows scoring walks).  S is symmetric to the bit, so "i in N_k(j)" is tested on S_ij while row i
//      of S is walked contiguously:  keep j iff S_ij finite and (S_ij > tau_j.value or (S_ij == tau_j.value and i <= tau_j.id)).
//      count per row -> scan -> ordered fill by ballot compaction (the pattern of cond_rows.hip / k_dense_fill): the indices come out
//      ascending with no sort and no atomics.
//   5. Scores: k_knn_scores, a sparse-row x sparse-matrix product with float64 accumulators in LDS (below).
#include "../../include/rectorch_hip.h"
#include "rtx_dgemm.h"
#include "rtx_kernels.h"
#include "solver_common.h"

#include <math.h>
#include <limits.h>
#include <memory>
#include <vector>

struct rtx_knn {
    int n = 0;
    int64_t nnz = 0;
    int64_t* indptr = nullptr;   // [n + 1]
    int32_t* indices = nullptr;  // [nnz]: the j of row i, ascending
    double* values = nullptr;    // [nnz]
    double fit_ms = 0, gram_ms = 0, sim_ms = 0, select_ms = 0;
};

// ------------------------------------------------------------------------------------------------ kernels
// d[i] = sqrt(G_ii) (cosine) or G_ii (jaccard)
__global__ __launch_bounds__(256) void k_knn_diag(const double* G, long ldg, int n, int cosine, double* d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double g = G[(size_t)i * ldg + i];
    d[i] = cosine ? sqrt(g) : g;
}

// S[i][j] from G[i][j] and the diagonal terms; -inf on the diagonal and where G_ij <= 0.  No contraction: the denominators are a
// rounded product plus shrink (cosine) and ((G_ii + G_jj) - G_ij) + shrink (jaccard), as the host restatements compute them.
__global__ __launch_bounds__(256) void k_knn_sim(const double* G, long ldg, const double* d, double* S, long lds, int n, int cosine,
                                                 double shrink)
{
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx % n);
    const double g = G[(size_t)i * ldg + j];
    double s = -INFINITY;
    if (i != j && g > 0.0) {
        const double den = cosine ? d[i] * d[j] + shrink : ((d[i] + d[j]) - g) + shrink;
        s = g / den;
    }
    S[(size_t)i * lds + j] = s;
}

// From the ranked list of each row j (vals / items [rows][K], best first, -inf entries last): the threshold of N_k(j) -- the K-th
// entry when it is finite, else (-inf, INT_MAX) = "every finite entry" -- and d_j = the finite entries added in list order.
__global__ __launch_bounds__(256) void k_knn_thresh(const double* vals, const int32_t* items, int rows, int K, double* tau_v, int32_t* tau_id,
                                                    double* dsum)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= rows) return;
    const double* v = vals + (size_t)j * K;
    const double last = v[K - 1];
    const bool full = last > -INFINITY;
    tau_v[j] = full ? last : -INFINITY;
    tau_id[j] = full ? items[(size_t)j * K + K - 1] : INT_MAX;
    double d = 0.0;
    for (int t = 0; t < K; ++t) {
        const double x = v[t];
        if (!(x > -INFINITY)) break;
        d += x;
    }
    dsum[j] = d;
}

__device__ __forceinline__ bool knn_keep(double s, int i, double tv, int32_t ti)
{
    return s > -INFINITY && (s > tv || (s == tv && i <= ti));
}

// counts[i] = stored entries of row i of W
__global__ __launch_bounds__(256) void k_knn_count(const double* S, int n, const double* tau_v, const int32_t* tau_id, int32_t* counts)
{
    __shared__ int wave_cnt[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    int c = 0;
    for (int j = tid; j < n; j += 256) c += knn_keep(S[(size_t)i * n + j], i, tau_v[j], tau_id[j]) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((tid & 63) == 0) wave_cnt[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) counts[i] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// row i of W: the kept j in ascending order, W_ij = S_ij [/ d_j]
__global__ __launch_bounds__(256) void k_knn_fill(const double* S, int n, const double* tau_v, const int32_t* tau_id, const double* dsum,
                                                  int normalize, const int64_t* indptr, int32_t* indices, double* values)
{
    __shared__ int wave_cnt[4];
    __shared__ int base_sh;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base_sh = 0;
    __syncthreads();
    const int64_t out0 = indptr[i];
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int j = c0 + tid;
        const double s = (j < n) ? S[(size_t)i * n + j] : -INFINITY;
        const bool keep = (j < n) && knn_keep(s, i, tau_v[j], tau_id[j]);
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wave_cnt[w];
        const int base = base_sh;
        if (keep) {
            const int64_t o = out0 + base + woff + before;
            indices[o] = j;
            values[o] = normalize ? s / dsum[j] : s;
        }
        __syncthreads();
        if (tid == 0) base_sh = base + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
}

// scores[b][j] = sum over the stored entries (i, v) of user row u_b, in stored order, of v * W_ij  -- fma(v, w, acc) per term.
// One workgroup per (user, block of RTX_KNN_BLOCK_COLS columns); the block's float64 accumulators live in LDS.  Each of the four
// waves owns a quarter of the block: a wave's LDS operations execute in order, so entry after entry is added with no barrier and no
// atomic, and the targets of one row of W are distinct.  Per 64 entries of the user: (1) lane l binary-searches the sorted indices
// of the row of W of entry l for the wave's first column -- 64 searches in flight; (2) entry by entry the wave walks the slice of
// that row that falls into its columns, 64 stored weights per step, the next entry's first step already requested.
// Width: 4096 columns = 32 KiB of LDS per workgroup -> 5 workgroups per CU by LDS (160 KiB), 4 by the guide's advice for 256-thread
// blocks = 16 waves per CU, the 4 waves per SIMD that 8-byte LDS accesses need to reach their rate; a wider block halves the
// searches per user but leaves 2 waves per SIMD to hide the latency of the dependent index loads.
#define RTX_KNN_WAVE_COLS 1024
#define RTX_KNN_BLOCK_COLS (4 * RTX_KNN_WAVE_COLS)
__global__ __launch_bounds__(256) void k_knn_scores(const RtxCsrView x, const RtxCsrView mask, const int64_t* __restrict__ wptr,
                                                    const int32_t* __restrict__ widx, const double* __restrict__ wval, int n, double* out)
{
    __shared__ double acc[RTX_KNN_BLOCK_COLS];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * RTX_KNN_BLOCK_COLS + wave * RTX_KNN_WAVE_COLS;
    const int c1 = min(c0 + RTX_KNN_WAVE_COLS, n);
    double* a = acc + wave * RTX_KNN_WAVE_COLS;
    for (int t = lane; t < RTX_KNN_WAVE_COLS; t += 64) a[t] = 0.0;
    const int64_t u = x.row_ids ? (int64_t)x.row_ids[b] : (int64_t)b;
    const int64_t beg = x.indptr[u], end = x.indptr[u + 1];
    if (c0 < n) {
        for (int64_t e0 = beg; e0 < end; e0 += 64) {
            // (1) this lane's entry: its value, and where the wave's columns start in its row of W
            const int64_t e = e0 + lane;
            int64_t lo = 0, row_end = 0;
            double v = 0.0;
            if (e < end) {
                const int i = x.indices[e];
                v = x.values ? (double)x.values[e] : 1.0;
                if ((unsigned)i < (unsigned)n) {
                    lo = wptr[i];
                    row_end = wptr[i + 1];
                    int64_t hi = row_end;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (widx[mid] < c0) lo = mid + 1;
                        else hi = mid;
                    }
                }
            }
            // (2) the entries in stored order
            const int cnt = (int)min((int64_t)64, end - e0);
            int64_t p = __shfl(lo, 0) + lane, re = __shfl(row_end, 0);
            bool in = p < re;
            int j = in ? widx[p] : INT_MAX;
            double w = in ? wval[p] : 0.0;
            for (int q = 0; q < cnt; ++q) {
                const double vq = __shfl(v, q);
                // the next entry's first step
                const int qn = q + 1 < cnt ? q + 1 : q;
                const int64_t pn = __shfl(lo, qn) + lane, ren = __shfl(row_end, qn);
                const bool inn = pn < ren;
                const int jn = inn ? widx[pn] : INT_MAX;
                const double wn = inn ? wval[pn] : 0.0;
                for (;;) {
                    const bool hit = in && j < c1;
                    if (hit) a[j - c0] = fma(vq, w, a[j - c0]);
                    if (__ballot(hit) != ~0ull) break;   // sorted indices: a lane past the slice ends it
                    p += 64;
                    in = p < re;
                    j = in ? widx[p] : INT_MAX;
                    w = in ? wval[p] : 0.0;
                }
                p = pn; re = ren; in = inn; j = jn; w = wn;
            }
        }
        double* o = out + (size_t)b * n + c0;
        for (int t = lane; t < c1 - c0; t += 64) o[t] = a[t];
    }
    if (mask.indptr) {
        __syncthreads();
        const int lo = blockIdx.x * RTX_KNN_BLOCK_COLS;
        rtx_mask_neg_inf(mask, b, lo, min(lo + RTX_KNN_BLOCK_COLS, n), out + (size_t)b * n, tid);
    }
}

// ------------------------------------------------------------------------------------------------ host side
static void knn_free(rtx_knn* h)
{
    if (h->indptr) (void)hipFree(h->indptr);
    if (h->indices) (void)hipFree(h->indices);
    if (h->values) (void)hipFree(h->values);
    delete h;
}

// the refusals shared by rtx_knn_similarity and rtx_knn_fit: nothing is launched before they pass
static int knn_check(const char* who, const rtx_csr* X, double shrink, int32_t similarity)
{
    RTX_CHECK(X, RTX_EINVAL, "%s: NULL argument", who);
    RTX_CHECK(X->n_rows > 0 && X->n_cols > 0, RTX_EINVAL, "%s: empty matrix", who);
    RTX_CHECK(isfinite(shrink) && shrink >= 0.0, RTX_EINVAL, "%s: shrink must be finite and >= 0, got %g", who, shrink);
    RTX_CHECK(similarity == RTX_KNN_COSINE || similarity == RTX_KNN_JACCARD, RTX_EINVAL,
              "%s: unknown similarity %d (supported: RTX_KNN_COSINE = 0, RTX_KNN_JACCARD = 1)", who, similarity);
    if (similarity == RTX_KNN_JACCARD && X->values && X->nnz > 0) {
        std::vector<float> hv((size_t)X->nnz);
        RTX_HIP(hipMemcpy(hv.data(), X->values, sizeof(float) * X->nnz, hipMemcpyDeviceToHost));
        for (float v : hv)
            RTX_CHECK(v == 1.f, RTX_EINVAL,
                      "%s: the jaccard similarity is defined on binary data and the matrix stores the value %g: binarise it first "
                      "(every stored value 1)", who, (double)v);
    }
    return RTX_OK;
}

// S (device double [n][n]) from X: Gram matrix, diagonal, similarity.  G and the diagonal go into `work`; ev_gram (nullable) is
// recorded between the Gram matrix and the similarity kernels.
static int knn_similarity_into(const rtx_csr* X, double shrink, int32_t similarity, double* S, std::vector<void*>& work, hipEvent_t ev_gram,
                               hipStream_t st)
{
    const int n = X->n_cols;
    const int np = ((n + 127) / 128) * 128;
    double *G = nullptr, *d = nullptr;
    RTX_TRY(rtx_pool_alloc("knn", (void**)&G, sizeof(double) * (size_t)np * np, work));
    RTX_TRY(rtx_pool_alloc("knn", (void**)&d, sizeof(double) * n, work));
    RTX_TRY(rtx_gram_full(X, G, np, work, st));
    if (ev_gram) RTX_HIP(hipEventRecord(ev_gram, st));
    const int cosine = similarity == RTX_KNN_COSINE;
    hipLaunchKernelGGL(k_knn_diag, dim3((n + 255) / 256), dim3(256), 0, st, G, (long)np, n, cosine, d);
    hipLaunchKernelGGL(k_knn_sim, dim3((unsigned)(((long)n * n + 255) / 256)), dim3(256), 0, st, G, (long)np, d, S, (long)n, n, cosine, shrink);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

#define RTX_KNN_SELECT_ROWS 4096   // rows of S ranked per launch of the list kernel: lists of 4096 x K x 12 bytes

extern "C" {

int rtx_knn_similarity(const rtx_csr* X, double shrink, int32_t similarity, double* S_dev, void* stream)
{
    RTX_TRY(knn_check("knn_similarity", X, shrink, similarity));
    RTX_CHECK(S_dev, RTX_EINVAL, "knn_similarity: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    std::vector<void*> work;
    int rc = knn_similarity_into(X, shrink, similarity, S_dev, work, nullptr, st);
    hipError_t e = hipStreamSynchronize(st);   // the work buffers are freed below
    rtx_free_all(work);
    if (rc == RTX_OK && e != hipSuccess) {
        rtx_set_error("knn_similarity: %s", hipGetErrorString(e));
        rc = RTX_EHIP;
    }
    return rc;
}

int rtx_knn_fit(const rtx_csr* X, int32_t k, double shrink, int32_t similarity, int32_t normalize, rtx_knn** out, void* stream)
{
    RTX_CHECK(out, RTX_EINVAL, "knn_fit: NULL argument");
    RTX_CHECK(k >= 1 && k <= 1024, RTX_EINVAL, "knn_fit: k must be in [1, 1024] (the selection kernel's limit), got %d", k);
    RTX_TRY(knn_check("knn_fit", X, shrink, similarity));
    hipStream_t st = (hipStream_t)stream;
    const int n = X->n_cols;
    const int K = k < n ? k : n;
    RtxFitScope<5> fs;   // events: start, Gram, similarity, selection, end
    std::unique_ptr<rtx_knn, decltype(&knn_free)> h(new rtx_knn(), knn_free);
    h->n = n;
    const int rc = [&]() -> int {
        hipEvent_t* ev = fs.ev;
        RTX_TRY(fs.create_events());
        double *S = nullptr, *tau_v = nullptr, *dsum = nullptr, *lvals = nullptr;
        int32_t *tau_id = nullptr, *counts = nullptr, *litems = nullptr;
        const int chunk = n < RTX_KNN_SELECT_ROWS ? n : RTX_KNN_SELECT_ROWS;
        RTX_TRY(rtx_pool_alloc("knn", (void**)&S, sizeof(double) * (size_t)n * n, fs.pool));
        RTX_TRY(rtx_pool_alloc("knn", (void**)&tau_v, sizeof(double) * n, fs.pool));
        RTX_TRY(rtx_pool_alloc("knn", (void**)&dsum, sizeof(double) * n, fs.pool));
        RTX_TRY(rtx_pool_alloc("knn", (void**)&tau_id, sizeof(int32_t) * n, fs.pool));
        RTX_TRY(rtx_pool_alloc("knn", (void**)&counts, sizeof(int32_t) * n, fs.pool));
        RTX_TRY(rtx_pool_alloc("knn", (void**)&lvals, sizeof(double) * (size_t)chunk * K, fs.pool));
        RTX_TRY(rtx_pool_alloc("knn", (void**)&litems, sizeof(int32_t) * (size_t)chunk * K, fs.pool));
        RTX_HIP(hipMalloc((void**)&h->indptr, sizeof(int64_t) * ((size_t)n + 1)));
        RTX_HIP(hipEventRecord(ev[0], st));
        // ---- 1, 2. G and S
        RTX_TRY(knn_similarity_into(X, shrink, similarity, S, fs.pool, ev[1], st));
        RTX_HIP(hipEventRecord(ev[2], st));
        // ---- 3. thresholds and list sums, row chunk by row chunk
        for (int r0 = 0; r0 < n; r0 += chunk) {
            const int rows = n - r0 < chunk ? n - r0 : chunk;
            RTX_TRY(rtx_launch_topk_items(S + (size_t)r0 * n, 1, n, rows, n, nullptr, K, litems, lvals, st));
            hipLaunchKernelGGL(k_knn_thresh, dim3((rows + 255) / 256), dim3(256), 0, st, lvals, litems, rows, K, tau_v + r0, tau_id + r0, dsum + r0);
            RTX_HIP(hipGetLastError());
        }
        RTX_HIP(hipEventRecord(ev[3], st));
        // ---- 4. W by source item
        hipLaunchKernelGGL(k_knn_count, dim3(n), dim3(256), 0, st, S, n, tau_v, tau_id, counts);
        RTX_HIP(hipGetLastError());
        RTX_TRY(rtx_launch_scan_counts(counts, n, h->indptr, st));
        RTX_HIP(hipStreamSynchronize(st));
        RTX_HIP(hipMemcpy(&h->nnz, h->indptr + n, sizeof(int64_t), hipMemcpyDeviceToHost));
        RTX_HIP(hipMalloc((void**)&h->indices, sizeof(int32_t) * (size_t)(h->nnz ? h->nnz : 4)));
        RTX_HIP(hipMalloc((void**)&h->values, sizeof(double) * (size_t)(h->nnz ? h->nnz : 2)));
        hipLaunchKernelGGL(k_knn_fill, dim3(n), dim3(256), 0, st, S, n, tau_v, tau_id, dsum, normalize ? 1 : 0, h->indptr, h->indices, h->values);
        RTX_HIP(hipGetLastError());
        RTX_HIP(hipEventRecord(ev[4], st));
        RTX_HIP(hipStreamSynchronize(st));
        h->gram_ms = rtx_elapsed_ms(ev[0], ev[1]);
        h->sim_ms = rtx_elapsed_ms(ev[1], ev[2]);
        h->select_ms = rtx_elapsed_ms(ev[2], ev[3]);
        h->fit_ms = rtx_elapsed_ms(ev[0], ev[4]);
        return RTX_OK;
    }();
    if (rc) {
        (void)hipStreamSynchronize(st);   // launches already queued may use the pool, which is freed on return
        return rc;
    }
    *out = h.release();
    return RTX_OK;
}

int rtx_knn_load(int32_t n_items, const int64_t* indptr_host, const int32_t* indices_host, const double* values_host, rtx_knn** out)
{
    RTX_CHECK(indptr_host && out, RTX_EINVAL, "knn_load: NULL argument");
    RTX_CHECK(n_items > 0, RTX_EINVAL, "knn_load: n_items = %d", n_items);
    RTX_CHECK(indptr_host[0] == 0, RTX_EINVAL, "knn_load: indptr[0] = %lld, expected 0", (long long)indptr_host[0]);
    for (int i = 0; i < n_items; ++i)
        RTX_CHECK(indptr_host[i + 1] >= indptr_host[i], RTX_EINVAL, "knn_load: indptr decreases at row %d", i);
    const int64_t nnz = indptr_host[n_items];
    RTX_CHECK(nnz == 0 || (indices_host && values_host), RTX_EINVAL, "knn_load: NULL argument");
    for (int i = 0; i < n_items; ++i)
        for (int64_t p = indptr_host[i]; p < indptr_host[i + 1]; ++p) {
            RTX_CHECK(indices_host[p] >= 0 && indices_host[p] < n_items, RTX_EINVAL, "knn_load: row %d holds the column %d, outside [0, %d)", i,
                      indices_host[p], n_items);
            RTX_CHECK(p == indptr_host[i] || indices_host[p] > indices_host[p - 1], RTX_EINVAL,
                      "knn_load: the indices of row %d are not sorted (strictly ascending): sort_indices() / sum_duplicates() first", i);
        }
    rtx_knn* h = new rtx_knn();
    h->n = n_items;
    h->nnz = nnz;
    hipError_t e = hipMalloc((void**)&h->indptr, sizeof(int64_t) * ((size_t)n_items + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&h->indices, sizeof(int32_t) * (size_t)(nnz ? nnz : 4));
    if (e == hipSuccess) e = hipMalloc((void**)&h->values, sizeof(double) * (size_t)(nnz ? nnz : 2));
    if (e == hipSuccess) e = hipMemcpy(h->indptr, indptr_host, sizeof(int64_t) * ((size_t)n_items + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(h->indices, indices_host, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(h->values, values_host, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        rtx_set_error("knn_load: %s", hipGetErrorString(e));
        knn_free(h);
        return RTX_EHIP;
    }
    *out = h;
    return RTX_OK;
}

int rtx_knn_destroy(rtx_knn* h)
{
    if (h) knn_free(h);
    return RTX_OK;
}

int rtx_knn_shape(const rtx_knn* h, int32_t* n_items, int64_t* nnz)
{
    RTX_CHECK(h, RTX_EINVAL, "knn: NULL handle");
    if (n_items) *n_items = h->n;
    if (nnz) *nnz = h->nnz;
    return RTX_OK;
}

int rtx_knn_copy(const rtx_knn* h, int64_t* indptr_dev, int32_t* indices_dev, double* values_dev, void* stream)
{
    RTX_CHECK(h, RTX_EINVAL, "knn: NULL handle");
    hipStream_t st = (hipStream_t)stream;
    if (indptr_dev) RTX_HIP(hipMemcpyAsync(indptr_dev, h->indptr, sizeof(int64_t) * ((size_t)h->n + 1), hipMemcpyDeviceToDevice, st));
    if (indices_dev && h->nnz) RTX_HIP(hipMemcpyAsync(indices_dev, h->indices, sizeof(int32_t) * (size_t)h->nnz, hipMemcpyDeviceToDevice, st));
    if (values_dev && h->nnz) RTX_HIP(hipMemcpyAsync(values_dev, h->values, sizeof(double) * (size_t)h->nnz, hipMemcpyDeviceToDevice, st));
    return RTX_OK;
}

int rtx_knn_timings(const rtx_knn* h, double* fit_ms, double* gram_ms, double* sim_ms, double* select_ms)
{
    RTX_CHECK(h, RTX_EINVAL, "knn: NULL handle");
    if (fit_ms) *fit_ms = h->fit_ms;
    if (gram_ms) *gram_ms = h->gram_ms;
    if (sim_ms) *sim_ms = h->sim_ms;
    if (select_ms) *select_ms = h->select_ms;
    return RTX_OK;
}

int rtx_knn_scores(const rtx_knn* h, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const rtx_csr* mask,
                   const int32_t* mask_row_ids, double* out, void* stream)
{
    RTX_CHECK(h && X && out, RTX_EINVAL, "knn_scores: NULL argument");
    RtxCsrView v, mv;
    RTX_TRY(rtx_scores_args("knn_scores", h->n, X, row_ids, batch, mask, mask_row_ids, &v, &mv));
    if (batch == 0) return RTX_OK;
    hipLaunchKernelGGL(k_knn_scores, dim3((h->n + RTX_KNN_BLOCK_COLS - 1) / RTX_KNN_BLOCK_COLS, batch), dim3(256), 0, (hipStream_t)stream, v,
                       mv, h->indptr, h->indices, h->values, h->n, out);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

}  // extern "C"
