// list_metrics.hip -- ranking metrics of READY-MADE item lists on gfx950 (k_list_metrics): nDCG@k, Recall@k, hit@k and mrr@k of every
// user's ranked list (what rtx_topk_items / rtx_engine_recommend write) against the user's held-out CSR row.
//
// k_topk_metrics (topk.hip) selects and scores in one kernel, float32 rows only; the item-item models score in float64 and rank with
// k_topk_items.  This kernel is the second half on its own: it never sees a score, so it serves every family and every list length.
// The definitions are rectorch_amd/metrics.py's (reference rectorch/metrics.py:136-147, 187-196, 231-238, 272-285) with the list in
// the place of the argpartition + argsort, kk = min(k, K):
//   rel_r   = the held-out row's stored value at items[r], 0 when the row has no such entry (binary search: column ids are sorted)
//   nDCG    = sum_{r < kk} rel_r / log2(r + 2)  /  sum_{j < min(int(sum of the row), kk)} 1 / log2(j + 2)
//   Recall  = float32(#{r < kk : rel_r > 0}) / min(kk, #{row values > 0})
//   hit     = 1.0 / 0.0: some rel_r > 0 below kk;   mrr = 1 / (1 + first r < kk with rel_r != 0), else 0
// An empty held-out row gives what k_topk_metrics gives: both quotients are 0 / 0 = NaN, hit = mrr = 0.
//
// One wavefront per user, four users per workgroup (the shape of k_opr_rank).  A lane owns the ranks lane, lane + 64, ...; it walks
// them ONCE, looks the item up in the held-out row (global memory: the row is a few hundred bytes, read by one wave, L1-resident
// after the first probe) and adds the rank's terms to every cut-off that contains it.  The per-cut-off sums then cross the 64 lanes
// by a fixed-order butterfly: nothing depends on scheduling, two runs give the same bits.  The ideal DCG alone is not summed that
// way: it does not depend on the list, and Metrics takes it from a cumsum, so its discounts are added rank after rank (the lanes hand
// theirs round in order).  log2(r + 2) of the ranks below RTX_LIST_LOG2 comes from a table the host writes once per device with glibc's
// log2, the function numpy calls in Metrics (what g_topk_log2 is to k_topk_metrics); longer lists compute the rest here.  So where a
// list holds at most two hits (a sum of two terms has one order) nDCG equals Metrics' to the bit.
#include "../../include/rectorch_hip.h"
#include "rtx_device.h"
#include <cmath>

#include <mutex>
#include <vector>

#define RTX_LIST_MAX_KS 16
#define RTX_LIST_LOG2 1024
__device__ double g_list_log2[RTX_LIST_LOG2];

struct RtxListArgs {
    const int32_t* items;   // [n][ld], the first K of a row ranked best first
    long ld;
    int n, K;
    int r_end;              // min(K, max cut-off): ranks at or above it belong to no cut-off
    RtxCsrView held;
    long held_rows;         // rows of the held-out matrix: a row id outside [0, held_rows) reads as an empty row
    int n_k;
    int ks[RTX_LIST_MAX_KS];
    double *ndcg, *recall, *hit, *mrr;   // [n_k][out_ld], each nullable
    long out_ld;
};

__global__ __launch_bounds__(256) void k_list_metrics(const RtxListArgs a)
{
    const int c = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= a.n) return;                      // (whole waves leave: no barrier follows)
    const int64_t u = csr_row(a.held, c);
    int64_t hb = 0, he = 0;
    if (u >= 0 && u < a.held_rows) { hb = a.held.indptr[u]; he = a.held.indptr[u + 1]; }
    // ---- the held-out row's sum and positive count (values are ratings or ones: exact in double in any order)
    double gs = 0.0;
    int np = 0;
    for (int64_t k = hb + lane; k < he; k += 64) {
        const float v = a.held.values ? a.held.values[k] : 1.f;
        gs += (double)v;
        np += v > 0.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { gs += __shfl_xor(gs, o, 64); np += __shfl_xor(np, o, 64); }
    // ---- one pass over the ranks
    double dcg[RTX_LIST_MAX_KS], idcg[RTX_LIST_MAX_KS];
    int hits[RTX_LIST_MAX_KS], first[RTX_LIST_MAX_KS], kk[RTX_LIST_MAX_KS], nid[RTX_LIST_MAX_KS];
#pragma unroll
    for (int q = 0; q < RTX_LIST_MAX_KS; ++q) {
        dcg[q] = 0.0; idcg[q] = 0.0; hits[q] = 0; first[q] = 0x7fffffff;
        kk[q] = q < a.n_k ? min(a.ks[q], a.K) : 0;
        nid[q] = gs >= (double)kk[q] ? kk[q] : (gs > 0.0 ? (int)gs : 0);     // tp[:min(int(n), k)].sum()   (metrics.py:146)
    }
    int nid_max = 0;
#pragma unroll
    for (int q = 0; q < RTX_LIST_MAX_KS; ++q) nid_max = max(nid_max, nid[q]);
    const int32_t* __restrict__ row = a.items + (size_t)c * a.ld;
    double ideal = 0.0;                        // the discounts added IN RANK ORDER, as Metrics' cumsum adds them (uniform over the lanes)
    for (int base = 0; base < a.r_end; base += 64) {      // (uniform trip count: the lanes exchange their discounts below)
        const int r = base + lane;
        double disc = 0.0;
        if (r < a.r_end) {
            const int item = row[r];
            float rel = 0.f;
            int64_t lo = hb, hi = he;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.held.indices[mid] < item) lo = mid + 1; else hi = mid;
            }
            if (lo < he && a.held.indices[lo] == item) rel = a.held.values ? a.held.values[lo] : 1.f;
            const double l2 = r < RTX_LIST_LOG2 ? g_list_log2[r] : log2((double)(r + 2));
            const double gain = (double)rel / l2;
            disc = 1.0 / l2;
#pragma unroll
            for (int q = 0; q < RTX_LIST_MAX_KS; ++q) {
                if (r < kk[q]) {
                    dcg[q] += gain;
                    hits[q] += rel > 0.f;
                    if (rel != 0.f) first[q] = min(first[q], r);       // (metrics.py:283: != 0, not > 0)
                }
            }
        }
        // ideal DCG: rank after rank up to the largest min(int(sum of the row), kk); a cut-off takes the running sum at its own
        const int steps = min(64, nid_max - base);
        for (int t = 0; t < steps; ++t) {
            ideal += __shfl(disc, t, 64);
#pragma unroll
            for (int q = 0; q < RTX_LIST_MAX_KS; ++q)
                if (q < a.n_k && base + t + 1 == nid[q]) idcg[q] = ideal;
        }
    }
    // ---- per cut-off: fixed-order butterfly over the 64 lanes, lane 0 writes
#pragma unroll
    for (int q = 0; q < RTX_LIST_MAX_KS; ++q) {
        if (q < a.n_k) {                       // (uniform)
            double d = dcg[q];
            const double id = idcg[q];         // (already whole, and the same in every lane)
            int h = hits[q], f = first[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                d += __shfl_xor(d, o, 64);
                h += __shfl_xor(h, o, 64); f = min(f, __shfl_xor(f, o, 64));
            }
            if (lane == 0) {
                const size_t at = (size_t)q * a.out_ld + c;
                if (a.ndcg) a.ndcg[at] = d / id;
                if (a.recall) a.recall[at] = (double)(float)h / (double)min(kk[q], np);       // metrics.py:194-195
                if (a.hit) a.hit[at] = h > 0 ? 1.0 : 0.0;
                if (a.mrr) a.mrr[at] = f < kk[q] ? 1.0 / (1.0 + (double)f) : 0.0;
            }
        }
    }
}

int rtx_launch_list_metrics(const int32_t* items, long ld, int n, int K, const RtxCsrView& held, long held_rows, const int* ks, int n_k,
                            double* ndcg, double* recall, double* hit, double* mrr, long out_ld, hipStream_t stream)
{
    if (n <= 0) return RTX_OK;
    RTX_CHECK(n_k >= 1 && n_k <= RTX_LIST_MAX_KS, RTX_EINVAL, "list_metrics: 1..%d cut-offs supported, got %d", RTX_LIST_MAX_KS, n_k);
    RtxListArgs a = {};
    a.items = items; a.ld = ld; a.n = n; a.K = K;
    a.held = held; a.held_rows = held_rows; a.n_k = n_k;
    int kmax = 0;
    for (int q = 0; q < n_k; ++q) {
        RTX_CHECK(ks[q] >= 1, RTX_EINVAL, "list_metrics: cut-off must be >= 1");
        a.ks[q] = ks[q];
        kmax = ks[q] > kmax ? ks[q] : kmax;
    }
    a.r_end = kmax < K ? kmax : K;
    a.ndcg = ndcg; a.recall = recall; a.hit = hit; a.mrr = mrr; a.out_ld = out_ld;
    {
        static bool table_ready[64] = {};
        static std::mutex table_mutex;          // two host threads on their first call: one fills, the other waits for the fill
        int devid = 0;
        RTX_HIP(hipGetDevice(&devid));
        RTX_CHECK(devid >= 0 && devid < 64, RTX_EINVAL, "list_metrics: device index %d", devid);
        std::lock_guard<std::mutex> lock(table_mutex);
        if (!table_ready[devid]) {
            std::vector<double> t(RTX_LIST_LOG2);
            for (int r = 0; r < RTX_LIST_LOG2; ++r) t[r] = std::log2((double)(r + 2));
            RTX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_list_log2), t.data(), sizeof(double) * RTX_LIST_LOG2));
            RTX_HIP(hipStreamSynchronize(nullptr));   // (the copy runs on the NULL stream, which a non-blocking caller's stream does not wait for)
            table_ready[devid] = true;
        }
    }
    hipLaunchKernelGGL(k_list_metrics, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, a);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

extern "C" int rtx_list_metrics(const int32_t* items, int64_t ld, int32_t n, int32_t K, const rtx_csr* heldout, const int32_t* row_ids,
                                const int32_t* ks_host, int32_t n_k, double* ndcg, double* recall, double* hit, double* mrr,
                                int64_t out_ld, void* stream)
{
    RTX_CHECK(n >= 0 && K >= 1 && ld >= K && out_ld >= n, RTX_EINVAL, "list_metrics: n = %d, K = %d, ld = %lld, out_ld = %lld", n, K,
              (long long)ld, (long long)out_ld);
    RTX_CHECK(n_k >= 1 && n_k <= RTX_LIST_MAX_KS, RTX_EINVAL, "list_metrics: 1..%d cut-offs supported, got %d", RTX_LIST_MAX_KS, n_k);
    if (n == 0) return RTX_OK;
    RTX_CHECK(items && heldout && ks_host, RTX_EINVAL, "list_metrics: NULL argument");
    RTX_CHECK(row_ids || n <= heldout->n_rows, RTX_EINVAL, "list_metrics: %d lists for a held-out matrix of %lld rows", n,
              (long long)heldout->n_rows);
    RtxCsrView v = {heldout->indptr, heldout->indices, heldout->values, row_ids};
    return rtx_launch_list_metrics(items, (long)ld, n, K, v, (long)heldout->n_rows, ks_host, n_k, ndcg, recall, hit, mrr, (long)out_ld,
                                   (hipStream_t)stream);
}
