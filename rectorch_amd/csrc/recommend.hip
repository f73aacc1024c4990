// recommend.hip -- top-N recommendation lists on gfx950 (k_topk_items): per user row the K best items and their scores.
#include "rtx_device.h"
#include "topk_select.h"
#include <cmath>

// ------------------------------------------------------------------------------------------------
// What a recommender is for (reference: the lists behind rectorch/metrics.py's argpartition + argsort; evaluation.py:100-106 hands the
// score matrix to the host for it).  One workgroup per user row; the selection is topk_select.h's, stage by stage the one of
// k_topk_metrics (topk.hip): per-thread maxima, a lower bound L of the K-th largest score by counting, the elements >= L collected and
// ranked, a radix select when more than RTX_TOPK_MAX elements reach the bound.  What is this kernel's own:
//   * the ORDER is total: score descending, item id ascending among equal scores, and "equal" is floating-point equality -- the key
//     maps -0.0 and +0.0 to one value (ScoreKey of topk.hip orders them, which no metric notices and a list shows);
//   * float64 rows (EASE, ADMM_Slim) on 64-bit keys: scores that differ below float32 resolution keep their order;
//   * the exclusion bitmap (the user's train items rank as -inf, nothing is written to the scores) sits in dynamic LDS sized by the
//     row, so the streamed form of the kernel has it too;
//   * every candidate is ranked exactly (ties by id) and the list is written with its scores.
// NaN scores are out of contract (their keys sort above +inf or below -inf by sign).
// ------------------------------------------------------------------------------------------------
template <typename T> using ItemKey = TopkKey<T, true>;

struct RtxItemsArgs {
    const void* scores;     // T [B][ld]
    long ld;
    int n_items, K;         // 1 <= K <= min(RTX_TOPK_MAX, n_items)
    RtxCsrView excl;        // has_excl: batch row b's stored non-zero entries (< n_items) rank as -inf
    int has_excl;
    int32_t* items;         // [B][K]
    void* item_scores;      // T [B][K]  (nullable)
};

// NV > 0 (float rows only): the whole row (<= NV * 1024 items, 16-byte aligned) is loaded ONCE, NV 16-byte loads per thread in one
// burst, and stays in registers as keys for every pass over it; NV = 0: every pass streams the row (any length / alignment; the
// passes after the first find it in L2).  float64 rows take the streamed form only: a 20 108-wide row is 79 doubles = 158 VGPRs per
// thread as keys, which does not fit beside the selection's own registers (DESIGN.md has the compile's numbers).
template <typename T, int NV>
__global__ __launch_bounds__(256) void k_topk_items(const RtxItemsArgs a)
{
    typedef ItemKey<T> KT;
    typedef typename KT::key_t key_t;
    static_assert(NV == 0 || KT::VEC == 4, "the burst form holds float rows");
    __shared__ TopkLds<key_t> sel;               // the selection's arrays; sel.ckey / sel.cidx: the candidates
    extern __shared__ uint32_t excl_bm[];       // has_excl: one bit per item of the row, ceil(n_items / 32) words
    const int b = blockIdx.x, tid = threadIdx.x;
    const T* row = (const T*)a.scores + (size_t)b * a.ld;
    const int K = a.K, n_items = a.n_items;
    // ---- 0. the row is requested first (burst form), then the exclusion bitmap is built under its latency
    float4 rv[NV > 0 ? NV : 1];
    const int n4 = n_items >> 2;
    if constexpr (NV > 0) {
        const float4* __restrict__ r4 = (const float4*)row;
#pragma unroll
        for (int q = 0; q < NV; ++q) rv[q] = r4[min(tid + q * 256, n4 > 0 ? n4 - 1 : 0)];   // (clamped: the guard is at the use)
    }
    const uint32_t* bm = nullptr;
    if (a.has_excl) {
        topk_excl_build(excl_bm, (n_items + 31) >> 5, a.excl, b, n_items, tid);
        bm = excl_bm;
    }
    uint4 kv[NV > 0 ? NV : 1];
    if constexpr (NV > 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            kv[q] = make_uint4(KT::key(rv[q].x), KT::key(rv[q].y), KT::key(rv[q].z), KT::key(rv[q].w));
            if (bm && tid + q * 256 < n4) topk_excl_mask4(kv[q], bm, tid + q * 256, KT::neg_key());
        }
    }
    auto key_at = [&](int i) __attribute__((always_inline)) -> key_t { return topk_key_at<KT>(row, bm, i); };
    // f(key, index) for every element of the row, exclusion applied
    auto scan = [&](auto&& f) __attribute__((always_inline)) {
        if constexpr (NV > 0) {
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int j = tid + q * 256;
                if (j < n4) { f(kv[q].x, j * 4); f(kv[q].y, j * 4 + 1); f(kv[q].z, j * 4 + 2); f(kv[q].w, j * 4 + 3); }
            }
            for (int i = n4 * 4 + tid; i < n_items; i += 256) f(key_at(i), i);
        } else {
            topk_scan_row<KT>(row, n_items, tid, bm, f);
        }
    };
    // ---- 1. per-thread maxima: the c = ceil(K / 256) largest keys of the thread's elements
    const int c = (K + 255) / 256;              // 1 .. 4
    TopkMaxima<key_t> mx;
    if (c == 1) scan([&](key_t k, int) { mx.t0 = k > mx.t0 ? k : mx.t0; });
    else scan([&](key_t k, int) { mx.ins(k); });
    // ---- 2. the lower bound L of the row's K-th largest key
    const key_t L = topk_lower_bound(sel, mx, c, K, tid);
    // ---- 3. collect the elements >= L: per-thread counts, block prefix sum, placement (any order: they are ranked next); more than
    //         RTX_TOPK_MAX of them: the K largest by radix select, the lowest ids among the ties at the K-th place
    uint32_t mine = 0;
    scan([&](key_t k, int) { mine += k >= L; });
    uint32_t n_cand;
    uint32_t pos = topk_place_prefix(sel, mine, tid, n_cand);
    int n_rank = (int)n_cand;
    if (n_cand <= (uint32_t)RTX_TOPK_MAX) {
        scan([&](key_t k, int i) { if (k >= L) { sel.ckey[pos] = k; sel.cidx[pos] = i; ++pos; } });
    } else {
        topk_radix_select(sel, scan, key_at, L, K, n_items, tid);
        n_rank = K;
    }
    __syncthreads();
    // ---- 4. rank the candidates (key descending, id ascending among equal keys): the ranks < K are the list, in order.  The score
    //         is the input element itself (its sign of zero included); an excluded item reports -inf
    const int r4n = (n_rank + 3) >> 2;
    T* out_scores = (T*)a.item_scores;
    for (int p = tid; p < n_rank; p += 256) {
        const int32_t id = sel.cidx[p];
        const uint32_t r = topk_rank_of(sel.ckey, sel.cidx, r4n, sel.ckey[p], id);
        if (r < (uint32_t)K) {
            a.items[(size_t)b * K + r] = id;
            if (out_scores) out_scores[(size_t)b * K + r] = (bm && topk_excl_bit(bm, id)) ? KT::neg_inf() : row[id];
        }
    }
}

#define RTX_ITEMS_BURST 20                  // float rows of up to 20 * 1024 items stay in registers (ml-20m: 20 108)
#define RTX_ITEMS_EXCL_LDS (48 * 1024)      // bytes of dynamic LDS the exclusion bitmap may take: rows of up to 393 216 items

int rtx_launch_topk_items(const void* scores, int is_f64, long ld, int B, int n_items, const RtxCsrView* excl, int k, int32_t* items,
                          void* item_scores, hipStream_t stream)
{
    RTX_CHECK(k >= 1 && k <= RTX_TOPK_MAX, RTX_EINVAL, "topk_items: k must be in [1, %d], got %d", RTX_TOPK_MAX, k);
    RTX_CHECK(n_items >= 1 && ld >= n_items, RTX_EINVAL, "topk_items: n_items = %d, ld = %ld", n_items, ld);
    if (B <= 0) return RTX_OK;
    RtxItemsArgs a = {};
    a.scores = scores; a.ld = ld; a.n_items = n_items; a.K = k < n_items ? k : n_items;
    a.items = items; a.item_scores = item_scores;
    size_t lds = 0;
    if (excl) {
        lds = (size_t)((n_items + 31) / 32) * sizeof(uint32_t);
        RTX_CHECK(lds <= RTX_ITEMS_EXCL_LDS, RTX_EINVAL, "topk_items: the exclusion bitmap of a %d-item row needs %zu bytes of LDS (limit %d: %d items)",
                  n_items, lds, RTX_ITEMS_EXCL_LDS, RTX_ITEMS_EXCL_LDS * 8);
        a.excl = *excl; a.has_excl = 1;
    }
    if (is_f64) {
        hipLaunchKernelGGL((k_topk_items<double, 0>), dim3(B), dim3(256), lds, stream, a);
    } else {
        const bool burst = (((uintptr_t)scores) & 15) == 0 && (ld & 3) == 0 && n_items <= RTX_ITEMS_BURST * 1024;
        if (burst) hipLaunchKernelGGL((k_topk_items<float, RTX_ITEMS_BURST>), dim3(B), dim3(256), lds, stream, a);
        else hipLaunchKernelGGL((k_topk_items<float, 0>), dim3(B), dim3(256), lds, stream, a);
    }
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
