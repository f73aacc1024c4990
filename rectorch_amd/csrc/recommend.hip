// recommend.hip -- top-N recommendation lists on gfx950 (k_topk_items): per user row the K best items and their scores.
#include "rtx_device.h"
#include "topk_select.h"
#include <cmath>

// ------------------------------------------------------------------------------------------------
// What a recommender is for (reference: the lists behind rectorch/metrics.py's argpartition + argsort; evaluation.py:100-106 hands the
// score matrix to the host for it).  One workgroup per user row; the selection scheme is k_topk_metrics' (topk.hip): per-thread maxima,
// a lower bound L of the K-th largest score by counting, the elements >= L collected and ranked, a radix select when more than
// RTX_TOPK_MAX elements reach the bound.  What differs:
//   * the ORDER is total: score descending, item id ascending among equal scores, and "equal" is floating-point equality -- the key
//     maps -0.0 and +0.0 to one value (score_key of topk.hip orders them, which no metric notices and a list shows);
//   * float64 rows (EASE, ADMM_Slim) on 64-bit keys: scores that differ below float32 resolution keep their order;
//   * the exclusion bitmap (the user's train items rank as -inf, nothing is written to the scores) sits in dynamic LDS sized by the
//     row, so the streamed form of the kernel has it too;
//   * the radix select looks only at the elements >= L (the K-th largest is among them), so its LDS atomics are per candidate, not per
//     item, and takes the LOWEST ids among the ties at the K-th place: a wave walks its quarter of the row in id order and places by
//     ballot prefix -- no atomic counter.
// NaN scores are out of contract (their keys sort above +inf or below -inf by sign).
// ------------------------------------------------------------------------------------------------
template <typename T> struct ItemKey;
template <> struct ItemKey<float> {
    typedef uint32_t key_t;
    typedef float4 vec_t;
    static constexpr int VEC = 4;
    static __device__ __forceinline__ key_t key(float f)
    {
        uint32_t b = __float_as_uint(f);
        b = b == 0x80000000u ? 0u : b;                         // -0.0 == +0.0
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);     // ascending in the float order, -inf lowest, every real key > 0
    }
    static __device__ __forceinline__ float neg_inf() { return -INFINITY; }
};
template <> struct ItemKey<double> {
    typedef uint64_t key_t;
    typedef double2 vec_t;
    static constexpr int VEC = 2;
    static __device__ __forceinline__ key_t key(double f)
    {
        uint64_t b = (uint64_t)__double_as_longlong(f);
        b = b == 0x8000000000000000ull ? 0ull : b;
        return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double neg_inf() { return -(double)INFINITY; }
};

struct RtxItemsArgs {
    const void* scores;     // T [B][ld]
    long ld;
    int n_items, K;         // 1 <= K <= min(RTX_TOPK_MAX, n_items)
    RtxCsrView excl;        // has_excl: batch row b's stored non-zero entries (< n_items) rank as -inf
    int has_excl;
    int32_t* items;         // [B][K]
    void* item_scores;      // T [B][K]  (nullable)
};

__device__ __forceinline__ bool items_bit(const uint32_t* bm, int i) { return (bm[i >> 5] >> (i & 31)) & 1u; }

// f(key, index) for the VEC neighbours of one 16-byte load, items i0 .. i0 + VEC - 1 (i0 a multiple of VEC: their exclusion bits lie
// in one bitmap word)
template <typename T, typename F>
__device__ __forceinline__ void items_emit(const typename ItemKey<T>::vec_t& v, int i0, const uint32_t* bm, F&& f)
{
    typedef ItemKey<T> KT;
    const typename KT::key_t NEG = KT::key(KT::neg_inf());
    const uint32_t bits = bm ? (bm[i0 >> 5] >> (i0 & 31)) : 0u;
    f((bits & 1u) ? NEG : KT::key(v.x), i0);
    f((bits & 2u) ? NEG : KT::key(v.y), i0 + 1);
    if constexpr (KT::VEC == 4) {
        f((bits & 4u) ? NEG : KT::key(v.z), i0 + 2);
        f((bits & 8u) ? NEG : KT::key(v.w), i0 + 3);
    }
}

// f(key, index) for every element of a score row read from memory (topk_scan_row of topk.hip for both element types, with the
// exclusion): 16-byte loads, eight in flight per thread, wherever the row is 16-byte aligned; bm: the exclusion bitmap (nullable)
template <typename T, typename F>
__device__ __forceinline__ void items_scan_row(const T* __restrict__ row, int n_items, int tid, const uint32_t* bm, F&& f)
{
    typedef ItemKey<T> KT;
    typedef typename KT::vec_t vec_t;
    constexpr int VEC = KT::VEC;
    int done = 0;
    if ((((uintptr_t)row) & 15) == 0) {
        const int nv = n_items / VEC;
        const vec_t* __restrict__ rv = (const vec_t*)row;
        int j = tid;
        for (; j + 7 * 256 < nv; j += 8 * 256) {
            vec_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = rv[j + u * 256];
#pragma unroll
            for (int u = 0; u < 8; ++u) items_emit<T>(v[u], (j + u * 256) * VEC, bm, f);
        }
        for (; j < nv; j += 256) items_emit<T>(rv[j], j * VEC, bm, f);
        done = nv * VEC;
    }
    const typename KT::key_t NEG = KT::key(KT::neg_inf());
    for (int i = done + tid; i < n_items; i += 256) f((bm && items_bit(bm, i)) ? NEG : KT::key(row[i]), i);
}

template <typename KEY> __device__ __forceinline__ KEY items_shfl_xor(KEY v, int o);
template <> __device__ __forceinline__ uint32_t items_shfl_xor<uint32_t>(uint32_t v, int o) { return (uint32_t)__shfl_xor((int)v, o, 64); }
template <> __device__ __forceinline__ uint64_t items_shfl_xor<uint64_t>(uint64_t v, int o)
{
    return (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
}

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
    __shared__ __attribute__((aligned(16))) key_t ckey[RTX_TOPK_MAX];
    __shared__ __attribute__((aligned(16))) int32_t cidx[RTX_TOPK_MAX];
    __shared__ uint32_t hist[256];
    __shared__ key_t wmin[4];
    __shared__ uint32_t wsum[8];
    __shared__ key_t sh_prefix, sh_mask;
    __shared__ uint32_t sh_need;
    extern __shared__ uint32_t excl_bm[];       // has_excl: one bit per item of the row, ceil(n_items / 32) words
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* row = (const T*)a.scores + (size_t)b * a.ld;
    const int K = a.K, n_items = a.n_items;
    const key_t NEG = KT::key(KT::neg_inf());
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
        const int nw = (n_items + 31) >> 5;
        for (int i = tid; i < nw; i += 256) excl_bm[i] = 0u;
        __syncthreads();
        const int64_t ue = csr_row(a.excl, b);
        for (int64_t k = a.excl.indptr[ue] + tid; k < a.excl.indptr[ue + 1]; k += 256) {
            const float val = a.excl.values ? a.excl.values[k] : 1.f;
            const int i = a.excl.indices[k];
            if (val != 0.f && i >= 0 && i < n_items) atomicOr(&excl_bm[i >> 5], 1u << (i & 31));
        }
        __syncthreads();
        bm = excl_bm;
    }
    uint4 kv[NV > 0 ? NV : 1];
    if constexpr (NV > 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            kv[q] = make_uint4(KT::key(rv[q].x), KT::key(rv[q].y), KT::key(rv[q].z), KT::key(rv[q].w));
            const int j = tid + q * 256;              // items 4 j .. 4 j + 3: bits (4 j) & 31 .. of word j >> 3
            const uint32_t nib = (bm && j < n4) ? (bm[j >> 3] >> ((j & 7) * 4)) & 15u : 0u;
            if (nib) {
                if (nib & 1u) kv[q].x = NEG;
                if (nib & 2u) kv[q].y = NEG;
                if (nib & 4u) kv[q].z = NEG;
                if (nib & 8u) kv[q].w = NEG;
            }
        }
    }
    auto key_at = [&](int i) __attribute__((always_inline)) -> key_t { return (bm && items_bit(bm, i)) ? NEG : KT::key(row[i]); };
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
            items_scan_row<T>(row, n_items, tid, bm, f);
        }
    };
    // ---- 1. per-thread maxima: the c = ceil(K / 256) largest keys of the thread's elements (0 = below every real key)
    const int c = (K + 255) / 256;              // 1 .. 4
    key_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    if (c == 1) {
        scan([&](key_t k, int) { t0 = k > t0 ? k : t0; });
    } else {
        scan([&](key_t k, int) {
            if (k > t0) { const key_t x = t0; t0 = k; k = x; }
            if (k > t1) { const key_t x = t1; t1 = k; k = x; }
            if (k > t2) { const key_t x = t2; t2 = k; k = x; }
            if (k > t3) t3 = k;
        });
    }
    // ---- 2. L = K-th largest of the 256 c thread maxima: a LOWER BOUND of the row's K-th largest key (they are distinct elements).
    //         L = the smallest maximum that fewer than K maxima exceed
    const int n1 = c == 1 ? 256 : (c == 2 ? 512 : 1024);
    ckey[tid] = t0;
    if (c >= 2) ckey[256 + tid] = t1;
    if (c >= 3) { ckey[512 + tid] = t2; ckey[768 + tid] = c >= 4 ? t3 : (key_t)0; }
    __syncthreads();
    {
        key_t cand = ~(key_t)0;
        if (topk_count_gt(ckey, n1 / 4, t0) < (uint32_t)K) cand = t0;
        if (c >= 2) {
            if (topk_count_gt(ckey, n1 / 4, t1) < (uint32_t)K) cand = t1 < cand ? t1 : cand;
            if (c >= 3) {
                if (topk_count_gt(ckey, n1 / 4, t2) < (uint32_t)K) cand = t2 < cand ? t2 : cand;
                if (c >= 4 && topk_count_gt(ckey, n1 / 4, t3) < (uint32_t)K) cand = t3 < cand ? t3 : cand;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const key_t x = items_shfl_xor<key_t>(cand, o);
            cand = x < cand ? x : cand;
        }
        if (lane == 0) wmin[wave] = cand;
    }
    __syncthreads();
    key_t L = wmin[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) L = wmin[w] < L ? wmin[w] : L;
    // ---- 3. collect the elements >= L: per-thread counts, block prefix sum, placement (any order: they are ranked next)
    uint32_t mine = 0;
    scan([&](key_t k, int) { mine += k >= L; });
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    for (int i = tid; i < RTX_TOPK_MAX; i += 256) { ckey[i] = 0; cidx[i] = 0x7fffffff; }   // (everybody has read the maxima: barrier above)
    __syncthreads();
    uint32_t base = incl - mine;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    const uint32_t n_cand = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    int n_rank = (int)n_cand;
    if (n_cand <= (uint32_t)RTX_TOPK_MAX) {
        uint32_t pos = base;
        scan([&](key_t k, int i) { if (k >= L) { ckey[pos] = k; cidx[pos] = i; ++pos; } });
    } else {
        // ---- more than RTX_TOPK_MAX elements at / above the bound (ties, K near a multiple of 256, few items left by the exclusion):
        //      radix select of the K-th largest key T among them, one byte per pass from the top
        if (tid == 0) { sh_prefix = 0; sh_mask = 0; sh_need = (uint32_t)K; }
        for (int shift = (int)sizeof(key_t) * 8 - 8; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            const key_t prefix = sh_prefix, mask = sh_mask;
            scan([&](key_t k, int) { if (k >= L && (k & mask) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & 255u], 1u); });
            __syncthreads();
            if (tid == 0) {
                uint32_t need = sh_need, d = 255;
                for (;; --d) {            // from the largest digit down
                    if (hist[d] >= need || d == 0) break;
                    need -= hist[d];
                }
                sh_need = need;           // rank inside digit d
                sh_prefix = prefix | ((key_t)d << shift);
                sh_mask = mask | ((key_t)255 << shift);
            }
            __syncthreads();
        }
        const key_t Tk = sh_prefix;
        const uint32_t need_eq = sh_need;   // how many elements equal to Tk belong to the top K: the K - need_eq above it all do
        // wave w owns items [w * seg, (w + 1) * seg) and walks them in id order: counts first, then placement by ballot prefix.
        // Above Tk: slots [0, K - need_eq), any order; equal to Tk: the need_eq lowest ids, slots behind them
        const int seg = (((n_items + 3) >> 2) + 63) & ~63;
        const int lo = min(wave * seg, n_items), hi = min(lo + seg, n_items);
        uint32_t cgt = 0, ceq = 0;
        for (int i = lo + lane; i < hi; i += 64) {
            const key_t k = key_at(i);
            cgt += k > Tk;
            ceq += k == Tk;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { cgt += __shfl_xor(cgt, o, 64); ceq += __shfl_xor(ceq, o, 64); }
        if (lane == 0) { wsum[wave] = cgt; wsum[4 + wave] = ceq; }
        __syncthreads();
        uint32_t pgt = 0, peq = 0;
        for (int w = 0; w < wave; ++w) { pgt += wsum[w]; peq += wsum[4 + w]; }
        const uint32_t n_gt = (uint32_t)K - need_eq;
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int i0 = lo; i0 < hi; i0 += 64) {
            const int i = i0 + lane;
            const key_t k = i < hi ? key_at(i) : (key_t)0;
            const bool gt = k > Tk, eq = k == Tk;
            const unsigned long long mg = __ballot(gt), me = __ballot(eq);
            if (gt) {
                const uint32_t p = pgt + (uint32_t)__popcll(mg & below);
                if (p < n_gt) { ckey[p] = k; cidx[p] = i; }
            }
            if (eq) {
                const uint32_t p = peq + (uint32_t)__popcll(me & below);
                if (p < need_eq) { ckey[n_gt + p] = k; cidx[n_gt + p] = i; }
            }
            pgt += (uint32_t)__popcll(mg);
            peq += (uint32_t)__popcll(me);
        }
        n_rank = K;
    }
    __syncthreads();
    // ---- 4. rank the candidates (key descending, id ascending among equal keys): the ranks < K are the list, in order.  The score
    //         is the input element itself (its sign of zero included); an excluded item reports -inf
    const int r4n = (n_rank + 3) >> 2;
    T* out_scores = (T*)a.item_scores;
    for (int p = tid; p < n_rank; p += 256) {
        const int32_t id = cidx[p];
        const uint32_t r = topk_rank_of(ckey, cidx, r4n, ckey[p], id);
        if (r < (uint32_t)K) {
            a.items[(size_t)b * K + r] = id;
            if (out_scores) out_scores[(size_t)b * K + r] = (bm && items_bit(bm, id)) ? KT::neg_inf() : row[id];
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
