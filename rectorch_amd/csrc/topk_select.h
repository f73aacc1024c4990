// topk_select.h -- exact top-K selection of a score row by one workgroup of 256 threads: every stage that the ranking-metrics kernel
// (topk.hip, float rows, 32-bit keys) and the top-N list kernel (recommend.hip, float / double rows, 32- / 64-bit keys) share.
//   keys        TopkKey<T, ZERO_EQ>: order-preserving unsigned keys of float / double scores
//   exclusion   topk_excl_build / topk_excl_bit / topk_excl_mask4: a bitmap of the batch row's stored entries, which rank as -inf
//   row access  topk_key_at, topk_scan_row: the row streamed from memory as keys, exclusion applied
//   selection   TopkMaxima (per-thread maxima) -> topk_lower_bound (L, by counting) -> topk_place_prefix (slots of the elements >= L)
//               -> topk_radix_select (more than RTX_TOPK_MAX elements >= L) -> topk_count_gt / topk_rank_of (ranks by counting)
#pragma once
#include <stdint.h>

#define RTX_TOPK_MAX 1024

#ifdef __HIPCC__
#include "rtx_device.h"

// Order-preserving keys: ascending in the floating-point order, -inf lowest, every real key > 0 (key 0 pads the candidate arrays).
// ZERO_EQ: -0.0 and +0.0 share one key (equal keys are equal VALUES: what a list needs); without it the map is monotonic in the
// bit pattern and -0.0 sorts below +0.0 (no metric notices).
template <typename T> struct TopkBits;
template <> struct TopkBits<float> {
    typedef uint32_t key_t;
    typedef float4 vec_t;
    static constexpr int VEC = 4;               // elements per 16-byte load
    static __device__ __forceinline__ key_t bits(float f) { return __float_as_uint(f); }
};
template <> struct TopkBits<double> {
    typedef uint64_t key_t;
    typedef double2 vec_t;
    static constexpr int VEC = 2;
    static __device__ __forceinline__ key_t bits(double f) { return (uint64_t)__double_as_longlong(f); }
};
template <typename T, bool ZERO_EQ> struct TopkKey : TopkBits<T> {
    typedef T elem_t;
    typedef typename TopkBits<T>::key_t key_t;
    static constexpr key_t SIGN = (key_t)1 << (sizeof(key_t) * 8 - 1);
    static __device__ __forceinline__ key_t key(T f)
    {
        key_t b = TopkBits<T>::bits(f);
        if constexpr (ZERO_EQ) b = b == SIGN ? (key_t)0 : b;
        return (b & SIGN) ? ~b : (b | SIGN);
    }
    static __device__ __forceinline__ T neg_inf() { return -(T)INFINITY; }
    static __device__ __forceinline__ key_t neg_key() { return key(neg_inf()); }
};

// ---- exclusion bitmap: one bit per item of the row, set where batch row b of `excl` stores a non-zero entry.  nw words are cleared
//      (>= ceil(n_items / 32)); one atomicOr per stored entry; both barriers are inside
__device__ __forceinline__ void topk_excl_build(uint32_t* bm, int nw, const RtxCsrView& excl, int b, int n_items, int tid)
{
    for (int i = tid; i < nw; i += 256) bm[i] = 0u;
    __syncthreads();
    const int64_t ue = csr_row(excl, b);
    for (int64_t k = excl.indptr[ue] + tid; k < excl.indptr[ue + 1]; k += 256) {
        const float val = excl.values ? excl.values[k] : 1.f;
        const int i = excl.indices[k];
        if (val != 0.f && i >= 0 && i < n_items) atomicOr(&bm[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
}

__device__ __forceinline__ bool topk_excl_bit(const uint32_t* bm, int i) { return (bm[i >> 5] >> (i & 31)) & 1u; }

// the register keys of items 4 j .. 4 j + 3 (bits (4 j) & 31 .. of word j >> 3, which the caller knows to exist): excluded ones become neg
__device__ __forceinline__ void topk_excl_mask4(uint4& kv, const uint32_t* bm, int j, uint32_t neg)
{
    const uint32_t nib = (bm[j >> 3] >> ((j & 7) * 4)) & 15u;
    if (nib) {
        if (nib & 1u) kv.x = neg;
        if (nib & 2u) kv.y = neg;
        if (nib & 4u) kv.z = neg;
        if (nib & 8u) kv.w = neg;
    }
}

// ---- the row read from memory as keys; bm: the exclusion bitmap (nullable)
template <typename KP>
__device__ __forceinline__ typename KP::key_t topk_key_at(const typename KP::elem_t* __restrict__ row, const uint32_t* bm, int i)
{
    return (bm && topk_excl_bit(bm, i)) ? KP::neg_key() : KP::key(row[i]);
}

// f(key, index) for the VEC neighbours of one 16-byte load, items i0 .. i0 + VEC - 1 (i0 a multiple of VEC: their exclusion bits lie
// in one bitmap word)
template <typename KP, typename F> __device__ __forceinline__ void topk_emit(const typename KP::vec_t& v, int i0, const uint32_t* bm, F&& f)
{
    const typename KP::key_t NEG = KP::neg_key();
    const uint32_t bits = bm ? (bm[i0 >> 5] >> (i0 & 31)) : 0u;
    f((bits & 1u) ? NEG : KP::key(v.x), i0);
    f((bits & 2u) ? NEG : KP::key(v.y), i0 + 1);
    if constexpr (KP::VEC == 4) {
        f((bits & 4u) ? NEG : KP::key(v.z), i0 + 2);
        f((bits & 8u) ? NEG : KP::key(v.w), i0 + 3);
    }
}

// f(key, index) for every element of a score row streamed from memory.  16-byte loads, eight of them in flight per thread, wherever
// the row is 16-byte aligned (4-byte loads walked an 80-KB row in 79 dependent round trips per thread -- with two workgroups per CU
// there is nothing to hide them behind: profiles/r5_eval_kernel_stats.txt); a scalar loop for the tail or an unaligned row
template <typename KP, typename F>
__device__ __forceinline__ void topk_scan_row(const typename KP::elem_t* __restrict__ row, int n_items, int tid, const uint32_t* bm, F&& f)
{
    typedef typename KP::vec_t vec_t;
    constexpr int VEC = KP::VEC;
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
            for (int u = 0; u < 8; ++u) topk_emit<KP>(v[u], (j + u * 256) * VEC, bm, f);
        }
        for (; j < nv; j += 256) topk_emit<KP>(rv[j], j * VEC, bm, f);
        done = nv * VEC;
    }
    for (int i = done + tid; i < n_items; i += 256) f(topk_key_at<KP>(row, bm, i), i);
}

// ---- order statistics by counting over (key, id) pairs in LDS: every thread compares its key with all the others through broadcast
//      reads (16 bytes per instruction, every lane the same address: no bank conflict).
// rank (0 = first) of element (k, id) among the n (key, id) pairs in LDS, ordered by key descending, id ascending among equal keys;
// n4 = ceil(n / 4): the arrays are padded to a multiple of 4 with (key 0, id INT_MAX): below every real element
__device__ __forceinline__ uint32_t topk_rank_of(const uint32_t* __restrict__ keys, const int32_t* __restrict__ ids, int n4, uint32_t k, int32_t id)
{
    uint32_t r0 = 0, r1 = 0;
    const uint4* k4 = (const uint4*)keys;
    const int4* i4 = (const int4*)ids;
    for (int i = 0; i < n4; ++i) {
        const uint4 q = k4[i];
        const int4 d = i4[i];
        r0 += (q.x > k) + ((q.x == k) & (d.x < id)) + (q.y > k) + ((q.y == k) & (d.y < id));
        r1 += (q.z > k) + ((q.z == k) & (d.z < id)) + (q.w > k) + ((q.w == k) & (d.w < id));
    }
    return r0 + r1;
}

// number of keys greater than k among the n4 * 4 keys in LDS (two instructions per key: a compare and an add-with-carry)
__device__ __forceinline__ uint32_t topk_count_gt(const uint32_t* __restrict__ keys, int n4, uint32_t k)
{
    uint32_t g0 = 0, g1 = 0;
    const uint4* k4 = (const uint4*)keys;
    for (int i = 0; i < n4; ++i) {
        const uint4 q = k4[i];
        g0 += (q.x > k) + (q.y > k);
        g1 += (q.z > k) + (q.w > k);
    }
    return g0 + g1;
}

// the same two for 64-bit keys (float64 score rows): 16 bytes = 2 keys per LDS read
__device__ __forceinline__ uint32_t topk_rank_of(const uint64_t* __restrict__ keys, const int32_t* __restrict__ ids, int n4, uint64_t k, int32_t id)
{
    uint32_t r0 = 0, r1 = 0;
    const ulonglong2* k2 = (const ulonglong2*)keys;
    const int4* i4 = (const int4*)ids;
    for (int i = 0; i < n4; ++i) {
        const ulonglong2 qa = k2[2 * i], qb = k2[2 * i + 1];
        const int4 d = i4[i];
        r0 += (qa.x > k) + ((qa.x == k) & (d.x < id)) + (qa.y > k) + ((qa.y == k) & (d.y < id));
        r1 += (qb.x > k) + ((qb.x == k) & (d.z < id)) + (qb.y > k) + ((qb.y == k) & (d.w < id));
    }
    return r0 + r1;
}

__device__ __forceinline__ uint32_t topk_count_gt(const uint64_t* __restrict__ keys, int n4, uint64_t k)
{
    uint32_t g0 = 0, g1 = 0;
    const ulonglong2* k2 = (const ulonglong2*)keys;
    for (int i = 0; i < n4; ++i) {
        const ulonglong2 qa = k2[2 * i], qb = k2[2 * i + 1];
        g0 += (qa.x > k) + (qa.y > k);
        g1 += (qb.x > k) + (qb.y > k);
    }
    return g0 + g1;
}

__device__ __forceinline__ uint32_t topk_shfl_xor(uint32_t v, int o) { return (uint32_t)__shfl_xor((int)v, o, 64); }
__device__ __forceinline__ uint64_t topk_shfl_xor(uint64_t v, int o) { return (uint64_t)__shfl_xor((unsigned long long)v, o, 64); }

// ---- the selection's LDS: one __shared__ object per kernel
template <typename KEY> struct TopkLds {
    __attribute__((aligned(16))) KEY ckey[RTX_TOPK_MAX];        // the thread maxima, then the candidates' keys (padding: 0)
    __attribute__((aligned(16))) int32_t cidx[RTX_TOPK_MAX];    // the candidates' item ids (padding: INT_MAX)
    // radix select: a counter per digit.  Outside its passes the first words carry the few values that cross the waves: before
    // them the four wave minima of the bound (wmin), after them the waves' counts of keys above / equal to the K-th (wcnt)
    __attribute__((aligned(8))) uint32_t hist[256];
    uint32_t wsum[4];                                           // the waves' candidate counts
    KEY prefix;                                                 // radix select: the digits fixed so far
    uint32_t need;                                              //   and the rank looked for among the keys that share them
    __device__ __forceinline__ KEY* wmin() { return (KEY*)hist; }
    __device__ __forceinline__ uint32_t* wcnt() { return hist; }
};

// ---- 1. the thread's four largest keys, descending (0 = below every real key)
template <typename KEY> struct TopkMaxima {
    KEY t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    __device__ __forceinline__ void ins(KEY k)
    {
        if (k > t0) { const KEY x = t0; t0 = k; k = x; }
        if (k > t1) { const KEY x = t1; t1 = k; k = x; }
        if (k > t2) { const KEY x = t2; t2 = k; k = x; }
        if (k > t3) t3 = k;
    }
};

// ---- 2. L = K-th largest of the 256 c thread maxima (c = ceil(K / 256) per thread): a LOWER BOUND of the row's K-th largest key
//         (they are distinct elements).  L = the smallest maximum that fewer than K maxima exceed: only "greater than" counts are
//         needed, ties included.  A row of fewer than K elements gives a padding key, 0: everything is collected.
//         Two barriers; whatever the caller stored to LDS before the call is visible after it
template <typename KEY> __device__ __forceinline__ KEY topk_lower_bound(TopkLds<KEY>& s, const TopkMaxima<KEY>& m, int c, int K, int tid)
{
    const int n1 = c == 1 ? 256 : (c == 2 ? 512 : 1024);
    s.ckey[tid] = m.t0;
    if (c >= 2) s.ckey[256 + tid] = m.t1;
    if (c >= 3) { s.ckey[512 + tid] = m.t2; s.ckey[768 + tid] = c >= 4 ? m.t3 : (KEY)0; }
    __syncthreads();
    KEY cand = ~(KEY)0;
    if (topk_count_gt(s.ckey, n1 / 4, m.t0) < (uint32_t)K) cand = m.t0;
    if (c >= 2) {
        if (topk_count_gt(s.ckey, n1 / 4, m.t1) < (uint32_t)K) cand = m.t1 < cand ? m.t1 : cand;
        if (c >= 3) {
            if (topk_count_gt(s.ckey, n1 / 4, m.t2) < (uint32_t)K) cand = m.t2 < cand ? m.t2 : cand;
            if (c >= 4 && topk_count_gt(s.ckey, n1 / 4, m.t3) < (uint32_t)K) cand = m.t3 < cand ? m.t3 : cand;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const KEY x = topk_shfl_xor(cand, o);
        cand = x < cand ? x : cand;
    }
    if ((tid & 63) == 0) s.wmin()[tid >> 6] = cand;
    __syncthreads();
    KEY L = s.wmin()[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) L = s.wmin()[w] < L ? s.wmin()[w] : L;
    return L;
}

// ---- 3. slots for the elements >= L: `mine` of them in this thread; returns the thread's first slot (block prefix sum: no
//         atomics; any order will do, they are ranked next) and their number in the row.  The candidate arrays are cleared to
//         padding (everybody has read the maxima: the barrier of topk_lower_bound).  One barrier
template <typename KEY> __device__ __forceinline__ uint32_t topk_place_prefix(TopkLds<KEY>& s, uint32_t mine, int tid, uint32_t& n_cand)
{
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s.wsum[wave] = incl;
    for (int i = tid; i < RTX_TOPK_MAX; i += 256) { s.ckey[i] = 0; s.cidx[i] = 0x7fffffff; }
    __syncthreads();
    uint32_t base = incl - mine;
    for (int w = 0; w < wave; ++w) base += s.wsum[w];
    n_cand = s.wsum[0] + s.wsum[1] + s.wsum[2] + s.wsum[3];
    return base;
}

// ---- more than RTX_TOPK_MAX elements at / above the bound.  Not a tie path only: L is the K-th of 256 c maxima, so this runs on
//      most rows for K at or just below a multiple of 256 and for K >= ~500 at ml-20m width, and on every row whose excluded items
//      leave fewer than K finite scores.  Radix select of the K-th largest key T, one byte per pass from the top, over the elements
//      >= L only (T is among them: the LDS atomics are per candidate, not per item); then the K - need_eq keys above T and the
//      need_eq LOWEST ids among the keys equal to T are placed: a wave walks its quarter of the row in id order and places by
//      ballot prefix -- no atomic counter, whose order would change from launch to launch.
//      scan(f): f(key, index) for every element of the row; key_at(i): element i's key -- both with the exclusion applied.
//      The candidate arrays hold padding on entry (topk_place_prefix) and K candidates after the caller's next barrier
template <typename KEY, typename SCAN, typename KEYAT>
__device__ __forceinline__ void topk_radix_select(TopkLds<KEY>& s, SCAN&& scan, KEYAT&& key_at, KEY L, int K, int n_items, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s.prefix = 0; s.need = (uint32_t)K; }
    for (int shift = (int)sizeof(KEY) * 8 - 8; shift >= 0; shift -= 8) {
        s.hist[tid] = 0;
        __syncthreads();
        const KEY prefix = s.prefix, mask = ~(((KEY)256 << shift) - 1);      // the digits above this pass's
        scan([&](KEY k, int) { if (k >= L && (k & mask) == prefix) atomicAdd(&s.hist[(uint32_t)(k >> shift) & 255u], 1u); });
        __syncthreads();
        if (tid == 0) {
            uint32_t need = s.need, d = 255;
            for (;; --d) {            // from the largest digit down
                if (s.hist[d] >= need || d == 0) break;
                need -= s.hist[d];
            }
            s.need = need;            // rank inside digit d
            s.prefix = prefix | ((KEY)d << shift);
        }
        __syncthreads();
    }
    const KEY T = s.prefix;
    const uint32_t need_eq = s.need;    // how many elements equal to T belong to the top K: the K - need_eq above it all do
    // wave w owns items [w * seg, (w + 1) * seg) and walks them in id order: counts first, then placement by ballot prefix.
    // Above T: slots [0, K - need_eq), any order; equal to T: the need_eq lowest ids, slots behind them
    const int seg = (((n_items + 3) >> 2) + 63) & ~63;
    const int lo = min(wave * seg, n_items), hi = min(lo + seg, n_items);
    uint32_t cgt = 0, ceq = 0;
    for (int i = lo + lane; i < hi; i += 64) {
        const KEY k = key_at(i);
        cgt += k > T;
        ceq += k == T;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cgt += __shfl_xor(cgt, o, 64); ceq += __shfl_xor(ceq, o, 64); }
    uint32_t* wcnt = s.wcnt();          // (thread 0 has read the last pass's counters: the barrier above)
    if (lane == 0) { wcnt[wave] = cgt; wcnt[4 + wave] = ceq; }
    __syncthreads();
    uint32_t pgt = 0, peq = 0;
    for (int w = 0; w < wave; ++w) { pgt += wcnt[w]; peq += wcnt[4 + w]; }
    const uint32_t n_gt = (uint32_t)K - need_eq;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const KEY k = i < hi ? key_at(i) : (KEY)0;
        const bool gt = k > T, eq = k == T;
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        if (gt) {
            const uint32_t p = pgt + (uint32_t)__popcll(mg & below);
            if (p < n_gt) { s.ckey[p] = k; s.cidx[p] = i; }
        }
        if (eq) {
            const uint32_t p = peq + (uint32_t)__popcll(me & below);
            if (p < need_eq) { s.ckey[n_gt + p] = k; s.cidx[n_gt + p] = i; }
        }
        pgt += (uint32_t)__popcll(mg);
        peq += (uint32_t)__popcll(me);
    }
}
#endif
