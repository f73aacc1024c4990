// topk.hip -- device-side ranking metrics for evaluate() on gfx950 (k_topk_metrics).
#include "rtx_device.h"
#include "topk_select.h"
#include <cmath>
#include <vector>

// ------------------------------------------------------------------------------------------------
// Device-side ranking metrics for evaluate() (reference rectorch/metrics.py:136-147, 187-196):
// per user, exact top-K of the score row on order-preserving keys (a lower bound from per-thread maxima, the few hundred elements above
// it ranked by counting; a radix select only for rows of > 1024 ties), then nDCG@k / Recall@k for every requested k <= K against the held-out CSR row.  Only
// [n_k][B] doubles leave the GPU instead of the [B, n_items] score matrix (40 MB per 500 users at ml-20m).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t score_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending in the float order, -inf lowest
}

struct RtxTopkArgs {
    const float* scores;
    long ld;
    int n_items, K, Kp2;
    RtxCsrView held;
    int n_k;
    int ks[16];
    double* ndcg;     // [n_k][B]  (nullable)
    double* recall;   // [n_k][B]  (nullable)
    int32_t* topk;    // [B][K]    (nullable)
    int B;
    RtxCsrView excl;  // has_excl: the users' rows of the TRAIN matrix -- their stored items (< n_items) rank as -inf without the
    int has_excl;     //   scores being touched (predict(remove_train=True) folded into the selection: rtx_engine_evaluate_topk)
    long out_ld;      // doubles between two cut-offs' rows of ndcg / recall (>= B; B = one [n_k][B] block per call)
    double* hit;      // [n_k][out_ld] 1.0 / 0.0   (nullable; read only by the RANKM instantiations)
    double* mrr;      // [n_k][out_ld]              (nullable; read only by the RANKM instantiations)
};

// Exact top-K of a score row + the ranking metrics.  Round 4: the selection no longer histograms the row.  The 4-pass radix
// select of rounds 1-3 put 20 108 LDS atomics per pass on one or two bins (the scores of a row share sign and exponent bits, so
// the first digits are the same for nearly all of them): 285 us per 500 users, half of evaluate_device (profiles/r4_eval_kernel_stats.txt).
//   1. every thread keeps the c = ceil(K / 256) largest keys of its 79 elements (registers, no atomics);
//   2. the K-th largest of these 256 c keys -- all distinct elements -- is a LOWER BOUND L of the K-th largest score of the row
//      (rounds 4-5: a bitonic sort of <= 1024 keys in LDS; round 6: counting, see k_topk_metrics);
//   3. the elements >= L (a few hundred) are collected and ranked; the first K are the answer.
// More than RTX_TOPK_MAX elements >= L: the radix select below takes over.  It is not a tie path only: L is the K-th of 256 c maxima,
// so it runs on most rows for K at or just below a multiple of 256 and for K >= ~500 at ml-20m width, and on every row whose train
// items leave fewer than K finite scores.  Its passes read the row through key_at, with the train items' exclusion of steps 1-3.
// f(key, index) for every element of a score row.  16-byte loads, eight of them in flight per thread, wherever the row is 16-byte
// aligned (round 5: the 4-byte loads of rounds 1-4 walked the 80-KB row in 79 dependent round trips per thread -- with two
// workgroups per CU there is nothing to hide them behind; 71 -> see profiles/r5_eval_kernel_stats.txt)
template <typename F> __device__ __forceinline__ void topk_scan_row(const float* __restrict__ row, int n_items, int tid, F&& f)
{
    int done = 0;
    if ((((uintptr_t)row) & 15) == 0) {
        const int n4 = n_items >> 2;
        const float4* __restrict__ r4 = (const float4*)row;
        int j = tid;
        for (; j + 7 * 256 < n4; j += 8 * 256) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = r4[j + u * 256];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i0 = (j + u * 256) * 4;
                f(score_key(v[u].x), i0); f(score_key(v[u].y), i0 + 1); f(score_key(v[u].z), i0 + 2); f(score_key(v[u].w), i0 + 3);
            }
        }
        for (; j < n4; j += 256) {
            const float4 v = r4[j];
            const int i0 = j * 4;
            f(score_key(v.x), i0); f(score_key(v.y), i0 + 1); f(score_key(v.z), i0 + 2); f(score_key(v.w), i0 + 3);
        }
        done = n4 * 4;
    }
    for (int i = done + tid; i < n_items; i += 256) f(score_key(row[i]), i);
}

// NV > 0: the whole row (<= NV * 1024 items, 16-byte aligned) is loaded ONCE, NV 16-byte loads per thread in one burst, and stays in
// registers for both passes over it (maxima, collection); NV = 0: the row is streamed twice (any length / alignment).
//
// Round 6: the kernel is ONE workgroup's latency (500 rows = 500 workgroups, all resident at once), and that latency was barriers:
// two bitonic sorts in LDS (36 + 36..45 compare-exchange steps, a __syncthreads each), six two-barrier block sums per cut-off,
// a serial atomic counter for the candidates and four double-precision log2 per thread.  Now
//   * order statistics by COUNTING: every thread ranks its own keys against all the others through broadcast LDS reads (16 bytes
//     = 4 keys per instruction, every lane the same address: no bank conflict) -- one barrier per "sort";
//   * candidates placed by a block prefix sum of per-thread counts (no atomics; the order is irrelevant, they are ranked next);
//   * the held-out row (indices, values) requested at kernel entry together with the score row, parked in LDS: the relevance look-up
//     searches LDS, and its sum / positive count are block sums instead of a serial loop per thread;
//   * every cut-off's three sums reduced together: one barrier for all of them;  log2 only for ranks < K.
// (reference: rectorch/metrics.py:136-147, 187-196; evaluation.py:100-106)
// log2(r + 2) for every rank r < RTX_TOPK_MAX, written once per device by the host (glibc's log2, the function numpy calls in the
// reference's metrics): four software double-precision logarithms per thread were ~8 us of this kernel
__device__ double g_topk_log2[RTX_TOPK_MAX];
#define RTX_TOPK_HELD_CAP 512      // held-out entries of a row parked in LDS (longer rows: the global-memory look-up of rounds 1-5)

__device__ __forceinline__ uint32_t topk_max4(const uint4& q) { return max(max(q.x, q.y), max(q.z, q.w)); }

// RANKM: also hit@k and mrr@k (reference metrics.py:231-238, 272-285).  A template flag, so that the nDCG / Recall launches compile
// to the instructions they had before: the two extra reductions cost registers and a wider LDS block only where they are asked for.
template <int NV, bool RANKM>
__global__ __launch_bounds__(256) void k_topk_metrics(const RtxTopkArgs a)
{
    constexpr int DS = RANKM ? 16 : 12;         // doubles of dred per cut-off: dcg, idcg, hits (+ first relevant rank) per wave
    __shared__ uint32_t hist[256];
    __shared__ __attribute__((aligned(16))) uint32_t ckey[RTX_TOPK_MAX];
    __shared__ __attribute__((aligned(16))) int32_t cidx[RTX_TOPK_MAX];
    __shared__ int32_t sidx[RTX_TOPK_MAX];       // the ranked items
    __shared__ uint32_t relb[RTX_TOPK_MAX];      // step 4: a counter per rank; from step 5 on: the relevance of the ranked item as float bits
    __shared__ int32_t hidx[RTX_TOPK_HELD_CAP];
    __shared__ float hval[RTX_TOPK_HELD_CAP];
    __shared__ double dred[16 * DS];
    __shared__ double hred[8];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t sh_prefix, sh_mask, sh_need, sh_cnt_gt, sh_cnt_eq, sh_L, sh_tie;
    __shared__ uint32_t excl_bm[NV > 0 ? NV * 32 : 1];      // one bit per item of the row: stored in the user's train row
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = a.scores + (size_t)b * a.ld;
    const int K = a.K;
    // ---- 0. everything this workgroup will read from memory is requested here: the held-out row's bounds (uniform: scalar loads),
    //         the score row (NV x 16 B per thread), the held-out entries (<= 2 per thread)
    const int64_t u = csr_row(a.held, b);
    const int64_t hb = a.held.indptr[u], he = a.held.indptr[u + 1];
    const int hn = (int)(he - hb);
    const bool held_in_lds = hn <= RTX_TOPK_HELD_CAP;
    float4 rv[NV > 0 ? NV : 1];
    const int n4 = a.n_items >> 2;
    if constexpr (NV > 0) {
        const float4* __restrict__ r4 = (const float4*)row;
#pragma unroll
        for (int q = 0; q < NV; ++q) rv[q] = r4[min(tid + q * 256, n4 > 0 ? n4 - 1 : 0)];   // (clamped: the guard is at the use)
    }
    double l2r[RTX_TOPK_MAX / 256];             // log2(r + 2) of this thread's ranks (only ranks < K are ever used)
#pragma unroll
    for (int m = 0; m < RTX_TOPK_MAX / 256; ++m) l2r[m] = g_topk_log2[tid + 256 * m];
    int32_t hi0 = 0x7fffffff, hi1 = 0x7fffffff;
    float hv0 = 0.f, hv1 = 0.f;
    if (held_in_lds) {
        if (tid < hn) { hi0 = a.held.indices[hb + tid]; hv0 = a.held.values ? a.held.values[hb + tid] : 1.f; }
        if (tid + 256 < hn) { hi1 = a.held.indices[hb + tid + 256]; hv1 = a.held.values ? a.held.values[hb + tid + 256] : 1.f; }
    }
    // the row as order-preserving keys (registers); f4(keys of four neighbours, index of the first) / f1(key, index) visit every element
    uint4 kv[NV > 0 ? NV : 1];
    if constexpr (NV > 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) kv[q] = make_uint4(score_key(rv[q].x), score_key(rv[q].y), score_key(rv[q].z), score_key(rv[q].w));
    }
    // the user's train items rank as -inf (reference models.py:470-471, 952-953: recon_x[x.nonzero()] = -inf): a bitmap of the row in
    // LDS, set from the train row's stored entries, read back four bits per group of neighbours -- instead of a scatter kernel of its
    // own over the score matrix (5 us per batch of 500)
    const bool use_excl = NV > 0 && a.has_excl;
    if constexpr (NV > 0) {
        if (use_excl) {
            for (int i = tid; i < NV * 32; i += 256) excl_bm[i] = 0u;
            __syncthreads();
            const int64_t ue = csr_row(a.excl, b);
            for (int64_t k = a.excl.indptr[ue] + tid; k < a.excl.indptr[ue + 1]; k += 256) {
                const float val = a.excl.values ? a.excl.values[k] : 1.f;
                const int i = a.excl.indices[k];
                if (val != 0.f && i < a.n_items) atomicOr(&excl_bm[i >> 5], 1u << (i & 31));
            }
            __syncthreads();
            const uint32_t NEG = score_key(-INFINITY);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int j = tid + q * 256;          // items 4 j .. 4 j + 3: bits (4 j) & 31 .. of word j >> 3
                const uint32_t nib = (excl_bm[j >> 3] >> ((j & 7) * 4)) & 15u;
                if (nib) {
                    if (nib & 1u) kv[q].x = NEG;
                    if (nib & 2u) kv[q].y = NEG;
                    if (nib & 4u) kv[q].z = NEG;
                    if (nib & 8u) kv[q].w = NEG;
                }
            }
        }
    }
    // the key of element i read back from memory, with the exclusion applied as in kv[]: the < 4 elements behind the last whole group
    // (NV > 0) and every pass of the radix fall-back read the row through it
    auto key_at = [&](int i) __attribute__((always_inline)) -> uint32_t {
        if (use_excl && ((excl_bm[i >> 5] >> (i & 31)) & 1u)) return score_key(-INFINITY);
        return score_key(row[i]);
    };
    auto scan = [&](auto&& f4, auto&& f1) __attribute__((always_inline)) {
        if constexpr (NV > 0) {
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int j = tid + q * 256;
                if (j < n4) f4(kv[q], j * 4);
            }
            for (int i = n4 * 4 + tid; i < a.n_items; i += 256) f1(key_at(i), i);
        } else {
            topk_scan_row(row, a.n_items, tid, f1);
        }
    };
    // ---- 1. per-thread maxima
    const int c = (K + 255) / 256;              // 1 .. 4
    uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;    // this thread's largest keys, descending (0 = below every real key)
    auto ins = [&](uint32_t k) __attribute__((always_inline)) {
        if (k > t0) { const uint32_t x = t0; t0 = k; k = x; }
        if (k > t1) { const uint32_t x = t1; t1 = k; k = x; }
        if (k > t2) { const uint32_t x = t2; t2 = k; k = x; }
        if (k > t3) t3 = k;
    };
    if (c == 1) scan([&](const uint4& q, int) { t0 = max(t0, topk_max4(q)); }, [&](uint32_t k, int) { t0 = max(t0, k); });
    else scan([&](const uint4& q, int) { ins(q.x); ins(q.y); ins(q.z); ins(q.w); }, [&](uint32_t k, int) { ins(k); });
    // ---- 2. L = K-th largest of the 256 c thread maxima: a LOWER BOUND of the row's K-th largest score (they are distinct elements).
    //         L = the smallest key that fewer than K keys exceed: only "greater than" counts are needed, ties included
    const int n1 = c == 1 ? 256 : (c == 2 ? 512 : 1024);
    ckey[tid] = t0;
    if (c >= 2) ckey[256 + tid] = t1;
    if (c >= 3) { ckey[512 + tid] = t2; ckey[768 + tid] = c >= 4 ? t3 : 0u; }
    if (held_in_lds) { hidx[tid] = hi0; hval[tid] = hv0; hidx[tid + 256] = hi1; hval[tid + 256] = hv1; }
    if (tid == 0) { sh_L = 0xffffffffu; sh_tie = 0; }
    __syncthreads();
    {
        uint32_t cand = 0xffffffffu;
        if (topk_count_gt(ckey, n1 / 4, t0) < (uint32_t)K) cand = t0;
        if (c >= 2) {
            if (topk_count_gt(ckey, n1 / 4, t1) < (uint32_t)K) cand = min(cand, t1);
            if (c >= 3) {
                if (topk_count_gt(ckey, n1 / 4, t2) < (uint32_t)K) cand = min(cand, t2);
                if (c >= 4 && topk_count_gt(ckey, n1 / 4, t3) < (uint32_t)K) cand = min(cand, t3);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cand = min(cand, (uint32_t)__shfl_xor((int)cand, o, 64));
        if (lane == 0) atomicMin(&sh_L, cand);
    }
    __syncthreads();
    const uint32_t L = sh_L;                    // (a row of fewer than K elements: a padding key, 0 -- everything is collected)
    // ---- 3. collect the elements >= L: per-thread counts, block prefix sum, placement.  One element in a hundred qualifies: a group of
    //         four neighbours is looked at only when its maximum does
    uint32_t mine = 0;
    scan([&](const uint4& q, int) { if (topk_max4(q) >= L) mine += (q.x >= L) + (q.y >= L) + (q.z >= L) + (q.w >= L); },
         [&](uint32_t k, int) { mine += k >= L; });
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    for (int i = tid; i < RTX_TOPK_MAX; i += 256) { ckey[i] = 0; cidx[i] = 0x7fffffff; relb[i] = 0u; }   // (everybody has read the maxima: barrier above)
    __syncthreads();
    uint32_t base = incl - mine;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    const uint32_t n_cand = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (n_cand <= (uint32_t)RTX_TOPK_MAX) {
        uint32_t pos = base;
        auto put = [&](uint32_t k, int i) __attribute__((always_inline)) { if (k >= L) { ckey[pos] = k; cidx[pos] = i; ++pos; } };
        scan([&](const uint4& q, int i0) { if (topk_max4(q) >= L) { put(q.x, i0); put(q.y, i0 + 1); put(q.z, i0 + 2); put(q.w, i0 + 3); } }, put);
    }
    __syncthreads();
    int n_rank = (int)n_cand;                   // candidates to rank
    if (n_cand > (uint32_t)RTX_TOPK_MAX) {
        // ---- more than RTX_TOPK_MAX elements at / above the bound: radix select of the K-th largest key T, then everything above T
        //      and need_eq of the ties (ties at the K-th place are arbitrary in the reference's argpartition too); train items as -inf
        if (tid == 0) { sh_prefix = 0; sh_mask = 0; sh_need = (uint32_t)K; }
        __syncthreads();
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            const uint32_t prefix = sh_prefix, mask = sh_mask;
            for (int i = tid; i < a.n_items; i += 256) {
                const uint32_t k = key_at(i);
                if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t need = sh_need, d = 255;
                for (;; --d) {            // from the largest digit down
                    if (hist[d] >= need || d == 0) break;
                    need -= hist[d];
                }
                sh_need = need;           // rank inside digit d
                sh_prefix = prefix | (d << shift);
                sh_mask = mask | (255u << shift);
            }
            __syncthreads();
        }
        const uint32_t T = sh_prefix;
        const uint32_t need_eq = sh_need;   // how many elements equal to T belong to the top K
        if (tid == 0) { sh_cnt_gt = 0; sh_cnt_eq = 0; }
        for (int i = tid; i < RTX_TOPK_MAX; i += 256) { ckey[i] = 0; cidx[i] = 0x7fffffff; }
        __syncthreads();
        for (int i = tid; i < a.n_items; i += 256) {
            const uint32_t k = key_at(i);
            if (k > T) {
                const uint32_t p = atomicAdd(&sh_cnt_gt, 1u);
                if (p < (uint32_t)K) { ckey[p] = k; cidx[p] = i; }
            }
        }
        __syncthreads();
        const uint32_t n_gt = sh_cnt_gt;
        for (int i = tid; i < a.n_items; i += 256) {
            const uint32_t k = key_at(i);
            if (k == T) {
                const uint32_t p = atomicAdd(&sh_cnt_eq, 1u);
                if (p < need_eq && n_gt + p < (uint32_t)K) { ckey[n_gt + p] = k; cidx[n_gt + p] = i; }
            }
        }
        __syncthreads();
        n_rank = K;
    }
    // ---- 4. rank the candidates (key descending, index ascending among equal keys): the ranks < K are the answer, in order.
    //         First by "greater than" counts alone (two instructions per pair); two candidates of one rank below K -- equal scores
    //         among the ranked items: rare -- are noticed through a counter per rank, and only then the exact ranks (ties by index)
    //         are computed.
    for (int i = tid; i < K; i += 256) sidx[i] = 0x7fffffff;     // (a row of fewer than K elements: the tail stays "no item")
    __syncthreads();
    const int r4n = (n_rank + 3) >> 2;
    for (int p = tid; p < n_rank; p += 256) {
        const uint32_t r = topk_count_gt(ckey, r4n, ckey[p]);
        if (r < (uint32_t)K) {
            if (atomicAdd(&relb[r], 1u) != 0u) sh_tie = 1;
            sidx[r] = cidx[p];
        }
    }
    __syncthreads();
    if (sh_tie) {
        for (int p = tid; p < n_rank; p += 256) {
            const int32_t id = cidx[p];
            const uint32_t r = topk_rank_of(ckey, cidx, r4n, ckey[p], id);
            if (r < (uint32_t)K) sidx[r] = id;
        }
        __syncthreads();
    }
    // ---- 5. relevance of every ranked item: value of the held-out row at that item (0 if absent)
    for (int r = tid; r < K; r += 256) {
        const int item = sidx[r];
        float v = 0.f;
        if (held_in_lds) {
            int lo = 0, hi = hn;          // binary search (column ids are sorted within a row)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (hidx[mid] < item) lo = mid + 1; else hi = mid;
            }
            if (lo < hn && hidx[lo] == item) v = hval[lo];
        } else {
            int64_t lo = hb, hi = he;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                const int cc = a.held.indices[mid];
                if (cc < item) lo = mid + 1; else hi = mid;
            }
            if (lo < he && a.held.indices[lo] == item) v = a.held.values ? a.held.values[lo] : 1.f;
        }
        relb[r] = __float_as_uint(v);
        if (a.topk) a.topk[(size_t)b * K + r] = item;
    }
    // ---- 6. metrics.  The terms are the reference's (metrics.py:136-147, 187-196: rel / log2(r + 2), 1 / log2(r + 2)), one rank per
    //      thread and pass, summed in double by a fixed-order block reduction (64-lane butterfly, then the four waves pairwise).
    //      Sum and positive count of the held-out row: block sums over its parked entries (float values are small integers or
    //      ratings: exact in double in any order).
    double gs = 0.0, np = 0.0;
    if (held_in_lds) {
        gs = (double)hv0 + (double)hv1;
        np = (hv0 > 0.f ? 1.0 : 0.0) + (hv1 > 0.f ? 1.0 : 0.0);
    } else {
        for (int64_t k = hb + tid; k < he; k += 256) {
            const float v = a.held.values ? a.held.values[k] : 1.f;
            gs += (double)v;
            np += v > 0.f ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { gs += __shfl_xor(gs, o, 64); np += __shfl_xor(np, o, 64); }
    if (lane == 0) { hred[wave] = gs; hred[4 + wave] = np; }
    __syncthreads();    // (also: the relevances are complete)
    const double gsum = (hred[0] + hred[1]) + (hred[2] + hred[3]);
    const long npos = (long)((hred[4] + hred[5]) + (hred[6] + hred[7]));
    for (int q = 0; q < a.n_k; ++q) {
        const int kk = min(min(a.ks[q], a.n_items), K);
        const long nid = min((long)gsum, (long)min(a.ks[q], a.n_items));      // tp[:min(int(n), k)].sum()   (metrics.py:146)
        double dcg = 0.0, idcg = 0.0, hits = 0.0;
        int first = RTX_TOPK_MAX;               // RANKM: the first rank < kk whose relevance is != 0 (metrics.py:283: != 0, not > 0)
#pragma unroll
        for (int m = 0; m < RTX_TOPK_MAX / 256; ++m) {
            const int r = tid + 256 * m;
            const double l2 = l2r[m];
            if (r < kk) {
                const float rl = __uint_as_float(relb[r]);
                dcg += (double)rl / l2; hits += rl > 0.f ? 1.0 : 0.0;
                if constexpr (RANKM) { if (rl != 0.f) first = min(first, r); }
            }
            if (r < nid && r < K) idcg += 1.0 / l2;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { dcg += __shfl_xor(dcg, o, 64); idcg += __shfl_xor(idcg, o, 64); hits += __shfl_xor(hits, o, 64); }
        if constexpr (RANKM) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        }
        if (lane == 0) {
            dred[q * DS + wave] = dcg; dred[q * DS + 4 + wave] = idcg; dred[q * DS + 8 + wave] = hits;
            if constexpr (RANKM) dred[q * DS + 12 + wave] = (double)first;
        }
    }
    __syncthreads();
    if (tid < a.n_k) {
        const int q = tid;
        const double* d = dred + q * DS;
        const double dcg = (d[0] + d[1]) + (d[2] + d[3]), idcg = (d[4] + d[5]) + (d[6] + d[7]), hits = (d[8] + d[9]) + (d[10] + d[11]);
        if (a.ndcg) a.ndcg[(size_t)q * a.out_ld + b] = dcg / idcg;
        if (a.recall) a.recall[(size_t)q * a.out_ld + b] = (double)(float)hits / (double)min((long)min(a.ks[q], a.n_items), npos);   // metrics.py:194-195
        if constexpr (RANKM) {
            const double first = fmin(fmin(d[12], d[13]), fmin(d[14], d[15]));
            const int kk = min(min(a.ks[q], a.n_items), K);
            if (a.hit) a.hit[(size_t)q * a.out_ld + b] = hits > 0.0 ? 1.0 : 0.0;                               // metrics.py:236-238
            if (a.mrr) a.mrr[(size_t)q * a.out_ld + b] = first < (double)kk ? 1.0 / (1.0 + first) : 0.0;       // metrics.py:281-285
        }
    }
}

int rtx_launch_topk_metrics(const float* scores, long ld, int B, int n_items, const RtxCsrView& held, const int* ks, int n_k,
                            int kmax, double* ndcg, double* recall, int32_t* topk, hipStream_t stream, long out_ld, const RtxCsrView* excl,
                            double* hit, double* mrr)
{
    if (B <= 0) return RTX_OK;
    RTX_CHECK(n_k >= 1 && n_k <= 16, RTX_EINVAL, "topk_metrics: 1..16 cut-offs supported, got %d", n_k);
    const int K = kmax < n_items ? kmax : n_items;
    RTX_CHECK(K >= 1 && K <= RTX_TOPK_MAX, RTX_EINVAL, "topk_metrics: k must be in [1, %d], got %d", RTX_TOPK_MAX, K);
    RtxTopkArgs a = {};
    a.scores = scores; a.ld = ld; a.n_items = n_items; a.K = K;
    a.Kp2 = 2;
    while (a.Kp2 < K) a.Kp2 <<= 1;
    a.held = held; a.n_k = n_k;
    for (int q = 0; q < n_k; ++q) {
        RTX_CHECK(ks[q] >= 1, RTX_EINVAL, "topk_metrics: cut-off must be >= 1");
        a.ks[q] = ks[q];
    }
    a.ndcg = ndcg; a.recall = recall; a.topk = topk; a.B = B;
    a.hit = hit; a.mrr = mrr;
    a.out_ld = out_ld > 0 ? out_ld : B;
    const bool burst = (((uintptr_t)scores) & 15) == 0 && (ld & 3) == 0 && n_items <= 20 * 1024;
    if (excl) {
        if (burst) { a.excl = *excl; a.has_excl = 1; }
        else RTX_TRY(rtx_launch_neg_inf(*excl, B, (float*)scores, ld, n_items, stream));   // (the streamed form of the kernel: the scatter kernel first)
    }
    {
        static bool table_ready[64] = {};
        int devid = 0;
        RTX_HIP(hipGetDevice(&devid));
        if (devid >= 0 && devid < 64 && !table_ready[devid]) {
            std::vector<double> t(RTX_TOPK_MAX);
            for (int r = 0; r < RTX_TOPK_MAX; ++r) t[r] = std::log2((double)(r + 2));
            RTX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_topk_log2), t.data(), sizeof(double) * RTX_TOPK_MAX));
            RTX_HIP(hipStreamSynchronize(nullptr));   // (the copy runs on the NULL stream, which a non-blocking caller's stream does not wait for: engine.hip dev_alloc has the story)
            table_ready[devid] = true;
        }
        RTX_CHECK(devid >= 0 && devid < 64, RTX_EINVAL, "topk_metrics: device index %d", devid);
    }
    const bool rankm = hit || mrr;
    if (burst && !rankm)
        hipLaunchKernelGGL((k_topk_metrics<20, false>), dim3(B), dim3(256), 0, stream, a);
    else if (!rankm)
        hipLaunchKernelGGL((k_topk_metrics<0, false>), dim3(B), dim3(256), 0, stream, a);
    else if (burst)
        hipLaunchKernelGGL((k_topk_metrics<20, true>), dim3(B), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((k_topk_metrics<0, true>), dim3(B), dim3(256), 0, stream, a);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
