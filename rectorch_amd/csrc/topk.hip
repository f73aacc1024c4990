// topk.hip -- device-side ranking metrics for evaluate() on gfx950 (k_topk_metrics).
#include "rtx_device.h"
#include "topk_select.h"
#include <cmath>
#include <mutex>
#include <vector>

// ------------------------------------------------------------------------------------------------
// Device-side ranking metrics for evaluate() (reference rectorch/metrics.py:136-147, 187-196):
// per user, exact top-K of the score row on order-preserving keys (a lower bound from per-thread maxima, the few hundred elements above
// it ranked by counting; a radix select only for rows of > 1024 ties), then nDCG@k / Recall@k for every requested k <= K against the held-out CSR row.  Only
// [n_k][B] doubles leave the GPU instead of the [B, n_items] score matrix (40 MB per 500 users at ml-20m).
// ------------------------------------------------------------------------------------------------
// -0.0 sorts below +0.0 here: no metric notices (the list kernel's keys tie them)
typedef TopkKey<float, false> ScoreKey;

struct RtxTopkArgs {
    const float* scores;
    long ld;
    int n_items, K;
    RtxCsrView held;
    int n_k;
    int ks[16];
    double* ndcg;     // [n_k][B]  (nullable)
    double* recall;   // [n_k][B]  (nullable)
    int32_t* topk;    // [B][K]    (nullable)
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
// More than RTX_TOPK_MAX elements >= L: the radix select takes over.  The stages are topk_select.h's, shared with the list kernel
// (recommend.hip); what is this kernel's own: the keys (ScoreKey), the burst scan over groups of four neighbours, the ranking by
// "greater than" counts with a counter per rank, and the metrics.
//
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
    __shared__ TopkLds<uint32_t> sel;            // the selection's arrays; sel.ckey / sel.cidx: the candidates
    __shared__ int32_t sidx[RTX_TOPK_MAX];       // the ranked items
    __shared__ uint32_t relb[RTX_TOPK_MAX];      // step 4: a counter per rank; from step 5 on: the relevance of the ranked item as float bits
    __shared__ int32_t hidx[RTX_TOPK_HELD_CAP];
    __shared__ float hval[RTX_TOPK_HELD_CAP];
    __shared__ double dred[16 * DS];
    __shared__ double hred[8];
    __shared__ uint32_t sh_tie;
    __shared__ uint32_t excl_bm[NV > 0 ? NV * 32 : 1];      // one bit per item of the row: stored in the user's train row
    uint32_t* const ckey = sel.ckey;
    int32_t* const cidx = sel.cidx;
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
        for (int q = 0; q < NV; ++q) kv[q] = make_uint4(ScoreKey::key(rv[q].x), ScoreKey::key(rv[q].y), ScoreKey::key(rv[q].z), ScoreKey::key(rv[q].w));
    }
    // the user's train items rank as -inf (reference models.py:470-471, 952-953: recon_x[x.nonzero()] = -inf): a bitmap of the row in
    // LDS, set from the train row's stored entries, read back four bits per group of neighbours -- instead of a scatter kernel of its
    // own over the score matrix (5 us per batch of 500)
    const uint32_t* bm = nullptr;                // (the streamed form: the launcher has written -inf to the scores)
    if constexpr (NV > 0) {
        if (a.has_excl) {
            topk_excl_build(excl_bm, NV * 32, a.excl, b, a.n_items, tid);
            bm = excl_bm;
#pragma unroll
            for (int q = 0; q < NV; ++q) topk_excl_mask4(kv[q], bm, tid + q * 256, ScoreKey::neg_key());    // (NV * 32 words: every group has its bits)
        }
    }
    // the key of element i read back from memory, with the exclusion applied as in kv[]: the < 4 elements behind the last whole group
    // (NV > 0) and the placement of the radix fall-back read the row through it
    auto key_at = [&](int i) __attribute__((always_inline)) -> uint32_t { return topk_key_at<ScoreKey>(row, bm, i); };
    auto scan = [&](auto&& f4, auto&& f1) __attribute__((always_inline)) {
        if constexpr (NV > 0) {
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int j = tid + q * 256;
                if (j < n4) f4(kv[q], j * 4);
            }
            for (int i = n4 * 4 + tid; i < a.n_items; i += 256) f1(key_at(i), i);
        } else {
            topk_scan_row<ScoreKey>(row, a.n_items, tid, bm, f1);
        }
    };
    // ---- 1. per-thread maxima
    const int c = (K + 255) / 256;              // 1 .. 4
    TopkMaxima<uint32_t> mx;
    if (c == 1) scan([&](const uint4& q, int) { mx.t0 = max(mx.t0, topk_max4(q)); }, [&](uint32_t k, int) { mx.t0 = max(mx.t0, k); });
    else scan([&](const uint4& q, int) { mx.ins(q.x); mx.ins(q.y); mx.ins(q.z); mx.ins(q.w); }, [&](uint32_t k, int) { mx.ins(k); });
    // ---- 2. the lower bound L of the row's K-th largest key (its first barrier also covers the held-out row parked here)
    if (held_in_lds) { hidx[tid] = hi0; hval[tid] = hv0; hidx[tid + 256] = hi1; hval[tid + 256] = hv1; }
    if (tid == 0) sh_tie = 0;
    const uint32_t L = topk_lower_bound(sel, mx, c, K, tid);
    // ---- 3. collect the elements >= L: per-thread counts, block prefix sum, placement.  One element in a hundred qualifies: a group of
    //         four neighbours is looked at only when its maximum does
    uint32_t mine = 0;
    scan([&](const uint4& q, int) { if (topk_max4(q) >= L) mine += (q.x >= L) + (q.y >= L) + (q.z >= L) + (q.w >= L); },
         [&](uint32_t k, int) { mine += k >= L; });
    uint32_t n_cand;
    uint32_t pos = topk_place_prefix(sel, mine, tid, n_cand);
    int n_rank = (int)n_cand;                   // candidates to rank
    if (n_cand <= (uint32_t)RTX_TOPK_MAX) {
        auto put = [&](uint32_t k, int i) __attribute__((always_inline)) { if (k >= L) { ckey[pos] = k; cidx[pos] = i; ++pos; } };
        scan([&](const uint4& q, int i0) { if (topk_max4(q) >= L) { put(q.x, i0); put(q.y, i0 + 1); put(q.z, i0 + 2); put(q.w, i0 + 3); } }, put);
    } else {
        // more than RTX_TOPK_MAX elements at / above the bound: the K largest by radix select, the lowest ids among the ties at the K-th place
        auto scan1 = [&](auto&& f) __attribute__((always_inline)) {
            scan([&](const uint4& q, int i0) { if (topk_max4(q) >= L) { f(q.x, i0); f(q.y, i0 + 1); f(q.z, i0 + 2); f(q.w, i0 + 3); } }, f);
        };
        topk_radix_select(sel, scan1, key_at, L, K, a.n_items, tid);
        n_rank = K;
    }
    // ---- 4. rank the candidates (key descending, index ascending among equal keys): the ranks < K are the answer, in order.
    //         First by "greater than" counts alone (two instructions per pair); two candidates of one rank below K -- equal scores
    //         among the ranked items: rare -- are noticed through a counter per rank, and only then the exact ranks (ties by index)
    //         are computed.
    for (int i = tid; i < K; i += 256) { sidx[i] = 0x7fffffff; relb[i] = 0u; }     // (a row of fewer than K elements: the tail stays "no item")
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
    a.held = held; a.n_k = n_k;
    for (int q = 0; q < n_k; ++q) {
        RTX_CHECK(ks[q] >= 1, RTX_EINVAL, "topk_metrics: cut-off must be >= 1");
        a.ks[q] = ks[q];
    }
    a.ndcg = ndcg; a.recall = recall; a.topk = topk;
    a.hit = hit; a.mrr = mrr;
    a.out_ld = out_ld > 0 ? out_ld : B;
    const bool burst = (((uintptr_t)scores) & 15) == 0 && (ld & 3) == 0 && n_items <= 20 * 1024;
    if (excl) {
        if (burst) { a.excl = *excl; a.has_excl = 1; }
        else RTX_TRY(rtx_launch_neg_inf(*excl, B, (float*)scores, ld, n_items, stream));   // (the streamed form of the kernel: the scatter kernel first)
    }
    {
        static bool table_ready[64] = {};
        static std::mutex table_mutex;          // two host threads on their first call: one fills, the other waits for the fill
        int devid = 0;
        RTX_HIP(hipGetDevice(&devid));
        std::lock_guard<std::mutex> lock(table_mutex);
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
