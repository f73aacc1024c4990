// wmf.hip -- weighted matrix factorisation for implicit feedback (Hu, Koren, Volinsky 2008) by alternating least squares on MI355X,
// in float64.
//
// Definition (include/rectorch_hip.h has the full text, the operation order included):
//     A_u x_u = b_u,   A_u = G + sum_{i in I_u} (alpha r_ui) y_i y_i^T + lam I,   b_u = sum_{i in I_u} (1 + alpha r_ui) y_i,   G = Y^T Y
// Here:
//   k_wmf_solve<NT>  one row's system per 256-thread workgroup, fp = 16 NT = the factor width rounded up to 16.  The row's entries
//       are walked in stored order, WMF_CH at a time: their factor rows are gathered into an LDS stage (zeros in the pad), and
//       S = sum w y y^T is accumulated on v_mfma_f64_16x16x4_f64 over the NT (NT + 1) / 2 tiles of the lower triangle, which the
//       four waves share round-robin (fp = 128: 36 tiles, 9 a wave, 72 accumulator VGPRs); b is accumulated beside it by the
//       first fp threads.  The accumulators stay in registers for the whole walk.  Then the triangle (G + S + lam I, a unit
//       diagonal in the pad) goes to LDS, ALIASED over the stage ([fp][fp + 1] doubles: 129 KiB at fp = 128), and is factored
//       there in 16-column panels -- one wave factors the 16 x 16 diagonal block in registers and inverts its factor (the
//       scheme of potf2.hip's blocked leaf), the panel below it and the trailing update are 16 x 16 x 16 MFMA tile products --
//       three barriers a panel; two blocked triangular solves follow (two barriers a panel each) and x is written once.
//   modes of the same kernel: WMF_SYSTEMS writes A and b out instead of solving (rtx_wmf_systems); WMF_PARTIAL accumulates one
//       SEGMENT of a long row and writes its tiles and its b to a slab; WMF_GRAM does the same for a chunk of rows of a factor
//       table with w = 1 (the partial Gram matrices).  The solving workgroup of a long row adds the row's slabs in ascending
//       order instead of walking entries; k_wmf_gram_reduce adds the chunks' slabs in ascending order.  No atomics.
//   k_wmf_scores     x_b . y_j as an fma chain over k, eight users a workgroup, -inf at the mask row's entries.
#include "../../include/rectorch_hip.h"
#include "rtx_kernels.h"
#include "solver_common.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <vector>

typedef __attribute__((ext_vector_type(4))) double f64x4_t;

#define WMF_CH 32     // entries per LDS stage
#define WMF_YPAD 16   // the stage's row stride is fp + 16 doubles: the four rows of one MFMA operand fall into different banks
enum { WMF_SOLVE = 0, WMF_SYSTEMS = 1, WMF_PARTIAL = 2, WMF_GRAM = 3 };

struct rtx_wmf {
    int n_users = 0, n_items = 0, f = 0;
    double alpha = 0, lam = 0;
    double* Y = nullptr;      // [n_items][f]
    double* U = nullptr;      // [n_users][f]: the last user half-sweep (nullptr for a loaded model)
    double* G = nullptr;      // [f][f] = Y^T Y of the final item factors: what fold-in needs
    double* xbuf = nullptr;   // fold-in vectors of rtx_wmf_scores, grown on demand
    int64_t xcap = 0;
    int* status = nullptr;
    double fit_ms = 0, gram_ms = 0, user_ms = 0, item_ms = 0;
};

struct WmfArgs {
    const int64_t* indptr;
    const int32_t* indices;
    const float* values;
    const int32_t* row_ids;    // nullable
    const double* Y;           // [n_src][f]
    int n_src, f;
    double alpha, lam;
    const double* G;           // [f][f]
    int mode;
    const int32_t* seg_pos;    // WMF_PARTIAL: job -> position in the batch, segment number
    const int32_t* seg_idx;
    const int32_t* slab_of;    // [batch]: the first slab of a long row, -1 for the others (nullable: no long rows)
    double* slabs;             // slab s at s * (T * 256 + fp): T tiles of [reg][lane], then b
    double* out;               // WMF_SOLVE: x [batch][f];  WMF_SYSTEMS: A [batch][f][f]
    double* b_out;             // WMF_SYSTEMS: b [batch][f]
    int* status;
};

// ------------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ void wmf_tile(int t, int& ti, int& tj)   // tile t of the lower triangle, row-major: (0,0) (1,0) (1,1) (2,0) ...
{
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}

__device__ __forceinline__ double wmf_rl64(double v, int lane)
{
    const long long u = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffll), lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// 1 / sqrt(d): v_rsq_f64 + two Newton steps (potf2.hip)
__device__ __forceinline__ double wmf_rsqrt(double d)
{
    double y = __builtin_amdgcn_rsq(d);
    y = y * (1.5 - 0.5 * d * y * y);
    return y * (1.5 - 0.5 * d * y * y);
}

// the walk over the entries [e0, e1): S into acc (tiles wave, wave + 4, ...), b into bacc (thread c < fp holds b[c]).  identity: the
// "entries" are the rows e of the table themselves with w = 1 (the Gram matrix).
template <int NT, int MAXS>
__device__ __forceinline__ void wmf_walk(const WmfArgs& a, int64_t e0, int64_t e1, bool identity, double* ys, double* ws, f64x4_t (&acc)[MAXS],
                                         const int (&offa)[MAXS], const int (&offb)[MAXS], double& bacc, int tid)
{
    constexpr int FP = 16 * NT, LDY = FP + WMF_YPAD, T = NT * (NT + 1) / 2;
    const int lane = tid & 63, wave = tid >> 6;
    for (int64_t c0 = e0; c0 < e1; c0 += WMF_CH) {
        const int cnt = (int)min((int64_t)WMF_CH, e1 - c0);
        __syncthreads();   // the previous stage has been consumed
        for (int idx = tid; idx < WMF_CH * FP; idx += 256) {
            const int k = idx / FP, c = idx - k * FP;
            double y = 0.0, w = 0.0;
            if (k < cnt) {
                const int64_t e = c0 + k;
                const int64_t col = identity ? e : (int64_t)a.indices[e];
                if (col >= 0 && col < a.n_src) {
                    w = identity ? 1.0 : a.alpha * (double)(a.values ? a.values[e] : 1.f);
                    if (c < a.f) y = a.Y[(size_t)col * a.f + c];
                }
            }
            ys[k * LDY + c] = y;
            if (c == 0) ws[k] = w;
        }
        __syncthreads();
        if (!identity && tid < FP)
            for (int k = 0; k < cnt; ++k) bacc = fma(1.0 + ws[k], ys[k * LDY + tid], bacc);
        const int groups = (cnt + 3) >> 2;
        for (int g = 0; g < groups; ++g) {
            const int k = 4 * g + (lane >> 4);
            const double w = ws[k];
            const double* yr = ys + k * LDY + (lane & 15);
#pragma unroll
            for (int s = 0; s < MAXS; ++s)
                if (wave + 4 * s < T) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(w * yr[offa[s]], yr[offb[s]], acc[s], 0, 0, 0);
        }
    }
}

template <int NT>
__global__ __launch_bounds__(256) void k_wmf_solve(const WmfArgs a)
{
    constexpr int FP = 16 * NT, LDY = FP + WMF_YPAD, LDM = FP + 1, T = NT * (NT + 1) / 2, MAXS = (T + 3) / 4;
    constexpr size_t SLAB = (size_t)T * 256 + FP;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* ys = sm;                    // the stage: [WMF_CH][LDY], then ws [WMF_CH]
    double* ws = sm + WMF_CH * LDY;
    double* M = sm;                     // aliased over the stage: [FP][LDM], then Wt [16][17]
    double* Wt = sm + FP * LDM;
    __shared__ double bv[FP], zp[16];
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = a.f;

    f64x4_t acc[MAXS];
    int offa[MAXS], offb[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        int ti, tj;
        wmf_tile(min(wave + 4 * s, T - 1), ti, tj);
        offa[s] = 16 * ti;
        offb[s] = 16 * tj;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[s][e] = 0.0;
    }
    double bacc = 0.0;

    const int job = blockIdx.x;
    int pos = job;
    if (a.mode == WMF_GRAM) {
        const int64_t e0 = (int64_t)job * RTX_WMF_GRAM_ROWS;
        wmf_walk<NT, MAXS>(a, e0, min(e0 + RTX_WMF_GRAM_ROWS, (int64_t)a.n_src), true, ys, ws, acc, offa, offb, bacc, tid);
    } else {
        int seg = -1;
        if (a.mode == WMF_PARTIAL) {
            pos = a.seg_pos[job];
            seg = a.seg_idx[job];
        }
        const int64_t u = a.row_ids ? (int64_t)a.row_ids[pos] : (int64_t)pos;
        int64_t beg = a.indptr[u], end = a.indptr[u + 1];
        if (a.mode == WMF_SOLVE && end == beg) {   // a row without entries: the zero vector
            if (tid < f) a.out[(size_t)pos * f + tid] = 0.0;
            return;
        }
        const int first = a.slab_of ? a.slab_of[pos] : -1;
        if (seg >= 0) {
            beg += (int64_t)seg * RTX_WMF_SEGMENT;
            end = min(end, beg + RTX_WMF_SEGMENT);
        }
        if (seg < 0 && first >= 0) {
            // a long row: its segments' slabs, added in ascending order
            const int nseg = (int)((end - beg + RTX_WMF_SEGMENT - 1) / RTX_WMF_SEGMENT);
            for (int q = 0; q < nseg; ++q) {
                const double* sl = a.slabs + (size_t)(first + q) * SLAB;
#pragma unroll
                for (int s = 0; s < MAXS; ++s)
                    if (wave + 4 * s < T)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const double v = sl[(size_t)(wave + 4 * s) * 256 + e * 64 + lane];
                            acc[s][e] = q ? acc[s][e] + v : v;
                        }
                if (tid < FP) {
                    const double v = sl[(size_t)T * 256 + tid];
                    bacc = q ? bacc + v : v;
                }
            }
        } else {
            wmf_walk<NT, MAXS>(a, beg, end, false, ys, ws, acc, offa, offb, bacc, tid);
        }
    }
    if (a.mode == WMF_PARTIAL || a.mode == WMF_GRAM) {
        double* sl = a.slabs + (size_t)(a.mode == WMF_GRAM ? job : a.slab_of[pos] + a.seg_idx[job]) * SLAB;
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (wave + 4 * s < T)
#pragma unroll
                for (int e = 0; e < 4; ++e) sl[(size_t)(wave + 4 * s) * 256 + e * 64 + lane] = acc[s][e];
        if (tid < FP) sl[(size_t)T * 256 + tid] = bacc;
        return;
    }

    // ---- the triangle to LDS, over the stage:  (G + S) + lam on the diagonal;  identity in the pad
    __syncthreads();
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (wave + 4 * s < T)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = offa[s] + (lane >> 4) + 4 * e, c = offb[s] + (lane & 15);
                double v = (r == c) ? 1.0 : 0.0;
                if (r < f && c < f) v = (a.G[(size_t)r * f + c] + acc[s][e]) + ((r == c) ? a.lam : 0.0);
                M[r * LDM + c] = v;
            }
    if (tid < FP) bv[tid] = (tid < f) ? bacc : 0.0;
    if (tid == 0) bad = 0;
    __syncthreads();

    if (a.mode == WMF_SYSTEMS) {
        double* Ao = a.out + (size_t)pos * f * f;
        for (int idx = tid; idx < f * f; idx += 256) {
            const int r = idx / f, c = idx - r * f;
            Ao[idx] = M[max(r, c) * LDM + min(r, c)];
        }
        if (tid < f) a.b_out[(size_t)pos * f + tid] = bv[tid];
        return;
    }

    // ---- Cholesky in 16-column panels
#pragma nounroll
    for (int p = 0; p < NT; ++p) {
        const int c0 = 16 * p;
        if (wave == 0) {
            // the diagonal block: lane i holds row i, the pivot column travels by readlane (both quarters of the wave beyond lane 15
            // compute copies: the readlanes name lanes < 16)
            const int i = lane & 15;
            double ar[16], x[16], rinv[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) ar[k] = (k <= i) ? M[(c0 + i) * LDM + c0 + k] : 0.0;
            bool ok = true;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double d = wmf_rl64(ar[j], j);
                if (!(d > 0.0)) ok = false;
                const double r = wmf_rsqrt(d);
                rinv[j] = r;
                const double lj = ar[j] * r;
                ar[j] = lj;
#pragma unroll
                for (int k = j + 1; k < 16; ++k) ar[k] -= lj * wmf_rl64(lj, k);
            }
            if (lane < 16) {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k <= i) M[(c0 + i) * LDM + c0 + k] = ar[k];
                if (!ok && i == 0) bad = 1;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes have landed
            // W_pp = inv(L_pp): lane j solves L x = e_j
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) {
                double s0 = (ii == i) ? 1.0 : 0.0, s1 = 0.0;
#pragma unroll
                for (int k = 0; k < ii; ++k) {
                    if (k & 1) s1 -= M[(c0 + ii) * LDM + c0 + k] * x[k];
                    else s0 -= M[(c0 + ii) * LDM + c0 + k] * x[k];
                }
                x[ii] = (ii >= i) ? (s0 + s1) * rinv[ii] : 0.0;
            }
            if (lane < 16) {
#pragma unroll
                for (int k = 0; k < 16; ++k) Wt[i * 17 + k] = x[k];   // Wt[c][k] = W_pp[k][c], zero for k < c
            }
        }
        __syncthreads();
        // W_pp (lower, zeros above) replaces L_pp: nothing below reads L_pp any more
        M[(c0 + (tid >> 4)) * LDM + c0 + (tid & 15)] = Wt[(tid & 15) * 17 + (tid >> 4)];
        // the panel: L21[r][c] = sum_k A21[r][k] W_pp[c][k], one 16 x 16 tile at a time
        for (int ii = p + 1 + wave; ii < NT; ii += 4) {
            f64x4_t t4 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int k = 4 * g + (lane >> 4);
                t4 = __builtin_amdgcn_mfma_f64_16x16x4f64(M[(16 * ii + (lane & 15)) * LDM + c0 + k], Wt[k * 17 + (lane & 15)], t4, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) M[(16 * ii + (lane >> 4) + 4 * e) * LDM + c0 + (lane & 15)] = t4[e];
        }
        __syncthreads();
        // the trailing update: A22[r][c] -= sum_k L21[r][k] L21[c][k] over the lower tiles
        const int nt = NT - p - 1, ntile = nt * (nt + 1) / 2;
        for (int t = wave; t < ntile; t += 4) {
            int ti, tj;
            wmf_tile(t, ti, tj);
            const int ii = p + 1 + ti, jj = p + 1 + tj;
            f64x4_t t4;
#pragma unroll
            for (int e = 0; e < 4; ++e) t4[e] = M[(16 * ii + (lane >> 4) + 4 * e) * LDM + 16 * jj + (lane & 15)];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int k = 4 * g + (lane >> 4);
                t4 = __builtin_amdgcn_mfma_f64_16x16x4f64(-M[(16 * ii + (lane & 15)) * LDM + c0 + k], M[(16 * jj + (lane & 15)) * LDM + c0 + k], t4,
                                                          0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) M[(16 * ii + (lane >> 4) + 4 * e) * LDM + 16 * jj + (lane & 15)] = t4[e];
        }
        __syncthreads();
    }

    // ---- L z = b, panel by panel (the diagonal blocks hold W_pp)
#pragma nounroll
    for (int p = 0; p < NT; ++p) {
        const int c0 = 16 * p;
        if (tid < 16) {
            double s = 0.0;
            for (int k = 0; k <= tid; ++k) s = fma(M[(c0 + tid) * LDM + c0 + k], bv[c0 + k], s);
            zp[tid] = s;
        }
        __syncthreads();
        if (tid < 16) bv[c0 + tid] = zp[tid];
        else if (tid >= c0 + 16 && tid < FP) {
            double s = bv[tid];
#pragma unroll
            for (int k = 0; k < 16; ++k) s = fma(-M[tid * LDM + c0 + k], zp[k], s);
            bv[tid] = s;
        }
        __syncthreads();
    }
    // ---- L^T x = z, from the last panel up
#pragma nounroll
    for (int p = NT - 1; p >= 0; --p) {
        const int c0 = 16 * p;
        if (tid < 16) {
            double s = 0.0;
            for (int k = tid; k < 16; ++k) s = fma(M[(c0 + k) * LDM + c0 + tid], bv[c0 + k], s);
            zp[tid] = s;
        }
        __syncthreads();
        if (tid < 16) bv[c0 + tid] = zp[tid];
        if (tid < c0) {
            double s = bv[tid];
#pragma unroll
            for (int k = 0; k < 16; ++k) s = fma(-M[(c0 + k) * LDM + tid], zp[k], s);
            bv[tid] = s;
        }
        __syncthreads();
    }
    if (tid < f) a.out[(size_t)pos * f + tid] = bv[tid];
    if (tid == 0 && bad) *a.status = 1;
}

// G [f][f] = the chunks' slabs added in ascending order; one workgroup per tile of the lower triangle, mirrored across the diagonal
__global__ __launch_bounds__(256) void k_wmf_gram_reduce(const double* slabs, size_t slab, int chunks, int f, double* G)
{
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, e = tid >> 6;
    int ti, tj;
    wmf_tile(t, ti, tj);
    double v = 0.0;
    for (int q = 0; q < chunks; ++q) {
        const double s = slabs[(size_t)q * slab + (size_t)t * 256 + tid];
        v = q ? v + s : s;
    }
    const int r = 16 * ti + (lane >> 4) + 4 * e, c = 16 * tj + (lane & 15);
    if (r < f && c <= r) {
        G[(size_t)r * f + c] = v;
        G[(size_t)c * f + r] = v;
    }
}

// out[b][j] = x_b . y_j as an fma chain over k = 0 .. f-1; WMF_SU users and 256 items a workgroup
#define WMF_SU 8
__global__ __launch_bounds__(256) void k_wmf_scores(const double* __restrict__ x, const double* __restrict__ Y, int f, int n, int batch,
                                                    const RtxCsrView mask, double* out, int64_t ld)
{
    __shared__ double xs[WMF_SU][RTX_WMF_MAX_FACTORS];
    __shared__ double yt[256][17];
    const int tid = threadIdx.x, b0 = blockIdx.y * WMF_SU, j = blockIdx.x * 256 + tid;
    const int nb = min(WMF_SU, batch - b0);
    for (int idx = tid; idx < WMF_SU * f; idx += 256) {
        const int q = idx / f, k = idx - q * f;
        xs[q][k] = (q < nb) ? x[(size_t)(b0 + q) * f + k] : 0.0;
    }
    double s[WMF_SU];
#pragma unroll
    for (int q = 0; q < WMF_SU; ++q) s[q] = 0.0;
    // the items' factors pass through LDS 16 columns at a time: coalesced 128-byte reads of the table, conflict-free rows of 17
    for (int k0 = 0; k0 < f; k0 += 16) {
        __syncthreads();
        for (int idx = tid; idx < 256 * 16; idx += 256) {
            const int it = idx >> 4, kk = idx & 15, jj = blockIdx.x * 256 + it;
            yt[it][kk] = (jj < n && k0 + kk < f) ? Y[(size_t)jj * f + k0 + kk] : 0.0;
        }
        __syncthreads();
        const int kn = min(16, f - k0);
        for (int kk = 0; kk < kn; ++kk) {
            const double y = yt[tid][kk];
#pragma unroll
            for (int q = 0; q < WMF_SU; ++q) s[q] = fma(xs[q][k0 + kk], y, s[q]);
        }
    }
    if (j < n) {
#pragma unroll
        for (int q = 0; q < WMF_SU; ++q)
            if (q < nb) out[(size_t)(b0 + q) * ld + j] = s[q];
    }
    if (mask.indptr) {
        __syncthreads();
        const int lo = blockIdx.x * 256, hi = min(lo + 256, n);
        for (int q = 0; q < nb; ++q) rtx_mask_neg_inf(mask, b0 + q, lo, hi, out + (size_t)(b0 + q) * ld, tid);
    }
}

// ------------------------------------------------------------------------------------------------ host side
static void wmf_free(rtx_wmf* h)
{
    if (h->Y) (void)hipFree(h->Y);
    if (h->U) (void)hipFree(h->U);
    if (h->G) (void)hipFree(h->G);
    if (h->xbuf) (void)hipFree(h->xbuf);
    if (h->status) (void)hipFree(h->status);
    delete h;
}

static inline int wmf_nt(int f) { return (f + 15) / 16; }
static inline size_t wmf_slab(int nt) { return (size_t)(nt * (nt + 1) / 2) * 256 + 16 * nt; }
static inline size_t wmf_lds(int nt)
{
    const size_t fp = 16 * (size_t)nt;
    return 8 * std::max<size_t>(WMF_CH * (fp + WMF_YPAD) + WMF_CH, fp * (fp + 1) + 16 * 17);
}

template <int NT>
static int wmf_launch_nt(const WmfArgs& a, int jobs, hipStream_t st)
{
    static bool configured = false;
    if (!configured) {
        RTX_HIP(hipFuncSetAttribute((const void*)k_wmf_solve<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wmf_lds(NT)));
        configured = true;
    }
    hipLaunchKernelGGL(k_wmf_solve<NT>, dim3(jobs), dim3(256), wmf_lds(NT), st, a);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

static int wmf_launch(const WmfArgs& a, int jobs, hipStream_t st)
{
    if (jobs <= 0) return RTX_OK;
    switch (wmf_nt(a.f)) {
    case 1: return wmf_launch_nt<1>(a, jobs, st);
    case 2: return wmf_launch_nt<2>(a, jobs, st);
    case 3: return wmf_launch_nt<3>(a, jobs, st);
    case 4: return wmf_launch_nt<4>(a, jobs, st);
    case 5: return wmf_launch_nt<5>(a, jobs, st);
    case 6: return wmf_launch_nt<6>(a, jobs, st);
    case 7: return wmf_launch_nt<7>(a, jobs, st);
    case 8: return wmf_launch_nt<8>(a, jobs, st);
    }
    rtx_set_error("wmf: f = %d is outside 1 .. %d", a.f, RTX_WMF_MAX_FACTORS);
    return RTX_EINVAL;
}

// the refusals every entry point shares; nothing is launched before they pass
static int wmf_check_params(const char* who, int f, double alpha, double lam)
{
    RTX_CHECK(f >= 1 && f <= RTX_WMF_MAX_FACTORS, RTX_EINVAL, "%s: f must be in [1, %d] (the solve kernel's limit), got %d", who, RTX_WMF_MAX_FACTORS, f);
    RTX_CHECK(isfinite(lam) && lam > 0.0, RTX_EINVAL, "%s: lam must be finite and > 0, got %g", who, lam);
    RTX_CHECK(isfinite(alpha) && alpha >= 0.0, RTX_EINVAL, "%s: alpha must be finite and >= 0, got %g", who, alpha);
    return RTX_OK;
}

// every stored value > 0: one host pass per matrix (it never changes after the upload)
static int wmf_check_values(const char* who, const rtx_csr* X)
{
    if (X->values_positive == 0) {
        int ok = 1;
        if (X->values && X->nnz > 0) {
            std::vector<float> hv((size_t)X->nnz);
            RTX_HIP(hipMemcpy(hv.data(), X->values, sizeof(float) * X->nnz, hipMemcpyDeviceToHost));
            for (float v : hv)
                if (!(v > 0.f)) {
                    ok = -1;
                    break;
                }
        }
        X->values_positive = ok;
    }
    RTX_CHECK(X->values_positive > 0, RTX_EINVAL,
              "%s: the matrix stores a value <= 0: the confidence 1 + alpha r is defined for stored values r > 0 (drop the explicit zeros)", who);
    return RTX_OK;
}

// The long rows of a batch: rows of more than RTX_WMF_SEGMENT entries get ceil(len / SEGMENT) slabs each.  A matrix whose longest
// row is short needs nothing (the common case: no host work); otherwise the row lengths are read on the host.
struct WmfPlan {
    int32_t* slab_of = nullptr;
    int32_t* seg_pos = nullptr;
    int32_t* seg_idx = nullptr;
    double* slabs = nullptr;
    int n_seg = 0;
};

static int wmf_plan(const rtx_csr* X, const int32_t* row_ids, int batch, int nt, WmfPlan* plan, std::vector<void*>& pool, hipStream_t st)
{
    *plan = WmfPlan();
    if (X->max_row_len <= RTX_WMF_SEGMENT || batch <= 0) return RTX_OK;
    RTX_HIP(hipStreamSynchronize(st));   // row_ids may have been written on the stream
    std::vector<int64_t> indptr((size_t)X->n_rows + 1);
    RTX_HIP(hipMemcpy(indptr.data(), X->indptr, sizeof(int64_t) * indptr.size(), hipMemcpyDeviceToHost));
    std::vector<int32_t> rows;
    if (row_ids) {
        rows.resize((size_t)batch);
        RTX_HIP(hipMemcpy(rows.data(), row_ids, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost));
    }
    std::vector<int32_t> slab_of((size_t)batch, -1), seg_pos, seg_idx;
    int n_seg = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t u = row_ids ? rows[(size_t)b] : b;
        RTX_CHECK(u >= 0 && u < X->n_rows, RTX_EINVAL, "wmf: row %lld is outside the matrix (%lld rows)", (long long)u, (long long)X->n_rows);
        const int64_t len = indptr[(size_t)u + 1] - indptr[(size_t)u];
        if (len <= RTX_WMF_SEGMENT) continue;
        const int ns = (int)((len + RTX_WMF_SEGMENT - 1) / RTX_WMF_SEGMENT);
        slab_of[(size_t)b] = n_seg;
        for (int q = 0; q < ns; ++q) {
            seg_pos.push_back(b);
            seg_idx.push_back(q);
        }
        n_seg += ns;
    }
    if (!n_seg) return RTX_OK;
    RTX_TRY(rtx_pool_alloc("wmf", (void**)&plan->slab_of, sizeof(int32_t) * (size_t)batch, pool));
    RTX_TRY(rtx_pool_alloc("wmf", (void**)&plan->seg_pos, sizeof(int32_t) * (size_t)n_seg, pool));
    RTX_TRY(rtx_pool_alloc("wmf", (void**)&plan->seg_idx, sizeof(int32_t) * (size_t)n_seg, pool));
    RTX_TRY(rtx_pool_alloc("wmf", (void**)&plan->slabs, sizeof(double) * wmf_slab(nt) * (size_t)n_seg, pool));
    RTX_HIP(hipMemcpy(plan->slab_of, slab_of.data(), sizeof(int32_t) * (size_t)batch, hipMemcpyHostToDevice));
    RTX_HIP(hipMemcpy(plan->seg_pos, seg_pos.data(), sizeof(int32_t) * (size_t)n_seg, hipMemcpyHostToDevice));
    RTX_HIP(hipMemcpy(plan->seg_idx, seg_idx.data(), sizeof(int32_t) * (size_t)n_seg, hipMemcpyHostToDevice));
    plan->n_seg = n_seg;
    return RTX_OK;
}

// G [f][f] (device) = Y^T Y of the table Y [n][f]: partial Gram matrices of RTX_WMF_GRAM_ROWS rows, then their ordered sum.
// gslabs: room for ceil(n / RTX_WMF_GRAM_ROWS) slabs.
static int wmf_gram(const double* Y, int n, int f, double* gslabs, double* G, hipStream_t st)
{
    const int nt = wmf_nt(f), chunks = (n + RTX_WMF_GRAM_ROWS - 1) / RTX_WMF_GRAM_ROWS;
    WmfArgs a;
    memset(&a, 0, sizeof a);
    a.Y = Y;
    a.n_src = n;
    a.f = f;
    a.mode = WMF_GRAM;
    a.slabs = gslabs;
    RTX_TRY(wmf_launch(a, chunks, st));
    hipLaunchKernelGGL(k_wmf_gram_reduce, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, gslabs, wmf_slab(nt), chunks, f, G);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
static inline size_t wmf_gram_slabs(int n, int f) { return wmf_slab(wmf_nt(f)) * (size_t)((n + RTX_WMF_GRAM_ROWS - 1) / RTX_WMF_GRAM_ROWS); }

// one half-sweep (mode WMF_SOLVE) or the systems alone (WMF_SYSTEMS) over `batch` rows of X, G given
static int wmf_rows(const rtx_csr* X, const int32_t* row_ids, int batch, const double* Y, int f, double alpha, double lam, const double* G,
                    const WmfPlan& plan, int mode, double* out, double* b_out, int* status, hipStream_t st)
{
    WmfArgs a;
    memset(&a, 0, sizeof a);
    a.indptr = X->indptr;
    a.indices = X->indices;
    a.values = X->values;
    a.row_ids = row_ids;
    a.Y = Y;
    a.n_src = X->n_cols;
    a.f = f;
    a.alpha = alpha;
    a.lam = lam;
    a.G = G;
    a.slab_of = plan.slab_of;
    a.seg_pos = plan.seg_pos;
    a.seg_idx = plan.seg_idx;
    a.slabs = plan.slabs;
    a.out = out;
    a.b_out = b_out;
    a.status = status;
    if (plan.n_seg) {
        a.mode = WMF_PARTIAL;
        RTX_TRY(wmf_launch(a, plan.n_seg, st));
    }
    a.mode = mode;
    return wmf_launch(a, batch, st);
}

static int wmf_status(const char* who, const int* status_dev)
{
    int s = 0;
    RTX_HIP(hipMemcpy(&s, status_dev, sizeof(int), hipMemcpyDeviceToHost));
    RTX_CHECK(s == 0, RTX_EINVAL, "%s: a system is not positive definite (a pivot of its Cholesky factorisation was not positive): the factors are not finite",
              who);
    return RTX_OK;
}

// systems or solves against a caller's table: G, the plan and the status word live for the call
static int wmf_call(const char* who, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const double* Y, int32_t f, double alpha,
                    double lam, int mode, double* out, double* b_out, hipStream_t st)
{
    std::vector<void*> work;
    double *G = nullptr, *gsl = nullptr;
    int* status = nullptr;
    WmfPlan plan;
    int rc = rtx_pool_alloc("wmf", (void**)&G, sizeof(double) * (size_t)f * f, work);
    if (!rc) rc = rtx_pool_alloc("wmf", (void**)&gsl, sizeof(double) * wmf_gram_slabs(X->n_cols, f), work);
    if (!rc) rc = rtx_pool_alloc("wmf", (void**)&status, sizeof(int), work);
    if (!rc) rc = wmf_plan(X, row_ids, batch, wmf_nt(f), &plan, work, st);
    if (!rc && hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
        rtx_set_error("%s: hipMemsetAsync failed", who);
        rc = RTX_EHIP;
    }
    if (!rc) rc = wmf_gram(Y, X->n_cols, f, gsl, G, st);
    if (!rc) rc = wmf_rows(X, row_ids, batch, Y, f, alpha, lam, G, plan, mode, out, b_out, status, st);
    hipError_t e = hipStreamSynchronize(st);   // the work buffers are freed below
    if (!rc && e != hipSuccess) {
        rtx_set_error("%s: %s", who, hipGetErrorString(e));
        rc = RTX_EHIP;
    }
    if (!rc && mode == WMF_SOLVE) rc = wmf_status(who, status);
    rtx_free_all(work);
    return rc;
}

extern "C" {

int rtx_wmf_systems(const rtx_csr* X, const int32_t* row_ids, int32_t batch, const double* Y, int32_t f, double alpha, double lam,
                    double* A_out, double* b_out, void* stream)
{
    RTX_CHECK(X && Y && A_out && b_out, RTX_EINVAL, "wmf_systems: NULL argument");
    RTX_TRY(wmf_check_params("wmf_systems", f, alpha, lam));
    RTX_CHECK(batch >= 0 && (row_ids || batch <= X->n_rows), RTX_EINVAL, "wmf_systems: bad batch %d", batch);
    RTX_TRY(wmf_check_values("wmf_systems", X));
    if (batch == 0) return RTX_OK;
    return wmf_call("wmf_systems", X, row_ids, batch, Y, f, alpha, lam, WMF_SYSTEMS, A_out, b_out, (hipStream_t)stream);
}

int rtx_wmf_solve_rows(const rtx_csr* X, const int32_t* row_ids, int32_t batch, const double* Y, int32_t n_src, int32_t f, double alpha,
                       double lam, double* out, void* stream)
{
    RTX_CHECK(X && Y && out, RTX_EINVAL, "wmf_solve_rows: NULL argument");
    RTX_TRY(wmf_check_params("wmf_solve_rows", f, alpha, lam));
    RTX_CHECK(n_src == X->n_cols, RTX_EINVAL, "wmf_solve_rows: the factor table has %d rows, the matrix has %d columns", n_src, X->n_cols);
    RTX_CHECK(batch >= 0 && (row_ids || batch <= X->n_rows), RTX_EINVAL, "wmf_solve_rows: bad batch %d", batch);
    RTX_TRY(wmf_check_values("wmf_solve_rows", X));
    if (batch == 0) return RTX_OK;
    return wmf_call("wmf_solve_rows", X, row_ids, batch, Y, f, alpha, lam, WMF_SOLVE, out, nullptr, (hipStream_t)stream);
}

int rtx_wmf_fit(const rtx_csr* X, const rtx_csr* XT, int32_t f, double alpha, double lam, int32_t n_iter, const double* Y0_host,
                rtx_wmf** out, void* stream)
{
    RTX_CHECK(X && XT && Y0_host && out, RTX_EINVAL, "wmf_fit: NULL argument");
    RTX_TRY(wmf_check_params("wmf_fit", f, alpha, lam));
    RTX_CHECK(n_iter >= 0, RTX_EINVAL, "wmf_fit: n_iter must be >= 0, got %d", n_iter);
    RTX_CHECK(X->n_rows > 0 && X->n_cols > 0 && X->n_rows <= INT32_MAX, RTX_EINVAL, "wmf_fit: empty matrix");
    RTX_CHECK(XT->n_rows == X->n_cols && XT->n_cols == X->n_rows && XT->nnz == X->nnz, RTX_EINVAL,
              "wmf_fit: the second matrix is not the transpose of the first (%lld x %d with %lld entries against %lld x %d with %lld)",
              (long long)XT->n_rows, XT->n_cols, (long long)XT->nnz, (long long)X->n_rows, X->n_cols, (long long)X->nnz);
    RTX_TRY(wmf_check_values("wmf_fit", X));
    RTX_TRY(wmf_check_values("wmf_fit", XT));
    hipStream_t st = (hipStream_t)stream;
    const int nu = (int)X->n_rows, ni = X->n_cols, nt = wmf_nt(f);
    RtxFitScope<7> fs;   // events 0 .. 4: the phases of one iteration, reused every iteration; 5, 6: the whole fit
    std::unique_ptr<rtx_wmf, decltype(&wmf_free)> h(new rtx_wmf(), wmf_free);
    h->n_users = nu; h->n_items = ni; h->f = f; h->alpha = alpha; h->lam = lam;
    const int rc = [&]() -> int {
        hipEvent_t* ev = fs.ev;
        RTX_TRY(fs.create_events());
        double* gsl = nullptr;
        double* Gw = nullptr;
        WmfPlan plan_u, plan_i;
        RTX_HIP(hipMalloc((void**)&h->Y, sizeof(double) * (size_t)ni * f));
        RTX_HIP(hipMalloc((void**)&h->U, sizeof(double) * (size_t)nu * f));
        RTX_HIP(hipMalloc((void**)&h->G, sizeof(double) * (size_t)f * f));
        RTX_HIP(hipMalloc((void**)&h->status, sizeof(int)));
        RTX_TRY(rtx_pool_alloc("wmf", (void**)&Gw, sizeof(double) * (size_t)f * f, fs.pool));
        RTX_TRY(rtx_pool_alloc("wmf", (void**)&gsl, sizeof(double) * wmf_gram_slabs(std::max(nu, ni), f), fs.pool));
        RTX_TRY(wmf_plan(X, nullptr, nu, nt, &plan_u, fs.pool, st));
        RTX_TRY(wmf_plan(XT, nullptr, ni, nt, &plan_i, fs.pool, st));
        RTX_HIP(hipMemcpy(h->Y, Y0_host, sizeof(double) * (size_t)ni * f, hipMemcpyHostToDevice));
        RTX_HIP(hipMemsetAsync(h->U, 0, sizeof(double) * (size_t)nu * f, st));
        RTX_HIP(hipMemsetAsync(h->status, 0, sizeof(int), st));
        RTX_HIP(hipEventRecord(ev[5], st));
        for (int it = 0; it < n_iter; ++it) {
            RTX_HIP(hipEventRecord(ev[0], st));
            RTX_TRY(wmf_gram(h->Y, ni, f, gsl, Gw, st));
            RTX_HIP(hipEventRecord(ev[1], st));
            RTX_TRY(wmf_rows(X, nullptr, nu, h->Y, f, alpha, lam, Gw, plan_u, WMF_SOLVE, h->U, nullptr, h->status, st));
            RTX_HIP(hipEventRecord(ev[2], st));
            RTX_TRY(wmf_gram(h->U, nu, f, gsl, Gw, st));
            RTX_HIP(hipEventRecord(ev[3], st));
            RTX_TRY(wmf_rows(XT, nullptr, ni, h->U, f, alpha, lam, Gw, plan_i, WMF_SOLVE, h->Y, nullptr, h->status, st));
            RTX_HIP(hipEventRecord(ev[4], st));
            RTX_HIP(hipStreamSynchronize(st));   // the events are reused; an iteration is milliseconds at least
            h->gram_ms += rtx_elapsed_ms(ev[0], ev[1]) + rtx_elapsed_ms(ev[2], ev[3]);
            h->user_ms += rtx_elapsed_ms(ev[1], ev[2]);
            h->item_ms += rtx_elapsed_ms(ev[3], ev[4]);
        }
        RTX_TRY(wmf_gram(h->Y, ni, f, gsl, h->G, st));
        RTX_HIP(hipEventRecord(ev[6], st));
        RTX_HIP(hipStreamSynchronize(st));
        h->fit_ms = rtx_elapsed_ms(ev[5], ev[6]);
        RTX_TRY(wmf_status("wmf_fit", h->status));
        return RTX_OK;
    }();
    if (rc) {
        (void)hipStreamSynchronize(st);   // launches already queued may use the pool, which is freed on return
        return rc;
    }
    *out = h.release();
    return RTX_OK;
}

int rtx_wmf_load(int32_t n_items, int32_t f, double alpha, double lam, const double* Y_host, rtx_wmf** out)
{
    RTX_CHECK(Y_host && out, RTX_EINVAL, "wmf_load: NULL argument");
    RTX_TRY(wmf_check_params("wmf_load", f, alpha, lam));
    RTX_CHECK(n_items > 0, RTX_EINVAL, "wmf_load: n_items = %d", n_items);
    rtx_wmf* h = new rtx_wmf();
    h->n_items = n_items; h->f = f; h->alpha = alpha; h->lam = lam;
    std::vector<void*> work;
    double* gsl = nullptr;
    int rc = RTX_OK;
    hipError_t e = hipMalloc((void**)&h->Y, sizeof(double) * (size_t)n_items * f);
    if (e == hipSuccess) e = hipMalloc((void**)&h->G, sizeof(double) * (size_t)f * f);
    if (e == hipSuccess) e = hipMalloc((void**)&h->status, sizeof(int));
    if (e == hipSuccess) e = hipMemset(h->status, 0, sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(h->Y, Y_host, sizeof(double) * (size_t)n_items * f, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        rtx_set_error("wmf_load: %s", hipGetErrorString(e));
        rc = RTX_EHIP;
    }
    if (!rc) rc = rtx_pool_alloc("wmf", (void**)&gsl, sizeof(double) * wmf_gram_slabs(n_items, f), work);
    if (!rc) rc = wmf_gram(h->Y, n_items, f, gsl, h->G, nullptr);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) {
        rtx_set_error("wmf_load: the Gram matrix of the factors failed");
        rc = RTX_EHIP;
    }
    rtx_free_all(work);
    if (rc) {
        wmf_free(h);
        return rc;
    }
    *out = h;
    return RTX_OK;
}

int rtx_wmf_destroy(rtx_wmf* h)
{
    if (h) wmf_free(h);
    return RTX_OK;
}

int rtx_wmf_shape(const rtx_wmf* h, int32_t* n_users, int32_t* n_items, int32_t* f)
{
    RTX_CHECK(h, RTX_EINVAL, "wmf: NULL handle");
    if (n_users) *n_users = h->U ? h->n_users : 0;
    if (n_items) *n_items = h->n_items;
    if (f) *f = h->f;
    return RTX_OK;
}

int rtx_wmf_copy(const rtx_wmf* h, int32_t what, double* dst_dev, void* stream)
{
    RTX_CHECK(h && dst_dev, RTX_EINVAL, "wmf_copy: NULL argument");
    RTX_CHECK(what == RTX_WMF_ITEMS || what == RTX_WMF_USERS, RTX_EINVAL, "wmf_copy: unknown table %d (RTX_WMF_ITEMS = 0, RTX_WMF_USERS = 1)", what);
    RTX_CHECK(what == RTX_WMF_ITEMS || h->U, RTX_EINVAL, "wmf_copy: this model was loaded from its item factors and holds no user factors");
    const double* src = what == RTX_WMF_ITEMS ? h->Y : h->U;
    const size_t n = what == RTX_WMF_ITEMS ? (size_t)h->n_items : (size_t)h->n_users;
    RTX_HIP(hipMemcpyAsync(dst_dev, src, sizeof(double) * n * h->f, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RTX_OK;
}

int rtx_wmf_timings(const rtx_wmf* h, double* fit_ms, double* gram_ms, double* user_ms, double* item_ms)
{
    RTX_CHECK(h, RTX_EINVAL, "wmf: NULL handle");
    if (fit_ms) *fit_ms = h->fit_ms;
    if (gram_ms) *gram_ms = h->gram_ms;
    if (user_ms) *user_ms = h->user_ms;
    if (item_ms) *item_ms = h->item_ms;
    return RTX_OK;
}

int rtx_wmf_scores(rtx_wmf* h, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const rtx_csr* mask, const int32_t* mask_row_ids,
                   double* out, int64_t ld, void* stream)
{
    RTX_CHECK(h && X && out, RTX_EINVAL, "wmf_scores: NULL argument");
    RtxCsrView xv, mv;   // (the rows are folded in by wmf_rows, which takes the matrix itself: only the mask's view is used)
    RTX_TRY(rtx_scores_args("wmf_scores", h->n_items, X, row_ids, batch, mask, mask_row_ids, &xv, &mv));
    RTX_CHECK(ld >= h->n_items, RTX_EINVAL, "wmf_scores: ld = %lld is below the model's %d items", (long long)ld, h->n_items);
    RTX_TRY(wmf_check_values("wmf_scores", X));
    if (batch == 0) return RTX_OK;
    hipStream_t st = (hipStream_t)stream;
    if (batch > h->xcap) {
        RTX_HIP(hipStreamSynchronize(st));   // launches that read the old buffer
        if (h->xbuf) (void)hipFree(h->xbuf);
        h->xbuf = nullptr;
        h->xcap = 0;
        RTX_HIP(hipMalloc((void**)&h->xbuf, sizeof(double) * (size_t)batch * h->f));
        h->xcap = batch;
    }
    std::vector<void*> work;
    WmfPlan plan;
    int rc = wmf_plan(X, row_ids, batch, wmf_nt(h->f), &plan, work, st);
    if (!rc) rc = wmf_rows(X, row_ids, batch, h->Y, h->f, h->alpha, h->lam, h->G, plan, WMF_SOLVE, h->xbuf, nullptr, h->status, st);
    if (!rc) {
        hipLaunchKernelGGL(k_wmf_scores, dim3((h->n_items + 255) / 256, (batch + WMF_SU - 1) / WMF_SU), dim3(256), 0, st, h->xbuf, h->Y, h->f,
                           h->n_items, batch, mv, out, ld);
        if (hipGetLastError() != hipSuccess) {
            rtx_set_error("wmf_scores: the launch failed");
            rc = RTX_EHIP;
        }
    }
    if (!work.empty()) {   // a batch with long rows: its slabs are freed once the stream has run
        (void)hipStreamSynchronize(st);
        rtx_free_all(work);
    }
    return rc;
}

}  // extern "C"
