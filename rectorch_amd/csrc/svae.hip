// svae.hip -- Sequential VAE (BASELINE.json configs[4]) on MI355X: one user sequence per optimizer step (the reference's
// semantics), or a pack of users per step.
//
// Reference: rectorch/nets.py:624-693 (SVAE_net: Embedding -> 1-layer GRU (batch_first) -> VAE head that ALWAYS samples
// (VAE_net._reparameterize, nets.py:316-319) -> tanh MLP decoder), rectorch/models.py:1609-1635 (SVAE: loss =
// sum_t NLL_t / #target-ones + beta * mean_t KL_t; Adam with weight_decay 5e-3; predict = last time step, -inf at the
// items of the input sequence).
//
// The reference trains one user (T ~ 100 time steps) per Adam step, so every contraction is a [T, small] x [small, *]
// product: the step is bound by launch latency and by the strictly sequential GRU recurrence, not by MFMA throughput.
// Design for that regime (all float32, so parity with the reference is ~1e-6):
//   * one generic strided GEMM kernel (64x64 tile on the exact-float32 MFMA, bias / tanh / tanh'-mask epilogues) serves every
//     forward, backward-data and weight-gradient product -- operands are read in place with strides, no padded copies;
//   * the GRU recurrence (forward and BPTT) runs as ONE persistent workgroup per sequence and direction (svae_gru.hip: the kernels,
//     their LDS sizing and the choice among them; this file sees a plan and two launch functions, svae_internal.h); the input
//     projections x_t W_ih^T for all t are one GEMM before the loop, and the weight gradients are two GEMMs over all t after it;
//   * Adam over the 5 + 2(n_enc + n_dec) tensors is the one fused multi-tensor kernel of the Mult-VAE path (k_adam).
// rtx_svae_train_pack (round 2) takes several users per optimizer step: concatenated rows, one recurrence workgroup per user
// side by side, [sum T, .] products on the float32 MFMA, the recurrences with W_hh resident in registers + LDS -- 440 -> 806 users/s
// per user, 21 600 users/s with packs of 128 at the ml-1m shape (SVAE_Sampler(pack=N)).
// Round 3: both recurrences with the mat-vec split over K inside the wave (1.43 us per forward time step, 3.6 in round 2; backward
// 1.63, was 2.06) -- 1 175-1 196 users/s per user, 26 900 with packs of 64.
// rtx_svae_predict_pack: SVAE.predict for a pack of users -- the packed recurrence, then only each user's last GRU state through the
// encoder head and the decoder ([n_seq, .] products instead of [sum T, .]); evaluate() 1.94 K -> 47.2 K users/s with packs of 128.
// rtx_svae_forward_train / rtx_svae_backward / rtx_svae_apply_adam: the training step cut into its forward, its backward chain entered
// from a caller's d loss / d logits, d mu, d logvar, and its Adam -- a loss_function the handle does not know (SVAE.custom_loss,
// SVAE_net.differentiable).  sv_train runs the same static functions with its own loss between them.
#include "../../include/rectorch_hip.h"
#include "rtx_kernels.h"
#include "svae_internal.h"

#include <math.h>
#include <string.h>
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <vector>

#define SV_MAX_LAYERS RTX_MAX_LAYERS

struct SvLayer {
    int in = 0, out = 0;
    bool tanh_act = false;
    float* A = nullptr;     // [Tmax][out] activation (post-tanh, or raw for the linear layers)
    float* D = nullptr;     // [Tmax][out] gradient w.r.t. the pre-activation
};

struct rtx_svae {
    rtx_svae_cfg cfg;
    int I = 0, E = 0, R = 0, Z = 0, NL = 0, n_enc = 0, Tmax = 0;
    std::vector<SvLayer> L;          // encoder layers then decoder layers
    int n_tensors = 0;
    std::vector<float*> params, grads, m, v;
    bool bound = false, can_train = false;
    // activations / scratch (device)
    float *X = nullptr, *GI = nullptr, *Hout = nullptr, *Hprev = nullptr, *Gr = nullptr, *Gz = nullptr, *Gn = nullptr, *Ghn = nullptr;
    float *mu = nullptr, *lv = nullptr, *eps = nullptr, *zl = nullptr, *dz = nullptr;
    float *dH = nullptr, *dGI = nullptr, *dGH = nullptr, *dX = nullptr;
    float *row_loss = nullptr, *kl_rows = nullptr;
    float* part = nullptr;           // split-K partial sums
    float* part2 = nullptr;          // ... of the GEMMs on the side stream
    hipStream_t side = nullptr;      // weight-gradient GEMMs of the MLPs: they overlap the single-workgroup GRU backward
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_fork2 = nullptr, ev_join2 = nullptr;
    float* WhhT = nullptr;           // [R][3R] transposed recurrent weights: scratch of the generic forward recurrence
    SvGruPlan gru;                   // which recurrence kernels this handle launches (svae_gru.hip), fixed at create time
    int opt_gemm_bf16 = 0;           // rtx_svae_set_option "gemm_bf16": bf16 operands (f32 accumulate) in every k_sv_gemm product
    RtxOptim optim;                  // rtx_svae_set_optimizer: the update rule of sv_adam (default: Adam, coupled decay)
    RtxClipState clip;               // rtx_svae_set_grad_clip: sv_adam's norm pass / clipping instantiation (default: none)
    size_t part_elems = 0;
    std::vector<void*> allocs;
    // rtx_svae_loss_mailbox: {loss bits, ticket} in coherent host memory, stored by k_sv_final_loss -- train_batch returns THIS step's
    // loss (reference models.py:835) as soon as the forward half of the step has run, without draining the stream behind it
    uint32_t* loss_mailbox = nullptr;
    uint32_t loss_ticket = 0;
    // rtx_svae_forward_train / rtx_svae_backward: the name of the activations this handle holds.  Every sv_rnn -- so every forward,
    // prediction and training step -- takes the next one of a process-wide sequence (tickets of two handles never coincide);
    // act_T / act_nseq: the rows and sequences of the training forward the ticket was handed out for (0: none)
    uint64_t act_ticket = 0;
    int act_T = 0, act_nseq = 0;
};

// ------------------------------------------------------------------------------------------------ kernels
// C[m][n] (ldc) = epi( alpha * sum_k A(m,k) * B(n,k) (+ C if accumulate) ), A(m,k) = A[m*sam + k*sak], B(n,k) = B[n*sbn + k*sbk]
enum { SV_EPI_NONE = 0, SV_EPI_BIAS = 1, SV_EPI_BIAS_TANH = 2, SV_EPI_TANH_GRAD = 3 };
struct SvGemm {
    const float* A; long sam, sak;
    const float* B; long sbn, sbk;
    float* C; long ldc;
    int M, N, K;
    float alpha;
    int epi;
    const float* bias;   // [N]        (SV_EPI_BIAS*)
    const float* Q;      // [M][ldq]   (SV_EPI_TANH_GRAD: C = acc * (1 - Q^2))
    long ldq;
    int kchunk;          // split-K: workgroup z handles k in [z * kchunk, (z + 1) * kchunk) and stores its raw partial
    float* part;         //          sums to part[z][M][N]; k_sv_splitk_reduce then applies the epilogue (0 / NULL = off)
};

typedef __attribute__((ext_vector_type(16))) float sv_f32x16;
typedef __attribute__((ext_vector_type(4))) float sv_f32x4;
// LDS read with a compile-time byte offset (the GEMM kernels' idiom: an asm read is issued where it is written)
#define sv_lds_rd128(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF))

// 64 x 64 tile per workgroup, 4 waves, each a 32 x 32 block on the exact-float32 MFMA (v_mfma_f32_32x32x2_f32: lane l feeds
// A[l & 31][k = l >> 5] and B[k = l >> 5][l & 31], products and sums in float32).  Round 1 computed the tile with scalar FMAs
// (8 LDS floats per 16 FMAs per thread: LDS-bound); with several users packed per step these products are [sum T, .] GEMMs of
// tens of GFLOP and the matrix pipes carry them.  The operands are still read in place with two strides.
// BF = true (rtx_svae_set_option "gemm_bf16", the dtype BASELINE.json configs[4] names): the operands are rounded to bf16
// (round-to-nearest-even) on their way into LDS, stored row-major [m][16 k] so that a lane's eight k values are ONE 16-byte read,
// and a chunk is ONE v_mfma_f32_32x32x16_bf16 per wave instead of eight float32 MFMAs; sums, outputs, master weights stay float32.
typedef __attribute__((ext_vector_type(8))) __bf16 sv_bf16x8;
template <bool BF>
__global__ __launch_bounds__(256) void k_sv_gemm(const SvGemm g)
{
    // (K chunks of 32 instead of 16 -- twice the MFMA time per chunk over the next chunk's load latency -- measured slower per
    //  user, 1 164 vs 1 194 users/s: the per-user products are a handful of workgroups each, bound by their first loads and the launch)
    constexpr int KC = 16, NQ = KC / 4;
    __shared__ float sA[BF ? 1 : KC][65], sB[BF ? 1 : KC][65];
    __shared__ __attribute__((aligned(16))) bf16_t hA[BF ? 64 : 1][24], hB[BF ? 64 : 1][24];   // rows of 48 bytes: 16 k + padding
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int li = lane & 31, lk = lane >> 5;
    sv_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int kbeg = g.kchunk ? blockIdx.z * g.kchunk : 0;
    const int kend = g.kchunk ? min(g.K, kbeg + g.kchunk) : g.K;
    // 64 x KC elements per operand and K chunk, NQ per thread; the faster-varying thread index follows the unit-stride axis.
    // The next chunk's values are requested (into registers) before this chunk's MFMAs, so their latency runs under them.
    int amm[NQ], akk[NQ], bnn[NQ], bkk[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = tid + q * 256;
        if (g.sak == 1) { akk[q] = e % KC; amm[q] = e / KC; } else { amm[q] = e & 63; akk[q] = e >> 6; }
        if (g.sbk == 1) { bkk[q] = e % KC; bnn[q] = e / KC; } else { bnn[q] = e & 63; bkk[q] = e >> 6; }
    }
    float ra[NQ], rb[NQ];
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int m = m0 + amm[q], k = k0 + akk[q];
            ra[q] = (m < g.M && k < kend) ? g.A[(size_t)m * g.sam + (size_t)k * g.sak] : 0.f;
            const int n = n0 + bnn[q], kb = k0 + bkk[q];
            rb[q] = (n < g.N && kb < kend) ? g.B[(size_t)n * g.sbn + (size_t)kb * g.sbk] : 0.f;
        }
    };
    if (kbeg < kend) fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += KC) {
        if constexpr (BF) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) { hA[amm[q]][akk[q]] = f32_to_bf16(ra[q]); hB[bnn[q]][bkk[q]] = f32_to_bf16(rb[q]); }
        } else {
#pragma unroll
            for (int q = 0; q < NQ; ++q) { sA[akk[q]][amm[q]] = ra[q]; sB[bkk[q]][bnn[q]] = rb[q]; }
        }
        __syncthreads();
        if (k0 + KC < kend) fetch(k0 + KC);
        if constexpr (BF) {
            // 32x32x16: lane l feeds row l & 31, k = 8 (l >> 5) .. + 7 of both operands
            const sv_bf16x8 a = *(const sv_bf16x8*)&hA[wm + li][lk * 8];
            const sv_bf16x8 b = *(const sv_bf16x8*)&hB[wn + li][lk * 8];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
        } else {
#pragma unroll
            for (int kk = 0; kk < KC; kk += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[kk + lk][wm + li], sB[kk + lk][wn + li], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    // What the epilogue reads is requested ONCE, up front, from clamped addresses (the bias of this lane's column; for the tanh'
    // mask all 16 values of Q): read per element under the row guard they were 16 dependent L2 round trips -- a load and a
    // vmcnt(0) per element -- about 3 us per launch of a kernel that takes 12.
    const int n = n0 + wn + li;
    if (n >= g.N) return;
    const int mb = m0 + wm + 4 * lk;
    const bool raw = g.kchunk != 0;
    float bv = 0.f;
    if (!raw && (g.epi == SV_EPI_BIAS || g.epi == SV_EPI_BIAS_TANH)) bv = g.bias[n];
    float qv[16];
    if (!raw && g.epi == SV_EPI_TANH_GRAD) {
#pragma unroll
        for (int e = 0; e < 16; ++e) qv[e] = g.Q[(size_t)min(mb + (e & 3) + 8 * (e >> 2), g.M - 1) * g.ldq + n];
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) qv[e] = 0.f;
    }
    float* out = raw ? g.part + (size_t)blockIdx.z * g.M * g.N : g.C;
    const size_t ldo = raw ? (size_t)g.N : (size_t)g.ldc;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = mb + (e & 3) + 8 * (e >> 2);
        float v = g.alpha * acc[e];
        if (!raw) {
            v += bv;
            if (g.epi == SV_EPI_BIAS_TANH) v = tanhf(v);
            v *= (1.f - qv[e] * qv[e]);
        }
        if (m < g.M) out[(size_t)m * ldo + n] = v;
    }
}

__global__ __launch_bounds__(256) void k_sv_splitk_reduce(const SvGemm g, int splits)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)g.M * g.N) return;
    const int m = (int)(idx / g.N), n = (int)(idx % g.N);
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += g.part[(size_t)z * g.M * g.N + idx];
    if (g.epi == SV_EPI_BIAS || g.epi == SV_EPI_BIAS_TANH) v += g.bias[n];
    if (g.epi == SV_EPI_BIAS_TANH) v = tanhf(v);
    if (g.epi == SV_EPI_TANH_GRAD) { const float q = g.Q[(size_t)m * g.ldq + n]; v *= (1.f - q * q); }
    g.C[(size_t)m * g.ldc + n] = v;
}

// out[n] = sum_t D[t][n]  (bias gradients): a workgroup sums 32 time steps of 256 columns; the row blocks meet through
// atomicAdd on the zeroed output
__global__ __launch_bounds__(256) void k_sv_colsum(const float* D, long ld, int T, int N, float* out)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int t0 = blockIdx.y * 32, t1 = min(T, t0 + 32);
    float s = 0.f;
    for (int t = t0; t < t1; ++t) s += D[(size_t)t * ld + n];
    atomicAdd(out + n, s);
}

// the same in ONE pass for short inputs (one user: T ~ 150): a workgroup owns 64 columns, its four waves take every fourth row and
// meet in LDS -- no zero fill of the output, no atomics (round 3: the per-user step issued six 5-us memsets for these sums)
__global__ __launch_bounds__(256) void k_sv_colsum1(const float* D, long ld, int T, int N, float* out)
{
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6, n = blockIdx.x * 64 + c;
    float s0 = 0.f, s1 = 0.f;
    if (n < N) {
        int t = rg;
        for (; t + 4 < T; t += 8) { s0 += D[(size_t)t * ld + n]; s1 += D[(size_t)(t + 4) * ld + n]; }
        if (t < T) s0 += D[(size_t)t * ld + n];
    }
    part[rg][c] = s0 + s1;
    __syncthreads();
    if (rg == 0 && n < N) out[n] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

__global__ __launch_bounds__(256) void k_sv_embed(const int32_t* items, int T, int E, const float* emb, float* X)
{
    const int t = blockIdx.x;
    const float* src = emb + (size_t)items[t] * E;
    for (int e = threadIdx.x; e < E; e += 256) X[(size_t)t * E + e] = src[e];
}

__global__ __launch_bounds__(256) void k_sv_embed_grad(const int32_t* items, int T, int E, const float* dX, float* demb)
{
    const int t = blockIdx.x;
    float* dst = demb + (size_t)items[t] * E;
    for (int e = threadIdx.x; e < E; e += 256) atomicAdd(dst + e, dX[(size_t)t * E + e]);   // an item may repeat in a sequence
}

// block-wide reductions for 256-thread blocks; red must hold >= 4 floats; result broadcast to all threads
__device__ __forceinline__ float block_sum(float v, float* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max(float v, float* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// encoder head: out [T][2Z] = mu | logvar; z = mu + eps * exp(logvar / 2) with eps injected or Philox (always sampled)
// `last_of` (rtx_svae_predict_pack: seq_ptr, row t = user t's last step): the draw of row t is the one row last_of[t + 1] - 1 of the
// all-rows forward takes -- its injected row, or its Philox counter -- so a pack scores what that forward scores in those rows
__global__ __launch_bounds__(256) void k_sv_reparam(const float* out, int T, int Z, const float* eps_in, uint64_t seed, uint64_t offset,
                                                    const int32_t* __restrict__ last_of, float* mu, float* lv, float* eps_out, float* z)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * Z) return;
    const int t = idx / Z, j = idx % Z;
    const float m = out[(size_t)t * 2 * Z + j], l = out[(size_t)t * 2 * Z + Z + j];
    const size_t src = last_of ? (size_t)(last_of[t + 1] - 1) * Z + j : (size_t)idx;
    const float e = eps_in ? eps_in[src] : rtx_normal(seed, offset, (uint64_t)src);
    mu[idx] = m; lv[idx] = l; eps_out[idx] = e;
    z[idx] = m + e * expf(0.5f * l);
}

// gradient w.r.t. the encoder head output [T][2Z] from dz and
//   KL = true:  the KL term  beta * mean_t(-0.5 sum_j (1 + lv - mu^2 - e^lv));  kl_rows[t] = -0.5 sum_j(...)
//   KL = false: the caller's d loss / d mu, d loss / d logvar [T][Z] (rtx_svae_backward; either NULL = zero, as is a NULL dz: a
//               loss that does not reach the decoder) -- no KL sum, no kl_rows
template <bool KL>
__global__ __launch_bounds__(256) void k_sv_reparam_bwd(const float* dz, const float* mu, const float* lv, const float* eps, int T, int Z,
                                                        float beta_over_T, const float* __restrict__ kl_scale /* per row, or NULL */,
                                                        const float* __restrict__ d_mu, const float* __restrict__ d_lv, float* dout,
                                                        float* kl_rows)
{
    const int t = blockIdx.x;
    if constexpr (KL) {
        __shared__ float red[4];
        if (kl_scale) beta_over_T = kl_scale[t];   // packed users: beta / (T_user * n_users)
        float kl = 0.f;
        for (int j = threadIdx.x; j < Z; j += 256) {
            const int idx = t * Z + j;
            const float m = mu[idx], l = lv[idx], el = expf(l), sd = expf(0.5f * l);
            kl += -0.5f * (1.f + l - m * m - el);
            if (dout) {
                const float d = dz[idx];
                dout[(size_t)t * 2 * Z + j] = d + beta_over_T * m;
                dout[(size_t)t * 2 * Z + Z + j] = d * eps[idx] * 0.5f * sd + beta_over_T * 0.5f * (el - 1.f);
            }
        }
        kl = block_sum(kl, red);
        if (threadIdx.x == 0) kl_rows[t] = kl;
    } else {
        for (int j = threadIdx.x; j < Z; j += 256) {
            const int idx = t * Z + j;
            const float d = dz ? dz[idx] : 0.f;
            dout[(size_t)t * 2 * Z + j] = d + (d_mu ? d_mu[idx] : 0.f);
            dout[(size_t)t * 2 * Z + Z + j] = d * eps[idx] * 0.5f * expf(0.5f * lv[idx]) + (d_lv ? d_lv[idx] : 0.f);
        }
    }
}

// rtx_svae_backward with a row stride above n_items: dst [T][I] = src [T][ld] (a contiguous gradient is read in place instead)
__global__ __launch_bounds__(256) void k_sv_import_rows(const float* __restrict__ src, long ld, int T, int I, float* __restrict__ dst)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)T * I) return;
    const long t = idx / I, i = idx % I;
    dst[idx] = src[t * ld + i];
}

// per time step: log-softmax NLL against the target row (CSR, or dense [T][I]) and the logits gradient
//   nll_t = -sum_i y_ti (x_ti - lse_t);  dlogits = (s_t softmax - y) * inv_d
__global__ __launch_bounds__(256) void k_sv_loss(const float* logits, int T, int I, const int64_t* tptr, const int32_t* tidx,
                                                 const float* ydense, float inv_d, const float* __restrict__ nll_scale /* per row, or NULL */,
                                                 float* dlogits, float* row_loss)
{
    __shared__ float red[4];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (nll_scale) inv_d = nll_scale[t];   // packed users: 1 / (d_user * n_users)
    const float* x = logits + (size_t)t * I;
    float mx = -INFINITY;
    for (int i = tid; i < I; i += 256) mx = fmaxf(mx, x[i]);
    mx = block_max(mx, red);
    float se = 0.f;
    for (int i = tid; i < I; i += 256) se += expf(x[i] - mx);
    se = block_sum(se, red);
    const float lse = mx + logf(se);
    float s = 0.f, dot = 0.f;
    if (ydense) {
        const float* y = ydense + (size_t)t * I;
        for (int i = tid; i < I; i += 256) { s += y[i]; dot += y[i] * x[i]; }
    } else {
        for (int64_t k = tptr[t] + tid; k < tptr[t + 1]; k += 256) { s += 1.f; dot += x[tidx[k]]; }
    }
    s = block_sum(s, red);
    dot = block_sum(dot, red);
    if (tid == 0) row_loss[t] = s * lse - dot;
    if (dlogits) {
        float* d = dlogits + (size_t)t * I;
        if (ydense) {
            const float* y = ydense + (size_t)t * I;
            for (int i = tid; i < I; i += 256) d[i] = (s * expf(x[i] - lse) - y[i]) * inv_d;
        } else {
            for (int i = tid; i < I; i += 256) d[i] = s * expf(x[i] - lse) * inv_d;
            __syncthreads();
            for (int64_t k = tptr[t] + tid; k < tptr[t + 1]; k += 256) d[tidx[k]] -= inv_d;   // indices are distinct within a row
        }
    }
}

__global__ __launch_bounds__(256) void k_sv_final_loss(const float* row_loss, const float* kl_rows, int T, float inv_d, float beta_over_T,
                                                       const float* __restrict__ nll_scale, const float* __restrict__ kl_scale, float* loss_out,
                                                       float* loss_accum, uint32_t* mailbox, uint32_t seq)
{
    __shared__ float red[4];
    float a = 0.f, b = 0.f;
    if (nll_scale) {   // packed users: every row carries its user's factors
        for (int t = threadIdx.x; t < T; t += 256) { a += row_loss[t] * nll_scale[t]; b += kl_rows[t] * kl_scale[t]; }
        inv_d = 1.f; beta_over_T = 1.f;
    } else {
        for (int t = threadIdx.x; t < T; t += 256) { a += row_loss[t]; b += kl_rows[t]; }
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        const float l = a * inv_d + beta_over_T * b;
        if (loss_out) loss_out[0] = l;
        if (loss_accum) loss_accum[0] += l;
        if (mailbox) {   // (system scope: the host spins on the ticket -- rtx_svae_wait_loss)
            __hip_atomic_store(mailbox, __float_as_uint(l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(mailbox + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

__global__ __launch_bounds__(256) void k_sv_mask_items(const int32_t* items, int T, float* row)
{
    for (int t = threadIdx.x; t < T; t += 256) row[items[t]] = -INFINITY;
}

// rtx_svae_predict_pack: row u of `out` [n_seq][R] = the GRU state after user u's LAST step, row seq_ptr[u + 1] - 1 of Hout [T][R]
// (one workgroup per user, consecutive lanes copy consecutive floats; 16 bytes per lane when the rows are 16-byte aligned)
__global__ __launch_bounds__(256) void k_sv_gather_last(const float* __restrict__ Hout, const int32_t* __restrict__ seq_ptr, int T, int R,
                                                        float* __restrict__ out)
{
    const int u = blockIdx.x, row = seq_ptr[u + 1] - 1;
    if (row < 0 || row >= T) return;   // a malformed seq_ptr reads nothing out of bounds
    const float* src = Hout + (size_t)row * R;
    float* dst = out + (size_t)u * R;
    if ((R & 3) == 0) {
        for (int j = threadIdx.x; j < R / 4; j += 256) ((sv_f32x4*)dst)[j] = ((const sv_f32x4*)src)[j];
    } else {
        for (int j = threadIdx.x; j < R; j += 256) dst[j] = src[j];
    }
}

// the pack form of k_sv_mask_items (models.py:1633-1634 per user): one workgroup per user stores -inf at
// scores[u][items[seq_ptr[u] .. seq_ptr[u + 1])]
__global__ __launch_bounds__(256) void k_sv_mask_items_pack(const int32_t* __restrict__ items, const int32_t* __restrict__ seq_ptr, int T, int I,
                                                            float* __restrict__ scores)
{
    const int u = blockIdx.x;
    const int lo = max(seq_ptr[u], 0), hi = min(seq_ptr[u + 1], T);
    float* row = scores + (size_t)u * I;
    for (int t = lo + threadIdx.x; t < hi; t += 256) {
        const int it = items[t];
        if ((unsigned)it < (unsigned)I) row[it] = -INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ host side
static int sv_alloc(rtx_svae* s, float** p, size_t n)
{
    hipError_t rc = hipMalloc((void**)p, sizeof(float) * (n ? n : 4));
    if (rc != hipSuccess) {
        rtx_set_error("svae: hipMalloc(%zu floats) failed: %s", n, hipGetErrorString(rc));
        return RTX_ENOMEM;
    }
    s->allocs.push_back(*p);
    return RTX_OK;
}

static int sv_gemm(rtx_svae* s, hipStream_t st, const float* A, long sam, long sak, const float* B, long sbn, long sbk, float* C, long ldc, int M,
                   int N, int K, int epi = SV_EPI_NONE, const float* bias = nullptr, const float* Q = nullptr, long ldq = 0, int lane = 0)
{
    if (M <= 0 || N <= 0) return RTX_OK;
    SvGemm g = {A, sam, sak, B, sbn, sbk, C, ldc, M, N, K, 1.f, epi, bias, Q, ldq, 0, nullptr};
    const int tiles = ((N + 63) / 64) * ((M + 63) / 64);
    // few output tiles and a long K (the [T, hidden] = [T, n_items] x [n_items, hidden] backward-data product): split K
    // so that a few hundred workgroups share the reduction instead of a handful walking it end to end
    // (with packed users K = sum T reaches tens of thousands in the weight-gradient products while their outputs are a few
    // hundred tiles: the [n_items, 150] decoder gradient ran 162 workgroups for 1 ms until it was split as well)
    int splits = 1;
    if (tiles < 512 && K >= 512) {
        splits = std::min((K + 255) / 256, std::max(1, 1024 / tiles));
        if ((size_t)splits * M * N > s->part_elems) splits = (int)(s->part_elems / ((size_t)M * N));
    }
    if (splits > 1) {
        g.kchunk = ((K + splits - 1) / splits + 15) / 16 * 16;
        splits = (K + g.kchunk - 1) / g.kchunk;
        g.part = lane ? s->part2 : s->part;   // the side stream sums into its own buffer
        if (s->opt_gemm_bf16) hipLaunchKernelGGL(k_sv_gemm<true>, dim3((N + 63) / 64, (M + 63) / 64, splits), dim3(256), 0, st, g);
        else hipLaunchKernelGGL(k_sv_gemm<false>, dim3((N + 63) / 64, (M + 63) / 64, splits), dim3(256), 0, st, g);
        hipLaunchKernelGGL(k_sv_splitk_reduce, dim3((unsigned)(((long)M * N + 255) / 256)), dim3(256), 0, st, g, splits);
    } else {
        if (s->opt_gemm_bf16) hipLaunchKernelGGL(k_sv_gemm<true>, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, st, g);
        else hipLaunchKernelGGL(k_sv_gemm<false>, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, st, g);
    }
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

static int sv_colsum(hipStream_t st, const float* D, long ld, int T, int N, float* out)
{
    if (T <= 2048) {
        hipLaunchKernelGGL(k_sv_colsum1, dim3((N + 63) / 64), dim3(256), 0, st, D, ld, T, N, out);
        RTX_HIP(hipGetLastError());
        return RTX_OK;
    }
    RTX_HIP(hipMemsetAsync(out, 0, sizeof(float) * N, st));
    hipLaunchKernelGGL(k_sv_colsum, dim3((N + 255) / 256, (T + 31) / 32), dim3(256), 0, st, D, ld, T, N, out);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// parameter order = SVAE_net.parameters(): enc W,b ..., dec W,b ..., item_embed.weight, gru.weight_ih_l0, weight_hh_l0,
// bias_ih_l0, bias_hh_l0 (VAE_net.__init__ registers the MLPs before SVAE_net adds the embedding and the GRU)
enum { SV_T_EMB = 0, SV_T_WIH = 1, SV_T_WHH = 2, SV_T_BIH = 3, SV_T_BHH = 4 };
static int sv_tail(const rtx_svae* s, int which) { return 2 * s->NL + which; }

static void sv_shape(const rtx_svae* s, int t, int* rows, int* cols)
{
    if (t < 2 * s->NL) {
        const SvLayer& l = s->L[t / 2];
        *rows = l.out;
        *cols = (t & 1) ? 1 : l.in;
        return;
    }
    switch (t - 2 * s->NL) {
    case SV_T_EMB: *rows = s->I; *cols = s->E; break;
    case SV_T_WIH: *rows = 3 * s->R; *cols = s->E; break;
    case SV_T_WHH: *rows = 3 * s->R; *cols = s->R; break;
    default: *rows = 3 * s->R; *cols = 1; break;
    }
}

static SvGruBufs sv_gru_bufs(const rtx_svae* s)
{
    return {s->params[sv_tail(s, SV_T_WHH)], s->params[sv_tail(s, SV_T_BHH)], s->WhhT, s->GI, s->Hout, s->Hprev, s->Gr, s->Gz, s->Gn, s->Ghn,
            s->dH, s->dGI, s->dGH};
}

static uint64_t sv_next_ticket()
{
    static std::atomic<uint64_t> seq{0};
    return ++seq;
}

// embedding -> input projection -> GRU recurrence: rnn_out[t] = h after step t lands in Hout [T][R]
// `seq_ptr` (device, n_seq + 1 entries) cuts the T rows into independent sequences; NULL = one sequence
static int sv_rnn(rtx_svae* s, const int32_t* items, int T, const int32_t* seq_ptr, int n_seq, hipStream_t st)
{
    const int E = s->E, R = s->R;
    s->act_ticket = sv_next_ticket();   // whatever activations a training forward left are being overwritten (rtx_svae_backward)
    s->act_T = s->act_nseq = 0;
    hipLaunchKernelGGL(k_sv_embed, dim3(T), dim3(256), 0, st, items, T, E, s->params[sv_tail(s, SV_T_EMB)], s->X);
    RTX_TRY(sv_gemm(s, st, s->X, E, 1, s->params[sv_tail(s, SV_T_WIH)], E, 1, s->GI, 3 * R, T, 3 * R, E, SV_EPI_BIAS,
                    s->params[sv_tail(s, SV_T_BIH)]));
    sv_gru_forward(s->gru, sv_gru_bufs(s), seq_ptr, n_seq, T, R, st);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// encoder -> (sampled) z -> decoder on the M rows of `in` [M][R]; the logits land in `logits` (NULL: L.back().A), mu / logvar /
// eps / z of the M rows in s->mu / lv / eps / zl.  `last_of`: see k_sv_reparam
static int sv_mlp(rtx_svae* s, const float* in, int M, const int32_t* last_of, const float* eps_in, uint64_t seed, uint64_t offset, float* logits,
                  hipStream_t st)
{
    const int Z = s->Z;
    long ld_in = s->R;
    for (int li = 0; li < s->NL; ++li) {
        SvLayer& l = s->L[li];
        float* out = (li == s->NL - 1 && logits) ? logits : l.A;
        RTX_TRY(sv_gemm(s, st, in, ld_in, 1, s->params[2 * li], l.in, 1, out, l.out, M, l.out, l.in, l.tanh_act ? SV_EPI_BIAS_TANH : SV_EPI_BIAS,
                        s->params[2 * li + 1]));
        in = out;
        ld_in = l.out;
        if (li == s->n_enc - 1) {
            hipLaunchKernelGGL(k_sv_reparam, dim3((M * Z + 255) / 256), dim3(256), 0, st, l.A, M, Z, eps_in, seed, offset, last_of, s->mu, s->lv,
                               s->eps, s->zl);
            in = s->zl;
            ld_in = Z;
        }
    }
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// embedding -> GRU -> encoder -> (sampled) z -> decoder; logits of all T steps land in `logits` [T][n_items] (NULL: L.back().A)
static int sv_forward(rtx_svae* s, const int32_t* items, int T, const int32_t* seq_ptr, int n_seq, const float* eps_in, uint64_t seed, uint64_t offset,
                      float* logits, hipStream_t st)
{
    RTX_TRY(sv_rnn(s, items, T, seq_ptr, n_seq, st));
    return sv_mlp(s, s->Hout, T, nullptr, eps_in, seed, offset, logits, st);
}

static int sv_check(const rtx_svae* s, const int32_t* items, int T, bool train)
{
    RTX_CHECK(s, RTX_EINVAL, "svae: NULL handle");
    RTX_CHECK(s->bound, RTX_ESTATE, "svae: parameters are not bound (rtx_svae_bind)");
    RTX_CHECK(!train || s->can_train, RTX_ESTATE, "svae: gradient / Adam buffers are not bound");
    RTX_CHECK(items && T >= 1 && T <= s->Tmax, RTX_EINVAL, "svae: sequence length %d outside [1, max_len = %d]", T, s->Tmax);
    return RTX_OK;
}

extern "C" {

int rtx_svae_create(const rtx_svae_cfg* cfg, rtx_svae** out)
{
    RTX_CHECK(cfg && out, RTX_EINVAL, "svae_create: NULL argument");
    RTX_CHECK(cfg->n_items > 0 && cfg->embed_size > 0 && cfg->rnn_size > 0 && cfg->max_len > 0, RTX_EINVAL, "svae_create: bad sizes");
    RTX_CHECK(cfg->n_enc >= 1 && cfg->n_dec >= 1 && cfg->n_enc <= SV_MAX_LAYERS && cfg->n_dec <= SV_MAX_LAYERS, RTX_EINVAL,
              "svae_create: bad layer counts %d/%d", cfg->n_enc, cfg->n_dec);
    RTX_CHECK(cfg->enc_dims[0] == cfg->rnn_size, RTX_EINVAL, "svae_create: enc_dims[0] = %d must equal rnn_size = %d", cfg->enc_dims[0],
              cfg->rnn_size);
    RTX_CHECK(cfg->enc_dims[cfg->n_enc] == cfg->dec_dims[0], RTX_EINVAL, "svae_create: latent size mismatch");
    RTX_CHECK(cfg->dec_dims[cfg->n_dec] == cfg->n_items, RTX_EINVAL, "svae_create: dec_dims[-1] = %d must equal n_items = %d",
              cfg->dec_dims[cfg->n_dec], cfg->n_items);
    RTX_CHECK(cfg->rnn_size <= 1024, RTX_EINVAL, "svae_create: rnn_size %d exceeds the LDS budget of the recurrent kernels (1024)", cfg->rnn_size);
    RTX_CHECK(2 * (cfg->n_enc + cfg->n_dec) + 5 <= RTX_MAX_TENSORS, RTX_EINVAL, "svae_create: too many parameter tensors for one Adam launch");
    int ndev = 0;
    hipError_t h = hipGetDeviceCount(&ndev);
    RTX_CHECK(h == hipSuccess && ndev > 0, RTX_EHIP, "no HIP device available (%s): librectorch_hip has no CPU path", hipGetErrorString(h));
    rtx_svae* s = new rtx_svae();
    s->cfg = *cfg;
    s->I = cfg->n_items; s->E = cfg->embed_size; s->R = cfg->rnn_size; s->Z = cfg->enc_dims[cfg->n_enc];
    s->n_enc = cfg->n_enc; s->NL = cfg->n_enc + cfg->n_dec; s->Tmax = cfg->max_len;
    for (int i = 0; i < cfg->n_enc; ++i) {
        SvLayer l;
        l.in = cfg->enc_dims[i];
        l.out = (i == cfg->n_enc - 1) ? 2 * cfg->enc_dims[i + 1] : cfg->enc_dims[i + 1];   // mu | logvar (nets.py:262-265)
        l.tanh_act = (i != cfg->n_enc - 1);                                                   // VAE_net.encode (nets.py:287-294)
        s->L.push_back(l);
    }
    for (int i = 0; i < cfg->n_dec; ++i) {
        SvLayer l;
        l.in = cfg->dec_dims[i]; l.out = cfg->dec_dims[i + 1];
        l.tanh_act = (i != cfg->n_dec - 1);                                                   // SVAE_net.decode (nets.py:683-687)
        s->L.push_back(l);
    }
    s->n_tensors = 2 * s->NL + 5;
    s->params.assign(s->n_tensors, nullptr);
    s->grads = s->m = s->v = s->params;
    const size_t T = s->Tmax, R = s->R, E = s->E, Z = s->Z;
    int rc = RTX_OK;
#define SV_ALLOC(p, n) do { rc = sv_alloc(s, &(p), (n)); if (rc) { rtx_svae_destroy(s); return rc; } } while (0)
    SV_ALLOC(s->X, T * E); SV_ALLOC(s->GI, T * 3 * R); SV_ALLOC(s->Hout, T * R); SV_ALLOC(s->Hprev, T * R);
    SV_ALLOC(s->Gr, T * R); SV_ALLOC(s->Gz, T * R); SV_ALLOC(s->Gn, T * R); SV_ALLOC(s->Ghn, T * R);
    SV_ALLOC(s->mu, T * Z); SV_ALLOC(s->lv, T * Z); SV_ALLOC(s->eps, T * Z); SV_ALLOC(s->zl, T * Z); SV_ALLOC(s->dz, T * Z);
    SV_ALLOC(s->dH, T * R); SV_ALLOC(s->dGI, T * 3 * R); SV_ALLOC(s->dGH, T * 3 * R); SV_ALLOC(s->dX, T * E);
    SV_ALLOC(s->row_loss, T); SV_ALLOC(s->kl_rows, T);
    SV_ALLOC(s->WhhT, 3 * R * R);
    {
        size_t widest = std::max((size_t)std::max(R, E), Z);
        for (auto& l : s->L) widest = std::max(widest, (size_t)std::min(l.in, l.out));
        s->part_elems = 16 * T * widest;   // up to 16 K-splits of the widest [T, hidden] product
        SV_ALLOC(s->part, s->part_elems);
        SV_ALLOC(s->part2, s->part_elems);
    }
    for (auto& l : s->L) { SV_ALLOC(l.A, T * l.out); SV_ALLOC(l.D, T * l.out); }
#undef SV_ALLOC
    rc = sv_gru_plan(s->R, &s->gru);
    if (rc) { rtx_svae_destroy(s); return rc; }
    if (hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_fork2, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&s->ev_join2, hipEventDisableTiming) != hipSuccess) {
        rtx_set_error("svae_create: cannot create the side stream");
        rtx_svae_destroy(s);
        return RTX_EHIP;
    }
    *out = s;
    return RTX_OK;
}

int rtx_svae_destroy(rtx_svae* s)
{
    if (!s) return RTX_OK;
    if (s->side) { (void)hipStreamSynchronize(s->side); (void)hipStreamDestroy(s->side); }
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    if (s->ev_fork2) (void)hipEventDestroy(s->ev_fork2);
    if (s->ev_join2) (void)hipEventDestroy(s->ev_join2);
    for (void* p : s->allocs) (void)hipFree(p);
    if (s->loss_mailbox) { (void)hipDeviceSynchronize(); (void)hipHostFree(s->loss_mailbox); }
    (void)hipDeviceSynchronize();
    rtx_clip_release(s->clip);
    delete s;
    return RTX_OK;
}

// The step's loss without draining the stream (ABI 8; the engine's rtx_engine_loss_mailbox / rtx_engine_wait_loss for the sequence model):
// `SVAE.train_batch` ends in `return loss.item()` (reference models.py:835), which made the host wait for the WHOLE step -- the loss is
// final before the backward recurrence starts -- and the GPU then idle while the host prepared the next user (60 us of 843 per user).
int rtx_svae_loss_mailbox(rtx_svae* s, int32_t enable)
{
    RTX_CHECK(s, RTX_EINVAL, "svae is NULL");
    if (enable && !s->loss_mailbox) {
        void* p = nullptr;
        RTX_HIP(hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped));
        memset(p, 0, 64);
        s->loss_mailbox = (uint32_t*)p;
        s->loss_ticket = 0;
    } else if (!enable && s->loss_mailbox) {
        RTX_HIP(hipDeviceSynchronize());
        (void)hipHostFree(s->loss_mailbox);
        s->loss_mailbox = nullptr;
    }
    return RTX_OK;
}

int rtx_svae_wait_loss(rtx_svae* s, float* loss_host, double timeout_s)
{
    RTX_CHECK(s && loss_host, RTX_EINVAL, "svae_wait_loss: NULL argument");
    RTX_CHECK(s->loss_mailbox && s->loss_ticket != 0, RTX_ESTATE, "svae_wait_loss: no training step has reported to the mailbox (rtx_svae_loss_mailbox(s, 1) first)");
    volatile uint32_t* mb = s->loss_mailbox;
    const uint32_t want = s->loss_ticket;       // the LAST step enqueued: steps are waited for in order
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
        if (__atomic_load_n(&mb[1], __ATOMIC_ACQUIRE) == want) break;
        if ((spin & 0x3ff) == 0x3ff) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            RTX_CHECK(el < (timeout_s > 0 ? timeout_s : 60.0), RTX_EHIP, "svae_wait_loss: the step did not report its loss within %.1f s (ticket %u of %u)", el,
                      (unsigned)mb[1], (unsigned)want);
            if (el > 0.002) sched_yield();
        }
    }
    const uint32_t bits = __atomic_load_n(&mb[0], __ATOMIC_RELAXED);
    memcpy(loss_host, &bits, 4);
    return RTX_OK;
}

int32_t rtx_svae_n_tensors(const rtx_svae* s) { return s ? s->n_tensors : 0; }

int rtx_svae_set_option(rtx_svae* s, const char* key, int32_t value)
{
    RTX_CHECK(s && key, RTX_EINVAL, "svae_set_option: NULL argument");
    if (!strcmp(key, "gemm_bf16")) s->opt_gemm_bf16 = value != 0;
    else {
        rtx_set_error("svae_set_option: unknown key '%s' (gemm_bf16)", key);
        return RTX_EINVAL;
    }
    return RTX_OK;
}

int rtx_svae_set_optimizer(rtx_svae* s, const rtx_optim* optim)
{
    RTX_CHECK(s && optim, RTX_EINVAL, "svae_set_optimizer: NULL argument");
    RtxOptim o;
    o.kind = optim->kind; o.flags = optim->flags; o.momentum = optim->momentum; o.dampening = optim->dampening; o.alpha = optim->alpha; o.lr_decay = optim->lr_decay;
    RTX_TRY(rtx_optim_validate(o));
    s->optim = o;
    return RTX_OK;
}

// gradient clipping for the sequence model (rtx_engine_set_grad_clip / rtx_engine_wait_grad_norm): every optimizer launch of the
// handle -- one sequence, packs, rtx_svae_apply_adam -- goes through sv_adam
int rtx_svae_set_grad_clip(rtx_svae* s, int32_t mode, double bound)
{
    RTX_CHECK(s, RTX_EINVAL, "svae_set_grad_clip: NULL handle");
    RTX_TRY(rtx_clip_validate(mode, bound, "svae_set_grad_clip"));
    s->clip.mode = mode;
    s->clip.bound = mode == RTX_CLIPM_NONE ? 0.0 : bound;
    return RTX_OK;
}

int rtx_svae_wait_grad_norm(rtx_svae* s, float* host, double timeout_s)
{
    RTX_CHECK(s, RTX_EINVAL, "svae_wait_grad_norm: NULL handle");
    return rtx_clip_wait_norm(s->clip, "svae_wait_grad_norm", host, timeout_s, nullptr);
}

int rtx_svae_get_option(const rtx_svae* s, const char* key, int32_t* value)
{
    RTX_CHECK(s && key && value, RTX_EINVAL, "svae_get_option: NULL argument");
    if (!strcmp(key, "gemm_bf16")) *value = s->opt_gemm_bf16;
    else if (!strcmp(key, "gru_fwd")) *value = s->gru.fwd;
    else if (!strcmp(key, "gru_bwd")) *value = s->gru.bwd;
    else {
        rtx_set_error("svae_get_option: unknown key '%s' (gemm_bf16, gru_fwd, gru_bwd)", key);
        return RTX_EINVAL;
    }
    return RTX_OK;
}

int rtx_svae_tensor_shape(const rtx_svae* s, int32_t t, int32_t* rows, int32_t* cols)
{
    RTX_CHECK(s && t >= 0 && t < s->n_tensors && rows && cols, RTX_EINVAL, "svae_tensor_shape: bad arguments");
    int r, c;
    sv_shape(s, t, &r, &c);
    *rows = r; *cols = c;
    return RTX_OK;
}

int rtx_svae_bind(rtx_svae* s, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq)
{
    RTX_CHECK(s && params, RTX_EINVAL, "svae_bind: NULL argument");
    for (int t = 0; t < s->n_tensors; ++t) {
        RTX_CHECK(params[t], RTX_EINVAL, "svae_bind: parameter %d is NULL", t);
        s->params[t] = params[t];
    }
    s->bound = true;
    s->can_train = grads && exp_avg && exp_avg_sq;
    if (s->can_train)
        for (int t = 0; t < s->n_tensors; ++t) {
            RTX_CHECK(grads[t] && exp_avg[t] && exp_avg_sq[t], RTX_EINVAL, "svae_bind: training buffer %d is NULL", t);
            s->grads[t] = grads[t]; s->m[t] = exp_avg[t]; s->v[t] = exp_avg_sq[t];
        }
    return RTX_OK;
}

int rtx_svae_forward(rtx_svae* s, const int32_t* items, int32_t T, const float* eps_noise, uint64_t seed, uint64_t offset,
                     int32_t remove_train, float* logits_all, float* logits_last, float* mu, float* logvar, void* stream)
{
    RTX_TRY(sv_check(s, items, T, false));
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(sv_forward(s, items, T, nullptr, 1, eps_noise, seed, offset, nullptr, st));
    const float* Y = s->L.back().A;
    const size_t I = s->I;
    if (logits_all) RTX_HIP(hipMemcpyAsync(logits_all, Y, sizeof(float) * T * I, hipMemcpyDeviceToDevice, st));
    if (logits_last) {
        RTX_HIP(hipMemcpyAsync(logits_last, Y + (size_t)(T - 1) * I, sizeof(float) * I, hipMemcpyDeviceToDevice, st));
        if (remove_train) hipLaunchKernelGGL(k_sv_mask_items, dim3(1), dim3(256), 0, st, items, T, logits_last);   // models.py:1633-1634
    }
    if (mu) RTX_HIP(hipMemcpyAsync(mu, s->mu, sizeof(float) * T * s->Z, hipMemcpyDeviceToDevice, st));
    if (logvar) RTX_HIP(hipMemcpyAsync(logvar, s->lv, sizeof(float) * T * s->Z, hipMemcpyDeviceToDevice, st));
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// Where the backward chain of the MLPs starts: the fused step's own loss (ext = false: `d_last` is the last layer's D as k_sv_loss
// wrote it, the head adds the KL term) or a gradient from outside (rtx_svae_backward: ext = true; `d_last` [T][n_items] is the caller's
// d loss / d logits or NULL = the loss does not reach the decoder, the head adds d_mu / d_lv, either nullable)
struct SvBwdStart {
    const float* d_last;
    bool ext;
    float beta_over_T;
    const float* kl_scale;
    const float *d_mu, *d_lv;
};

// ---- backward through decoder and encoder down to dH.  D of layer l = gradient w.r.t. its pre-activation
static int sv_backward_mlp(rtx_svae* s, int T, const SvBwdStart& b, hipStream_t st)
{
    const int E = s->E, R = s->R, Z = s->Z, I = s->I, NL = s->NL;
    const bool dec = b.d_last != nullptr;   // (always so in the fused step)
    auto D_of = [&](int li) { return li == NL - 1 ? b.d_last : (const float*)s->L[li].D; };
    // Only the chain of input gradients is on the critical path (it feeds the GRU's backward pass) ...
    for (int li = dec ? NL - 1 : s->n_enc; li >= 0; --li) {
        SvLayer& l = s->L[li];
        // gradient w.r.t. the layer input: [T][in] = D [T][out] x W [out][in]
        if (li == 0) {
            RTX_TRY(sv_gemm(s, st, l.D, l.out, 1, s->params[0], 1, l.in, s->dH, R, T, R, l.out));
        } else if (li == s->n_enc) {
            if (dec) RTX_TRY(sv_gemm(s, st, D_of(li), l.out, 1, s->params[2 * li], 1, l.in, s->dz, Z, T, Z, l.out));
            if (b.ext)
                hipLaunchKernelGGL(k_sv_reparam_bwd<false>, dim3(T), dim3(256), 0, st, dec ? s->dz : nullptr, s->mu, s->lv, s->eps, T, Z, 0.f,
                                   nullptr, b.d_mu, b.d_lv, s->L[li - 1].D, nullptr);
            else
                hipLaunchKernelGGL(k_sv_reparam_bwd<true>, dim3(T), dim3(256), 0, st, s->dz, s->mu, s->lv, s->eps, T, Z, b.beta_over_T, b.kl_scale,
                                   nullptr, nullptr, s->L[li - 1].D, s->kl_rows);
        } else {
            SvLayer& p = s->L[li - 1];   // tanh layer: D_prev = (D W) * (1 - A_prev^2)
            RTX_TRY(sv_gemm(s, st, D_of(li), l.out, 1, s->params[2 * li], 1, l.in, p.D, p.out, T, p.out, l.out, SV_EPI_TANH_GRAD, nullptr, p.A, p.out));
        }
    }
    // ... the weight gradients of the MLPs only feed Adam: on a side stream they run under the GRU's backward pass, which
    //     is ONE workgroup for ~0.85 ms while 255 compute units would otherwise idle
    RTX_HIP(hipEventRecord(s->ev_fork, st));
    RTX_HIP(hipStreamWaitEvent(s->side, s->ev_fork, 0));
    for (int li = NL - 1; li >= 0; --li) {
        SvLayer& l = s->L[li];
        if (li >= s->n_enc && !dec) {   // a loss that does not reach the decoder: its gradients are zeros, and are written
            RTX_HIP(hipMemsetAsync(s->grads[2 * li], 0, sizeof(float) * (size_t)l.out * l.in, s->side));
            RTX_HIP(hipMemsetAsync(s->grads[2 * li + 1], 0, sizeof(float) * (size_t)l.out, s->side));
            continue;
        }
        const float* in;
        long ld_in;
        if (li == 0) { in = s->Hout; ld_in = R; }
        else if (li == s->n_enc) { in = s->zl; ld_in = Z; }
        else { in = s->L[li - 1].A; ld_in = s->L[li - 1].out; }
        // dW[out][in] = sum_t D[t][out] * in[t][in];  db = column sums
        RTX_TRY(sv_gemm(s, s->side, D_of(li), 1, l.out, in, 1, ld_in, s->grads[2 * li], l.in, l.out, l.in, T, SV_EPI_NONE, nullptr, nullptr, 0, 1));
        RTX_TRY(sv_colsum(s->side, D_of(li), (long)l.out, T, l.out, s->grads[2 * li + 1]));
    }
    // (the zero fill of the embedding gradient -- I x E floats -- rides along: nothing reads it before the scatter-add at the end)
    RTX_HIP(hipMemsetAsync(s->grads[sv_tail(s, SV_T_EMB)], 0, sizeof(float) * (size_t)I * E, s->side));
    RTX_HIP(hipEventRecord(s->ev_join, s->side));
    return RTX_OK;
}

// ---- GRU backward through time from dH, its weight gradients over all steps at once, the embedding's scatter-add; joins the side
//      stream: every gradient buffer is final behind it on `st`
static int sv_backward_rnn(rtx_svae* s, const int32_t* items, int T, const int32_t* seq_ptr, int n_seq, hipStream_t st)
{
    const int E = s->E, R = s->R;
    sv_gru_backward(s->gru, sv_gru_bufs(s), seq_ptr, n_seq, T, R, st);
    // the hidden-side gradients (dW_hh, db_hh) go to the side stream, the input-side ones and the embedding's stay here: five
    // independent ~12-us launches become two chains of 2 and 4
    RTX_HIP(hipEventRecord(s->ev_fork2, st));
    RTX_HIP(hipStreamWaitEvent(s->side, s->ev_fork2, 0));
    RTX_TRY(sv_gemm(s, s->side, s->dGH, 1, 3 * R, s->Hprev, 1, R, s->grads[sv_tail(s, SV_T_WHH)], R, 3 * R, R, T, SV_EPI_NONE, nullptr, nullptr, 0, 1));   // dW_hh = dGH^T H_prev
    RTX_TRY(sv_colsum(s->side, s->dGH, (long)3 * R, T, 3 * R, s->grads[sv_tail(s, SV_T_BHH)]));
    RTX_HIP(hipEventRecord(s->ev_join2, s->side));
    RTX_TRY(sv_gemm(s, st, s->dGI, 1, 3 * R, s->X, 1, E, s->grads[sv_tail(s, SV_T_WIH)], E, 3 * R, E, T));          // dW_ih = dGI^T X
    RTX_TRY(sv_colsum(st, s->dGI, (long)3 * R, T, 3 * R, s->grads[sv_tail(s, SV_T_BIH)]));
    RTX_TRY(sv_gemm(s, st, s->dGI, 3 * R, 1, s->params[sv_tail(s, SV_T_WIH)], 1, E, s->dX, E, T, E, 3 * R));        // dX = dGI W_ih
    RTX_HIP(hipStreamWaitEvent(st, s->ev_join, 0));     // the MLPs' gradients and the zeroed embedding gradient (done long ago)
    hipLaunchKernelGGL(k_sv_embed_grad, dim3(T), dim3(256), 0, st, items, T, E, s->dX, s->grads[sv_tail(s, SV_T_EMB)]);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipStreamWaitEvent(st, s->ev_join2, 0));
    return RTX_OK;
}

// ---- the handle's optimizer (default: torch.optim.Adam, coupled weight decay 5e-3, models.py:1618-1620) over every bound tensor
static int sv_adam(rtx_svae* s, const rtx_step* step, hipStream_t st)
{
    RtxAdamArgs a = {};
    a.n = 0;
    for (int t = 0; t < s->n_tensors; ++t) {
        RtxAdamTensor& w = a.t[a.n++];
        int r, c;
        sv_shape(s, t, &r, &c);
        w.p = s->params[t]; w.g = s->grads[t]; w.g16 = nullptr; w.m = s->m[t]; w.v = s->v[t];
        w.sh = nullptr; w.shT = nullptr; w.ld_sh = 0; w.ld_shT = 0;
        if (c == 1) { w.rows = 1; w.cols = r; } else { w.rows = r; w.cols = c; }
    }
    RTX_TRY(rtx_optim_scalars(s->optim, step->lr, step->beta1, step->beta2, step->eps, step->weight_decay, step->step, a));
    return rtx_launch_clipped_adam(a, 0, s->clip, (uint32_t)step->step, st);
}

// One optimizer step on T rows: one sequence (seq_ptr NULL; the reference's step) or n_seq packed sequences whose rows carry
// their own loss factors (nll_scale / kl_scale, device arrays of T floats).
static int sv_train(rtx_svae* s, const int32_t* items, int T, const int32_t* seq_ptr, int n_seq, const float* nll_scale, const float* kl_scale,
                    const int64_t* target_indptr, const int32_t* target_indices, const float* target_dense, const rtx_step* step, float* loss_out,
                    float* loss_accum, hipStream_t st)
{
    const float inv_d = step->inv_batch;                 // 1 / (number of ones in the target), models.py:1623
    const float beta_over_T = step->beta / (float)T;     // beta * mean over the time steps, models.py:1624-1625
    RTX_TRY(sv_forward(s, items, T, seq_ptr, n_seq, step->eps_noise, step->seed, step->offset, nullptr, st));
    // ---- loss and dlogits
    SvLayer& last = s->L[s->NL - 1];
    hipLaunchKernelGGL(k_sv_loss, dim3(T), dim3(256), 0, st, last.A, T, s->I, target_indptr, target_indices, target_dense, inv_d, nll_scale, last.D,
                       s->row_loss);
    RTX_TRY(sv_backward_mlp(s, T, SvBwdStart{last.D, false, beta_over_T, kl_scale, nullptr, nullptr}, st));
    hipLaunchKernelGGL(k_sv_final_loss, dim3(1), dim3(256), 0, st, s->row_loss, s->kl_rows, T, inv_d, beta_over_T, nll_scale, kl_scale, loss_out,
                       loss_accum, s->loss_mailbox, s->loss_mailbox ? ++s->loss_ticket : 0u);
    RTX_TRY(sv_backward_rnn(s, items, T, seq_ptr, n_seq, st));
    return sv_adam(s, step, st);
}

int rtx_svae_train_step(rtx_svae* s, const int32_t* items, int32_t T, const int64_t* target_indptr, const int32_t* target_indices,
                        const float* target_dense, const rtx_step* step, float* loss_out, float* loss_accum, void* stream)
{
    RTX_TRY(sv_check(s, items, T, true));
    RTX_CHECK(step && step->step >= 1, RTX_EINVAL, "svae_train_step: step count must be >= 1");
    RTX_CHECK((target_indptr && target_indices) || target_dense, RTX_EINVAL, "svae_train_step: no target");
    return sv_train(s, items, T, nullptr, 1, nullptr, nullptr, target_indptr, target_indices, target_dense, step, loss_out, loss_accum,
                    (hipStream_t)stream);
}

// Several users per optimizer step (NOT in the reference, which takes one Adam step per user): the sequences are concatenated,
// row t belongs to the sequence whose [seq_ptr[u], seq_ptr[u + 1]) contains it, and the step minimises
//     sum_t nll_scale[t] * NLL_t + sum_t kl_scale[t] * KL_t
// -- with nll_scale = 1 / (d_user * n_seq) and kl_scale = beta / (T_user * n_seq) the mean over the pack of the reference's
// per-user loss, i.e. gradient accumulation over the pack followed by ONE Adam step.  Every product becomes a [sum T, .] GEMM;
// the recurrences run one workgroup per sequence, side by side.
int rtx_svae_train_pack(rtx_svae* s, const int32_t* items, int32_t total_steps, const int32_t* seq_ptr, int32_t n_seq, const float* nll_scale,
                        const float* kl_scale, const int64_t* target_indptr, const int32_t* target_indices, const rtx_step* step, float* loss_out,
                        float* loss_accum, void* stream)
{
    RTX_TRY(sv_check(s, items, total_steps, true));
    RTX_CHECK(step && step->step >= 1, RTX_EINVAL, "svae_train_pack: step count must be >= 1");
    RTX_CHECK(seq_ptr && n_seq >= 1 && n_seq <= total_steps, RTX_EINVAL, "svae_train_pack: %d sequences over %d steps", n_seq, total_steps);
    RTX_CHECK(nll_scale && kl_scale && target_indptr && target_indices, RTX_EINVAL, "svae_train_pack: NULL argument");
    return sv_train(s, items, total_steps, seq_ptr, n_seq, nll_scale, kl_scale, target_indptr, target_indices, nullptr, step, loss_out, loss_accum,
                    (hipStream_t)stream);
}

// SVAE.predict (models.py:1628-1635) for a pack of users (NOT in the reference): the recurrences as in rtx_svae_train_pack, then ONLY each
// user's last GRU state -- gathered into a compact [n_seq][R] matrix (k_sv_gather_last; dH is free outside a training step) -- goes
// through the encoder head, the sampler and the decoder: n_seq rows of [., n_items] logits instead of total_steps, written straight
// into `scores`.
int rtx_svae_predict_pack(rtx_svae* s, const int32_t* items, int32_t total_steps, const int32_t* seq_ptr, int32_t n_seq,
                          const float* eps_noise, uint64_t seed, uint64_t offset, int32_t remove_train, float* scores, float* mu,
                          float* logvar, void* stream)
{
    RTX_TRY(sv_check(s, items, total_steps, false));
    RTX_CHECK(seq_ptr && n_seq >= 1 && n_seq <= total_steps, RTX_EINVAL, "svae_predict_pack: %d sequences over %d steps", n_seq, total_steps);
    RTX_CHECK(scores, RTX_EINVAL, "svae_predict_pack: scores is NULL");
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(sv_rnn(s, items, total_steps, seq_ptr, n_seq, st));
    hipLaunchKernelGGL(k_sv_gather_last, dim3(n_seq), dim3(256), 0, st, s->Hout, seq_ptr, total_steps, s->R, s->dH);
    RTX_TRY(sv_mlp(s, s->dH, n_seq, seq_ptr, eps_noise, seed, offset, scores, st));
    if (remove_train)
        hipLaunchKernelGGL(k_sv_mask_items_pack, dim3(n_seq), dim3(256), 0, st, items, seq_ptr, total_steps, s->I, scores);
    if (mu) RTX_HIP(hipMemcpyAsync(mu, s->mu, sizeof(float) * n_seq * s->Z, hipMemcpyDeviceToDevice, st));
    if (logvar) RTX_HIP(hipMemcpyAsync(logvar, s->lv, sizeof(float) * n_seq * s->Z, hipMemcpyDeviceToDevice, st));
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// ---- a loss computed outside the engine (rtx_engine_forward_train / rtx_engine_backward for the sequence model): the fused step cut
//      behind its forward, and entered again at its backward chain from the caller's gradient
static int sv_check_seqs(const char* who, const int32_t* seq_ptr, int n_seq, int T)
{
    RTX_CHECK(seq_ptr ? (n_seq >= 1 && n_seq <= T) : n_seq == 1, RTX_EINVAL, "%s: %d sequences over %d steps (seq_ptr %s)", who, n_seq, T,
              seq_ptr ? "given" : "NULL = one sequence");
    return RTX_OK;
}

int rtx_svae_forward_train(rtx_svae* s, const int32_t* items, int32_t total_steps, const int32_t* seq_ptr, int32_t n_seq, const float* eps_noise,
                           uint64_t seed, uint64_t offset, float* logits_out, float* mu, float* logvar, uint64_t* ticket, void* stream)
{
    RTX_TRY(sv_check(s, items, total_steps, true));
    RTX_CHECK(logits_out && ticket, RTX_EINVAL, "svae_forward_train: NULL argument");
    *ticket = 0;
    RTX_TRY(sv_check_seqs("svae_forward_train", seq_ptr, n_seq, total_steps));
    hipStream_t st = (hipStream_t)stream;
    // the last decoder layer is linear and nothing behind it reads its output: the logits go straight into the caller's tensor
    RTX_TRY(sv_forward(s, items, total_steps, seq_ptr, n_seq, eps_noise, seed, offset, logits_out, st));
    if (mu) RTX_HIP(hipMemcpyAsync(mu, s->mu, sizeof(float) * total_steps * s->Z, hipMemcpyDeviceToDevice, st));
    if (logvar) RTX_HIP(hipMemcpyAsync(logvar, s->lv, sizeof(float) * total_steps * s->Z, hipMemcpyDeviceToDevice, st));
    s->act_T = total_steps;
    s->act_nseq = n_seq;
    *ticket = s->act_ticket;
    return RTX_OK;
}

int rtx_svae_backward(rtx_svae* s, const int32_t* items, int32_t total_steps, const int32_t* seq_ptr, int32_t n_seq, uint64_t ticket,
                      const float* d_logits, int64_t ld, const float* d_mu, const float* d_logvar, void* stream)
{
    RTX_TRY(sv_check(s, items, total_steps, true));
    RTX_TRY(sv_check_seqs("svae_backward", seq_ptr, n_seq, total_steps));
    RTX_CHECK(!d_logits || ld >= s->I, RTX_EINVAL, "svae_backward: row stride %lld of d_logits is below n_items = %d", (long long)ld, s->I);
    // on the host, before anything is enqueued: do the activations in the handle still belong to the caller's forward?
    RTX_CHECK(ticket != 0 && ticket == s->act_ticket && s->act_T == total_steps && s->act_nseq == n_seq, RTX_ESTATE,
              "svae_backward: stale ticket %llu: the activations of that forward were overwritten by a later forward, prediction or training "
              "step of this handle (it now holds ticket %llu, %d steps in %d sequences); run rtx_svae_forward_train again",
              (unsigned long long)ticket, (unsigned long long)s->act_ticket, s->act_T, s->act_nseq);
    hipStream_t st = (hipStream_t)stream;
    const float* d_last = d_logits;   // a contiguous gradient is the last layer's D where it lies
    if (d_logits && ld != s->I) {
        float* D = s->L[s->NL - 1].D;
        hipLaunchKernelGGL(k_sv_import_rows, dim3((unsigned)(((long)total_steps * s->I + 255) / 256)), dim3(256), 0, st, d_logits, (long)ld,
                           total_steps, s->I, D);
        d_last = D;
    }
    RTX_TRY(sv_backward_mlp(s, total_steps, SvBwdStart{d_last, true, 0.f, nullptr, d_mu, d_logvar}, st));
    return sv_backward_rnn(s, items, total_steps, seq_ptr, n_seq, st);
}

int rtx_svae_apply_adam(rtx_svae* s, const rtx_step* step, void* stream)
{
    RTX_CHECK(s, RTX_EINVAL, "svae: NULL handle");
    RTX_CHECK(s->bound && s->can_train, RTX_ESTATE, "svae_apply_adam: gradient / Adam buffers are not bound");
    RTX_CHECK(step && step->step >= 1, RTX_EINVAL, "svae_apply_adam: step count must be >= 1");
    return sv_adam(s, step, (hipStream_t)stream);
}

}  // extern "C"
