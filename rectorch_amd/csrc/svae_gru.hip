// svae_gru.hip -- the GRU recurrences of the Sequential VAE (svae.hip): forward and back-propagation through time, one persistent
// workgroup per sequence.  The recurrence is a chain of T dependent mat-vecs against W_hh, so what matters is the latency of ONE
// time step.  Per direction there is a generic kernel that streams W_hh from L2 every step (any R <= 1024) and kernels that keep ALL
// of W_hh resident in the compute unit -- part of a thread's weights in its registers for the whole sequence, the rest in LDS -- so
// that a time step reads nothing from outside the CU but its own saved / projected values, requested one step ahead:
//   forward   k_sv_gru_fwd_rows  whole rows on 512 threads                R <= 128 (up to 200 with the K-sliced kernel off)
//             k_sv_gru_fwd_ks    the mat-vec split over K inside the wave  129 <= R <= 200
//             k_sv_gru_fwd       generic                                   the rest
//   backward  k_sv_gru_bwd_ks    the K-sliced layout transposed            129 <= R <= 200
//             k_sv_gru_bwd_all   (row chunk, column) on 1024 threads       wherever its LDS fits (R <= 204)
//             k_sv_gru_bwd       generic                                   the rest
// sv_gru_plan picks the pair once per handle; sv_gru_forward / sv_gru_backward launch it.  The input projections x_t W_ih^T for all t
// are one GEMM before the loop and the weight gradients two GEMMs over all t after it (svae.hip).  Measurements and the forms that
// were tried and dropped (among them round 2's 1024-thread forward, 3.6 us per step): profiles/HISTORY.md section 10.
#include "svae_internal.h"

#include <stdlib.h>
#include <algorithm>

#define SV_GRU_KRB 88  // weights of a row chunk the backward recurrence keeps in registers

// out[c][r] = in[r][c]  (W_hh -> W_hh^T once per sequence for the forward recurrence)
__global__ __launch_bounds__(256) void k_sv_transpose(const float* __restrict__ in, int rows, int cols, float* __restrict__ out)
{
    __shared__ float tile[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tid = threadIdx.x;
    for (int e = tid; e < 4096; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        tile[rr][cc] = (r0 + rr < rows && c0 + cc < cols) ? in[(size_t)(r0 + rr) * cols + c0 + cc] : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < 4096; e += 256) {
        const int cc = e >> 6, rr = e & 63;
        if (r0 + rr < rows && c0 + cc < cols) out[(size_t)(c0 + cc) * rows + r0 + rr] = tile[rr][cc];
    }
}

__device__ __forceinline__ float sv_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
// the recurrence's gate phase is one dependent chain per thread (200 of the 512 threads, nothing to hide it behind): libm's expf /
// tanhf / IEEE division make it ~1 000 cycles per time step.  v_exp_f32 / v_rcp_f32 (1 ulp each; the argument's scaling by log2 e
// adds |x| * 6e-8 relative) keep sigmoid within 3e-7 and tanh within 6e-7 absolute of libm's.
__device__ __forceinline__ float sv_sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
__device__ __forceinline__ float sv_tanh_fast(float x) { return 2.f * sv_sigmoid_fast(2.f * x) - 1.f; }
template <int CTRL> __device__ __forceinline__ float sv_dpp(float v)   // v of the lane DPP control CTRL points at (all rows, all banks)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// GRU forward, torch.nn.GRU gate order r | z | n (weight_hh_l0 [3R][R], bias_hh_l0 [3R]); GI = x W_ih^T + b_ih [T][3R].
//   r = sig(gi_r + W_hr h + b_hr), z = sig(gi_z + W_hz h + b_hz), n = tanh(gi_n + r * (W_hn h + b_hn)), h' = (1-z) n + z h
// One persistent workgroup of 1024 threads; the recurrence is a chain of T dependent mat-vecs, so what matters is the
// latency of ONE step.  Thread `row` streams its own row of W_hh (all loads independent: the only dependent chain is the
// FMA accumulation) against h broadcast from LDS -- no cross-lane reduction, one barrier per phase.  The weights are read
// from a transposed copy made once per sequence, so that a wave's load is 256 contiguous bytes.
// Measured per step at R = 200: 27 us with one wave per row + shuffle reduction (37 dependent L2 round trips), 8.7 us in
// this form.  Splitting the hidden units over 2 workgroups with W_hh resident in registers and an exchange of h through
// L2 per step was SLOWER (10.8 us): device-scope release/acquire between compute units costs microseconds on a
// multi-XCD part, more than re-reading 480 KB from L2.
__global__ __launch_bounds__(1024) void k_sv_gru_fwd(const float* __restrict__ GI, const float* __restrict__ WhhT, const float* __restrict__ bhh,
                                                     const int32_t* __restrict__ seq_ptr, int T_one, int R,
                                                     float* __restrict__ Hout /* [T][R]: h after step t */,
                                                     float* __restrict__ Hprev /* [T][R]: h before step t (0 at a sequence start) */,
                                                     float* __restrict__ Gr, float* __restrict__ Gz, float* __restrict__ Gn, float* __restrict__ Ghn)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];   // h [Rp] | gh [3R]   (Rp = R rounded up to 4)
    const int Rp = (R + 3) & ~3;
    float* h = sm;
    float* gh = sm + Rp;
    const int tid = threadIdx.x;
    // packed sequences: workgroup b owns rows [seq_ptr[b], seq_ptr[b + 1]) of every [T][.] buffer; one sequence: all T_one rows
    const int t0 = seq_ptr ? seq_ptr[blockIdx.x] : 0;
    const int T = seq_ptr ? seq_ptr[blockIdx.x + 1] - t0 : T_one;
    GI += (size_t)t0 * 3 * R;
    Hout += (size_t)t0 * R; Hprev += (size_t)t0 * R;
    Gr += (size_t)t0 * R; Gz += (size_t)t0 * R; Gn += (size_t)t0 * R; Ghn += (size_t)t0 * R;
    for (int j = tid; j < Rp; j += 1024) h[j] = 0.f;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        // this step's input projections are independent of h: fetch them before the mat-vec, not after its barrier
        const float* gi = GI + (size_t)t * 3 * R;
        float gir = 0.f, giz = 0.f, gin = 0.f;
        if (tid < R) { gir = gi[tid]; giz = gi[R + tid]; gin = gi[2 * R + tid]; }
        for (int row = tid; row < 3 * R; row += 1024) {
            // WhhT is [R][3R]: consecutive lanes (rows) read consecutive addresses -- 4 cache lines per wave load instead
            // of the 64 a row-major W_hh costs when every lane walks its own row
            const float* w = WhhT + row;
            const size_t ld = (size_t)3 * R;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            int k = 0;
            for (; k + 8 <= R; k += 8) {
                const float w0 = w[(k + 0) * ld], w1 = w[(k + 1) * ld], w2 = w[(k + 2) * ld], w3 = w[(k + 3) * ld];
                const float w4 = w[(k + 4) * ld], w5 = w[(k + 5) * ld], w6 = w[(k + 6) * ld], w7 = w[(k + 7) * ld];
                s0 += w0 * h[k] + w4 * h[k + 4];
                s1 += w1 * h[k + 1] + w5 * h[k + 5];
                s2 += w2 * h[k + 2] + w6 * h[k + 6];
                s3 += w3 * h[k + 3] + w7 * h[k + 7];
            }
            for (; k < R; ++k) s0 += w[k * ld] * h[k];
            gh[row] = (s0 + s1) + (s2 + s3) + bhh[row];
        }
        __syncthreads();
        for (int j = tid; j < R; j += 1024) {   // R <= 1024: one pass, j == tid
            const float r = sv_sigmoid(gir + gh[j]);
            const float z = sv_sigmoid(giz + gh[R + j]);
            const float hn = gh[2 * R + j];
            const float n = tanhf(gin + r * hn);
            const float hp = h[j];
            const float hv = (1.f - z) * n + z * hp;
            Gr[(size_t)t * R + j] = r; Gz[(size_t)t * R + j] = z; Gn[(size_t)t * R + j] = n; Ghn[(size_t)t * R + j] = hn;
            Hprev[(size_t)t * R + j] = hp;
            Hout[(size_t)t * R + j] = hv;
            h[j] = hv;   // element j is read and written by this thread only; the mat-vec above is behind the barrier
        }
        __syncthreads();
    }
}

// Round 3: the recurrence with ALL of W_hh resident in the compute unit, on 512 threads (8 waves, two per SIMD: 256 registers per
// lane).  The streaming kernel above re-reads W_hh (480 KB at R = 200) through one CU's 64-B/clk L1 path on every time step: 3.3 us
// of its 5.2 us.  Round 2's resident kernel (1024 threads, 80 weights of a half-row per thread; removed) had 128 registers to do it
// in: hipcc spilled ~17 of them and reloaded them every step (3.6 us per step).  Here a thread owns a WHOLE row of W_hh: its first
// KR = 160 weights in registers, the rest of the row
// in LDS ([chunk of 4 k][512][4]); rows beyond the 512th live in LDS entirely and are summed as two half-rows each by the first
// 2 NE threads (R = 200: 88 rows, 176 threads; as four quarter-rows on 352 threads the first waves' mat-vec is shorter but the
// others' longer -- the LDS pipe is shared -- and the step is 5 % slower).  512 x 160 registers + 82 KB + 70 KB of LDS hold the 120 000 weights of R = 200;
// the hidden state is read as broadcast float4s.  No spills (207 VGPRs), one mat-vec phase and one gate phase per step as before.
// Measured (tools/svae_stamps.py, shader clock): 6 300 cycles = 2.6 us per step -- mat-vec 4 700 (the LDS pipe: every thread
// reads all of h, 50 float4, plus its LDS-resident weights), barrier 180, gate phase 1 040, barrier + loop 340 -- against 3.6 us
// for the 1024-thread kernel: 806 -> 893 users/s with one user per optimizer step.  The first version of this kernel carried an
// `if (q < nq)` inside the unrolled loop and took 10 200 cycles: a guard per float4 makes every read its own basic block.
#define SV_GRU_KR2 160
__host__ __device__ inline void sv_gru_rows_shape(int R, int KR, int* NE, int* Kh, int* CA, int* CB, int* HS)
{
    const int R3 = 3 * R;
    *NE = R3 > 512 ? R3 - 512 : 0;
    *Kh = (((R + 1) / 2) + 3) & ~3;                  // extra rows: first half k < Kh, second half the rest
    *CA = R > KR ? (R - KR + 3) / 4 : 0;
    *CB = (*Kh + 3) / 4;
    const int reach_own = KR + 4 * *CA, reach_x = *Kh + 4 * *CB;   // the register-resident prefix is summed unconditionally (zero weights past R)
    const int reach = reach_own > reach_x ? reach_own : reach_x;
    *HS = ((reach > R ? reach : R) + 7) & ~3;
}
__host__ __device__ inline size_t sv_gru_rows_lds(int R, int KR)
{
    int NE, Kh, CA, CB, HS;
    sv_gru_rows_shape(R, KR, &NE, &Kh, &CA, &CB, &HS);
    return sizeof(float) * ((size_t)HS + ((3 * R + 3) & ~3) + ((2 * NE + 3) & ~3) + (size_t)CA * 512 * 4 + (size_t)CB * 2 * NE * 4);
}

__device__ unsigned long long* g_sv_stamps = nullptr;   // measurement: shader-clock stamps of the first steps of the forward recurrence
template <int KR>
__global__ __launch_bounds__(512) void k_sv_gru_fwd_rows(const float* __restrict__ GI, const float* __restrict__ Whh, const float* __restrict__ bhh,
                                                         const int32_t* __restrict__ seq_ptr, int T_one, int R, float* __restrict__ Hout,
                                                         float* __restrict__ Hprev, float* __restrict__ Gr, float* __restrict__ Gz,
                                                         float* __restrict__ Gn, float* __restrict__ Ghn)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];   // h [HS] | gp [3R] | gx [2 NE] | wlA [CA][512][4] | wlB [CB][2 NE][4]
    int NE, Kh, CA, CB, HS;
    sv_gru_rows_shape(R, KR, &NE, &Kh, &CA, &CB, &HS);
    const int R3 = 3 * R, NX = 2 * NE;
    float* h = sm;
    float* gp = sm + HS;
    float* gx = gp + ((R3 + 3) & ~3);
    float* wlA = gx + ((NX + 3) & ~3);
    float* wlB = wlA + (size_t)CA * 512 * 4;
    const int tid = threadIdx.x;
    const int t0 = seq_ptr ? seq_ptr[blockIdx.x] : 0;
    const int T = seq_ptr ? seq_ptr[blockIdx.x + 1] - t0 : T_one;
    GI += (size_t)t0 * R3;
    Hout += (size_t)t0 * R; Hprev += (size_t)t0 * R;
    Gr += (size_t)t0 * R; Gz += (size_t)t0 * R; Gn += (size_t)t0 * R; Ghn += (size_t)t0 * R;
    const bool own = tid < R3;                     // (R3 < 512: the upper threads idle through the mat-vec)
    const int row = own ? tid : 0;
    const int last = R3 * R - 1;
    float wr[KR];
    {
        const int base = row * R;
#pragma unroll
        for (int q = 0; q < KR; ++q) {
            const float v = Whh[min(base + q, last)];
            wr[q] = (own && q < R) ? v : 0.f;
        }
        for (int q = 0; q < CA * 4; ++q) {
            const float v = Whh[min(base + KR + q, last)];
            wlA[((size_t)(q >> 2) * 512 + tid) * 4 + (q & 3)] = (own && KR + q < R) ? v : 0.f;
        }
    }
    const bool extra = tid < NX;
    const int xrow = extra ? 512 + (tid >> 1) : 0, xk0 = (tid & 1) ? Kh : 0, xlen = extra ? ((tid & 1) ? R - Kh : Kh) : 0;
    if (extra)
        for (int q = 0; q < CB * 4; ++q) {
            const float v = Whh[min(xrow * R + xk0 + q, last)];
            wlB[((size_t)(q >> 2) * NX + tid) * 4 + (q & 3)] = q < xlen ? v : 0.f;
        }
    for (int j = tid; j < HS; j += 512) h[j] = 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const float4* hv = (const float4*)h;
    const float4* hvx = (const float4*)(h + xk0);
    constexpr int NQ = KR / 4;
    float gir = 0.f, giz = 0.f, gin = 0.f;
    if (tid < R && T > 0) { gir = GI[tid]; giz = GI[R + tid]; gin = GI[2 * R + tid]; }
    unsigned long long* stamps = (tid == 0 && blockIdx.x == 0) ? g_sv_stamps : nullptr;
    for (int t = 0; t < T; ++t) {
        if (stamps && t >= 8 && t < 12) stamps[(t - 8) * 4 + 0] = __builtin_readcyclecounter();
        float nir = 0.f, niz = 0.f, nin = 0.f;
        if (tid < R && t + 1 < T) {
            const float* gi = GI + (size_t)(t + 1) * R3;
            nir = gi[tid]; niz = gi[R + tid]; nin = gi[2 * R + tid];
        }
        {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            // no condition inside the unrolled loop: a (uniform) guard per float4 turned every read into its own basic block with its
            // own s_waitcnt -- 8 200 cycles for this phase instead of ~2 000 (tools/svae_stamps.py)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float4 x = hv[q];
                s0 += wr[4 * q] * x.x; s1 += wr[4 * q + 1] * x.y; s2 += wr[4 * q + 2] * x.z; s3 += wr[4 * q + 3] * x.w;
            }
#pragma unroll 5
            for (int c = 0; c < CA; ++c) {
                const float4 w = *(const float4*)(wlA + ((size_t)c * 512 + tid) * 4);
                const float4 x = hv[NQ + c];
                s0 += w.x * x.x; s1 += w.y * x.y; s2 += w.z * x.z; s3 += w.w * x.w;
            }
            if (own) gp[tid] = (s0 + s1) + (s2 + s3);
            if (extra) {
                float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
#pragma unroll 5
                for (int c = 0; c < CB; ++c) {
                    const float4 w = *(const float4*)(wlB + ((size_t)c * NX + tid) * 4);
                    const float4 x = hvx[c];
                    e0 += w.x * x.x; e1 += w.y * x.y; e2 += w.z * x.z; e3 += w.w * x.w;
                }
                gx[tid] = (e0 + e1) + (e2 + e3);
            }
        }
        if (stamps && t >= 8 && t < 12) stamps[(t - 8) * 4 + 1] = __builtin_readcyclecounter();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (stamps && t >= 8 && t < 12) stamps[(t - 8) * 4 + 2] = __builtin_readcyclecounter();
        if (tid < R) {
            const int j = tid;
            auto G = [&](int i) { return (i < 512 ? gp[i] : gx[2 * (i - 512)] + gx[2 * (i - 512) + 1]) + bhh[i]; };
            const float ghr = G(j), ghz = G(R + j), hn = G(2 * R + j);
            const float r = sv_sigmoid(gir + ghr);
            const float z = sv_sigmoid(giz + ghz);
            const float n = tanhf(gin + r * hn);
            const float hp = h[j];
            const float hvv = (1.f - z) * n + z * hp;
            Gr[(size_t)t * R + j] = r; Gz[(size_t)t * R + j] = z; Gn[(size_t)t * R + j] = n; Ghn[(size_t)t * R + j] = hn;
            Hprev[(size_t)t * R + j] = hp;
            Hout[(size_t)t * R + j] = hvv;
            h[j] = hvv;
        }
        if (stamps && t >= 8 && t < 12) stamps[(t - 8) * 4 + 3] = __builtin_readcyclecounter();
        gir = nir; giz = niz; gin = nin;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
}

// Round 3, second form: the mat-vec split over K inside the wave.  The whole-row kernel above is bound by the LDS pipe: every
// thread reads ALL of h (50 broadcast float4) plus its LDS-resident weights, ~520 LDS wave-instructions per step = the 4 700
// cycles of its mat-vec phase.  Here lane = (row group g = lane >> 3, K slice s = lane & 7): a thread owns NR rows (g + 64 i of
// the wave's... 64 row slots x NR covers 3R) times ONE slice of SL = R / 8 columns, so it reads only its slice of h (7 float4,
// all requested up front) and keeps the same ~250 weights (KG in registers, the rest in LDS as before).  The 8 slices of a row
// meet through three DPP adds per accumulator (quad_perm xor 1, xor 2, row_half_mirror: no LDS), then the 8 lanes of a group
// write one or two of the NR sums each.  ~180 LDS wave-instructions per step instead of ~520; the VALU work grows from 200 to
// ~280 operations per thread (the DPP reduction).  h lives slice-major ([8][SLP]) so a slice is 16-byte aligned.
template <int SL, int NR, int KG>
__global__ __launch_bounds__(512) void k_sv_gru_fwd_ks(const float* __restrict__ GI, const float* __restrict__ Whh, const float* __restrict__ bhh,
                                                       const int32_t* __restrict__ seq_ptr, int T_one, int R, float* __restrict__ Hout,
                                                       float* __restrict__ Hprev, float* __restrict__ Gr, float* __restrict__ Gz,
                                                       float* __restrict__ Gn, float* __restrict__ Ghn)
{
    constexpr int SLP = (SL + 3) & ~3, NQ = SLP / 4, NWT = NR * SL, CL = (NWT - KG + 3) / 4, GPN = 64 * NR;
    static_assert(KG % 4 == 0 && KG <= NWT, "register-resident weights: whole float4 groups");
    extern __shared__ __attribute__((aligned(16))) float sm[];   // h2 [8][SLP] | gp [64 NR] | wl [CL][512][4]
    float* h2 = sm;
    float* gp = sm + 8 * SLP;
    float* wl = gp + GPN;
    const int R3 = 3 * R;
    const int tid = threadIdx.x, lane = tid & 63, s = lane & 7, slot = (tid >> 6) * 8 + (lane >> 3);
    const int t0 = seq_ptr ? seq_ptr[blockIdx.x] : 0;
    const int T = seq_ptr ? seq_ptr[blockIdx.x + 1] - t0 : T_one;
    GI += (size_t)t0 * R3;
    Hout += (size_t)t0 * R; Hprev += (size_t)t0 * R;
    Gr += (size_t)t0 * R; Gz += (size_t)t0 * R; Gn += (size_t)t0 * R; Ghn += (size_t)t0 * R;
    // weight q = i * SL + kk of this thread is W_hh[slot + 64 i][s * SL + kk] (zero outside the matrix)
    const int last = R3 * R - 1;
    auto wload = [&](int q) {
        const int i = q / SL, kk = q % SL, row = slot + 64 * i, k = s * SL + kk;
        // every load unconditional (clamped address), the mask a factor: a select lets hipcc sink the load into a branch of its own,
        // and 250 such branches serialise the kernel's start
        const float v = Whh[min(row * R + k, last)];
        return v * ((row < R3 && k < R && q < NWT) ? 1.f : 0.f);
    };
    float wr[KG];
#pragma unroll
    for (int q = 0; q < KG; ++q) wr[q] = wload(q);
#pragma unroll 8
    for (int q = 0; q < CL * 4; ++q) wl[((size_t)(q >> 2) * 512 + tid) * 4 + (q & 3)] = wload(KG + q);
    for (int j = tid; j < 8 * SLP; j += 512) h2[j] = 0.f;
    for (int j = tid; j < GPN; j += 512) gp[j] = 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const float4* hs = (const float4*)(h2 + s * SLP);
    const int hj = (tid / SL) * SLP + (tid % SL);      // where h[tid] lives (gate-phase threads: tid < R)
    float gir = 0.f, giz = 0.f, gin = 0.f;
    if (tid < R && T > 0) { gir = GI[tid]; giz = GI[R + tid]; gin = GI[2 * R + tid]; }
    // the hidden-side biases of this thread's three gates, once (read inside the loop they are three global loads and a vmcnt(0)
    // -- an L2 round trip -- in every step's gate phase)
    const int bj = min(tid, R - 1);
    const float bh_r = bhh[bj], bh_z = bhh[R + bj], bh_n = bhh[2 * R + bj];
    unsigned long long* stamps = (tid == 0 && blockIdx.x == 0) ? g_sv_stamps : nullptr;
    for (int t = 0; t < T; ++t) {
        if (stamps && t >= 8 && t < 12) stamps[(t - 8) * 4 + 0] = __builtin_readcyclecounter();
        float nir = 0.f, niz = 0.f, nin = 0.f;
        if (tid < R && t + 1 < T) {
            const unsigned o = (unsigned)(t + 1) * (unsigned)R3 + (unsigned)tid;
            nir = GI[o]; niz = GI[o + (unsigned)R]; nin = GI[o + 2u * (unsigned)R];
        }
        {
            float4 hq[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) hq[q] = hs[q];
            float acc[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i) acc[i] = 0.f;
            auto hval = [&](int kk) { const float4 v = hq[kk >> 2]; return (kk & 3) == 0 ? v.x : (kk & 3) == 1 ? v.y : (kk & 3) == 2 ? v.z : v.w; };
#pragma unroll
            for (int q = 0; q < KG; ++q) acc[q / SL] += wr[q] * hval(q % SL);
#pragma unroll
            for (int c = 0; c < CL; ++c) {
                const float4 w = *(const float4*)(wl + ((size_t)c * 512 + tid) * 4);
                const float we[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = KG + 4 * c + e;
                    if (q < NWT) acc[q / SL] += we[e] * hval(q % SL);
                }
            }
            // the 8 K slices of a row sit in 8 neighbouring lanes
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                acc[i] += sv_dpp<0xB1>(acc[i]);    // quad_perm [1,0,3,2]
                acc[i] += sv_dpp<0x4E>(acc[i]);    // quad_perm [2,3,0,1]
                acc[i] += sv_dpp<0x141>(acc[i]);   // row_half_mirror: the other quad of the 8
            }
            // lane s of the group writes sums s and s + 8
            float v0 = acc[0], v1 = acc[NR > 8 ? 8 : 0];
#pragma unroll
            for (int i = 1; i < 8 && i < NR; ++i) v0 = (s == i) ? acc[i] : v0;
#pragma unroll
            for (int i = 9; i < NR; ++i) v1 = (s == i - 8) ? acc[i] : v1;
            if (s < NR) gp[slot + 64 * s] = v0;
            if (s + 8 < NR) gp[slot + 64 * (s + 8)] = v1;
        }
        if (stamps && t >= 8 && t < 12) stamps[(t - 8) * 4 + 1] = __builtin_readcyclecounter();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (stamps && t >= 8 && t < 12) stamps[(t - 8) * 4 + 2] = __builtin_readcyclecounter();
        if (tid < R) {
            const int j = tid;
            const float ghr = gp[j] + bh_r, ghz = gp[R + j] + bh_z, hn = gp[2 * R + j] + bh_n;
            const float r = sv_sigmoid_fast(gir + ghr);
            const float z = sv_sigmoid_fast(giz + ghz);
            const float n = sv_tanh_fast(gin + r * hn);
            const float hp = h2[hj];
            const float hvv = (1.f - z) * n + z * hp;
            const unsigned o = (unsigned)t * (unsigned)R + (unsigned)j;   // 32-bit offsets: scalar base + one VGPR per store
            Gr[o] = r; Gz[o] = z; Gn[o] = n; Ghn[o] = hn;
            Hprev[o] = hp;
            Hout[o] = hvv;
            h2[hj] = hvv;
        }
        if (stamps && t >= 8 && t < 12) stamps[(t - 8) * 4 + 3] = __builtin_readcyclecounter();
        gir = nir; giz = niz; gin = nin;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
}
#define SV_KS_SL 25
#define SV_KS_NR 10
#define SV_KS_KG 180
static size_t sv_gru_ks_lds() { return sizeof(float) * (8 * ((SV_KS_SL + 3) & ~3) + 64 * SV_KS_NR + (size_t)((SV_KS_NR * SV_KS_SL - SV_KS_KG + 3) / 4) * 512 * 4); }

// Backward recurrence in the K-sliced layout of k_sv_gru_fwd_ks (same thread -> weights map: rows slot + 64 i, columns of slice s):
// dh_{t-1}[k] += sum_i W_hh[i][k] dgh[i] -- a thread multiplies its 10 x 25 weights with its 10 values of dgh (LDS, slot-major: three
// float4) into 25 column sums, the 8 row groups of the wave meet by a reduce-scatter over lanes (permlane32_swap, permlane16_swap,
// row_ror:8 -- two values per instruction, ~50 operations for the 25 sums; lane group g ends with columns 8 m + bitrev3(g)), the 8
// waves through part [8][R] in LDS.  Two barriers per step (k_sv_gru_bwd_all: three), ~240 LDS wave-instructions (~650).
__device__ __forceinline__ void sv_permlane32_swap(float& x, float& y)   // rows 2,3 of x <-> rows 0,1 of y
{
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
}
__device__ __forceinline__ void sv_permlane16_swap(float& x, float& y)   // odd rows of x <-> even rows of y
{
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
}
template <int SL, int NR, int KG>
__global__ __launch_bounds__(512) void k_sv_gru_bwd_ks(const float* __restrict__ dHout, const float* __restrict__ Whh, const int32_t* __restrict__ seq_ptr,
                                                       int T_one, int R, const float* __restrict__ Hprev, const float* __restrict__ Gr,
                                                       const float* __restrict__ Gz, const float* __restrict__ Gn, const float* __restrict__ Ghn,
                                                       float* __restrict__ dGI, float* __restrict__ dGH)
{
    constexpr int GS = (NR + 3) & ~3, NWT = NR * SL, CL = (NWT - KG + 3) / 4, PS = 8 * SL;
    constexpr int N32 = (SL + 1) / 2, N16 = (N32 + 1) / 2, N8 = (N16 + 1) / 2;
    static_assert(KG % 4 == 0 && KG <= NWT, "register-resident weights: whole float4 groups");
    extern __shared__ __attribute__((aligned(16))) float sm[];   // dg2 [64][GS] | part [8][PS] | wl [CL][512][4]
    float* dg2 = sm;
    float* part = sm + 64 * GS;
    float* wl = part + 8 * PS;
    const int R3 = 3 * R;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, s = lane & 7, slot = wv * 8 + (lane >> 3);
    const int t0 = seq_ptr ? seq_ptr[blockIdx.x] : 0;
    const int T = seq_ptr ? seq_ptr[blockIdx.x + 1] - t0 : T_one;
    dHout += (size_t)t0 * R; Hprev += (size_t)t0 * R;
    Gr += (size_t)t0 * R; Gz += (size_t)t0 * R; Gn += (size_t)t0 * R; Ghn += (size_t)t0 * R;
    dGI += (size_t)t0 * R3; dGH += (size_t)t0 * R3;
    const int last = R3 * R - 1;
    auto wload = [&](int q) {
        const int i = q / SL, kk = q % SL, row = slot + 64 * i, k = s * SL + kk;
        const float v = Whh[min(row * R + k, last)];
        return v * ((row < R3 && k < R && q < NWT) ? 1.f : 0.f);
    };
    float wr[KG];
#pragma unroll
    for (int q = 0; q < KG; ++q) wr[q] = wload(q);
#pragma unroll 8
    for (int q = 0; q < CL * 4; ++q) wl[((size_t)(q >> 2) * 512 + tid) * 4 + (q & 3)] = wload(KG + q);
    for (int j = tid; j < 64 * GS + 8 * PS; j += 512) sm[j] = 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // gate threads: column gj = tid for tid < R; the threads beyond shadow column R - 1 (same loads, same arithmetic, same stores to
    // the same places) so that the step has NO divergent block around its global loads and stores: behind an `if (tid < R)` hipcc
    // cannot count the outstanding stores on both paths and waits vmcnt(0) -- a store round trip per time step
    const int gj = min(tid, R - 1);
    // where this gate thread's three rows of dgh live: row i -> [(i & 63)][i >> 6]
    const int p0 = (gj & 63) * GS + (gj >> 6), p1 = ((R + gj) & 63) * GS + ((R + gj) >> 6), p2 = ((2 * R + gj) & 63) * GS + ((2 * R + gj) >> 6);
    const bool b3 = (lane & 8) != 0;
    const int rev = ((lane >> 5) & 1) | (((lane >> 4) & 1) << 1) | (((lane >> 3) & 1) << 2);   // 4 b3 + 2 b4 + b5
    float dh = 0.f;
    float vd = 0.f, vr = 0.f, vz = 0.f, vn = 0.f, vhn = 0.f, vhp = 0.f;
    if (T > 0) {
        const size_t o = (size_t)(T - 1) * R + gj;
        vd = dHout[o]; vr = Gr[o]; vz = Gz[o]; vn = Gn[o]; vhn = Ghn[o]; vhp = Hprev[o];
    }
    const float4* gv = (const float4*)(dg2 + slot * GS);
    unsigned long long* stamps = (tid == 0 && blockIdx.x == 0 && g_sv_stamps) ? g_sv_stamps + 16 : nullptr;   // entries 16..31: this kernel
    for (int t = T - 1; t >= 0; --t) {
        const bool stamp = stamps && t >= T - 12 && t < T - 8;
        if (stamp) stamps[(T - 9 - t) * 4 + 0] = __builtin_readcyclecounter();
        {
            const int j = gj;
            const float d = dh + vd;
            const float dn = d * (1.f - vz);
            const float dzp = d * (vhp - vn) * vz * (1.f - vz);
            const float dnp = dn * (1.f - vn * vn);
            const float drp = dnp * vhn * vr * (1.f - vr);
            const unsigned o = (unsigned)t * (unsigned)R3 + (unsigned)j, oz = o + (unsigned)R, on = o + 2u * (unsigned)R;
            dGI[o] = drp; dGI[oz] = dzp; dGI[on] = dnp;
            dGH[o] = drp; dGH[oz] = dzp; dGH[on] = dnp * vr;
            dg2[p0] = drp; dg2[p1] = dzp; dg2[p2] = dnp * vr;
            dh = d * vz;   // the direct path h_{t-1} -> h_t; the path through the gates is added below
        }
        // the saved gate values of step t - 1, requested BEHIND this step's use of its own (and unconditionally, clamped): requested
        // in front of it, under a condition, hipcc waits vmcnt(0) before the gate arithmetic -- for the loads it has just issued,
        // a full L2 round trip per time step (1 200 cycles in this phase instead of ~300)
        float nd, nr, nz, nn, nhn, nhp;
        {
            const unsigned o = (unsigned)max(t - 1, 0) * (unsigned)R + (unsigned)gj;   // 32-bit offsets: scalar base + one VGPR
            nd = dHout[o]; nr = Gr[o]; nz = Gz[o]; nn = Gn[o]; nhn = Ghn[o]; nhp = Hprev[o];
        }
        if (stamp) stamps[(T - 9 - t) * 4 + 1] = __builtin_readcyclecounter();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (stamp) stamps[(T - 9 - t) * 4 + 2] = __builtin_readcyclecounter();
        {
            float4 gq[GS / 4];
#pragma unroll
            for (int q = 0; q < GS / 4; ++q) gq[q] = gv[q];
            auto gval = [&](int i) { const float4 v = gq[i >> 2]; return (i & 3) == 0 ? v.x : (i & 3) == 1 ? v.y : (i & 3) == 2 ? v.z : v.w; };
            float acc[SL];
#pragma unroll
            for (int kk = 0; kk < SL; ++kk) acc[kk] = 0.f;
#pragma unroll
            for (int q = 0; q < KG; ++q) acc[q % SL] += wr[q] * gval(q / SL);
#pragma unroll
            for (int c = 0; c < CL; ++c) {
                const float4 w = *(const float4*)(wl + ((size_t)c * 512 + tid) * 4);
                const float we[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = KG + 4 * c + e;
                    if (q < NWT) acc[q % SL] += we[e] * gval(q / SL);
                }
            }
            // reduce-scatter over the 8 row groups of the wave (lane bits 5, 4, 3)
            float u[N32];
#pragma unroll
            for (int p = 0; p < N32; ++p) {
                float x = acc[2 * p], y = acc[2 * p + 1 < SL ? 2 * p + 1 : 2 * p];
                sv_permlane32_swap(x, y);
                u[p] = x + y;          // lanes 0-31: column 2p summed over bit 5, lanes 32-63: column 2p + 1
            }
            float v[N16];
#pragma unroll
            for (int n = 0; n < N16; ++n) {
                float x = u[2 * n], y = u[2 * n + 1 < N32 ? 2 * n + 1 : 2 * n];
                sv_permlane16_swap(x, y);
                v[n] = x + y;          // even rows: u[2n] summed over bit 4, odd rows: u[2n + 1]
            }
#pragma unroll
            for (int m = 0; m < N8; ++m) {
                const float pz = v[2 * m], qz = v[2 * m + 1 < N16 ? 2 * m + 1 : 2 * m];
                const float keep = b3 ? qz : pz, send = b3 ? pz : qz;
                const float f = keep + sv_dpp<0x128>(send);   // row_ror:8
                const int idx = 8 * m + rev;
                if (idx < SL) part[wv * PS + s * SL + idx] = f;
            }
        }
        if (stamp) stamps[(T - 9 - t) * 4 + 3] = __builtin_readcyclecounter();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) a += part[w * PS + gj];
            dh += a;
        }
        asm volatile("" : "+v"(nd), "+v"(nr), "+v"(nz), "+v"(nn), "+v"(nhn), "+v"(nhp));   // they landed a mat-vec ago: the wait belongs HERE
        vd = nd; vr = nr; vz = nz; vn = nn; vhn = nhn; vhp = nhp;
    }
}

extern "C" void rtxdbg_svae_set_stamps(unsigned long long* dev)   // measurement hook (tools/svae_stamps.py): 32 device entries (forward 0..15, backward 16..31); not part of the ABI
{
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sv_stamps), &dev, sizeof(dev));
}

// GRU backward through time.  dHout[t] = gradient w.r.t. the GRU output at step t.  Writes the gate pre-activation
// gradients dGI [T][3R] (input side) and dGH [T][3R] (hidden side; differs in the n block by the factor r).
// dh_{t-1} += W_hh^T dgh: thread (column k, row chunk c) sums W_hh[i][k] dgh[i] over its chunk of rows -- consecutive
// lanes read consecutive k (coalesced rows), every load is independent -- and the chunks meet in LDS (5.5 us per step).
__global__ __launch_bounds__(1024) void k_sv_gru_bwd(const float* __restrict__ dHout, const float* __restrict__ Whh,
                                                     const int32_t* __restrict__ seq_ptr, int T_one, int R,
                                                     const float* __restrict__ Hprev, const float* __restrict__ Gr, const float* __restrict__ Gz,
                                                     const float* __restrict__ Gn, const float* __restrict__ Ghn, float* __restrict__ dGI,
                                                     float* __restrict__ dGH)
{
    const int t0 = seq_ptr ? seq_ptr[blockIdx.x] : 0;
    const int T = seq_ptr ? seq_ptr[blockIdx.x + 1] - t0 : T_one;
    dHout += (size_t)t0 * R; Hprev += (size_t)t0 * R;
    Gr += (size_t)t0 * R; Gz += (size_t)t0 * R; Gn += (size_t)t0 * R; Ghn += (size_t)t0 * R;
    dGI += (size_t)t0 * 3 * R; dGH += (size_t)t0 * 3 * R;
    extern __shared__ __attribute__((aligned(16))) float sm[];   // dh [R] | dgh [3R] | part [NC][R]
    float* dh = sm;
    float* dgh = sm + R;
    float* part = sm + 4 * R;
    const int tid = threadIdx.x;
    const int NC = max(1, min(16, 1024 / R));     // row chunks: as many as the workgroup has threads for
    const int rows_per = (3 * R + NC - 1) / NC;
    for (int j = tid; j < R; j += 1024) dh[j] = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        for (int j = tid; j < R; j += 1024) {
            const float d = dh[j] + dHout[(size_t)t * R + j];
            const float r = Gr[(size_t)t * R + j], z = Gz[(size_t)t * R + j], n = Gn[(size_t)t * R + j], hn = Ghn[(size_t)t * R + j];
            const float hp = Hprev[(size_t)t * R + j];
            const float dn = d * (1.f - z);
            const float dzp = d * (hp - n) * z * (1.f - z);
            const float dnp = dn * (1.f - n * n);
            const float drp = dnp * hn * r * (1.f - r);
            float* gi = dGI + (size_t)t * 3 * R;
            float* gh = dGH + (size_t)t * 3 * R;
            gi[j] = drp; gi[R + j] = dzp; gi[2 * R + j] = dnp;
            gh[j] = drp; gh[R + j] = dzp; gh[2 * R + j] = dnp * r;
            dgh[j] = drp; dgh[R + j] = dzp; dgh[2 * R + j] = dnp * r;
            dh[j] = d * z;   // the direct path h_{t-1} -> h_t; the path through the gates is added below
        }
        __syncthreads();
        for (int e = tid; e < NC * R; e += 1024) {
            const int c = e / R, k = e - c * R;
            const int i0 = c * rows_per, i1 = min(3 * R, i0 + rows_per);
            const float* w = Whh + (size_t)i0 * R + k;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            int i = i0;
            for (; i + 4 <= i1; i += 4) {
                a0 += w[0] * dgh[i];
                a1 += w[R] * dgh[i + 1];
                a2 += w[2 * (size_t)R] * dgh[i + 2];
                a3 += w[3 * (size_t)R] * dgh[i + 3];
                w += 4 * (size_t)R;
            }
            for (; i < i1; ++i) { a0 += w[0] * dgh[i]; w += R; }
            part[c * R + k] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
        for (int j = tid; j < R; j += 1024) {
            float s = dh[j];
            for (int c = 0; c < NC; ++c) s += part[c * R + j];
            dh[j] = s;
        }
        __syncthreads();
    }
}

// Backward recurrence with ALL of W_hh resident (as in k_sv_gru_fwd_rows): thread (row chunk c, column k) keeps the first KRB
// weights W[c * RP + i][k] of its chunk in registers and the rest in LDS ([chunk of 4 i][thread][4]); a time step reads from
// outside the CU only its six saved gate values, requested one step ahead.  Raw s_barriers behind LDS-only waits.
template <int KRB>
__global__ __launch_bounds__(1024) void k_sv_gru_bwd_all(const float* __restrict__ dHout, const float* __restrict__ Whh,
                                                         const int32_t* __restrict__ seq_ptr, int T_one, int R, int NC, int RP /* rows per chunk, % 4 == 0 */,
                                                         const float* __restrict__ Hprev, const float* __restrict__ Gr, const float* __restrict__ Gz,
                                                         const float* __restrict__ Gn, const float* __restrict__ Ghn, float* __restrict__ dGI,
                                                         float* __restrict__ dGH)
{
    const int t0 = seq_ptr ? seq_ptr[blockIdx.x] : 0;
    const int T = seq_ptr ? seq_ptr[blockIdx.x + 1] - t0 : T_one;
    const int R3 = 3 * R;
    dHout += (size_t)t0 * R; Hprev += (size_t)t0 * R;
    Gr += (size_t)t0 * R; Gz += (size_t)t0 * R; Gn += (size_t)t0 * R; Ghn += (size_t)t0 * R;
    dGI += (size_t)t0 * R3; dGH += (size_t)t0 * R3;
    extern __shared__ __attribute__((aligned(16))) float sm[];   // dh [Rp] | dgh [NC * RP + KRB + 4] | part [NC * R] | wl [CL][1024][4]
    const int Rp = (R + 3) & ~3;
    // dgh is read up to KRB + 4 CL floats past a chunk's start whatever R is (zero weights there, but zero times an uninitialised
    // LDS word may be NaN): its area covers every such read and is zeroed once
    const int DGS = NC * RP + KRB + 4;
    float* dh = sm;
    float* dgh = sm + Rp;
    float* part = dgh + DGS;
    float* wl = part + ((NC * R + 3) & ~3);
    const int tid = threadIdx.x;
    const bool own = tid < NC * R;
    const int c = own ? tid / R : 0, k = own ? tid - c * R : 0;
    const int i0 = c * RP;
    const int CL = RP > KRB ? (RP - KRB + 3) / 4 : 0;
    float wr[KRB];
    {
        const int last = R3 * R - 1;
#pragma unroll
        for (int i = 0; i < KRB; ++i) {
            const float v = Whh[min((i0 + i) * R + k, last)];
            wr[i] = (own && i < RP && i0 + i < R3) ? v : 0.f;
        }
        for (int i = 0; i < CL * 4; ++i) {
            const float v = Whh[min((i0 + KRB + i) * R + k, last)];
            wl[((size_t)(i >> 2) * 1024 + tid) * 4 + (i & 3)] = (own && KRB + i < RP && i0 + KRB + i < R3) ? v : 0.f;
        }
    }
    for (int j = tid; j < Rp; j += 1024) dh[j] = 0.f;
    for (int j = tid; j < DGS; j += 1024) dgh[j] = 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bool gate = tid < R;
    float vd = 0.f, vr = 0.f, vz = 0.f, vn = 0.f, vhn = 0.f, vhp = 0.f;
    if (gate && T > 0) {
        const size_t o = (size_t)(T - 1) * R + tid;
        vd = dHout[o]; vr = Gr[o]; vz = Gz[o]; vn = Gn[o]; vhn = Ghn[o]; vhp = Hprev[o];
    }
    const float4* dv = (const float4*)(dgh + i0);
    for (int t = T - 1; t >= 0; --t) {
        float nd = 0.f, nr = 0.f, nz = 0.f, nn = 0.f, nhn = 0.f, nhp = 0.f;
        if (gate && t > 0) {
            const size_t o = (size_t)(t - 1) * R + tid;
            nd = dHout[o]; nr = Gr[o]; nz = Gz[o]; nn = Gn[o]; nhn = Ghn[o]; nhp = Hprev[o];
        }
        if (gate) {
            const int j = tid;
            const float d = dh[j] + vd;
            const float dn = d * (1.f - vz);
            const float dzp = d * (vhp - vn) * vz * (1.f - vz);
            const float dnp = dn * (1.f - vn * vn);
            const float drp = dnp * vhn * vr * (1.f - vr);
            float* gi = dGI + (size_t)t * R3;
            float* gh = dGH + (size_t)t * R3;
            gi[j] = drp; gi[R + j] = dzp; gi[2 * R + j] = dnp;
            gh[j] = drp; gh[R + j] = dzp; gh[2 * R + j] = dnp * vr;
            dgh[j] = drp; dgh[R + j] = dzp; dgh[2 * R + j] = dnp * vr;
            dh[j] = d * vz;   // the direct path h_{t-1} -> h_t; the path through the gates is added below
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int i = 0; i < KRB; i += 4) {
                const float4 x = dv[i >> 2];
                a0 += wr[i] * x.x; a1 += wr[i + 1] * x.y; a2 += wr[i + 2] * x.z; a3 += wr[i + 3] * x.w;
            }
#pragma nounroll   // (unrolling by 4 / 2 spills 8 / 3 registers at the 128-VGPR cap of a 1024-thread workgroup: 896 -> 799 users/s)
            for (int q = 0; q < CL; ++q) {
                const float4 w = *(const float4*)(wl + ((size_t)q * 1024 + tid) * 4);
                const float4 x = dv[(KRB >> 2) + q];
                a0 += w.x * x.x; a1 += w.y * x.y; a2 += w.z * x.z; a3 += w.w * x.w;
            }
            if (own) part[tid] = (a0 + a1) + (a2 + a3);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (gate) {
            float sacc = dh[tid];
            for (int q = 0; q < NC; ++q) sacc += part[q * R + tid];
            dh[tid] = sacc;
        }
        vd = nd; vr = nr; vz = nz; vn = nn; vhn = nhn; vhp = nhp;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
}

// ------------------------------------------------------------------------------------------------ host side
// Dynamic LDS each weight-resident kernel needs at this R; 0 = R is outside the kernel's range or the need above the 160 KB of a CU
static size_t sv_lds_fits(size_t bytes) { return bytes <= 160 * 1024 ? bytes : 0; }
static size_t sv_gru_fwd_rows_need(size_t R)
{
    // rows beyond the 512th must find their two halves a thread each (2 NE <= 512)
    const size_t ne = 3 * R > 512 ? 3 * R - 512 : 0;
    if (3 * R > 1024 || R > SV_GRU_KR2 + 4 * 64 || 2 * ne > 512) return 0;
    return sv_lds_fits(sv_gru_rows_lds((int)R, SV_GRU_KR2));
}
static bool sv_gru_ks_range(size_t R) { return R > 128 && R <= 8 * SV_KS_SL && 3 * R <= 64 * SV_KS_NR; }   // (narrower GRUs: the whole-row form wastes less)
static size_t sv_gru_fwd_ks_need(size_t R) { return sv_gru_ks_range(R) ? sv_lds_fits(sv_gru_ks_lds()) : 0; }
static size_t sv_gru_bwd_ks_need(size_t R)
{
    // dg2 [64][GS] | part [8][8 SL] | wl [CL][512][4]
    const size_t lds = sizeof(float) * (64 * ((SV_KS_NR + 3) & ~3) + 8 * 8 * SV_KS_SL + (size_t)((SV_KS_NR * SV_KS_SL - SV_KS_KG + 3) / 4) * 512 * 4);
    return sv_gru_ks_range(R) ? sv_lds_fits(lds) : 0;
}
static size_t sv_gru_bwd_all_need(size_t R, int* nc, int* rp)
{
    // dh [Rp] | dgh [NC * RP + KRB + 4] | part [NC * R] | wl [CL][1024][4]
    const size_t NC = std::max<size_t>(1, std::min<size_t>(16, 1024 / R)), RP = (((3 * R + NC - 1) / NC) + 3) & ~(size_t)3;
    const size_t CL = RP > SV_GRU_KRB ? (RP - SV_GRU_KRB + 3) / 4 : 0;
    *nc = (int)NC;
    *rp = (int)RP;
    return sv_lds_fits(sizeof(float) * (((R + 3) & ~(size_t)3) + NC * RP + SV_GRU_KRB + 4 + ((NC * R + 3) & ~(size_t)3) + CL * 1024 * 4));
}

static bool sv_switched_off(const char* name)   // measurement switches, read when the handle is created
{
    const char* v = getenv(name);
    return v && v[0] == '0';
}
template <class K> static bool sv_reserve_lds(K kernel, size_t lds)
{
    return lds > 0 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

int sv_gru_plan(int R, SvGruPlan* p)
{
    *p = SvGruPlan();
    size_t lds;
    if (!sv_switched_off("RTX_SVAE_GRU_KS") && sv_reserve_lds(k_sv_gru_fwd_ks<SV_KS_SL, SV_KS_NR, SV_KS_KG>, lds = sv_gru_fwd_ks_need(R))) {
        p->fwd = SV_GRU_KS;
        p->fwd_lds = lds;
    } else if (!sv_switched_off("RTX_SVAE_GRU_ROWS") && sv_reserve_lds(k_sv_gru_fwd_rows<SV_GRU_KR2>, lds = sv_gru_fwd_rows_need(R))) {
        p->fwd = SV_GRU_ROWS;
        p->fwd_lds = lds;
    } else {
        p->fwd_lds = sizeof(float) * (4 * (size_t)R + 4);   // h [Rp] | gh [3R]: inside the 64 KB every kernel may have
    }
    int nc, rp;
    if (!sv_switched_off("RTX_SVAE_GRU_BWD_KS") && sv_reserve_lds(k_sv_gru_bwd_ks<SV_KS_SL, SV_KS_NR, SV_KS_KG>, lds = sv_gru_bwd_ks_need(R))) {
        p->bwd = SV_GRU_KS;
        p->bwd_lds = lds;
    } else if (sv_reserve_lds(k_sv_gru_bwd_all<SV_GRU_KRB>, lds = sv_gru_bwd_all_need(R, &nc, &rp))) {
        p->bwd = SV_GRU_ALL;
        p->bwd_lds = lds;
        p->nc = nc;
        p->rp = rp;
    } else {
        p->bwd_lds = sizeof(float) * 20 * (size_t)R;        // dh [R] | dgh [3R] | part [16][R]
    }
    // (whichever pair runs: a handle that could not even fall back to the generic backward is refused)
    const size_t lds_bwd = sizeof(float) * 20 * (size_t)R;
    if (hipFuncSetAttribute((const void*)k_sv_gru_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bwd) != hipSuccess) {
        rtx_set_error("svae_create: cannot reserve %zu bytes of LDS for the GRU backward kernel", lds_bwd);
        return RTX_EHIP;
    }
    return RTX_OK;
}

void sv_gru_forward(const SvGruPlan& p, const SvGruBufs& b, const int32_t* seq_ptr, int n_seq, int T, int R, hipStream_t st)
{
    const dim3 grid(seq_ptr ? n_seq : 1);
    if (p.fwd == SV_GRU_KS) {
        hipLaunchKernelGGL((k_sv_gru_fwd_ks<SV_KS_SL, SV_KS_NR, SV_KS_KG>), grid, dim3(512), p.fwd_lds, st, b.GI, b.Whh, b.bhh, seq_ptr, T, R, b.Hout,
                           b.Hprev, b.Gr, b.Gz, b.Gn, b.Ghn);
    } else if (p.fwd == SV_GRU_ROWS) {
        hipLaunchKernelGGL(k_sv_gru_fwd_rows<SV_GRU_KR2>, grid, dim3(512), p.fwd_lds, st, b.GI, b.Whh, b.bhh, seq_ptr, T, R, b.Hout, b.Hprev, b.Gr,
                           b.Gz, b.Gn, b.Ghn);
    } else {
        hipLaunchKernelGGL(k_sv_transpose, dim3((R + 63) / 64, (3 * R + 63) / 64), dim3(256), 0, st, b.Whh, 3 * R, R, b.WhhT);
        hipLaunchKernelGGL(k_sv_gru_fwd, grid, dim3(1024), p.fwd_lds, st, b.GI, b.WhhT, b.bhh, seq_ptr, T, R, b.Hout, b.Hprev, b.Gr, b.Gz, b.Gn,
                           b.Ghn);
    }
}

void sv_gru_backward(const SvGruPlan& p, const SvGruBufs& b, const int32_t* seq_ptr, int n_seq, int T, int R, hipStream_t st)
{
    const dim3 grid(seq_ptr ? n_seq : 1);
    if (p.bwd == SV_GRU_KS)
        hipLaunchKernelGGL((k_sv_gru_bwd_ks<SV_KS_SL, SV_KS_NR, SV_KS_KG>), grid, dim3(512), p.bwd_lds, st, b.dH, b.Whh, seq_ptr, T, R, b.Hprev, b.Gr,
                           b.Gz, b.Gn, b.Ghn, b.dGI, b.dGH);
    else if (p.bwd == SV_GRU_ALL)
        hipLaunchKernelGGL(k_sv_gru_bwd_all<SV_GRU_KRB>, grid, dim3(1024), p.bwd_lds, st, b.dH, b.Whh, seq_ptr, T, R, p.nc, p.rp, b.Hprev, b.Gr, b.Gz,
                           b.Gn, b.Ghn, b.dGI, b.dGH);
    else
        hipLaunchKernelGGL(k_sv_gru_bwd, grid, dim3(1024), p.bwd_lds, st, b.dH, b.Whh, seq_ptr, T, R, b.Hprev, b.Gr, b.Gz, b.Gn, b.Ghn, b.dGI,
                           b.dGH);
}
