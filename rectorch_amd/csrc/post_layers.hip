// post_layers.hip -- the generic / float32 layer chain for gfx950: split-K slabs of a GEMM -> bias + tanh (forward) or x (1 - o^2)
// (backward) in the compute type (k_post), and the VAE head in both directions (k_vae_fwd, k_vae_bwd).
#include "rtx_kernels.h"

// ------------------------------------------------------------------------------------------------
// post kernels: fp32 GEMM output (split-K slabs) -> bias + tanh (forward) / x (1 - o^2) (backward), written
// row-major in the compute type.  16 x 64 tiles, one float4 per thread and slab; latency-bound, so small
// tiles = many workgroups.  (Round 1 also wrote every result transposed through LDS; the K-major operand
// reads of the weight-gradient kernel made those copies unnecessary.)
// ------------------------------------------------------------------------------------------------
// BURST: slab loads in flight per thread (16 or 32): 88 or 153 registers.  <= 16 slabs (the data-gradient product's) take the 16-deep form.
// (Built to test whether register occupancy is what makes this kernel queue beside the weight kernel: it is not -- DESIGN 4.1 -- but the
// smaller form costs nothing.)
template <typename T, int MODE, int BURST = 32>
__global__ __launch_bounds__(256) void k_post(const RtxPostArgs a)
{
    const int tid = threadIdx.x;
    const int n = blockIdx.x * 64 + (tid & 15) * 4, b = blockIdx.y * 16 + (tid >> 4);
    const float* __restrict__ C = a.C + (size_t)b * a.ldc + n;
    // slab sums, up to 32 slabs per round trip: every load of a batch is issued before the first add (the data-gradient chain
    // runs beside a streaming weight kernel, where a dependent load costs 3-5 us: 25 slabs four at a time made this kernel 32 us).
    // Same order of additions as a plain loop (masked slabs add +0).
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s0 = 0; s0 < a.splits; s0 += BURST) {
        float4 t[BURST];
#pragma unroll
        for (int k = 0; k < BURST; ++k) t[k] = *(const float4*)(C + (size_t)min(s0 + k, a.splits - 1) * a.slab_stride);
#pragma unroll
        for (int k = 0; k < BURST; ++k) {
            const bool on = s0 + k < a.splits;
            c.x += on ? t[k].x : 0.f; c.y += on ? t[k].y : 0.f; c.z += on ? t[k].z : 0.f; c.w += on ? t[k].w : 0.f;
        }
    }
    float v[4] = {c.x, c.y, c.z, c.w};
    if (MODE == RTX_POST_BWD && a.tanh_act) {
        const float4 o = *(const float4*)(a.O32 + (size_t)b * a.Np + n);
        v[0] *= (1.f - o.x * o.x); v[1] *= (1.f - o.y * o.y);
        v[2] *= (1.f - o.z * o.z); v[3] *= (1.f - o.w * o.w);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool valid = (b < a.B) && (n + e < a.N_real);
        float x = v[e];
        if (MODE == RTX_POST_FWD && valid) {
            x += a.bias[n + e];
            if (a.tanh_act) x = tanhf(x);
        }
        v[e] = valid ? x : 0.f;
    }
    if (MODE == RTX_POST_FWD && a.O32) *(float4*)(a.O32 + (size_t)b * a.Np + n) = make_float4(v[0], v[1], v[2], v[3]);
    if (a.R) {
        if (MODE == RTX_POST_FWD && a.ones_col && b < a.B && a.N_real >= n && a.N_real < n + 4) v[a.N_real - n] = 1.f;
        store4<T>((T*)a.R + (size_t)b * a.Np + n, v[0], v[1], v[2], v[3]);
    }
}

int rtx_launch_post(const RtxPostArgs& a, int mode, int is_bf16, hipStream_t stream)
{
    RTX_CHECK(a.Np % 64 == 0 && a.Bp % 16 == 0 && a.ldc % 4 == 0, RTX_EINVAL, "post: bad padding");
    const dim3 block(256), grid(a.Np / 64, a.Bp / 16);
#define RTX_P(T, M) do { if (a.splits <= 16) hipLaunchKernelGGL((k_post<T, M, 16>), grid, block, 0, stream, a); \
                         else hipLaunchKernelGGL((k_post<T, M, 32>), grid, block, 0, stream, a); } while (0)
    if (is_bf16) {
        if (mode == RTX_POST_FWD) RTX_P(bf16_t, RTX_POST_FWD);
        else RTX_P(bf16_t, RTX_POST_BWD);
    } else {
        if (mode == RTX_POST_FWD) RTX_P(float, RTX_POST_FWD);
        else RTX_P(float, RTX_POST_BWD);
    }
#undef RTX_P
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// ------------------------------------------------------------------------------------------------
// VAE head.  forward: [mu | logvar] = C + b ; z = mu + eps * exp(logvar / 2)  (eval: z = mu)
//            backward: dmu = dz + beta*mu/B ; dlogvar = dz*eps*std/2 + beta*(exp(logvar)-1)/(2B)
// 16 x 64 tiles, 4 elements per thread; all loads of a thread are issued before the first use.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_vae_fwd(const RtxVaeFwdArgs a)
{
    const int tid = threadIdx.x;
    const int j = blockIdx.x * 64 + (tid & 63), b0 = blockIdx.y * 16;
    const float* __restrict__ C = a.C;
    // slab sums: every load of a split is issued before the first add (out-of-range threads read a valid, clamped
    // address and are masked later: a branch around the loads would serialise them)
    float m[4] = {0.f, 0.f, 0.f, 0.f}, lv[4] = {0.f, 0.f, 0.f, 0.f};
    {
        const int jc = min(j, a.Z - 1);
        const float* base[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) base[k] = C + (size_t)min(b0 + k * 4 + (tid >> 6), a.Bp - 1) * a.ldc + jc;
#pragma unroll 2
        for (int s = 0; s < a.splits; ++s) {
            float t0[4], t1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { t0[k] = base[k][(size_t)s * a.slab_stride]; t1[k] = base[k][(size_t)s * a.slab_stride + a.Z]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) { m[k] += t0[k]; lv[k] += t1[k]; }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = b0 + k * 4 + (tid >> 6);
        float z = 0.f;
        if (b < a.B && j < a.Z) {
            const float mm = m[k] + a.bias[j], l = lv[k] + a.bias[a.Z + j];
            float eps = 0.f;
            if (a.training)
                eps = a.eps_in ? a.eps_in[(size_t)b * a.Z + j] : rtx_normal(a.seed, a.offset, (uint64_t)b * a.Z + j);
            z = a.training ? mm + eps * expf(0.5f * l) : mm;
            const size_t o = (size_t)b * a.Z + j;
            a.mu32[o] = mm;
            a.lv32[o] = l;
            a.eps32[o] = eps;
            if (a.mu_out) a.mu_out[o] = mm;
            if (a.lv_out) a.lv_out[o] = l;
        }
        if (b < a.B && j == a.Z) z = 1.f;   // ones column -> bias gradient of the first decoder layer
        ((T*)a.Zr)[(size_t)b * a.Zp + j] = Elem<T>::from(z);
    }
}

int rtx_launch_vae_fwd(const RtxVaeFwdArgs& a, int is_bf16, hipStream_t stream)
{
    // (the kernel clamps its loads to column Z - 1 and row B - 1 and writes the ones column at index Z < Zp)
    RTX_CHECK(a.Z >= 1 && a.B >= 1, RTX_EINVAL, "vae_fwd: Z = %d, B = %d (both must be >= 1)", a.Z, a.B);
    RTX_CHECK(a.Zp % 64 == 0 && a.Zp > a.Z && a.Bp % 16 == 0, RTX_EINVAL, "vae_fwd: bad padding (Z %d, Zp %d, Bp %d)", a.Z, a.Zp, a.Bp);
    RTX_CHECK(a.ldc >= 2 * a.Z, RTX_EINVAL, "vae_fwd: ldc = %d holds no [mu | logvar] of width 2 x %d", a.ldc, a.Z);
    const dim3 grid(a.Zp / 64, a.Bp / 16), block(256);
    if (is_bf16)
        hipLaunchKernelGGL(k_vae_fwd<bf16_t>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(k_vae_fwd<float>, grid, block, 0, stream, a);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void k_vae_bwd(const RtxVaeBwdArgs a)
{
    const int tid = threadIdx.x;
    const int n = blockIdx.x * 64 + (tid & 63), b0 = blockIdx.y * 16;
    const float* __restrict__ C = a.C;
    const int j = (n < a.Z) ? n : n - a.Z;
    float dz[4] = {0.f, 0.f, 0.f, 0.f}, mu[4], lv[4], ep[4];
    {
        const int jc = min(j, a.Z - 1);
        const float* base[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int bc = min(b0 + k * 4 + (tid >> 6), a.Bp - 1);
            base[k] = C + (size_t)bc * a.ldc + jc;
            const size_t o = (size_t)min(bc, a.B - 1) * a.Z + jc;
            mu[k] = a.mu32[o]; lv[k] = a.lv32[o]; ep[k] = a.eps32[o];
        }
#pragma unroll 2
        for (int s = 0; s < a.splits; ++s) {
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = base[k][(size_t)s * a.slab_stride];
#pragma unroll
            for (int k = 0; k < 4; ++k) dz[k] += t[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = b0 + k * 4 + (tid >> 6);
        float d = 0.f;
        if (b < a.B && n < 2 * a.Z) {
            if (a.g_mu) {   // a loss from outside the engine: its own d / d mu, d / d logvar instead of the KL terms
                const size_t o = (size_t)b * a.Z + j;
                d = n < a.Z ? dz[k] + a.g_mu[o] : a.g_lv[o];
                if (n >= a.Z && a.training) d = dz[k] * ep[k] * 0.5f * expf(0.5f * lv[k]) + a.g_lv[o];
            } else if (n < a.Z) {
                d = dz[k] + a.beta * mu[k] * a.inv_batch;
            } else {
                d = a.beta * 0.5f * (expf(lv[k]) - 1.f) * a.inv_batch;
                if (a.training) d += dz[k] * ep[k] * 0.5f * expf(0.5f * lv[k]);
            }
        }
        ((T*)a.D)[(size_t)b * a.Np + n] = Elem<T>::from(d);
    }
}

int rtx_launch_vae_bwd(const RtxVaeBwdArgs& a, int is_bf16, hipStream_t stream)
{
    RTX_CHECK(a.Z >= 1 && a.B >= 1, RTX_EINVAL, "vae_bwd: Z = %d, B = %d (both must be >= 1)", a.Z, a.B);
    RTX_CHECK(a.Np % 64 == 0 && a.Np >= 2 * a.Z && a.Bp % 16 == 0, RTX_EINVAL, "vae_bwd: bad padding (Z %d, Np %d, Bp %d)", a.Z, a.Np, a.Bp);
    RTX_CHECK(a.ldc >= a.Z, RTX_EINVAL, "vae_bwd: ldc = %d holds no dz of width %d", a.ldc, a.Z);
    RTX_CHECK(!a.g_mu == !a.g_lv, RTX_EINVAL, "vae_bwd: the external gradients of mu and logvar come together");
    const dim3 grid(a.Np / 64, a.Bp / 16), block(256);
    if (is_bf16)
        hipLaunchKernelGGL(k_vae_bwd<bf16_t>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(k_vae_bwd<float>, grid, block, 0, stream, a);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
