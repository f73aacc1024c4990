// post_layers.hip -- the generic / float32 layer chain for gfx950: split-K slabs of a GEMM -> bias + tanh (forward) or x (1 - o^2)
// (backward) in the compute type (k_post), the VAE head in both directions (k_vae_fwd, k_vae_bwd), and the kernels of the cut between
// the encoder and the decoder half (k_reparam, k_reparam_grad, k_import_dh, k_export_dz).
#include "rtx_device.h"

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
            z = a.training ? rtx_reparam_z(mm, l, eps) : mm;
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

// ------------------------------------------------------------------------------------------------
// The cut between the encoder and the decoder half (rtx_engine_encode_train / decode_train and their backward calls; rtx_reparam):
// the sampling step as an operator of its own on unpadded float32 [n][Z], the import of d loss / d h into the encoder's chain
// (RTX_DAE / RTX_AE), the export of d loss / d z out of the decoder's.
// ------------------------------------------------------------------------------------------------
// z = mu + eps exp(logvar / 2) element by element; element i = b Z + j draws rtx_normal(seed, offset, i), the fused head's own
__global__ __launch_bounds__(256) void k_reparam(const float* __restrict__ mu, const float* __restrict__ lv, long count, const float* __restrict__ eps_in,
                                                 uint64_t seed, uint64_t offset, float* __restrict__ z, float* __restrict__ eps_out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float eps = eps_in ? eps_in[i] : rtx_normal(seed, offset, (uint64_t)i);
    z[i] = rtx_reparam_z(mu[i], lv[i], eps);
    if (eps_out) eps_out[i] = eps;
}

// d mu = d z, d logvar = d z eps exp(logvar / 2) / 2 (the product order of k_vae_bwd)
__global__ __launch_bounds__(256) void k_reparam_grad(const float* __restrict__ dz, const float* __restrict__ lv, const float* __restrict__ eps, long count,
                                                      float* __restrict__ dmu, float* __restrict__ dlv)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float d = dz[i];
    if (dmu) dmu[i] = d;
    if (dlv) dlv[i] = d * eps[i] * 0.5f * expf(0.5f * lv[i]);
}

int rtx_launch_reparam(const float* mu, const float* logvar, long n, int Z, const float* eps_in, uint64_t seed, uint64_t offset, float* z,
                       float* eps_out, hipStream_t stream)
{
    RTX_CHECK(mu && logvar && z && n >= 1 && Z >= 1, RTX_EINVAL, "reparam: bad arguments (n = %ld, latent = %d)", n, Z);
    const long count = n * Z;
    RTX_CHECK((count + 255) / 256 <= 0x7fffffffL, RTX_EINVAL, "reparam: %ld elements are more than one launch takes", count);
    hipLaunchKernelGGL(k_reparam, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, mu, logvar, count, eps_in, seed, offset, z, eps_out);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

int rtx_launch_reparam_grad(const float* d_z, const float* logvar, const float* eps, long n, int Z, float* d_mu, float* d_logvar, hipStream_t stream)
{
    RTX_CHECK(d_z && n >= 1 && Z >= 1 && (d_mu || d_logvar), RTX_EINVAL, "reparam_grad: bad arguments (n = %ld, latent = %d)", n, Z);
    RTX_CHECK(!d_logvar || (logvar && eps), RTX_EINVAL, "reparam_grad: d_logvar needs logvar and eps");
    const long count = n * Z;
    RTX_CHECK((count + 255) / 256 <= 0x7fffffffL, RTX_EINVAL, "reparam_grad: %ld elements are more than one launch takes", count);
    hipLaunchKernelGGL(k_reparam_grad, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, d_z, logvar, eps, count, d_mu, d_logvar);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// D [Bp][Np] = dh[b][n] (1 - o[b][n]^2) for b < B, n < N_real, zeros elsewhere: the layout contract of k_post (backward).  dh is the
// caller's UNPADDED [B][N_real] tensor: it is read under the mask only, never at a clamped row.  Four columns per thread.
template <typename T>
__global__ __launch_bounds__(256) void k_import_dh(const float* __restrict__ dh, int B, int N_real, int Bp, int Np, int tanh_act,
                                                   const float* __restrict__ O32, T* __restrict__ D)
{
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const int per_row = Np / 4;
    if (q >= (long)Bp * per_row) return;
    const int b = (int)(q / per_row), n = (int)(q % per_row) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (b < B) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (n + e < N_real) {
                float x = dh[(size_t)b * N_real + n + e];
                if (tanh_act) {
                    const float o = O32[(size_t)b * Np + n + e];
                    x *= (1.f - o * o);
                }
                v[e] = x;
            }
    }
    store4<T>(D + (size_t)b * Np + n, v[0], v[1], v[2], v[3]);
}

int rtx_launch_import_dh(const float* dh, int B, int N_real, int Bp, int Np, int tanh_act, const float* O32, void* D, int is_bf16,
                         hipStream_t stream)
{
    RTX_CHECK(dh && D && B >= 1 && B <= Bp && N_real >= 1 && N_real <= Np, RTX_EINVAL, "import_dh: bad arguments (B %d, Bp %d, N %d, Np %d)", B, Bp, N_real, Np);
    RTX_CHECK(Np % 4 == 0, RTX_EINVAL, "import_dh: Np = %d is no multiple of 4", Np);
    RTX_CHECK(!tanh_act || O32, RTX_EINVAL, "import_dh: the tanh derivative needs the saved activation");
    const long q = (long)Bp * (Np / 4);
    const dim3 grid((unsigned)((q + 255) / 256)), block(256);
    if (is_bf16)
        hipLaunchKernelGGL(k_import_dh<bf16_t>, grid, block, 0, stream, dh, B, N_real, Bp, Np, tanh_act, O32, (bf16_t*)D);
    else
        hipLaunchKernelGGL(k_import_dh<float>, grid, block, 0, stream, dh, B, N_real, Bp, Np, tanh_act, O32, (float*)D);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// d_z [n][Z] (unpadded float32) = the sum of the product's split-K slabs C [splits][..][ldc] in slab order
__global__ __launch_bounds__(256) void k_export_dz(const float* __restrict__ C, int splits, long slab_stride, int ldc, int n, int Z, float* __restrict__ dz)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * Z) return;
    const int b = (int)(i / Z), j = (int)(i % Z);
    const float* p = C + (size_t)b * ldc + j;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += p[(size_t)k * slab_stride];
    dz[i] = s;
}

int rtx_launch_export_dz(const float* C, int splits, long slab_stride, int ldc, int n, int Z, float* d_z, hipStream_t stream)
{
    RTX_CHECK(C && d_z && splits >= 1 && n >= 1 && Z >= 1 && ldc >= Z, RTX_EINVAL, "export_dz: bad arguments (splits %d, n %d, Z %d, ldc %d)", splits, n, Z, ldc);
    RTX_CHECK(splits == 1 || slab_stride >= (long)(n - 1) * ldc + Z, RTX_EINVAL, "export_dz: slabs of %ld floats overlap", slab_stride);
    const long count = (long)n * Z;
    hipLaunchKernelGGL(k_export_dz, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, C, splits, slab_stride, ldc, n, Z, d_z);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
