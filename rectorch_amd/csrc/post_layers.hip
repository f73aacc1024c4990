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
// USERS (CDAE's user node, rtx_kernels.h: RtxPostUsers): the kernel takes the table as a second member of its argument block; the
// instantiations without it keep the argument block, and the code, they had before the table existed.
template <bool USERS> struct PostParam { RtxPostArgs a; };
template <> struct PostParam<true> { RtxPostArgs a; RtxPostUsers u; };

// One element of torch.optim.SparseAdam's update (torch.optim._functional.sparse_adam), float32, in torch's operation order:
//   um = (g - m) * omb1      m' = m + um
//   uv = (g * g - v) * omb2  v' = v + uv
//   p' = p - step_size * (m' / (sqrt(v') + eps))
// omb1 = (float)(1 - beta1), omb2 = (float)(1 - beta2), step_size = (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t)), the three computed in
// double on the host.  There is NO fma anywhere: every product, sum, difference, the division and the square root are rounded once
// each (IEEE, round to nearest even), so a host loop of the same twelve float32 operations gives the same bits.
__device__ __forceinline__ void rtx_user_adam1(float& p, float& m, float& v, float g, float omb1, float omb2, float eps, float step_size)
{
#pragma clang fp contract(off)
    const float um = (g - m) * omb1;
    const float uv = (g * g - v) * omb2;
    m = m + um;
    v = v + uv;
    const float q = m / (sqrtf(v) + eps);
    p = p - step_size * q;
}

// the four elements (b, n .. n + 3) of a user's rows of V / exp_avg / exp_avg_sq: where they are, loaded, updated, stored.  A thread
// without a user (padding row, id outside [0, n_users)) or without a valid column reads a valid, clamped address and stores nothing.
struct UserQuad {
    size_t off[4];
    bool on[4], has;
};
__device__ __forceinline__ UserQuad user_quad(const RtxPostUsers& u, int b, int B, int n, int N_real)
{
    UserQuad q;
    const int id = u.uid[min(b, B - 1)];
    q.has = b < B && id >= 0 && id < u.n_users && n < N_real;
    const size_t row = (size_t)(q.has ? id : 0) * (size_t)u.ld;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        q.on[e] = q.has && n + e < N_real;
        // vec: one float4 at the first column of the thread's (clamped) quad -- ld >= roundup(N_real, 4) keeps it inside the row
        q.off[e] = row + (u.vec ? (size_t)(min(n, (N_real - 1) & ~3) + e) : (size_t)min(n + e, N_real - 1));
    }
    return q;
}
__device__ __forceinline__ void user_load4(const RtxPostUsers& u, const float* __restrict__ t, const UserQuad& q, float r[4])
{
    if (u.vec) {
        const float4 x = *(const float4*)(t + q.off[0]);
        r[0] = x.x; r[1] = x.y; r[2] = x.z; r[3] = x.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = t[q.off[e]];
    }
}
// (columns of the quad past N_real, inside the row's padding, get back the value that was loaded)
__device__ __forceinline__ void user_store4(const RtxPostUsers& u, float* t, const UserQuad& q, const float r[4])
{
    if (!q.has) return;
    if (u.vec) {
        *(float4*)(t + q.off[0]) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q.on[e]) t[q.off[e]] = r[e];
    }
}

template <typename T, int MODE, int BURST = 32, bool USERS = false>
__global__ __launch_bounds__(256) void k_post(const PostParam<USERS> pa)
{
    const RtxPostArgs& a = pa.a;
    const int tid = threadIdx.x;
    const int n = blockIdx.x * 64 + (tid & 15) * 4, b = blockIdx.y * 16 + (tid >> 4);
    const float* __restrict__ C = a.C + (size_t)b * a.ldc + n;
    // USERS: the row gather -- id, then the user's 16 bytes of V (backward: of both moments too) -- is issued in front of the slab loads,
    // so that the one dependent load of this kernel (the row behind the id) is in flight under them and not behind the sum
    UserQuad uq;
    float up[4], um[4], uv[4];
    if constexpr (USERS) {
        uq = user_quad(pa.u, b, a.B, n, a.N_real);
        user_load4(pa.u, pa.u.V, uq, up);
        if (MODE == RTX_POST_BWD) {
            user_load4(pa.u, pa.u.m, uq, um);
            user_load4(pa.u, pa.u.v, uq, uv);
        }
    }
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
            if constexpr (USERS) {
                if (uq.on[e]) x += up[e];     // (c + bias) + V[u][n]; no user: the sum stays what the table-less kernel computes
            }
            if (a.tanh_act) x = tanhf(x);
        }
        v[e] = valid ? x : 0.f;
    }
    if constexpr (USERS) {
        if (MODE == RTX_POST_BWD) {
            // v[e] is the float32 gradient of V[uid[b]][n + e], before the cast to the compute type: the rows' lazy update, no
            // gradient buffer.  The ids of a launch are distinct, so no other thread of the grid touches these 3 x 16 bytes.
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (uq.on[e]) rtx_user_adam1(up[e], um[e], uv[e], v[e], pa.u.omb1, pa.u.omb2, pa.u.eps, pa.u.step_size);
            user_store4(pa.u, pa.u.V, uq, up);
            user_store4(pa.u, pa.u.m, uq, um);
            user_store4(pa.u, pa.u.v, uq, uv);
        }
    }
    if (MODE == RTX_POST_FWD && a.O32) *(float4*)(a.O32 + (size_t)b * a.Np + n) = make_float4(v[0], v[1], v[2], v[3]);
    if (a.R) {
        if (MODE == RTX_POST_FWD && a.ones_col && b < a.B && a.N_real >= n && a.N_real < n + 4) v[a.N_real - n] = 1.f;
        store4<T>((T*)a.R + (size_t)b * a.Np + n, v[0], v[1], v[2], v[3]);
    }
}

template <bool USERS>
static int launch_post(const PostParam<USERS>& pa, int mode, int is_bf16, hipStream_t stream)
{
    const RtxPostArgs& a = pa.a;
    RTX_CHECK(a.Np % 64 == 0 && a.Bp % 16 == 0 && a.ldc % 4 == 0, RTX_EINVAL, "post: bad padding");
    const dim3 block(256), grid(a.Np / 64, a.Bp / 16);
    // (the update's 12 more values per thread do not fit beside 32 slabs in flight: with a table the backward walks them 16 at a time)
#define RTX_P(T, M) do { if constexpr (USERS && M == RTX_POST_BWD) hipLaunchKernelGGL((k_post<T, M, 16, USERS>), grid, block, 0, stream, pa); \
                         else if (a.splits <= 16) hipLaunchKernelGGL((k_post<T, M, 16, USERS>), grid, block, 0, stream, pa); \
                         else hipLaunchKernelGGL((k_post<T, M, 32, USERS>), grid, block, 0, stream, pa); } while (0)
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

int rtx_launch_post(const RtxPostArgs& a, int mode, int is_bf16, hipStream_t stream)
{
    PostParam<false> pa;
    pa.a = a;
    return launch_post<false>(pa, mode, is_bf16, stream);
}

static int check_users(const RtxPostUsers& u, int latent, bool update, const char* who)
{
    RTX_CHECK(u.uid && u.V && u.n_users > 0 && u.ld >= latent && latent > 0, RTX_EINVAL, "%s: the user table needs ids, V, n_users > 0 and ld >= latent", who);
    RTX_CHECK(!update || (u.m && u.v), RTX_EINVAL, "%s: the update needs exp_avg and exp_avg_sq", who);
    RTX_CHECK(!u.vec || rtx_user_rows_vec(u.V, update ? u.m : u.V, update ? u.v : u.V, u.ld, latent), RTX_EINVAL, "%s: rows marked float4-readable are not", who);
    return RTX_OK;
}

bool rtx_user_rows_vec(const float* V, const float* m, const float* v, long ld, int latent)
{
    return ld % 4 == 0 && ld >= (latent + 3) / 4 * 4 && (((uintptr_t)V | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
}

void rtx_user_adam_scalars(float lr, float beta1, float beta2, float eps, int step, RtxPostUsers& u)
{
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    u.omb1 = (float)(1.0 - (double)beta1);
    u.omb2 = (float)(1.0 - (double)beta2);
    u.eps = eps;
    u.step_size = (float)((double)lr * sqrt(bc2) / bc1);
}

int rtx_launch_post_users(const RtxPostArgs& a, const RtxPostUsers& u, int mode, int is_bf16, hipStream_t stream)
{
    RTX_CHECK(a.B >= 1, RTX_EINVAL, "post: empty batch");
    RTX_TRY(check_users(u, a.N_real, mode == RTX_POST_BWD, "post"));
    PostParam<true> pa;
    pa.a = a;
    pa.u = u;
    return launch_post<true>(pa, mode, is_bf16, stream);
}

// the update of k_post<.., RTX_POST_BWD, .., USERS> on its own: thread (b, n .. n + 3) of 16 x 64 tiles, g float32 [batch][ldg]
__global__ __launch_bounds__(256) void k_user_rows_adam(const RtxPostUsers u, const float* __restrict__ g, long ldg, int batch, int latent)
{
    const int tid = threadIdx.x;
    const int n = blockIdx.x * 64 + (tid & 15) * 4, b = blockIdx.y * 16 + (tid >> 4);
    const UserQuad uq = user_quad(u, b, batch, n, latent);
    float up[4], um[4], uv[4], gg[4];
    user_load4(u, u.V, uq, up);
    user_load4(u, u.m, uq, um);
    user_load4(u, u.v, uq, uv);
#pragma unroll
    for (int e = 0; e < 4; ++e) gg[e] = g[(size_t)min(b, batch - 1) * ldg + min(n + e, latent - 1)];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (uq.on[e]) rtx_user_adam1(up[e], um[e], uv[e], gg[e], u.omb1, u.omb2, u.eps, u.step_size);
    user_store4(u, u.V, uq, up);
    user_store4(u, u.m, uq, um);
    user_store4(u, u.v, uq, uv);
}

int rtx_launch_user_rows_adam(const RtxPostUsers& u, const float* g, long ldg, int batch, int latent, hipStream_t stream)
{
    RTX_CHECK(g && batch >= 1 && ldg >= latent, RTX_EINVAL, "user_rows_adam: g must be [batch >= 1][ldg >= latent]");
    RTX_TRY(check_users(u, latent, true, "user_rows_adam"));
    const dim3 block(256), grid((latent + 63) / 64, (batch + 15) / 16);
    hipLaunchKernelGGL(k_user_rows_adam, grid, block, 0, stream, u, g, ldg, batch, latent);
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
