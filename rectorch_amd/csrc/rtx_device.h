// rtx_device.h -- device helpers shared by the non-GEMM kernel files: wave and block reductions, the CSR row of a batch row.
// Wave = 64 lanes throughout.
#pragma once
#include "rtx_kernels.h"

#ifdef __HIPCC__
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// block-wide sum for NT-thread blocks (256, or 512: k_in_chunks); red must hold >= NT / 64 floats; result broadcast to all threads.
// Fixed order: the 64-lane butterfly, then the wave partials in index order.
template <int NT = 256>
__device__ __forceinline__ float block_sum(float v, float* red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red)
{
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The reparameterisation z = mu + eps exp(logvar / 2) of the VAE heads (post_layers.hip: k_vae_fwd, small_layers.hip: k_fwd_head) and
// of the stand-alone operator (post_layers.hip: k_reparam): ONE expression, so that all three compile the same arithmetic and a z
// sampled outside the head equals the head's own to the bit.
__device__ __forceinline__ float rtx_reparam_z(float mu, float logvar, float eps) { return mu + eps * expf(0.5f * logvar); }

__device__ __forceinline__ int64_t csr_row(const RtxCsrView& v, int b) { return v.row_ids ? (int64_t)v.row_ids[b] : (int64_t)b; }
#endif
