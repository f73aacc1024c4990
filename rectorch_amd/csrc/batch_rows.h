// batch_rows.h -- the sampler's row arithmetic, defined once: what a stored entry of a user's CSR row becomes in the batch the
// first layer reads.  k_gather, k_gather_scatter (batch_rows.hip: the dense image) and k_in_chunks (spmm_in.hip: the chunk stream
// of the sparse first layer) all call these, so the three forms of a batch agree to the bit.
// Reference: F.normalize(x) then dropout (nets.py:394-399); a conditioned row (Iin > I) is normalised and dropped out over its item
// columns only, the condition columns are concatenated raw afterwards (CMultiVAE_net.encode, nets.py:467-471).
// NT = threads of the workgroup (all of them call; `red` holds >= NT / 64 floats).
#pragma once
#include "rtx_device.h"

#ifdef __HIPCC__
// ||x||^2 over the item columns of CSR entries [beg, end).  Implicit feedback (no value array, no condition columns): the number
// of stored entries.
template <int NT>
__device__ __forceinline__ float row_sumsq(const RtxCsrView& in, int64_t beg, int64_t end, int I, int Iin, float* red)
{
    const bool cond = Iin > I;
    if (!in.values && !cond) return (float)(end - beg);
    float ss = 0.f;
    for (int64_t k = beg + threadIdx.x; k < end; k += NT) {
        const float v = in.values ? in.values[k] : 1.f;
        if (!cond || in.indices[k] < I) ss += v * v;
    }
    return block_sum<NT>(ss, red);
}

// s_b = sum of the TARGET row of batch row b over the item columns (the multinomial likelihood's weight)
template <int NT>
__device__ __forceinline__ float row_target_sum(const RtxCsrView& target, int b, int I, int Iin, float* red)
{
    const bool cond = Iin > I;
    const int64_t ut = csr_row(target, b);
    const int64_t tb = target.indptr[ut], te = target.indptr[ut + 1];
    if (!target.values && !cond) return (float)(te - tb);
    float ts = 0.f;
    for (int64_t k = tb + threadIdx.x; k < te; k += NT)
        if (!cond || target.indices[k] < I) ts += target.values ? target.values[k] : 1.f;
    return block_sum<NT>(ts, red);
}

// the row's two factors: inv = 1 / max(||x||, 1e-12) (F.normalize; 1 for a raw row: VAE_net, nets.py:287) and the dropout scale
struct RowScale {
    float inv, scale;
    bool drop;
};
__device__ __forceinline__ RowScale row_scale(float ss, int raw, int training, float dropout_p)
{
    RowScale s;
    s.inv = raw ? 1.f : 1.f / fmaxf(sqrtf(ss), 1e-12f);
    s.drop = training && dropout_p > 0.f;
    s.scale = s.drop ? (dropout_p < 1.f ? 1.f / (1.f - dropout_p) : 0.f) : 1.f;
    return s;
}

// value of the stored entry v at column i of batch row b: normalised, then kept or dropped by the injected mask or the Philox
// decision of element b * I + i; a condition column (i >= I) stays as stored
__device__ __forceinline__ float row_entry(float v, int i, int b, int I, const RowScale& s, const uint8_t* mask, uint64_t seed,
                                           uint64_t offset, float dropout_p)
{
    if (i < I) v *= s.inv;
    if (s.drop && i < I) {
        const uint64_t e = (uint64_t)b * (uint64_t)I + (uint64_t)i;
        const bool keep = mask ? (mask[e] != 0) : rtx_dropout_keep(seed, offset, e, dropout_p);
        v = keep ? v * s.scale : 0.f;
    }
    return v;
}
#endif
