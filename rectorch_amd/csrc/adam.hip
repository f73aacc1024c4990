// adam.hip -- the optimizer side of the step for gfx950: the fused multi-tensor update of the model's optimizer (Adam, decoupled Adam /
// AdamW, SGD, Adagrad, RMSprop: one walk, k_optim<T, Rule>) with the refresh of the compute-precision shadows, the per-tensor squared
// norms of Mult-DAE's regulariser (k_sumsq), and what the float32 and data-parallel steps put in front of it: the split-K slab sum of a
// small weight gradient (k_dw_slab_reduce), the bf16 cast of a gradient range (k_cast_f32_bf16).
#include "rtx_device.h"

// ------------------------------------------------------------------------------------------------
// The update rules of the multi-tensor walk below (torch 2.10 torch.optim, single-tensor form).  A rule is the update of ONE element:
// step(a, reg, p, g_in, m, v) with the prepared gradient g = g_in grad_scale + reg p (+ weight_decay p where the decay is coupled);
// M / V say which of the two state slots of RtxAdamTensor the rule keeps -- the walk neither loads nor stores the other.
// ------------------------------------------------------------------------------------------------
// torch.optim.Adam, amsgrad off.  DECOUPLED = false: coupled weight decay, the arithmetic of every release so far (k_adam);
// true (AdamW): p <- p (1 - lr wd) first, the decay stays out of g.  m = exp_avg, v = exp_avg_sq: 28 B/parameter.
template <bool DECOUPLED>
struct RuleAdam {
    static constexpr bool M = true, V = true, INLINE_TEXT = !DECOUPLED;
    static __device__ __forceinline__ void step(const RtxAdamArgs& a, float reg, float& p, float gv, float& mq, float& vq)
    {
        float g = gv * a.grad_scale + reg * p;
        if constexpr (DECOUPLED) p = p * a.decay;
        else if (a.weight_decay != 0.f) g += a.weight_decay * p;
        const float m = mq + (g - mq) * (1.f - a.beta1);
        const float v = vq * a.beta2 + (1.f - a.beta2) * g * g;
        const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
        p = p - a.step_size * (m / denom);
        mq = m;
        vq = v;
    }
};
// torch.optim.SGD.  MOM = false (momentum == 0): no state, 12 B/parameter; true: m = momentum_buffer, 20 B/parameter; a.first: the
// parameter's first update, buf = g without dampening (torch clones the gradient where momentum_buffer is absent)
template <bool MOM>
struct RuleSgd {
    static constexpr bool M = MOM, V = false, INLINE_TEXT = false;
    static __device__ __forceinline__ void step(const RtxAdamArgs& a, float reg, float& p, float gv, float& mq, float&)
    {
        float g = gv * a.grad_scale + reg * p;
        if (a.weight_decay != 0.f) g += a.weight_decay * p;
        if constexpr (MOM) {
            const float buf = a.first ? g : mq * a.momentum + a.damp1 * g;
            mq = buf;
            g = a.nesterov ? g + a.momentum * buf : buf;
        }
        p = p - a.lr * g;
    }
};
// torch.optim.Adagrad: v = sum, a.lr = clr = lr / (1 + (t - 1) lr_decay).  20 B/parameter.
struct RuleAdagrad {
    static constexpr bool M = false, V = true, INLINE_TEXT = false;
    static __device__ __forceinline__ void step(const RtxAdamArgs& a, float reg, float& p, float gv, float&, float& vq)
    {
        float g = gv * a.grad_scale + reg * p;
        if (a.weight_decay != 0.f) g += a.weight_decay * p;
        const float v = vq + g * g;
        p = p - a.lr * (g / (sqrtf(v) + a.eps));
        vq = v;
    }
};
// torch.optim.RMSprop, centered off: v = square_avg (20 B/parameter); MOM: m = momentum_buffer (28 B/parameter)
template <bool MOM>
struct RuleRmsprop {
    static constexpr bool M = MOM, V = true, INLINE_TEXT = false;
    static __device__ __forceinline__ void step(const RtxAdamArgs& a, float reg, float& p, float gv, float& mq, float& vq)
    {
        float g = gv * a.grad_scale + reg * p;
        if (a.weight_decay != 0.f) g += a.weight_decay * p;
        const float v = vq * a.alpha + a.alpha1 * g * g;
        const float q = g / (sqrtf(v) + a.eps);
        vq = v;
        if constexpr (MOM) {
            const float buf = mq * a.momentum + q;
            mq = buf;
            p = p - a.lr * buf;
        } else {
            p = p - a.lr * q;
        }
    }
};

// ------------------------------------------------------------------------------------------------
// fused multi-tensor update (Rule) + refresh of the compute-precision shadows in both orientations.
// One launch for all tensors: 64x64 tiles.
//   HBM per parameter: read p, g and the rule's state + write p and the state (Adam: 16 B + 12 B) + shadows.
// ------------------------------------------------------------------------------------------------
// The update of element e inside the walk.  Coupled Adam -- the rule of every release so far, and of the data-parallel and fused
// paths that must stay bit-compatible with dw_adam.hip's epilogue -- is kept as TEXT in the walk, not as a call of RuleAdam::step:
// hipcc contracts multiply-adds after inlining, and which product of  v b2 + (1 - b2) g g  it fuses differs between the inlined call
// and the text (measured: the stored exp_avg_sq differs in the last bit).  The text below is k_adam's, expression for expression, so
// the Adam instantiation compiles to the code it always did; RuleAdam<false>::step above restates it for reading and is not called.
#define RTX_UPDATE_ELEM(e)                                                          \
    if constexpr (Rule::INLINE_TEXT) {                                              \
        float g = gv[e] * a.grad_scale + reg * pv[e];                               \
        if (a.weight_decay != 0.f) g += a.weight_decay * pv[e];                     \
        const float m = mv[e] + (g - mv[e]) * (1.f - a.beta1);                      \
        const float v = vv[e] * a.beta2 + (1.f - a.beta2) * g * g;                  \
        const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;                          \
        pv[e] = pv[e] - a.step_size * (m / denom);                                  \
        mv[e] = m;                                                                  \
        vv[e] = v;                                                                  \
    } else {                                                                        \
        Rule::step(a, reg, pv[e], gv[e], mv[e], vv[e]);                             \
    }

template <typename T, typename Rule>
__global__ __launch_bounds__(256) void k_optim(const RtxAdamArgs a)
{
    __shared__ float tile[64][65];
    const int tid = threadIdx.x;
    // XCD-aware order: workgroup b runs on XCD b % 8; give every XCD one CONTIGUOUS run of tiles so that the
    // 128-byte lines straddling two neighbouring column tiles (rows are not line-aligned: 2400-B and 80432-B
    // strides) are re-read from that XCD's L2 instead of being fetched from HBM by two different L2s
    // (PMC: FETCH_SIZE was 1.37x the algorithmic read bytes with the plain order).
    const int per_xcd = (a.total_tiles + 7) / 8;
    const int tile_id = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (tile_id >= a.total_tiles) return;
    int ti = 0;
#pragma unroll 1
    for (int k = 1; k < a.n; ++k)
        if (tile_id >= a.t[k].tile_start) ti = k;
    const RtxAdamTensor& t = a.t[ti];
    const int local = tile_id - t.tile_start;
    float reg = 0.f;
    if (a.lam != 0.f && t.sumsq) {
        const float nrm = sqrtf(*t.sumsq);
        reg = nrm > 0.f ? a.lam / nrm : 0.f;
    }
    if (t.flat) {
        // Rows whose length is not a multiple of 4 floats (n_items = 17 769 of the Netflix shape) start at every 16-byte
        // phase, so the 2-D tiles fall back to 4-byte accesses (measured: 2x the time of the whole launch).  Without a
        // transposed copy to produce, the tensor is walked as ONE contiguous array instead: float4 everywhere, and the
        // compute copy gets its (row, column) back from the flat index.
        const long n = (long)t.rows * t.cols;
        if ((long)local * 4096 + 4096 <= n) {
            // a whole 4096-element tile (all but the tensor's last): EVERY load of the four passes is issued before the first update is
            // computed -- one round trip per tile, as the 2-D walk below does.  Round 6: this walk now serves every tensor without a
            // transposed copy, also rows of whole float4s.  The state-stream micro-benchmark (tests/native/test_gemm.cpp "streams")
            // measures the same six streams at 5.9-6.2 TB/s walked flat and at 3.8-4.7 TB/s as 64 x 128 tiles (64 x 64 here: worse).
            float4 P4[4], M4[4], V4[4], G4[4];
            const long f0 = (long)local * 4096 + tid * 4;
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const long f = f0 + pass * 1024;
                P4[pass] = *(const float4*)(t.p + f);
                if (a.update) {
                    if constexpr (Rule::M) M4[pass] = *(const float4*)(t.m + f);
                    if constexpr (Rule::V) V4[pass] = *(const float4*)(t.v + f);
                    if (t.g16) {
                        const uint2 u = *(const uint2*)(t.g16 + f);
                        G4[pass] = make_float4(bf16_to_f32((bf16_t)(u.x & 0xffff)), bf16_to_f32((bf16_t)(u.x >> 16)),
                                               bf16_to_f32((bf16_t)(u.y & 0xffff)), bf16_to_f32((bf16_t)(u.y >> 16)));
                    } else {
                        G4[pass] = *(const float4*)(t.g + f);
                    }
                }
            }
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const long f = f0 + pass * 1024;
                float pv[4] = {P4[pass].x, P4[pass].y, P4[pass].z, P4[pass].w};
                if (a.update) {
                    const float gv[4] = {G4[pass].x, G4[pass].y, G4[pass].z, G4[pass].w};
                    float mv[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (Rule::M) { mv[0] = M4[pass].x; mv[1] = M4[pass].y; mv[2] = M4[pass].z; mv[3] = M4[pass].w; }
                    if constexpr (Rule::V) { vv[0] = V4[pass].x; vv[1] = V4[pass].y; vv[2] = V4[pass].z; vv[3] = V4[pass].w; }
#pragma unroll
                    for (int e = 0; e < 4; ++e) { RTX_UPDATE_ELEM(e) }
                    *(float4*)(t.p + f) = make_float4(pv[0], pv[1], pv[2], pv[3]);
                    if constexpr (Rule::M) *(float4*)(t.m + f) = make_float4(mv[0], mv[1], mv[2], mv[3]);
                    if constexpr (Rule::V) *(float4*)(t.v + f) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                }
                if (t.sh) {
                    int r = (int)(f / t.cols), c = (int)(f - (long)r * t.cols);
                    if ((t.cols & 3) == 0) {      // the four elements share a row, ld_sh is a multiple of 128: one 8- / 16-byte store
                        store4<T>((T*)t.sh + (size_t)r * t.ld_sh + c, pv[0], pv[1], pv[2], pv[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            ((T*)t.sh)[(size_t)r * t.ld_sh + c] = Elem<T>::from(pv[e]);
                            if (++c == t.cols) { c = 0; ++r; }
                        }
                    }
                }
            }
            return;
        }
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const long f = (long)local * 4096 + pass * 1024 + tid * 4;
            if (f >= n) continue;
            const int nv = (int)min((long)4, n - f);
            float pv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
            if (nv == 4) {
                const float4 p4 = *(const float4*)(t.p + f);
                pv[0] = p4.x; pv[1] = p4.y; pv[2] = p4.z; pv[3] = p4.w;
                if (a.update) {
                    float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = m4;
                    if constexpr (Rule::M) m4 = *(const float4*)(t.m + f);
                    if constexpr (Rule::V) v4 = *(const float4*)(t.v + f);
                    if (t.g16) {
                        const uint2 u = *(const uint2*)(t.g16 + f);
                        gv[0] = bf16_to_f32((bf16_t)(u.x & 0xffff)); gv[1] = bf16_to_f32((bf16_t)(u.x >> 16));
                        gv[2] = bf16_to_f32((bf16_t)(u.y & 0xffff)); gv[3] = bf16_to_f32((bf16_t)(u.y >> 16));
                    } else {
                        const float4 g4 = *(const float4*)(t.g + f);
                        gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
                    }
                    mv[0] = m4.x; mv[1] = m4.y; mv[2] = m4.z; mv[3] = m4.w;
                    vv[0] = v4.x; vv[1] = v4.y; vv[2] = v4.z; vv[3] = v4.w;
                }
            } else {
                for (int e = 0; e < nv; ++e) {
                    pv[e] = t.p[f + e];
                    if (a.update) { gv[e] = t.g16 ? bf16_to_f32(t.g16[f + e]) : t.g[f + e]; if constexpr (Rule::M) mv[e] = t.m[f + e]; if constexpr (Rule::V) vv[e] = t.v[f + e]; }
                }
            }
            if (a.update) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nv) { RTX_UPDATE_ELEM(e) }
                if (nv == 4) {
                    *(float4*)(t.p + f) = make_float4(pv[0], pv[1], pv[2], pv[3]);
                    if constexpr (Rule::M) *(float4*)(t.m + f) = make_float4(mv[0], mv[1], mv[2], mv[3]);
                    if constexpr (Rule::V) *(float4*)(t.v + f) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                } else {
                    for (int e = 0; e < nv; ++e) { t.p[f + e] = pv[e]; if constexpr (Rule::M) t.m[f + e] = mv[e]; if constexpr (Rule::V) t.v[f + e] = vv[e]; }
                }
            }
            if (t.sh) {
                int r = (int)(f / t.cols), c = (int)(f - (long)r * t.cols);
                for (int e = 0; e < nv; ++e) {
                    ((T*)t.sh)[(size_t)r * t.ld_sh + c] = Elem<T>::from(pv[e]);
                    if (++c == t.cols) { c = 0; ++r; }
                }
            }
        }
        return;
    }
    const int tiles_c = (t.cols + 63) / 64;
    const int r0 = (local / tiles_c) * 64, c0 = (local % tiles_c) * 64;
    const int cl = (tid & 15) * 4;
    const bool vec = (t.cols & 3) == 0;
    if (vec && t.cols >= 4) {
        // Rows of whole float4s: EVERY load of the thread's four passes (p, m, v, g: 16 x 16 B) is issued before the first
        // update is computed -- one round trip per tile instead of four (the passes' stores may alias the next pass's loads as
        // far as the compiler knows, so written pass by pass each pass waits for the one before).  Out-of-range threads load a
        // clamped (valid) address and skip the stores: no branch around a load.  A rank of the sharded optimizer runs this on
        // 1/8 of the rows, where the launch is all latency: 35 -> ~15 us in the data-parallel step (profiles/r3_adam_probe.txt).
        float4 P4[4], M4[4], V4[4], G4[4];
        const int cc = min(c0 + cl, t.cols - 4);
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int rc = min(r0 + pass * 16 + (tid >> 4), t.rows - 1);
            const size_t o = (size_t)rc * t.cols + cc;
            P4[pass] = *(const float4*)(t.p + o);
            if (a.update) {
                if constexpr (Rule::M) M4[pass] = *(const float4*)(t.m + o);
                if constexpr (Rule::V) V4[pass] = *(const float4*)(t.v + o);
                if (t.g16) {   // data parallel, bf16 exchange: the reduced gradient arrives as bf16
                    const uint2 u = *(const uint2*)(t.g16 + o);
                    G4[pass] = make_float4(bf16_to_f32((bf16_t)(u.x & 0xffff)), bf16_to_f32((bf16_t)(u.x >> 16)),
                                           bf16_to_f32((bf16_t)(u.y & 0xffff)), bf16_to_f32((bf16_t)(u.y >> 16)));
                } else {
                    G4[pass] = *(const float4*)(t.g + o);
                }
            }
        }
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int rl = pass * 16 + (tid >> 4);
            const int r = r0 + rl, c = c0 + cl;
            const bool ok = r < t.rows && c < t.cols;
            float pv[4] = {P4[pass].x, P4[pass].y, P4[pass].z, P4[pass].w};
            if (ok) {
                const size_t o = (size_t)r * t.cols + c;
                if (a.update) {
                    const float gv[4] = {G4[pass].x, G4[pass].y, G4[pass].z, G4[pass].w};
                    float mv[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (Rule::M) { mv[0] = M4[pass].x; mv[1] = M4[pass].y; mv[2] = M4[pass].z; mv[3] = M4[pass].w; }
                    if constexpr (Rule::V) { vv[0] = V4[pass].x; vv[1] = V4[pass].y; vv[2] = V4[pass].z; vv[3] = V4[pass].w; }
#pragma unroll
                    for (int e = 0; e < 4; ++e) { RTX_UPDATE_ELEM(e) }
                    *(float4*)(t.p + o) = make_float4(pv[0], pv[1], pv[2], pv[3]);
                    if constexpr (Rule::M) *(float4*)(t.m + o) = make_float4(mv[0], mv[1], mv[2], mv[3]);
                    if constexpr (Rule::V) *(float4*)(t.v + o) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                }
                if (t.sh) store4<T>((T*)t.sh + (size_t)r * t.ld_sh + c, pv[0], pv[1], pv[2], pv[3]);   // ld_sh is a multiple of 128 -> aligned
            }
            if (t.shT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) tile[rl][cl + e] = ok ? pv[e] : 0.f;
            }
        }
    } else {
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int rl = pass * 16 + (tid >> 4);
        const int r = r0 + rl, c = c0 + cl;
        float pv[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < t.rows && c < t.cols) {
            const size_t o = (size_t)r * t.cols + c;
            const int nv = min(4, t.cols - c);
            float gv[4], mv[4], vv[4];
            for (int e = 0; e < nv; ++e) {
                pv[e] = t.p[o + e];
                if (a.update) { gv[e] = t.g16 ? bf16_to_f32(t.g16[o + e]) : t.g[o + e]; if constexpr (Rule::M) mv[e] = t.m[o + e]; if constexpr (Rule::V) vv[e] = t.v[o + e]; }
            }
            if (a.update) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nv) { RTX_UPDATE_ELEM(e) }
                for (int e = 0; e < nv; ++e) { t.p[o + e] = pv[e]; if constexpr (Rule::M) t.m[o + e] = mv[e]; if constexpr (Rule::V) t.v[o + e] = vv[e]; }
            }
            if (t.sh) {
                T* s = (T*)t.sh + (size_t)r * t.ld_sh + c;
                if (nv == 4) store4<T>(s, pv[0], pv[1], pv[2], pv[3]);
                else for (int e = 0; e < nv; ++e) s[e] = Elem<T>::from(pv[e]);
            }
        }
        if (t.shT) {
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[rl][cl + e] = (r < t.rows && c + e < t.cols) ? pv[e] : 0.f;
        }
    }
    }
    if (t.shT) {
        __syncthreads();
        // transposed shadow [cols_p][ld_shT]: thread -> column c0+nl, 16 consecutive rows
        const int nl = tid >> 2, rq = (tid & 3) * 16;
        if (c0 + nl < t.cols) {
            T* dst = (T*)t.shT + (size_t)(c0 + nl) * t.ld_shT + r0 + rq;
            if (r0 + rq + 16 <= t.rows) {
#pragma unroll
                for (int e = 0; e < 16; e += 4)
                    store4<T>(dst + e, tile[rq + e][nl], tile[rq + e + 1][nl], tile[rq + e + 2][nl], tile[rq + e + 3][nl]);
            } else {
                for (int e = 0; e < 16; ++e)
                    if (r0 + rq + e < t.rows) dst[e] = Elem<T>::from(tile[rq + e][nl]);
            }
        }
    }
}

template <typename Rule>
static void launch_rule(const RtxAdamArgs& a, int is_bf16, int grid, hipStream_t stream)
{
    if (is_bf16)
        hipLaunchKernelGGL((k_optim<bf16_t, Rule>), dim3(grid), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((k_optim<float, Rule>), dim3(grid), dim3(256), 0, stream, a);
}

#undef RTX_UPDATE_ELEM

int rtx_launch_adam(RtxAdamArgs& a, int is_bf16, hipStream_t stream)
{
    RTX_CHECK(a.n > 0 && a.n <= RTX_MAX_TENSORS, RTX_EINVAL, "adam: bad tensor count %d", a.n);
    RTX_CHECK(a.rule >= 0 && a.rule < RTX_RULE_COUNT, RTX_EINVAL, "adam: unknown update rule %d", a.rule);
    const bool use_m = a.rule == RTX_RULE_ADAM || a.rule == RTX_RULE_ADAMW || a.rule == RTX_RULE_SGD_MOM || a.rule == RTX_RULE_RMSPROP_MOM;
    const bool use_v = a.rule != RTX_RULE_SGD && a.rule != RTX_RULE_SGD_MOM;
    int tiles = 0;
    for (int k = 0; k < a.n; ++k) {
        a.t[k].tile_start = tiles;
        // flat walk: no transposed copy to produce, rows not 16-byte periodic, buffers 16-byte aligned
        const RtxAdamTensor& tk = a.t[k];
        // (a state slot the rule does not keep is never dereferenced: its pointer does not count)
        const bool aligned = (((uintptr_t)tk.p | (use_m ? (uintptr_t)tk.m : 0) | (use_v ? (uintptr_t)tk.v : 0) | (uintptr_t)tk.g | (uintptr_t)tk.g16) & 15) == 0;
        // ... and a bias (one row) always: a handful of 4096-element tiles instead of one 64-column tile per workgroup
        // (round 6: every tensor without a transposed copy -- rows of whole float4s too: the flat walk streams at the rate of a copy, tiles do not)
        a.t[k].flat = (!tk.shT && aligned && ((long)tk.rows * tk.cols & 3) == 0) || (!tk.shT && aligned && (((tk.cols & 3) != 0 && tk.rows > 1) || tk.rows == 1)) ? 1 : 0;
        if (a.t[k].flat) tiles += (int)(((long)tk.rows * tk.cols + 4095) / 4096);
        else tiles += ((a.t[k].rows + 63) / 64) * ((a.t[k].cols + 63) / 64);
    }
    if (tiles == 0) return RTX_OK;
    a.total_tiles = tiles;
    const int grid = 8 * ((tiles + 7) / 8);
    switch (a.rule) {
    case RTX_RULE_ADAM: launch_rule<RuleAdam<false>>(a, is_bf16, grid, stream); break;
    case RTX_RULE_ADAMW: launch_rule<RuleAdam<true>>(a, is_bf16, grid, stream); break;
    case RTX_RULE_SGD: launch_rule<RuleSgd<false>>(a, is_bf16, grid, stream); break;
    case RTX_RULE_SGD_MOM: launch_rule<RuleSgd<true>>(a, is_bf16, grid, stream); break;
    case RTX_RULE_ADAGRAD: launch_rule<RuleAdagrad>(a, is_bf16, grid, stream); break;
    case RTX_RULE_RMSPROP: launch_rule<RuleRmsprop<false>>(a, is_bf16, grid, stream); break;
    default: launch_rule<RuleRmsprop<true>>(a, is_bf16, grid, stream); break;
    }
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// The scalars of update `step` (1-based) of optimizer `o` into `a`, computed in double as torch computes them on the host.  Adam's
// are those every release so far computed; lr is a.lr for SGD and RMSprop, clr for Adagrad.
int rtx_optim_scalars(const RtxOptim& o, float lr, float beta1, float beta2, float eps, float weight_decay, int step, RtxAdamArgs& a)
{
    a.update = 1;
    a.eps = eps; a.weight_decay = weight_decay;
    a.grad_scale = 1.f;
    a.lam = 0.f;
    a.first = 0; a.nesterov = 0;
    switch (o.kind) {
    case RTX_OPT_ADAM: {
        const double bc1 = 1.0 - pow((double)beta1, (double)step);
        const double bc2 = 1.0 - pow((double)beta2, (double)step);
        a.step_size = (float)((double)lr / bc1);
        a.bc2_sqrt = (float)sqrt(bc2);
        a.beta1 = beta1; a.beta2 = beta2;
        a.rule = (o.flags & RTX_OPTF_DECOUPLED) ? RTX_RULE_ADAMW : RTX_RULE_ADAM;
        a.decay = (float)(1.0 - (double)lr * (double)weight_decay);
        break;
    }
    case RTX_OPT_SGD:
        a.rule = o.momentum != 0 ? RTX_RULE_SGD_MOM : RTX_RULE_SGD;
        a.lr = lr; a.momentum = (float)o.momentum; a.damp1 = (float)(1.0 - o.dampening);
        a.nesterov = (o.flags & RTX_OPTF_NESTEROV) ? 1 : 0;
        a.first = (o.flags & RTX_OPTF_FIRST) ? 1 : 0;
        break;
    case RTX_OPT_ADAGRAD:
        a.rule = RTX_RULE_ADAGRAD;
        a.lr = (float)((double)lr / (1.0 + (double)(step - 1) * o.lr_decay));
        break;
    case RTX_OPT_RMSPROP:
        a.rule = o.momentum != 0 ? RTX_RULE_RMSPROP_MOM : RTX_RULE_RMSPROP;
        a.lr = lr; a.momentum = (float)o.momentum; a.alpha = (float)o.alpha; a.alpha1 = (float)(1.0 - o.alpha);
        break;
    default:
        rtx_set_error("optimizer: unknown kind %d (0 Adam, 1 SGD, 2 Adagrad, 3 RMSprop)", o.kind);
        return RTX_EINVAL;
    }
    return RTX_OK;
}

// what rtx_engine_set_optimizer / rtx_svae_set_optimizer accept
int rtx_optim_validate(const RtxOptim& o)
{
    RTX_CHECK(o.kind >= RTX_OPT_ADAM && o.kind <= RTX_OPT_RMSPROP, RTX_EINVAL, "set_optimizer: unknown kind %d (0 Adam, 1 SGD, 2 Adagrad, 3 RMSprop)", o.kind);
    RTX_CHECK((o.flags & ~(RTX_OPTF_DECOUPLED | RTX_OPTF_NESTEROV | RTX_OPTF_FIRST)) == 0, RTX_EINVAL, "set_optimizer: unknown flag bits %d", o.flags);
    RTX_CHECK(!(o.flags & RTX_OPTF_DECOUPLED) || o.kind == RTX_OPT_ADAM, RTX_EINVAL, "set_optimizer: decoupled weight decay is Adam's");
    RTX_CHECK(!(o.flags & (RTX_OPTF_NESTEROV | RTX_OPTF_FIRST)) || (o.kind == RTX_OPT_SGD && o.momentum != 0), RTX_EINVAL,
              "set_optimizer: nesterov / first need SGD with momentum");
    RTX_CHECK(!(o.flags & RTX_OPTF_NESTEROV) || (o.momentum > 0 && o.dampening == 0), RTX_EINVAL,
              "set_optimizer: nesterov needs a positive momentum and zero dampening (as torch.optim.SGD)");
    RTX_CHECK(o.momentum >= 0 && o.alpha >= 0 && o.lr_decay >= 0, RTX_EINVAL, "set_optimizer: negative momentum, alpha or lr_decay");
    return RTX_OK;
}

// sum of squares of each parameter tensor (Mult-DAE's lam * sum_W ||W||_2, models.py:702-706)
__global__ __launch_bounds__(256) void k_sumsq(const float* p, long n, float* out)
{
    __shared__ float red[4];
    float s = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += p[i] * p[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) atomicAdd(out, s);
}

int rtx_launch_sumsq(const float* const* params_host, const long* sizes, int n, float* sumsq, hipStream_t stream)
{
    RTX_HIP(hipMemsetAsync(sumsq, 0, sizeof(float) * n, stream));
    for (int t = 0; t < n; ++t) {
        const int blocks = (int)((sizes[t] + 256 * 16 - 1) / (256 * 16));
        hipLaunchKernelGGL(k_sumsq, dim3(blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks)), dim3(256), 0, stream, params_host[t],
                           sizes[t], sumsq + t);
    }
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// f32 -> bf16 (round to nearest even) of a gradient range before its RCCL all-reduce (data parallel, bf16 exchange)
__global__ __launch_bounds__(256) void k_cast_f32_bf16(const float* __restrict__ src, bf16_t* __restrict__ dst, long n)
{
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i + 8 <= n) {
        const float4 a = *(const float4*)(src + i), b = *(const float4*)(src + i + 4);
        uint4 o;
        o.x = (uint32_t)f32_to_bf16(a.x) | ((uint32_t)f32_to_bf16(a.y) << 16);
        o.y = (uint32_t)f32_to_bf16(a.z) | ((uint32_t)f32_to_bf16(a.w) << 16);
        o.z = (uint32_t)f32_to_bf16(b.x) | ((uint32_t)f32_to_bf16(b.y) << 16);
        o.w = (uint32_t)f32_to_bf16(b.z) | ((uint32_t)f32_to_bf16(b.w) << 16);
        *(uint4*)(dst + i) = o;
    } else {
        for (long k = i; k < n; ++k) dst[k] = f32_to_bf16(src[k]);
    }
}

// Split-K slabs of a small weight-gradient product -> the gradient tensors (float32 parity mode, round 4):
//   gW[m * N_real + n] = sum_s C[s * slab_stride + m * ldc + n]  (m < M_real, n < N_real);  gbias[m] = the same at n == N_real.
// Fixed summation order (s ascending): the step stays bit-reproducible.
__global__ __launch_bounds__(256) void k_dw_slab_reduce(const float* __restrict__ C, int splits, long slab_stride, long ldc, int M_real, int N_real,
                                                        float* __restrict__ gW, float* __restrict__ gbias)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)M_real * (N_real + 1);
    if (i >= total) return;
    const int m = (int)(i / (N_real + 1)), n = (int)(i - (long)m * (N_real + 1));
    const float* c = C + (size_t)m * ldc + n;
    float v = 0.f;
    for (int s2 = 0; s2 < splits; ++s2) v += c[(size_t)s2 * slab_stride];
    if (n < N_real) gW[(size_t)m * N_real + n] = v;
    else if (gbias) gbias[m] = v;
}

int rtx_launch_dw_slab_reduce(const float* C, int splits, long slab_stride, long ldc, int M_real, int N_real, float* gW, float* gbias, hipStream_t stream)
{
    const long total = (long)M_real * (N_real + 1);
    if (total <= 0) return RTX_OK;
    hipLaunchKernelGGL(k_dw_slab_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, C, splits, slab_stride, ldc, M_real, N_real, gW, gbias);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

int rtx_launch_cast_f32_bf16(const float* src, bf16_t* dst, long n, hipStream_t stream)
{
    if (n <= 0) return RTX_OK;
    RTX_CHECK(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, RTX_EINVAL, "cast: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(k_cast_f32_bf16, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, stream, src, dst, n);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
