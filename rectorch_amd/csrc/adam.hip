// adam.hip -- the optimizer side of the step for gfx950: the fused multi-tensor update of the model's optimizer (Adam, decoupled Adam /
// AdamW, SGD, Adagrad, RMSprop: one walk, k_optim<T, Rule>) with the refresh of the compute-precision shadows, the per-tensor squared
// norms of Mult-DAE's regulariser (k_sumsq), and what the float32 and data-parallel steps put in front of it: the split-K slab sum of a
// small weight gradient (k_dw_slab_reduce), the bf16 cast of a gradient range (k_cast_f32_bf16).  Gradient clipping lives here too: the
// deterministic global norm of the launch's gradients (k_grad_norm_part / k_grad_norm_finish) and the clip itself as a third compile-time
// parameter of the walk (k_optim<T, Rule, Clip>).
#include "rtx_device.h"
#include <chrono>
#include <sched.h>
#include <string.h>

// The clipped quantity G = g grad_scale + reg p, ONE expression with an explicit fused multiply-add: the norm kernels and the clipping
// instantiations of k_optim both call it, so the norm is the norm of exactly the values the optimizer scales.
__device__ __forceinline__ float rtx_prep_grad(float gv, float grad_scale, float reg, float p) { return __fmaf_rn(reg, p, gv * grad_scale); }

// ------------------------------------------------------------------------------------------------
// The update rules of the multi-tensor walk below (torch 2.10 torch.optim, single-tensor form).  A rule is the update of ONE element:
// step(a, reg, p, g_in, m, v) with the prepared gradient g = g_in grad_scale + reg p (+ weight_decay p where the decay is coupled);
// M / V say which of the two state slots of RtxAdamTensor the rule keeps -- the walk neither loads nor stores the other.
// step<true> (the clipping instantiations of the walk): gv IS the prepared gradient g grad_scale + reg p, already clipped; the rule
// goes on from there (the decay is added after the clip, as torch's optimizer.step() adds it to a clipped p.grad).
// ------------------------------------------------------------------------------------------------
// torch.optim.Adam, amsgrad off.  DECOUPLED = false: coupled weight decay, the arithmetic of every release so far (k_adam);
// true (AdamW): p <- p (1 - lr wd) first, the decay stays out of g.  m = exp_avg, v = exp_avg_sq: 28 B/parameter.
template <bool DECOUPLED>
struct RuleAdam {
    static constexpr bool M = true, V = true, INLINE_TEXT = !DECOUPLED;
    template <bool PRE = false>
    static __device__ __forceinline__ void step(const RtxAdamArgs& a, float reg, float& p, float gv, float& mq, float& vq)
    {
        float g;
        if constexpr (PRE) g = gv;
        else g = gv * a.grad_scale + reg * p;
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
    template <bool PRE = false>
    static __device__ __forceinline__ void step(const RtxAdamArgs& a, float reg, float& p, float gv, float& mq, float&)
    {
        float g;
        if constexpr (PRE) g = gv;
        else g = gv * a.grad_scale + reg * p;
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
    template <bool PRE = false>
    static __device__ __forceinline__ void step(const RtxAdamArgs& a, float reg, float& p, float gv, float&, float& vq)
    {
        float g;
        if constexpr (PRE) g = gv;
        else g = gv * a.grad_scale + reg * p;
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
    template <bool PRE = false>
    static __device__ __forceinline__ void step(const RtxAdamArgs& a, float reg, float& p, float gv, float& mq, float& vq)
    {
        float g;
        if constexpr (PRE) g = gv;
        else g = gv * a.grad_scale + reg * p;
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
    if constexpr (Clip != RTX_CLIPK_NONE) {                                         \
        float G = rtx_prep_grad(gv[e], a.grad_scale, reg, pv[e]);                   \
        if constexpr (Clip == RTX_CLIPK_COEF) G = G * clip_c;                       \
        else G = G < -clip_c ? -clip_c : (G > clip_c ? clip_c : G);                 \
        Rule::template step<true>(a, reg, pv[e], G, mv[e], vv[e]);                  \
    } else if constexpr (Rule::INLINE_TEXT) {                                       \
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

// Clip (RTX_CLIPK_*): none -- the text above, the kernels of every release so far; coefficient -- G times the coefficient that
// k_grad_norm_finish left on the device (one uniform load per workgroup); value -- G clamped to +-clip_value.  Both comparisons of
// the clamp are false for a NaN, which therefore stays one, as in torch.clamp.
template <typename T, typename Rule, int Clip = RTX_CLIPK_NONE>
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
    [[maybe_unused]] float clip_c = 0.f;
    if constexpr (Clip == RTX_CLIPK_COEF) clip_c = a.clip_coef[1];
    if constexpr (Clip == RTX_CLIPK_VALUE) clip_c = a.clip_value;
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
    if (a.clip == RTX_CLIPK_COEF) {
        if (is_bf16) hipLaunchKernelGGL((k_optim<bf16_t, Rule, RTX_CLIPK_COEF>), dim3(grid), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((k_optim<float, Rule, RTX_CLIPK_COEF>), dim3(grid), dim3(256), 0, stream, a);
        return;
    }
    if (a.clip == RTX_CLIPK_VALUE) {
        if (is_bf16) hipLaunchKernelGGL((k_optim<bf16_t, Rule, RTX_CLIPK_VALUE>), dim3(grid), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((k_optim<float, Rule, RTX_CLIPK_VALUE>), dim3(grid), dim3(256), 0, stream, a);
        return;
    }
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
    RTX_CHECK(a.clip >= RTX_CLIPK_NONE && a.clip <= RTX_CLIPK_VALUE, RTX_EINVAL, "adam: unknown clip mode %d", a.clip);
    RTX_CHECK(a.clip != RTX_CLIPK_COEF || a.clip_coef, RTX_EINVAL, "adam: clipping by a coefficient without the coefficient's device pair");
    RTX_CHECK(a.clip == RTX_CLIPK_NONE || a.update, RTX_EINVAL, "adam: a clip mode on a launch that only refreshes the compute copies");
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

// ------------------------------------------------------------------------------------------------
// Gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, norm_type 2 or inf): the norm of G over every tensor of an
// optimizer launch, before any parameter moves.  k_grad_norm_part walks the launch's own tensor table as flat 4096-element chunks (one
// workgroup each: float4 loads where the buffers are 16-byte aligned, 4-byte ones elsewhere and in a tensor's tail), accumulates in
// double per thread and stores ONE double per workgroup into its own slot; k_grad_norm_finish sums the slots in a fixed order.  No
// atomics anywhere: the result is the same bits on every run.
//   HBM per parameter: 4 B (the gradient) + 4 B where Mult-DAE's regulariser term is live (the parameter).
// ------------------------------------------------------------------------------------------------
struct RtxNormTab { int start[RTX_MAX_TENSORS + 1]; };   // first chunk of tensor k; start[n] = number of chunks

// max that keeps a NaN once it has one (fmax would drop it)
__device__ __forceinline__ double nan_max(double m, double x) { return m != m ? m : (!(x <= m) ? x : m); }

template <bool INF>
__device__ __forceinline__ double norm_block_reduce(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = INF ? nan_max(v, w) : v + w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) s = INF ? nan_max(s, red[w]) : s + red[w];
    return s;
}

template <bool INF>
__global__ __launch_bounds__(256) void k_grad_norm_part(const RtxAdamArgs a, const RtxNormTab tab, double* __restrict__ part)
{
    __shared__ double red[4];
    const int chunk = blockIdx.x, tid = threadIdx.x;
    int ti = 0;
#pragma unroll 1
    for (int k = 1; k < a.n; ++k)
        if (chunk >= tab.start[k]) ti = k;
    const RtxAdamTensor& t = a.t[ti];
    const long n = (long)t.rows * t.cols;
    float reg = 0.f;
    if (a.lam != 0.f && t.sumsq) {
        const float nrm = sqrtf(*t.sumsq);
        reg = nrm > 0.f ? a.lam / nrm : 0.f;
    }
    const bool live = reg != 0.f;      // the parameter is read only then
    const bool vec = !t.g16 && (((uintptr_t)t.g | (live ? (uintptr_t)t.p : 0)) & 15) == 0;
    double acc = 0.0;
    const long f0 = (long)(chunk - tab.start[ti]) * 4096 + tid * 4;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const long f = f0 + pass * 1024;
        if (f >= n) continue;
        const int nv = (int)min((long)4, n - f);
        float gv[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && nv == 4) {
            const float4 g4 = *(const float4*)(t.g + f);
            gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
            if (live) {
                const float4 p4 = *(const float4*)(t.p + f);
                pv[0] = p4.x; pv[1] = p4.y; pv[2] = p4.z; pv[3] = p4.w;
            }
        } else {
            for (int e = 0; e < nv; ++e) {
                gv[e] = t.g16 ? bf16_to_f32(t.g16[f + e]) : t.g[f + e];
                if (live) pv[e] = t.p[f + e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= nv) continue;
            const float G = live ? rtx_prep_grad(gv[e], a.grad_scale, reg, pv[e]) : gv[e] * a.grad_scale;
            if constexpr (INF) acc = nan_max(acc, (double)fabsf(G));
            else acc += (double)G * (double)G;
        }
    }
    acc = norm_block_reduce<INF>(acc, red);
    if (tid == 0) part[chunk] = acc;
}

// One workgroup: the partials in a fixed order (thread i takes i, i + 256, ...; then the block's fixed tree), in double; one rounding
// to float32 behind the double square root.  coef = max_norm / (total + 1e-6) in float32, clamped above at 1 the way torch.clamp
// does it: the comparison is false for a NaN, which stays (fminf would return 1).
template <bool INF>
__global__ __launch_bounds__(256) void k_grad_norm_finish(const double* __restrict__ part, long n_part, float max_norm, float* __restrict__ pair,
                                                          uint32_t* mailbox, uint32_t seq, uint32_t tag)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n_part; i += 256) acc = INF ? nan_max(acc, part[i]) : acc + part[i];
    acc = norm_block_reduce<INF>(acc, red);
    if (threadIdx.x == 0) {
        const float total = INF ? (float)acc : (float)sqrt(acc);
        float coef = max_norm / (total + 1e-6f);
        coef = coef > 1.f ? 1.f : coef;
        pair[0] = total;
        pair[1] = coef;
        if (mailbox) {
            __hip_atomic_store(mailbox, __float_as_uint(total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(mailbox + 1, __float_as_uint(coef), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(mailbox + 3, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(mailbox + 2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

static long norm_chunks(const RtxAdamArgs& a, RtxNormTab* tab)
{
    long chunks = 0;
    for (int k = 0; k < a.n; ++k) {
        if (tab) tab->start[k] = (int)chunks;
        chunks += ((long)a.t[k].rows * a.t[k].cols + 4095) / 4096;
    }
    if (tab)
        for (int k = a.n; k <= RTX_MAX_TENSORS; ++k) tab->start[k] = (int)chunks;
    return chunks;
}

long rtx_grad_norm_parts(const RtxAdamArgs& a) { return norm_chunks(a, nullptr); }

int rtx_launch_grad_norm(const RtxAdamArgs& a, int norm_inf, float max_norm, double* part, float* pair, uint32_t* mailbox, uint32_t seq,
                         uint32_t tag, hipStream_t stream)
{
    RTX_CHECK(a.n > 0 && a.n <= RTX_MAX_TENSORS, RTX_EINVAL, "grad_norm: bad tensor count %d", a.n);
    RTX_CHECK(pair, RTX_EINVAL, "grad_norm: no output");
    for (int k = 0; k < a.n; ++k)
        RTX_CHECK((a.t[k].g || a.t[k].g16) && a.t[k].rows >= 0 && a.t[k].cols >= 0, RTX_EINVAL, "grad_norm: tensor %d has no gradient buffer", k);
    RtxNormTab tab;
    const long chunks = norm_chunks(a, &tab);
    RTX_CHECK(chunks < (1L << 31), RTX_EINVAL, "grad_norm: %ld chunks", chunks);
    RTX_CHECK(chunks == 0 || part, RTX_EINVAL, "grad_norm: no scratch for the partial sums");
    if (chunks > 0) {
        if (norm_inf) hipLaunchKernelGGL(k_grad_norm_part<true>, dim3((unsigned)chunks), dim3(256), 0, stream, a, tab, part);
        else hipLaunchKernelGGL(k_grad_norm_part<false>, dim3((unsigned)chunks), dim3(256), 0, stream, a, tab, part);
    }
    if (norm_inf) hipLaunchKernelGGL(k_grad_norm_finish<true>, dim3(1), dim3(256), 0, stream, part, chunks, max_norm, pair, mailbox, seq, tag);
    else hipLaunchKernelGGL(k_grad_norm_finish<false>, dim3(1), dim3(256), 0, stream, part, chunks, max_norm, pair, mailbox, seq, tag);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// ---- the clip setting of a handle (rtx_engine_set_grad_clip / rtx_svae_set_grad_clip) and its optimizer launch
int rtx_clip_validate(int mode, double bound, const char* who)
{
    RTX_CHECK(mode >= RTX_CLIPM_NONE && mode <= RTX_CLIPM_VALUE, RTX_EINVAL,
              "%s: unknown mode %d (0 none, 1 global 2-norm, 2 global max-norm, 3 value)", who, mode);
    RTX_CHECK(mode == RTX_CLIPM_NONE || bound >= 0, RTX_EINVAL, "%s: the bound must be a number >= 0 (inf reports the norm and clips nothing), got %g", who, bound);
    return RTX_OK;
}

void rtx_clip_release(RtxClipState& cs)
{
    if (cs.part) (void)hipFree(cs.part);
    if (cs.pair) (void)hipFree(cs.pair);
    if (cs.mailbox) (void)hipHostFree(cs.mailbox);
    cs = RtxClipState();
}

int rtx_clip_prepare(RtxAdamArgs& a, RtxClipState& cs, uint32_t tag, hipStream_t stream)
{
    cs.last_has_norm = false;
    a.clip = RTX_CLIPK_NONE;
    if (cs.mode == RTX_CLIPM_NONE) return RTX_OK;
    if (cs.mode == RTX_CLIPM_VALUE) {
        a.clip = RTX_CLIPK_VALUE;
        a.clip_value = (float)cs.bound;
        return RTX_OK;
    }
    const long parts = rtx_grad_norm_parts(a);
    if (parts > cs.part_cap) {      // (hipFree waits for the device: no launch still reads the old scratch)
        if (cs.part) RTX_HIP(hipFree(cs.part));
        cs.part = nullptr; cs.part_cap = 0;
        RTX_HIP(hipMalloc((void**)&cs.part, sizeof(double) * (size_t)parts));
        cs.part_cap = parts;
    }
    if (!cs.pair) RTX_HIP(hipMalloc((void**)&cs.pair, 2 * sizeof(float)));
    if (!cs.mailbox) {
        void* p = nullptr;
        RTX_HIP(hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped));
        memset(p, 0, 64);
        cs.mailbox = (uint32_t*)p;
    }
    RTX_TRY(rtx_launch_grad_norm(a, cs.mode == RTX_CLIPM_NORMINF, (float)cs.bound, cs.part, cs.pair, cs.mailbox, ++cs.ticket, tag, stream));
    cs.last_has_norm = true;
    a.clip = RTX_CLIPK_COEF;
    a.clip_coef = cs.pair;
    return RTX_OK;
}

int rtx_launch_clipped_adam(RtxAdamArgs& a, int is_bf16, RtxClipState& cs, uint32_t tag, hipStream_t stream)
{
    RTX_TRY(rtx_clip_prepare(a, cs, tag, stream));
    return rtx_launch_adam(a, is_bf16, stream);
}

// {total, coef} of the LAST norm enqueued, from the host mailbox: the stream is not drained
int rtx_clip_wait_norm(RtxClipState& cs, const char* who, float* host2, double timeout_s, uint32_t* tag_out)
{
    RTX_CHECK(host2, RTX_EINVAL, "%s: NULL argument", who);
    RTX_CHECK(cs.last_has_norm && cs.mailbox && cs.ticket != 0, RTX_ESTATE,
              "%s: the last optimizer step computed no gradient norm (set RTX_CLIP_NORM2 or RTX_CLIP_NORMINF first)", who);
    volatile uint32_t* mb = cs.mailbox;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t want = cs.ticket;
    for (unsigned spin = 0;; ++spin) {
        if (__atomic_load_n(&mb[2], __ATOMIC_ACQUIRE) == want) break;
        if ((spin & 0x3ff) == 0x3ff) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            RTX_CHECK(el < (timeout_s > 0 ? timeout_s : 60.0), RTX_EHIP, "%s: the step did not report its gradient norm within %.1f s (ticket %u of %u)", who,
                      el, (unsigned)mb[2], (unsigned)want);
            if (el > 0.002) sched_yield();
        }
    }
    const uint32_t b0 = __atomic_load_n(&mb[0], __ATOMIC_RELAXED), b1 = __atomic_load_n(&mb[1], __ATOMIC_RELAXED);
    memcpy(host2, &b0, 4);
    memcpy(host2 + 1, &b1, 4);
    if (tag_out) *tag_out = __atomic_load_n(&mb[3], __ATOMIC_RELAXED);
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

// Gradient accumulation: the same sum (same order, from +0) weighted into accumulators that survive the launch -- ADD = false
// gW = scale * sum, ADD = true gW = fmaf(scale, sum, gW): one explicit operation per element, so the bits are defined.  The slabs
// stay as the product left them.
template <bool ADD>
__global__ __launch_bounds__(256) void k_dw_slab_reduce_acc(const float* __restrict__ C, int splits, long slab_stride, long ldc, int M_real, int N_real,
                                                            float* __restrict__ gW, float* __restrict__ gbias, float scale)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)M_real * (N_real + 1);
    if (i >= total) return;
    const int m = (int)(i / (N_real + 1)), n = (int)(i - (long)m * (N_real + 1));
    float* dst = n < N_real ? gW + (size_t)m * N_real + n : gbias + m;
    float acc = 0.f;
    if (ADD) acc = *dst;    // (issued before the slab walk: it arrives under it)
    const float* c = C + (size_t)m * ldc + n;
    float v = 0.f;
    for (int s2 = 0; s2 < splits; ++s2) v += c[(size_t)s2 * slab_stride];
    *dst = ADD ? __builtin_fmaf(scale, v, acc) : scale * v;
}

int rtx_launch_dw_slab_reduce_acc(const float* C, int splits, long slab_stride, long ldc, int M_real, int N_real, float* gW, float* gbias, int add,
                                  float scale, hipStream_t stream)
{
    const long total = (long)M_real * (N_real + 1);
    if (total <= 0) return RTX_OK;
    RTX_CHECK(C && gW && gbias && splits >= 1 && scale - scale == 0.f, RTX_EINVAL, "dw_slab_reduce_acc: slabs, both accumulators and a finite weight");
    const dim3 grid((unsigned)((total + 255) / 256));
    if (add) hipLaunchKernelGGL(k_dw_slab_reduce_acc<true>, grid, dim3(256), 0, stream, C, splits, slab_stride, ldc, M_real, N_real, gW, gbias, scale);
    else hipLaunchKernelGGL(k_dw_slab_reduce_acc<false>, grid, dim3(256), 0, stream, C, splits, slab_stride, ldc, M_real, N_real, gW, gbias, scale);
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
