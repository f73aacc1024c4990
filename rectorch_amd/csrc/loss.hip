// loss.hip -- losses of the Mult-VAE / Mult-DAE / VAE_net / AETrainer step for gfx950 and their gradients w.r.t. the logits: the
// multinomial likelihood (k_row_lse, k_dlogits, k_dlogits_row), the element-wise losses (k_elem_dlogits over a loss policy: VAE_net's
// binary cross-entropy + KL, AETrainer's mean squared error; k_sigmoid_rows), the import of a gradient w.r.t. the outputs that a loss
// outside the engine produced (k_import_dout: rtx_engine_backward), the fixed-order loss sum with its host mailbox
// (k_reduce_loss), predict()'s -inf mask (k_neg_inf), the public loss functions on dense tensors (k_dense_loss, k_dense_bce_kl,
// k_dense_mse) and the same with their gradients (k_dense_loss_grad, k_dense_elem_grad, k_norm_grad).  The row helpers the kernels share come first: log-sum-exp from (max, sum) partials, the KL row sum, the padding-row
// fill and the LDS image of a target row's chunk.
#include "rtx_device.h"
#include <algorithm>

// ------------------------------------------------------------------------------------------------
// multinomial log-likelihood: per row  lse_b = logsumexp(Y_b) ;  row_loss_b = (s_b*lse_b - <t_b,Y_b>)/B
//  (+ beta * KL_b / B for the VAE).   One workgroup per user, online max/sum, float4 reads.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void online_add(float& m, float& s, float x)
{
    if (x > m) {
        s = s * __expf(m - x) + 1.f;
        m = x;
    } else {
        s += __expf(x - m);
    }
}
__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2)
{
    const float mm = fmaxf(m, m2);
    if (mm == -INFINITY) { m = mm; s = 0.f; return; }
    s = s * __expf(m - mm) + s2 * __expf(m2 - mm);
    m = mm;
}

// log-sum-exp M + log S of a block's per-thread (max, sum) pairs: the 64-lane butterfly, then the four wave pairs through red (>= 8
// floats) in index order.  RED_BUSY: red may still be read from before this call, so a barrier precedes the write to it.  None
// follows the reads: a caller that writes red next places that barrier itself.
template <bool RED_BUSY>
__device__ __forceinline__ float block_lse_merge(float m, float s, float* red)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        online_merge(m, s, m2, s2);
    }
    if (RED_BUSY) __syncthreads();
    if ((tid & 63) == 0) { red[tid >> 6] = m; red[4 + (tid >> 6)] = s; }
    __syncthreads();
    float M = red[0], S = red[4];
    online_merge(M, S, red[1], red[5]);
    online_merge(M, S, red[2], red[6]);
    online_merge(M, S, red[3], red[7]);
    return M + logf(S);
}

// KL term of one latent: 1 + logvar - mu^2 - exp(logvar); a row's KL divergence is -0.5 times the sum
__device__ __forceinline__ float kl_term(float m, float lv) { return 1.f + lv - m * m - expf(lv); }

// block-wide sum of kl_term over the Z latents of row b of mu, lv [B][Z]: thread tid adds j = tid, tid + 256, ... in that order, then
// block_sum (red: >= 4 floats)
__device__ __forceinline__ float kl_row_sum(const float* mu, const float* lv, int b, int Z, float* red)
{
    float kl = 0.f;
    for (int j = threadIdx.x; j < Z; j += 256) kl += kl_term(mu[(size_t)b * Z + j], lv[(size_t)b * Z + j]);
    return block_sum(kl, red);
}

// a chunk's share (cn columns from Drow) of a padding row b >= B: zeros
template <typename T>
__device__ __forceinline__ void zero_chunk(T* Drow, int cn)
{
    for (int i = threadIdx.x * 4; i < cn; i += 256 * 4) store4<T>(Drow + i, 0.f, 0.f, 0.f, 0.f);
}

// the dense image in LDS of columns [c0, c0 + cn) of batch row b's target: zeros, barrier, the row's stored entries of
// [c0, c0 + cn) and [0, I) scattered in (as k_gather does for the input), barrier -- so that the pass over Y is purely streaming
__device__ __forceinline__ void target_image(float* timg, const RtxCsrView& target, int b, int c0, int cn, int I)
{
    const int tid = threadIdx.x;
    const int64_t u = csr_row(target, b);
    const int64_t tb = target.indptr[u], te = target.indptr[u + 1];
    for (int i = tid * 4; i < cn; i += 256 * 4) *(float4*)(timg + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int64_t k = tb + tid; k < te; k += 256) {
        const int i = target.indices[k];
        if (i >= c0 && i < c0 + cn && i < I) timg[i - c0] = target.values ? target.values[k] : 1.f;
    }
    __syncthreads();
}

// block-wide logsumexp of row y[0..I) (y 16-byte aligned); scratch: >= 8 floats
__device__ float block_lse(const float* y, int I, float* red)
{
    const int tid = threadIdx.x;
    float m = -INFINITY, s = 0.f;
    const int I4 = I & ~3;
    for (int i = tid * 4; i < I4; i += 256 * 4) {
        const float4 t = *(const float4*)(y + i);
        online_add(m, s, t.x); online_add(m, s, t.y); online_add(m, s, t.z); online_add(m, s, t.w);
    }
    for (int i = I4 + tid; i < I; i += 256) online_add(m, s, y[i]);
    return block_lse_merge<true>(m, s, red);
}

// `mailbox` (optional): three 32-bit words of COHERENT HOST memory, {loss, ticket, tag}: the loss and the caller's tag (the step
// count), then -- released at system scope -- the engine's ticket of this reduction (monotonic over the engine's life, so a step
// counter that restarts or repeats can never match a stale entry).  A host that wants THIS step's loss (the reference's
// `return loss.item()`) spins on the ticket word instead of draining the stream (rtx_engine_wait_loss).
__global__ __launch_bounds__(256) void k_reduce_loss(const float* row_loss, int B, float lam, const float* sumsq, int nt,
                                                     float* loss_out, float* loss_accum, uint32_t* mailbox, uint32_t seq, uint32_t tag)
{
    __shared__ float red[4];
    // fixed summation order -> bit-reproducible loss for a given batch
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) s += row_loss[b];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        if (sumsq)
            for (int t = 0; t < nt; ++t) s += lam * sqrtf(sumsq[t]);
        if (loss_out) loss_out[0] = s;
        if (loss_accum) loss_accum[0] += s;
        if (mailbox) {
            __hip_atomic_store(mailbox, __float_as_uint(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(mailbox + 2, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(mailbox + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

int rtx_launch_reduce_loss(const float* row_loss, int B, float lam, const float* sumsq, int n_tensors, float* loss_out,
                           float* loss_accum, hipStream_t stream, uint32_t* mailbox, uint32_t seq, uint32_t tag)
{
    hipLaunchKernelGGL(k_reduce_loss, dim3(1), dim3(256), 0, stream, row_loss, B, lam, sumsq, n_tensors, loss_out, loss_accum, mailbox, seq, tag);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Loss and its gradient w.r.t. the logits, one pass over Y.  One workgroup per (user, 4096-column chunk):
//   lse_b       = logsumexp(Y_b)            from the strip partials of the logits GEMM (or from k_row_lse)
//   D[b][i]     = (s_b * exp(Y_bi - lse_b) - t_bi) * inv_batch         (reference models.py:813-815 through autograd)
//   row_part[b][c] = -<t_b, Y_b>_chunk * inv_batch   (+ s_b * lse_b * inv_batch + beta * KL_b * inv_batch in chunk 0)
// The target row is sparse: its stored entries are scattered into an LDS image of the chunk (as k_gather does for the
// input), so the pass over Y is purely streaming: 16-byte loads of Y, 8 / 16-byte stores of D.  The loss is the
// fixed-order sum of row_part (k_reduce_loss).  Replaces round 1's k_lse_loss + dlogits post kernel (which also wrote D
// transposed) + k_target_fixup.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_row_lse(const float* Y, int ldy, int I, float* lse)
{
    __shared__ float red[8];
    const float v = block_lse(Y + (size_t)blockIdx.x * ldy, I, red);
    if (threadIdx.x == 0) lse[blockIdx.x] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void k_dlogits(const RtxDlogitsArgs a)
{
    __shared__ __attribute__((aligned(16))) float timg[RTX_GATHER_CHUNK];
    __shared__ float red[8];
    const RtxLossArgs& L = a.loss;
    const int b = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const int c0 = chunk * RTX_GATHER_CHUNK;
    const int cn = min(RTX_GATHER_CHUNK, a.ldd - c0);
    T* Drow = (T*)a.D + (size_t)b * a.ldd + c0;
    if (b >= L.B) {
        zero_chunk<T>(Drow, cn);
        return;
    }
    const float* y = L.Y + (size_t)b * L.ldy + c0;
    float lse;
    if (L.part) {
        float m = -INFINITY, s = 0.f;
        for (int k = tid; k < L.n_strips; k += 256) {
            const float2 pr = L.part[(size_t)b * L.part_ld + k];
            online_merge(m, s, pr.x, pr.y);
        }
        lse = block_lse_merge<false>(m, s, red);
    } else {
        lse = L.lse[b];     // k_row_lse ran first
    }
    const float sc = L.tsum[b] * L.inv_batch;
    target_image(timg, L.target, b, c0, cn, L.I);
    float dot = 0.f;
    if (sizeof(T) == 2 && a.Y16) {
        // half-precision logits, possibly in place (Y16 == D): 8 elements = 16 bytes in, 16 bytes out per thread and pass
        typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
        const _Float16* y16 = (const _Float16*)a.Y16 + (size_t)b * a.ldd + c0;
#pragma unroll 2
        for (int i = tid * 8; i < cn; i += 256 * 8) {
            const int col = c0 + i;
            const f16x8_t yy = *(const f16x8_t*)(y16 + i);
            const float4 t0 = *(const float4*)(timg + i), t1 = *(const float4*)(timg + i + 4);
            const float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
            float d[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool valid = col + e < L.I;
                const float yv = (float)yy[e];
                d[e] = valid ? sc * __expf(yv - lse) - tv[e] * L.inv_batch : 0.f;
                if (valid) dot += tv[e] * yv;
            }
            uint4 o;
            o.x = pack_bf16x2(d[0], d[1]);
            o.y = pack_bf16x2(d[2], d[3]);
            o.z = pack_bf16x2(d[4], d[5]);
            o.w = pack_bf16x2(d[6], d[7]);
            *(uint4*)((bf16_t*)Drow + i) = o;
        }
    } else
#pragma unroll 4
    for (int i = tid * 4; i < cn; i += 256 * 4) {
        const int col = c0 + i;
        float4 yy = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < L.ldy) yy = *(const float4*)(y + i);   // ldy is a multiple of 4: a group is inside the row or past it
        const float4 tt = *(const float4*)(timg + i);
        const float yv[4] = {yy.x, yy.y, yy.z, yy.w}, tv[4] = {tt.x, tt.y, tt.z, tt.w};
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool valid = col + e < L.I;
            d[e] = valid ? sc * __expf(yv[e] - lse) - tv[e] * L.inv_batch : 0.f;
            if (valid) dot += tv[e] * yv[e];
        }
        store4<T>(Drow + i, d[0], d[1], d[2], d[3]);
    }
    dot = block_sum(dot, red);
    float kl = 0.f;
    if (chunk == 0 && L.mu32) kl = kl_row_sum(L.mu32, L.lv32, b, L.Z, red);
    if (tid == 0) {
        float part = -dot * L.inv_batch;
        if (chunk == 0) {
            if (L.part) L.lse[b] = lse;
            part += L.tsum[b] * lse * L.inv_batch + L.beta * (-0.5f * kl) * L.inv_batch;
        }
        L.row_loss[(size_t)b * gridDim.y + chunk] = part;
    }
}

// The same, ONE WORKGROUP PER USER ROW (round 5; the training step's half-precision logits in place, D == Y16).  The chunked kernel
// above runs 5 workgroups per user; each re-merges the row's 316 strip partials, zeroes and fills a 16-KB target image in LDS, and
// the 2560 of them need 1.25 rounds of the chip: 16.4 us for 41 MB.  Here a row's logits (NV 16-byte loads per thread) leave for
// the registers in ONE burst at kernel entry and stay there; the partials are merged once per row; the target needs no dense image:
// its <= RTX_DLR_CAP stored entries are read (logit still in place), corrected and parked in LDS, the dense pass writes every element
// from the registers, and behind a barrier the corrected entries overwrite theirs.  512 workgroups, all resident, one round.
#define RTX_DLR_CAP 4096
template <int NV>
__global__ __launch_bounds__(256) void k_dlogits_row(const RtxDlogitsArgs a)
{
    typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
    __shared__ float red[8];
    __shared__ int32_t t_idx[RTX_DLR_CAP];
    __shared__ float t_val[RTX_DLR_CAP];
    const RtxLossArgs& L = a.loss;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n8 = a.ldd >> 3;
    // gridDim.y workgroups share a row: this one owns the 16-byte groups [j0, j1) (<= NV * 256 of them) = columns [8 j0, 8 j1)
    const int S = gridDim.y, part_y = blockIdx.y;
    const int j0 = (int)((long)n8 * part_y / S), j1 = (int)((long)n8 * (part_y + 1) / S);
    bf16_t* Drow = (bf16_t*)a.D + (size_t)b * a.ldd;
    if (b >= L.B) {
        for (int j = j0 + tid; j < j1; j += 256) *(uint4*)(Drow + (size_t)j * 8) = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    // (1) the row's logits: every load in flight before anything else -- behind the one load the longest dependent chain starts
    //     with (row number -> row bounds -> stored entries -> their logits: four round trips, all of them under the merge below)
    const int64_t uu = csr_row(L.target, b);
    const _Float16* y16 = (const _Float16*)a.Y16 + (size_t)b * a.ldd;
    f16x8_t yy[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) yy[u] = *(const f16x8_t*)(y16 + (size_t)min(j0 + tid + u * 256, n8 - 1) * 8);
    // (round 6) everything the tail of this kernel needs -- the row's target sum, the first 256 latent means / log-variances of the KL
    // term -- is requested here too: loaded where it is used, each was one more dependent round trip at the very end of the kernel
    const float tsum_b = L.tsum[b];
    float kl_m0 = 0.f, kl_lv0 = 0.f;
    const bool kl_here = L.mu32 && part_y == 0;
    if (kl_here && tid < L.Z) { kl_m0 = L.mu32[(size_t)b * L.Z + tid]; kl_lv0 = L.lv32[(size_t)b * L.Z + tid]; }
    float2 pr0 = make_float2(-INFINITY, 0.f), pr1 = make_float2(-INFINITY, 0.f);     // this thread's strip partials (n_strips <= 512 here)
    if (tid < L.n_strips) pr0 = L.part[(size_t)b * L.part_ld + tid];
    if (tid + 256 < L.n_strips) pr1 = L.part[(size_t)b * L.part_ld + tid + 256];
    const int64_t tb = L.target.indptr[uu], te = L.target.indptr[uu + 1];
    const int nt = (int)min((int64_t)RTX_DLR_CAP, te - tb);       // (the launcher checked the matrix's longest row)
    // the first 256 stored entries (nearly every row has fewer): index, value and logit, requested before the log-sum-exp exists
    int i0 = -1;
    float tv0 = 0.f, yv0 = 0.f;
    if (tid < nt) {
        const int i = L.target.indices[tb + tid];
        if (i < L.I && i >= 8 * j0 && i < 8 * j1) {      // (the entries of this workgroup's columns)
            i0 = i;
            tv0 = L.target.values ? L.target.values[tb + tid] : 1.f;
            yv0 = (float)y16[i];
        }
    }
    // (2) log-sum-exp of the row from the strip partials of the logits product
    float lse;
    {
        float m = pr0.x, s = pr0.y;
        online_merge(m, s, pr1.x, pr1.y);
        for (int k = tid + 512; k < L.n_strips; k += 256) {       // (rows of more than 32 768 items)
            const float2 pr = L.part[(size_t)b * L.part_ld + k];
            online_merge(m, s, pr.x, pr.y);
        }
        lse = block_lse_merge<false>(m, s, red);
        __syncthreads();          // (red is reused by the sums below)
    }
    const float sc = tsum_b * L.inv_batch;
    // (3) the target's stored entries, while their logits are still in place: <t, y>, and the corrected gradient parked in LDS
    float dot = 0.f;
    if (tid < nt) {               // the entries requested at kernel entry
        t_idx[tid] = i0;
        t_val[tid] = i0 >= 0 ? sc * __expf(yv0 - lse) - tv0 * L.inv_batch : 0.f;
        dot += tv0 * yv0;
    }
    for (int k = tid + 256; k < nt; k += 256) {
        const int i = L.target.indices[tb + k];
        int idx = -1;
        float d = 0.f;
        if (i < L.I && i >= 8 * j0 && i < 8 * j1) {
            const float tv = L.target.values ? L.target.values[tb + k] : 1.f;
            const float yv = (float)y16[i];
            dot += tv * yv;
            d = sc * __expf(yv - lse) - tv * L.inv_batch;
            idx = i;
        }
        t_idx[k] = idx;
        t_val[k] = d;
    }
    __syncthreads();              // every target logit of these columns has been read: they may be overwritten now
    // (4) the dense pass, from the registers: 16 bytes out per thread and load
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int j = j0 + tid + u * 256;
        if (j < j1) {
            const int col = j * 8;
            float d[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = (col + e < L.I) ? sc * __expf((float)yy[u][e] - lse) : 0.f;
            uint4 o;
            o.x = pack_bf16x2(d[0], d[1]);
            o.y = pack_bf16x2(d[2], d[3]);
            o.z = pack_bf16x2(d[4], d[5]);
            o.w = pack_bf16x2(d[6], d[7]);
            *(uint4*)(Drow + (size_t)col) = o;
        }
    }
    // (5) the stored entries' values replace what the dense pass wrote there (same workgroup: release, barrier, then the scatter)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    for (int k = tid; k < nt; k += 256)
        if (t_idx[k] >= 0) Drow[t_idx[k]] = f32_to_bf16(t_val[k]);
    // (6) row loss: -<t, y> / B + s lse / B + beta KL / B, all in partial 0 of the row (the others are zero)
    dot = block_sum(dot, red);
    float kl = 0.f;
    if (kl_here) {
        if (tid < L.Z) kl += kl_term(kl_m0, kl_lv0);
        for (int j = tid + 256; j < L.Z; j += 256) kl += kl_term(L.mu32[(size_t)b * L.Z + j], L.lv32[(size_t)b * L.Z + j]);
        kl = block_sum(kl, red);
    }
    // partial `part_y` of the row: this workgroup's share of -<t, y> / B; partial 0 also carries s lse / B + beta KL / B; the row's
    // remaining partials (the chunked kernel writes rtx_dlogits_chunks of them, and the loss sum reads them all) are zero
    const int chunks = (a.ldd + RTX_GATHER_CHUNK - 1) / RTX_GATHER_CHUNK;
    if (tid == 0) {
        float part = -dot * L.inv_batch;
        if (part_y == 0) {
            L.lse[b] = lse;
            part += tsum_b * lse * L.inv_batch + L.beta * (-0.5f * kl) * L.inv_batch;
        }
        L.row_loss[(size_t)b * chunks + part_y] = part;
    } else if (part_y == 0 && tid >= S && tid < chunks) {
        L.row_loss[(size_t)b * chunks + tid] = 0.f;
    }
}

int rtx_dlogits_chunks(int ldd) { return (ldd + RTX_GATHER_CHUNK - 1) / RTX_GATHER_CHUNK; }

// What the launchers of the chunked kernels share, in two steps, because rtx_launch_dlogits has its log-sum-exp pass and its row
// route between them.  First the check of the leading dimensions (`name` prefixes the error text):
static int check_chunked(const char* name, const RtxDlogitsArgs& a)
{
    RTX_CHECK(a.loss.ldy % 4 == 0 && a.ldd % 8 == 0 && a.ldd >= a.loss.I, RTX_EINVAL, "%s: bad leading dimensions", name);
    return RTX_OK;
}
// then the launch on the grid of one workgroup per (row of the padded batch, 4096-column chunk): the multinomial kernel, or the
// element-wise one with its inv_elems
static int launch_chunked(void (*kernel)(const RtxDlogitsArgs), const RtxDlogitsArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(kernel, dim3(a.Bp, rtx_dlogits_chunks(a.ldd)), dim3(256), 0, stream, a);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
static int launch_chunked(void (*kernel)(const RtxDlogitsArgs, float), const RtxDlogitsArgs& a, float inv_elems, hipStream_t stream)
{
    hipLaunchKernelGGL(kernel, dim3(a.Bp, rtx_dlogits_chunks(a.ldd)), dim3(256), 0, stream, a, inv_elems);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// a.loss.row_loss receives B * rtx_dlogits_chunks(a.ldd) partial sums (row-major [B][chunks]): sum them with
// rtx_launch_reduce_loss(row_loss, B * chunks, ...)
int rtx_launch_dlogits(const RtxDlogitsArgs& a, int is_bf16, hipStream_t stream)
{
    if (a.Bp <= 0) return RTX_OK;
    RTX_TRY(check_chunked("dlogits", a));
    RTX_CHECK(!a.Y16 || (is_bf16 && a.loss.part && (((uintptr_t)a.Y16 | (uintptr_t)a.D) & 15) == 0), RTX_EINVAL,
              "dlogits: half-precision logits need bf16 deltas, the log-sum-exp partials of the logits product and 16-byte aligned images");
    if (!a.loss.part && a.loss.B > 0) {
        hipLaunchKernelGGL(k_row_lse, dim3(a.loss.B), dim3(256), 0, stream, a.loss.Y, a.loss.ldy, a.loss.I, a.loss.lse);
        RTX_HIP(hipGetLastError());
    }
    // the training step's in-place half logits: one workgroup per row (k_dlogits_row) when the row fits its registers (<= 20 480
    // columns) and the target matrix's longest row its LDS list
    if (is_bf16 && a.Y16 && a.loss.part && a.ldd <= 20 * 1024 && a.loss.target.max_row_len > 0 &&
        a.loss.target.max_row_len <= RTX_DLR_CAP && rtx_dlogits_chunks(a.ldd) <= 256) {
        // NV = 5 loads x 256 threads x 8 columns = 10 240 columns per workgroup: two workgroups share a longer row
        const int S = std::min(rtx_dlogits_chunks(a.ldd), (a.ldd + 10239) / 10240);
        hipLaunchKernelGGL(k_dlogits_row<5>, dim3(a.Bp, S), dim3(256), 0, stream, a);
        RTX_HIP(hipGetLastError());
        return RTX_OK;
    }
    return launch_chunked(is_bf16 ? k_dlogits<bf16_t> : k_dlogits<float>, a, stream);
}

// ------------------------------------------------------------------------------------------------
// The element-wise losses and d loss / d logits, in one pass over Y: k_elem_dlogits over a loss policy.  One workgroup per (user,
// 4096-column chunk), the layout of k_dlogits: the target row's stored entries are scattered into an LDS image of the chunk, then
// Y streams through in 16-byte loads and D leaves in 8- (bf16) or 16-byte (f32) stores.  The row's partial sums are block sums in
// a fixed order; k_reduce_loss adds them in a fixed order: a deterministic loss.
//
// BceKlLoss -- VAE_net (RTX_GVAE): binary cross-entropy on the sigmoid of the logits + KL.  Every element is float32 arithmetic as
// torch does it on the reference's path: p = sigmoid(y) rounded to float (so p == 1.0 for y > ~16.6, where the -100 clamp of
// log1p(-p) applies and p (1 - p) == 0 gives a zero gradient), the element loss of F.binary_cross_entropy, and the two backward
// formulas of autograd (binary_cross_entropy_backward, then sigmoid_backward).
//
// MseLoss -- AETrainer(MultiDAE_net) (RTX_AE): torch.nn.MSELoss on the raw outputs against the target rows as stored.  Per element
// e = y - t, loss += e e, d = (2 / (B I)) e: mse_loss and its autograd backward w.r.t. the prediction, in float32.  A pure stream
// (Y in, D out), no KL term.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bce_sigmoid(float y) { return 1.f / (1.f + expf(-y)); }

// element loss (x - 1) max(log1p(-p), -100) - x max(log p, -100); log p only where the target is not zero (rare)
__device__ __forceinline__ float bce_elem_loss(float p, float x)
{
    const float l1p = fmaxf(log1pf(-p), -100.f);
    if (x == 0.f) return -l1p;
    return (x - 1.f) * l1p - x * fmaxf(logf(p), -100.f);
}

// d loss / d logit: (p - x) / max(p (1 - p), 1e-12) / n, then times p (1 - p)
__device__ __forceinline__ float bce_elem_grad(float p, float x, float inv_elems)
{
    const float s = p * (1.f - p);
    return (p - x) / fmaxf(s, 1e-12f) * inv_elems * s;
}

// A loss policy: built in the kernel from inv_elems = 1 / (B I) (not a kernel argument of its own: the kernarg layout is the one
// both losses had as kernels of their own, and passed as an argument the BCE policy cost two SGPRs); elem() adds one element's
// term to `loss` and returns d loss / d logit; KL: chunk 0 of a row adds beta KL_b / B.
struct BceKlLoss {
    static constexpr bool KL = true;
    float inv_elems;
    __device__ __forceinline__ explicit BceKlLoss(float inv_elems_) : inv_elems(inv_elems_) {}
    __device__ __forceinline__ float elem(float y, float t, float& loss) const
    {
        const float p = bce_sigmoid(y);
        loss += bce_elem_loss(p, t);
        return bce_elem_grad(p, t, inv_elems);
    }
};
struct MseLoss {
    static constexpr bool KL = false;
    float g;      // 2 / (B I)
    __device__ __forceinline__ explicit MseLoss(float inv_elems) : g(2.f * inv_elems) {}
    __device__ __forceinline__ float elem(float y, float t, float& loss) const
    {
        const float err = y - t;
        loss += err * err;
        return g * err;
    }
};

template <typename T, typename Loss>
__global__ __launch_bounds__(256) void k_elem_dlogits(const RtxDlogitsArgs a, float inv_elems)
{
    __shared__ __attribute__((aligned(16))) float timg[RTX_GATHER_CHUNK];
    __shared__ float red[4];
    const RtxLossArgs& L = a.loss;
    const int b = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const int c0 = chunk * RTX_GATHER_CHUNK;
    const int cn = min(RTX_GATHER_CHUNK, a.ldd - c0);
    T* Drow = (T*)a.D + (size_t)b * a.ldd + c0;
    if (b >= L.B) {
        zero_chunk<T>(Drow, cn);
        return;
    }
    const float* y = L.Y + (size_t)b * L.ldy + c0;
    target_image(timg, L.target, b, c0, cn, L.I);
    const Loss policy(inv_elems);
    float loss = 0.f;
#pragma unroll 4
    for (int i = tid * 4; i < cn; i += 256 * 4) {
        const int col = c0 + i;
        float4 yy = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < L.ldy) yy = *(const float4*)(y + i);   // ldy is a multiple of 4: a group is inside the row or past it
        const float4 tt = *(const float4*)(timg + i);
        const float yv[4] = {yy.x, yy.y, yy.z, yy.w}, tv[4] = {tt.x, tt.y, tt.z, tt.w};
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            d[e] = 0.f;
            if (col + e < L.I) d[e] = policy.elem(yv[e], tv[e], loss);
        }
        store4<T>(Drow + i, d[0], d[1], d[2], d[3]);
    }
    loss = block_sum(loss, red);
    float kl = 0.f;
    if (Loss::KL && chunk == 0 && L.mu32) kl = kl_row_sum(L.mu32, L.lv32, b, L.Z, red);
    if (tid == 0) {
        float part = loss * inv_elems;
        if (Loss::KL && chunk == 0) part += L.beta * (-0.5f * kl) * L.inv_batch;
        L.row_loss[(size_t)b * gridDim.y + chunk] = part;
    }
}

template <typename Loss>
static int launch_elem_dlogits(const char* name, const RtxDlogitsArgs& a, float inv_elems, int is_bf16, hipStream_t stream)
{
    if (a.Bp <= 0) return RTX_OK;
    RTX_TRY(check_chunked(name, a));
    RTX_CHECK(a.loss.ldy >= a.loss.I, RTX_EINVAL, "%s: bad leading dimensions", name);     // (these kernels read a.loss.Y only)
    RTX_CHECK(!a.Y16, RTX_EINVAL, "%s: reads the float32 logits only", name);
    return launch_chunked(is_bf16 ? k_elem_dlogits<bf16_t, Loss> : k_elem_dlogits<float, Loss>, a, inv_elems, stream);
}

int rtx_launch_bce_dlogits(const RtxDlogitsArgs& a, float inv_elems, int is_bf16, hipStream_t stream)
{
    return launch_elem_dlogits<BceKlLoss>("bce_dlogits", a, inv_elems, is_bf16, stream);
}

int rtx_launch_mse_dlogits(const RtxDlogitsArgs& a, float inv_elems, int is_bf16, hipStream_t stream)
{
    return launch_elem_dlogits<MseLoss>("mse_dlogits", a, inv_elems, is_bf16, stream);
}

// ------------------------------------------------------------------------------------------------
// d loss / d output from OUTSIDE the engine (rtx_engine_backward: the loss was computed by the caller on the outputs of
// rtx_engine_forward_train) into the last layer's D, with the layout contract of the kernels above.  A pure stream on their grid --
// one workgroup per (row of the padded batch, 4096-column chunk), padding rows through zero_chunk: 16 bytes of D per lane and pass
// (8 bf16 or 4 float32 columns) from 16-byte loads of g (and of Y for the sigmoid form).  A caller's [B][n_items] tensor has rows of
// any alignment: without G_VEC, and in a group that reaches past column I, g is read element by element.
//   SIGMOID == false:  D = g                 RTX_VAE, RTX_DAE, RTX_AE: the public output is the logits
//   SIGMOID == true:   D = (g (1 - p)) p     RTX_GVAE: the public output is p = sigmoid(y); torch's sigmoid_backward on bce_sigmoid's p,
//                                            so p == 1.0 (y > ~16.6) gives an exact zero and no logit gives a NaN
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store16(float* dst, const float* d) { store4<float>(dst, d[0], d[1], d[2], d[3]); }
__device__ __forceinline__ void store16(bf16_t* dst, const float* d)
{
    uint4 o;
    o.x = pack_bf16x2(d[0], d[1]);
    o.y = pack_bf16x2(d[2], d[3]);
    o.z = pack_bf16x2(d[4], d[5]);
    o.w = pack_bf16x2(d[6], d[7]);
    *(uint4*)dst = o;
}

template <typename T, bool SIGMOID, bool G_VEC>
__global__ __launch_bounds__(256) void k_import_dout(const RtxDlogitsArgs a, const float* __restrict__ G, long ldg)
{
    constexpr int V = 16 / (int)sizeof(T);
    const RtxLossArgs& L = a.loss;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int c0 = blockIdx.y * RTX_GATHER_CHUNK;
    const int cn = min(RTX_GATHER_CHUNK, a.ldd - c0);
    T* Drow = (T*)a.D + (size_t)b * a.ldd + c0;
    if (b >= L.B) {
        zero_chunk<T>(Drow, cn);
        return;
    }
    const float* g = G + (size_t)b * ldg + c0;
    const float* y = SIGMOID ? L.Y + (size_t)b * L.ldy + c0 : nullptr;
#pragma unroll 2
    for (int i = tid * V; i < cn; i += 256 * V) {     // (cn is a multiple of 8: ldd and the chunk are)
        float d[V];
#pragma unroll
        for (int q = 0; q < V; q += 4) {
            const int col = c0 + i + q;
            float gv[4] = {0.f, 0.f, 0.f, 0.f};
            if (G_VEC && col + 3 < L.I) {
                const float4 gg = *(const float4*)(g + i + q);
                gv[0] = gg.x; gv[1] = gg.y; gv[2] = gg.z; gv[3] = gg.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < L.I) gv[e] = g[i + q + e];
            }
            if (SIGMOID) {
                float4 yy = make_float4(0.f, 0.f, 0.f, 0.f);
                if (col < L.ldy) yy = *(const float4*)(y + i + q);   // ldy is a multiple of 4: a group is inside the row or past it
                const float yv[4] = {yy.x, yy.y, yy.z, yy.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = bce_sigmoid(yv[e]);
                    gv[e] = (col + e < L.I) ? (gv[e] * (1.f - p)) * p : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) d[q + e] = gv[e];
        }
        store16(Drow + i, d);
    }
}

template <typename T>
static int launch_import_dout(const RtxDlogitsArgs& a, const float* g, long ld, int sigmoid, hipStream_t stream)
{
    const dim3 grid(a.Bp, rtx_dlogits_chunks(a.ldd)), block(256);
    const bool vec = (((uintptr_t)g | (uintptr_t)(ld * sizeof(float))) & 15) == 0;
    if (sigmoid) {
        if (vec) hipLaunchKernelGGL((k_import_dout<T, true, true>), grid, block, 0, stream, a, g, ld);
        else hipLaunchKernelGGL((k_import_dout<T, true, false>), grid, block, 0, stream, a, g, ld);
    } else {
        if (vec) hipLaunchKernelGGL((k_import_dout<T, false, true>), grid, block, 0, stream, a, g, ld);
        else hipLaunchKernelGGL((k_import_dout<T, false, false>), grid, block, 0, stream, a, g, ld);
    }
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

int rtx_launch_import_dout(const RtxDlogitsArgs& a, const float* g, long ld, int sigmoid, int is_bf16, hipStream_t stream)
{
    if (a.Bp <= 0) return RTX_OK;
    RTX_TRY(check_chunked("import_dout", a));
    RTX_CHECK(g && a.D && ((uintptr_t)a.D & 15) == 0 && a.loss.B >= 0 && a.loss.B <= a.Bp && ld >= a.loss.I, RTX_EINVAL,
              "import_dout: bad arguments (B %d of %d rows, row stride %ld for %d columns)", a.loss.B, a.Bp, ld, a.loss.I);
    RTX_CHECK(!sigmoid || (a.loss.Y && a.loss.ldy >= a.loss.I && ((uintptr_t)a.loss.Y & 15) == 0), RTX_EINVAL,
              "import_dout: the sigmoid form reads the float32 logits");
    return is_bf16 ? launch_import_dout<bf16_t>(a, g, ld, sigmoid, stream) : launch_import_dout<float>(a, g, ld, sigmoid, stream);
}

__global__ __launch_bounds__(256) void k_sigmoid_rows(float* logits, long ld, int n_items)
{
    float* row = logits + (size_t)blockIdx.x * ld;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n_items; i += gridDim.y * 256) row[i] = bce_sigmoid(row[i]);
}

int rtx_launch_sigmoid_rows(float* logits, int B, long ld, int n_items, hipStream_t stream)
{
    if (B <= 0 || n_items <= 0) return RTX_OK;
    const int gy = std::min(16, (n_items + 1023) / 1024);
    hipLaunchKernelGGL(k_sigmoid_rows, dim3(B, gy), dim3(256), 0, stream, logits, ld, n_items);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// VAE.loss_function on dense tensors; P holds PROBABILITIES (the sigmoid outputs), where the chunked kernel takes logits: a kernel
// of its own, not an instance of the policy above
__global__ __launch_bounds__(256) void k_dense_bce_kl(const float* P, const float* X, int I, const float* mu, const float* lv, int Z,
                                                      float inv_elems, float inv_batch, float* row_loss)
{
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* p = P + (size_t)b * I;
    const float* x = X + (size_t)b * I;
    float loss = 0.f;
    for (int i = tid; i < I; i += 256) loss += bce_elem_loss(p[i], x[i]);   // rows of a [B][I] tensor: any alignment
    loss = block_sum(loss, red);
    float kl = 0.f;
    if (mu) kl = kl_row_sum(mu, lv, b, Z, red);
    if (tid == 0) row_loss[b] = loss * inv_elems + (-0.5f * kl) * inv_batch;
}

int rtx_launch_dense_bce_kl(const float* P, const float* X, int B, int I, const float* mu, const float* lv, int Z, float inv_elems,
                            float inv_batch, float* row_loss, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    hipLaunchKernelGGL(k_dense_bce_kl, dim3(B), dim3(256), 0, stream, P, X, I, mu, lv, Z, inv_elems, inv_batch, row_loss);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// AETrainer.loss_function on dense tensors: row_loss[b] = sum_i (x_bi - y_bi)^2 * inv_elems
__global__ __launch_bounds__(256) void k_dense_mse(const float* Y, const float* X, int I, float inv_elems, float* row_loss)
{
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* y = Y + (size_t)b * I;
    const float* x = X + (size_t)b * I;
    float loss = 0.f;
    for (int i = tid; i < I; i += 256) {   // rows of a [B][I] tensor: any alignment
        const float err = x[i] - y[i];
        loss += err * err;
    }
    loss = block_sum(loss, red);
    if (tid == 0) row_loss[b] = loss * inv_elems;
}

int rtx_launch_dense_mse(const float* Y, const float* X, int B, int I, float inv_elems, float* row_loss, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    hipLaunchKernelGGL(k_dense_mse, dim3(B), dim3(256), 0, stream, Y, X, I, inv_elems, row_loss);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// n_items bounds the masked columns: a conditioned input row carries its condition columns after the items
// (CMultiVAE.predict masks x[:, :-cond_dim].nonzero() only, reference models.py:952-953)
__global__ __launch_bounds__(256) void k_neg_inf(const RtxCsrView v, float* logits, long ld, int n_items)
{
    const int b = blockIdx.x;
    const int64_t u = csr_row(v, b);
    for (int64_t k = v.indptr[u] + threadIdx.x; k < v.indptr[u + 1]; k += 256) {
        const float val = v.values ? v.values[k] : 1.f;
        const int i = v.indices[k];
        if (val != 0.f && i < n_items) logits[(size_t)b * ld + i] = -INFINITY;
    }
}

int rtx_launch_neg_inf(const RtxCsrView& in, int B, float* logits, long ld, int n_items, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    hipLaunchKernelGGL(k_neg_inf, dim3(B), dim3(256), 0, stream, in, logits, ld, n_items);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// loss_function(recon_x, x, mu, logvar, beta) on dense tensors (reference models.py:813-815)
__global__ __launch_bounds__(256) void k_dense_loss(const float* Y, const float* X, int I, const float* mu, const float* lv, int Z,
                                                    float beta, float inv_batch, float* row_loss)
{
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* y = Y + (size_t)b * I;
    const float* x = X + (size_t)b * I;
    // rows of an [B][I] tensor are not 16-byte aligned in general: scalar online pass
    float m = -INFINITY, s = 0.f, dot = 0.f, sx = 0.f;
    for (int i = tid; i < I; i += 256) {
        const float yi = y[i], xi = x[i];
        online_add(m, s, yi);
        dot += xi * yi;
        sx += xi;
    }
    const float lse = block_lse_merge<true>(m, s, red);
    dot = block_sum(dot, red);
    sx = block_sum(sx, red);
    float kl = 0.f;
    if (mu) kl = kl_row_sum(mu, lv, b, Z, red);
    if (tid == 0) row_loss[b] = (sx * lse - dot) * inv_batch + beta * (-0.5f * kl) * inv_batch;
}

int rtx_launch_dense_loss(const float* Y, const float* X, int B, int I, const float* mu, const float* lv, int Z, float beta,
                          float inv_batch, float* row_loss, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    hipLaunchKernelGGL(k_dense_loss, dim3(B), dim3(256), 0, stream, Y, X, I, mu, lv, Z, beta, inv_batch, row_loss);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// ------------------------------------------------------------------------------------------------
// The dense loss functions WITH their gradients (rtx_*_loss_grad: the backward of the public loss operators).  One workgroup per row
// of the caller's [B][I] float32 tensors, as the three kernels above; the row loss comes from the SAME operations in the SAME order
// as theirs -- thread tid adds columns tid, tid + 256, ... -- so the value of a differentiable call is the value of the plain one to
// the bit, and two calls on the same data agree to the bit.  All gradients are at unit upstream gradient.
//
// VEC (every base 16-byte aligned and I % 4 == 0, so that every row is): the operands arrive in 16-byte loads, 1024 columns of the row
// at a time, and pass through an LDS tile from which every thread takes ITS columns of the scalar order; the gradient is computed from
// the registers the loads filled and leaves in 16-byte stores.  Otherwise (rows of any alignment, as a [B][I] tensor with odd I has)
// every access is a 4-byte one, a wave's 64 of them one contiguous 256 bytes.
//
// The multinomial gradient needs the row's log-sum-exp first: the same workgroup walks its row twice.  Why not the chunked scheme of
// k_elem_dlogits behind a row pass: that is two launches, and its second one finds the operands exactly where this kernel's second walk
// finds them -- behind the L1, in the XCD's 4-MiB L2 while the rows in flight on the XCD fit it (a row of both operands at 20 108 items
// is 161 KB; an XCD's 32 CUs hold 8 workgroups of this size each), else in the 256-MiB Infinity Cache, which holds the whole operand
// set of any batch this project trains (80 MB at B = 500): no second walk goes to HBM in either scheme, and this one keeps a row's
// target sum, its log-sum-exp and its KL term in the registers of the workgroup that needs them, with no partials through memory.
// ------------------------------------------------------------------------------------------------
#define RTX_LG_TILE 1024      // columns per LDS tile of the VEC route: 256 threads x one 16-byte group

// d KL term / d mu and d logvar of one latent at weight w = beta / B:  w mu  and  w (exp(logvar) - 1) / 2.  expm1f: exp(logvar) - 1
// cancels where logvar is near zero, which is where a trained encoder keeps most of them.
__device__ __forceinline__ void kl_row_grad(const float* mu, const float* lv, int b, int Z, float w, float* dmu, float* dlv)
{
    const float hw = 0.5f * w;
    for (int j = threadIdx.x; j < Z; j += 256) {
        const size_t at = (size_t)b * Z + j;
        dmu[at] = w * mu[at];
        dlv[at] = hw * expm1f(lv[at]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_dense_loss_grad(const float* Y, const float* X, int I, const float* mu, const float* lv, int Z,
                                                         float beta, float inv_batch, float* row_loss, float* dY, float* dmu, float* dlv)
{
    __shared__ float red[8];
    __shared__ __attribute__((aligned(16))) float ty[VEC ? RTX_LG_TILE : 4], tx[VEC ? RTX_LG_TILE : 4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* y = Y + (size_t)b * I;
    const float* x = X + (size_t)b * I;
    float* d = dY + (size_t)b * I;
    // walk 1: k_dense_loss's online pass
    float m = -INFINITY, s = 0.f, dot = 0.f, sx = 0.f;
    if (VEC) {
        for (int base = 0; base < I; base += RTX_LG_TILE) {
            const int i = base + tid * 4;
            float4 yy = make_float4(0.f, 0.f, 0.f, 0.f), xx = yy;
            if (i < I) { yy = *(const float4*)(y + i); xx = *(const float4*)(x + i); }     // I % 4 == 0: a group is inside the row or past it
            *(float4*)(ty + tid * 4) = yy;
            *(float4*)(tx + tid * 4) = xx;
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = tid + 256 * e;
                if (base + k < I) {
                    const float yi = ty[k], xi = tx[k];
                    online_add(m, s, yi);
                    dot += xi * yi;
                    sx += xi;
                }
            }
            __syncthreads();
        }
    } else {
        for (int i = tid; i < I; i += 256) {
            const float yi = y[i], xi = x[i];
            online_add(m, s, yi);
            dot += xi * yi;
            sx += xi;
        }
    }
    const float lse = block_lse_merge<true>(m, s, red);
    dot = block_sum(dot, red);
    sx = block_sum(sx, red);
    float kl = 0.f;
    if (mu) kl = kl_row_sum(mu, lv, b, Z, red);
    if (tid == 0) row_loss[b] = (sx * lse - dot) * inv_batch + beta * (-0.5f * kl) * inv_batch;
    // walk 2: d = (s_b softmax(y)_i - x_i) / B, k_dlogits's expression; a row without a target has sc == 0 and gets zeros
    const float sc = sx * inv_batch;
    if (VEC) {
#pragma unroll 2
        for (int i = tid * 4; i < I; i += 256 * 4) {
            const float4 yy = *(const float4*)(y + i), xx = *(const float4*)(x + i);
            store4<float>(d + i, sc * __expf(yy.x - lse) - xx.x * inv_batch, sc * __expf(yy.y - lse) - xx.y * inv_batch,
                          sc * __expf(yy.z - lse) - xx.z * inv_batch, sc * __expf(yy.w - lse) - xx.w * inv_batch);
        }
    } else {
        for (int i = tid; i < I; i += 256) d[i] = sc * __expf(y[i] - lse) - x[i] * inv_batch;
    }
    if (mu) kl_row_grad(mu, lv, b, Z, beta * inv_batch, dmu, dlv);
}

static bool rows_vectorizable(const void* a, const void* b, const void* c, int I)
{
    return ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0) && I % 4 == 0;
}

int rtx_launch_dense_loss_grad(const float* Y, const float* X, int B, int I, const float* mu, const float* lv, int Z, float beta,
                               float inv_batch, float* row_loss, float* dY, float* dmu, float* dlv, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    RTX_CHECK(Y && X && row_loss && dY && I >= 1, RTX_EINVAL, "dense_loss_grad: NULL argument");
    RTX_CHECK(!mu || (lv && dmu && dlv && Z >= 1), RTX_EINVAL, "dense_loss_grad: mu without logvar, d_mu or d_logvar");
    if (rows_vectorizable(Y, X, dY, I))
        hipLaunchKernelGGL(k_dense_loss_grad<true>, dim3(B), dim3(256), 0, stream, Y, X, I, mu, lv, Z, beta, inv_batch, row_loss, dY, dmu, dlv);
    else
        hipLaunchKernelGGL(k_dense_loss_grad<false>, dim3(B), dim3(256), 0, stream, Y, X, I, mu, lv, Z, beta, inv_batch, row_loss, dY, dmu, dlv);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// The two element-wise losses: one walk, a policy per loss.  term(): one element's share of the row sum, k_dense_bce_kl's /
// k_dense_mse's expression; grad(): d loss / d a (a: the probabilities p, or the prediction).
struct DenseBceKl {
    static constexpr bool KL = true;
    float inv_elems;
    __device__ __forceinline__ explicit DenseBceKl(float inv_elems_) : inv_elems(inv_elems_) {}
    __device__ __forceinline__ void add(float& loss, float p, float x) const { loss += bce_elem_loss(p, x); }
    // F.binary_cross_entropy's backward: (p - x) / max(p (1 - p), 1e-12) / N -- finite at p == 0 and p == 1
    __device__ __forceinline__ float grad(float p, float x) const { return (p - x) / fmaxf(p * (1.f - p), 1e-12f) * inv_elems; }
};
struct DenseMse {
    static constexpr bool KL = false;
    float g;      // 2 / (B I)
    __device__ __forceinline__ explicit DenseMse(float inv_elems) : g(2.f * inv_elems) {}
    __device__ __forceinline__ void add(float& loss, float y, float x) const
    {
        const float err = x - y;
        loss += err * err;
    }
    __device__ __forceinline__ float grad(float y, float x) const { return g * (y - x); }
};

template <typename Loss, bool VEC>
__global__ __launch_bounds__(256) void k_dense_elem_grad(const float* A, const float* X, int I, const float* mu, const float* lv, int Z,
                                                         float inv_elems, float inv_batch, float* row_loss, float* dA, float* dmu, float* dlv)
{
    __shared__ float red[4];
    __shared__ __attribute__((aligned(16))) float ta[VEC ? RTX_LG_TILE : 4], tx[VEC ? RTX_LG_TILE : 4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* a = A + (size_t)b * I;
    const float* x = X + (size_t)b * I;
    float* d = dA + (size_t)b * I;
    const Loss policy(inv_elems);
    float loss = 0.f;
    if (VEC) {
        for (int base = 0; base < I; base += RTX_LG_TILE) {
            const int i = base + tid * 4;
            float4 aa = make_float4(0.f, 0.f, 0.f, 0.f), xx = aa;
            if (i < I) {      // I % 4 == 0: a group is inside the row or past it
                aa = *(const float4*)(a + i);
                xx = *(const float4*)(x + i);
                store4<float>(d + i, policy.grad(aa.x, xx.x), policy.grad(aa.y, xx.y), policy.grad(aa.z, xx.z), policy.grad(aa.w, xx.w));
            }
            *(float4*)(ta + tid * 4) = aa;
            *(float4*)(tx + tid * 4) = xx;
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = tid + 256 * e;
                if (base + k < I) policy.add(loss, ta[k], tx[k]);
            }
            __syncthreads();
        }
    } else {
        for (int i = tid; i < I; i += 256) {
            const float ai = a[i], xi = x[i];
            policy.add(loss, ai, xi);
            d[i] = policy.grad(ai, xi);
        }
    }
    loss = block_sum(loss, red);
    float kl = 0.f;
    if (Loss::KL && mu) kl = kl_row_sum(mu, lv, b, Z, red);
    if (tid == 0) row_loss[b] = Loss::KL ? loss * inv_elems + (-0.5f * kl) * inv_batch : loss * inv_elems;
    if (Loss::KL && mu) kl_row_grad(mu, lv, b, Z, inv_batch, dmu, dlv);
}

template <typename Loss>
static int launch_dense_elem_grad(const float* A, const float* X, int B, int I, const float* mu, const float* lv, int Z, float inv_elems,
                                  float inv_batch, float* row_loss, float* dA, float* dmu, float* dlv, hipStream_t stream)
{
    if (rows_vectorizable(A, X, dA, I))
        hipLaunchKernelGGL((k_dense_elem_grad<Loss, true>), dim3(B), dim3(256), 0, stream, A, X, I, mu, lv, Z, inv_elems, inv_batch, row_loss, dA, dmu, dlv);
    else
        hipLaunchKernelGGL((k_dense_elem_grad<Loss, false>), dim3(B), dim3(256), 0, stream, A, X, I, mu, lv, Z, inv_elems, inv_batch, row_loss, dA, dmu, dlv);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

int rtx_launch_dense_bce_kl_grad(const float* P, const float* X, int B, int I, const float* mu, const float* lv, int Z, float inv_elems,
                                 float inv_batch, float* row_loss, float* dP, float* dmu, float* dlv, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    RTX_CHECK(P && X && row_loss && dP && I >= 1, RTX_EINVAL, "dense_bce_kl_grad: NULL argument");
    RTX_CHECK(!mu || (lv && dmu && dlv && Z >= 1), RTX_EINVAL, "dense_bce_kl_grad: mu without logvar, d_mu or d_logvar");
    return launch_dense_elem_grad<DenseBceKl>(P, X, B, I, mu, lv, Z, inv_elems, inv_batch, row_loss, dP, dmu, dlv, stream);
}

int rtx_launch_dense_mse_grad(const float* Y, const float* X, int B, int I, float inv_elems, float* row_loss, float* dY, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    RTX_CHECK(Y && X && row_loss && dY && I >= 1, RTX_EINVAL, "dense_mse_grad: NULL argument");
    return launch_dense_elem_grad<DenseMse>(Y, X, B, I, nullptr, nullptr, 0, inv_elems, 0.f, row_loss, dY, nullptr, nullptr, stream);
}

// The squared norms for the gradient below, in a FIXED order: k_sumsq's blocks (one per 4096 elements, at most 1024, the same
// grid-stride walk per thread) leave their block sums in part[t][block] instead of adding them to one word with atomics, and one
// workgroup per tensor folds them (thread tid adds partials tid, tid + 256, ...; block_sum).  Why not k_sumsq itself: its atomic adds
// arrive in any order, so a tensor of many blocks has a norm that differs from call to call, and 257 sequential additions at the
// magnitude of the total lose about 2e-7 of it (one standard deviation, at 2^20 elements) -- as much as the 4 float32 ulps a
// gradient element W / ||W|| is held to.  A tensor of one block (<= 4096 elements) gets k_sumsq's value to the bit.
#define RTX_SUMSQ_BLOCKS 1024
__device__ __forceinline__ int sumsq_blocks(long n)
{
    const long blocks = (n + 256 * 16 - 1) / (256 * 16);
    return (int)(blocks < 1 ? 1 : (blocks > RTX_SUMSQ_BLOCKS ? RTX_SUMSQ_BLOCKS : blocks));
}
__global__ __launch_bounds__(256) void k_sumsq_part(const RtxNormGradArgs a, float* part)
{
    __shared__ float red[4];
    const int t = blockIdx.y, nb = sumsq_blocks(a.n[t]);
    if ((int)blockIdx.x >= nb) return;
    const float* p = a.w[t];
    const long n = a.n[t];
    float s = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)nb * 256) s += p[i] * p[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[(size_t)t * RTX_SUMSQ_BLOCKS + blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_sumsq_fold(const RtxNormGradArgs a, const float* part, float* sumsq)
{
    __shared__ float red[4];
    const int t = blockIdx.x, nb = sumsq_blocks(a.n[t]);
    float s = 0.f;
    for (int k = threadIdx.x; k < nb; k += 256) s += part[(size_t)t * RTX_SUMSQ_BLOCKS + k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) sumsq[t] = s;
}

// d sum_t ||W_t||_2 / d W_t = W_t / ||W_t||_2 from the squared norms in sumsq[t]; zeros where the norm is zero
// (torch's norm backward).  ONE launch for all tensors: blockIdx.y is the tensor, its blocks stride over it; 16-byte accesses where
// both of the tensor's bases allow them, the scalar tail behind them.
__global__ __launch_bounds__(256) void k_norm_grad(const RtxNormGradArgs a, const float* sumsq)
{
    const int t = blockIdx.y;
    const float* w = a.w[t];
    float* g = a.g[t];
    const long n = a.n[t];
    const float nrm = sqrtf(sumsq[t]);
    const bool zero = !(nrm > 0.f);
    const long first = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    long done = 0;
    if ((((uintptr_t)w | (uintptr_t)g) & 15) == 0) {
        const long n4 = n >> 2;
        for (long q = first; q < n4; q += stride) {
            const float4 v = *(const float4*)(w + 4 * q);
            if (zero) store4<float>(g + 4 * q, 0.f, 0.f, 0.f, 0.f);
            else store4<float>(g + 4 * q, v.x / nrm, v.y / nrm, v.z / nrm, v.w / nrm);
        }
        done = n4 << 2;
    }
    for (long i = done + first; i < n; i += stride) g[i] = zero ? 0.f : w[i] / nrm;
}

static int norm_args(const char* name, const float* const* tensors_host, float* const* grads_host, const long* sizes, int n,
                     RtxNormGradArgs* a, long* longest)
{
    RTX_CHECK(tensors_host && sizes && n >= 1 && n <= RTX_MAX_TENSORS, RTX_EINVAL, "%s: bad arguments", name);
    *a = RtxNormGradArgs{};
    *longest = 0;
    for (int t = 0; t < n; ++t) {
        RTX_CHECK(sizes[t] >= 0 && (sizes[t] == 0 || (tensors_host[t] && (!grads_host || grads_host[t]))), RTX_EINVAL,
                  "%s: tensor %d is NULL", name, t);
        a->w[t] = tensors_host[t]; a->g[t] = grads_host ? grads_host[t] : nullptr; a->n[t] = sizes[t];
        *longest = std::max(*longest, sizes[t]);
    }
    return RTX_OK;
}

int rtx_sumsq_ordered_scratch(int n) { return n * RTX_SUMSQ_BLOCKS; }

int rtx_launch_sumsq_ordered(const float* const* tensors_host, const long* sizes, int n, float* sumsq, float* part, hipStream_t stream)
{
    RtxNormGradArgs a;
    long longest;
    RTX_TRY(norm_args("sumsq_ordered", tensors_host, nullptr, sizes, n, &a, &longest));
    RTX_CHECK(sumsq && part, RTX_EINVAL, "sumsq_ordered: NULL output");
    const long blocks = std::max<long>(1, std::min<long>(RTX_SUMSQ_BLOCKS, (longest + 256 * 16 - 1) / (256 * 16)));
    hipLaunchKernelGGL(k_sumsq_part, dim3((unsigned)blocks, n), dim3(256), 0, stream, a, part);
    hipLaunchKernelGGL(k_sumsq_fold, dim3(n), dim3(256), 0, stream, a, part, sumsq);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

int rtx_launch_norm_grad(const float* const* tensors_host, float* const* grads_host, const long* sizes, int n, const float* sumsq,
                         hipStream_t stream)
{
    RtxNormGradArgs a;
    long longest;
    RTX_CHECK(grads_host, RTX_EINVAL, "norm_grad: bad arguments");
    RTX_TRY(norm_args("norm_grad", tensors_host, grads_host, sizes, n, &a, &longest));
    RTX_CHECK(sumsq, RTX_EINVAL, "norm_grad: bad arguments");
    if (longest == 0) return RTX_OK;
    const long blocks = (longest + 256 * 16 - 1) / (256 * 16);      // 16 elements per thread, as k_sumsq
    hipLaunchKernelGGL(k_norm_grad, dim3((unsigned)std::min<long>(1024, blocks), n), dim3(256), 0, stream, a, sumsq);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
