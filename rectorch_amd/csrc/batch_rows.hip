// batch_rows.hip -- batch formation for gfx950: sparse user rows -> the dense, normalised, dropped-out input image (K1: k_gather,
// k_gather_scatter), the DataSampler's dense float32 batch (k_csr_to_dense) and dense -> CSR for callers that hand dense tensors.
#include "batch_rows.h"

// ------------------------------------------------------------------------------------------------
// K1: gather.  One workgroup per (padded) batch row.  The row's stored entries are read coalesced
// from the CSR arrays, normalised (F.normalize), dropped out, scattered into an LDS image of a chunk of
// the dense row, and the chunk is streamed to HBM with 16-byte stores.  Column Iin of a real row is set
// to one: read K-major by the weight-gradient kernel it turns into the bias-gradient column.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_gather(const RtxGatherArgs a)
{
    constexpr int CH = 16384 / sizeof(T);   // elements per 16-KB LDS chunk
    __shared__ __attribute__((aligned(16))) T row[CH];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    T* X = (T*)a.X + (size_t)b * a.ldx;
    if (b >= a.B) {  // padding row of the batch: zeros (it multiplies nothing that is kept)
        for (int i = tid * 4; i < a.ldx; i += 256 * 4) store4<T>(X + i, 0.f, 0.f, 0.f, 0.f);
        if (tid == 0) a.tsum[b] = 0.f;
        return;
    }
    const int64_t u = csr_row(a.in, b);
    const int64_t beg = a.in.indptr[u], end = a.in.indptr[u + 1];
    // the row's norm, target sum and dropout scale: batch_rows.h (shared with k_gather_scatter and k_in_chunks)
    const float ss = row_sumsq<256>(a.in, beg, end, a.I, a.Iin, red);
    const float ts = row_target_sum<256>(a.target, b, a.I, a.Iin, red);
    if (tid == 0) a.tsum[b] = ts;
    const RowScale rs = row_scale(ss, a.raw, a.training, a.dropout_p);
    for (int c0 = 0; c0 < a.ldx; c0 += CH) {
        const int cn = min(CH, a.ldx - c0);
        for (int i = tid * 4; i < cn; i += 256 * 4) store4<T>(row + i, 0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        for (int64_t k = beg + tid; k < end; k += 256) {
            const int i = a.in.indices[k];
            if (i >= c0 && i < c0 + cn) {
                const float v = row_entry(a.in.values ? a.in.values[k] : 1.f, i, b, a.I, rs, a.mask, a.seed, a.offset, a.dropout_p);
                row[i - c0] = Elem<T>::from(v);
            }
        }
        if (tid == 0 && a.Iin >= c0 && a.Iin < c0 + cn) row[a.Iin - c0] = Elem<T>::from(1.f);   // ones column -> bias gradient
        __syncthreads();
        if (sizeof(T) == 2) {
            for (int i = tid * 8; i < cn; i += 256 * 8) *(uint4*)(X + c0 + i) = *(const uint4*)(row + i);
        } else {
            for (int i = tid * 4; i < cn; i += 256 * 4) *(uint4*)(X + c0 + i) = *(const uint4*)(row + i);
        }
        __syncthreads();
    }
}

// The same batch image by SCATTER (RtxGatherArgs::written): one workgroup per row slot clears what the previous launch wrote
// there, then writes this user's stored entries.  Everything k_gather computes (norm, target sum, dropout, ones column) is
// computed the same way; only the zeros are not written again.  Reference: samplers.py:99-100 (.toarray()) + nets.py:395-399.
template <typename T>
__global__ __launch_bounds__(256) void k_gather_scatter(const RtxGatherArgs a)
{
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    T* X = (T*)a.X + (size_t)b * a.ldx;
    int32_t* wr = a.written + (size_t)b * a.written_cap;
    const int n_old = a.n_written[b];
    for (int k = tid; k < n_old; k += 256) X[wr[k]] = Elem<T>::from(0.f);
    __syncthreads();   // (a workgroup-scope fence: the clears are ordered before this launch's writes of the same columns)
    if (b >= a.B) {    // padding row of the batch: all zero, ones column included
        if (tid == 0) { a.n_written[b] = 0; a.tsum[b] = 0.f; }
        return;
    }
    const int64_t u = csr_row(a.in, b);
    const int64_t beg = a.in.indptr[u], end = a.in.indptr[u + 1];
    const float ss = row_sumsq<256>(a.in, beg, end, a.I, a.Iin, red);
    const float ts = row_target_sum<256>(a.target, b, a.I, a.Iin, red);
    if (tid == 0) a.tsum[b] = ts;
    const RowScale rs = row_scale(ss, a.raw, a.training, a.dropout_p);
    const int n = (int)(end - beg);   // < written_cap (the launcher checked the matrix's longest row)
    for (int k = tid; k < n; k += 256) {
        const int i = a.in.indices[beg + k];
        const float v = row_entry(a.in.values ? a.in.values[beg + k] : 1.f, i, b, a.I, rs, a.mask, a.seed, a.offset, a.dropout_p);
        if (i < a.ldx) X[i] = Elem<T>::from(v);
        wr[k] = i < a.ldx ? i : 0;
    }
    if (tid == 0) {
        X[a.Iin] = Elem<T>::from(1.f);   // ones column -> bias gradient
        wr[n] = a.Iin;
        a.n_written[b] = n + 1;
    }
}

int rtx_launch_gather(const RtxGatherArgs& a, int is_bf16, hipStream_t stream)
{
    RTX_CHECK(a.ldx % 8 == 0, RTX_EINVAL, "gather: ldx must be a multiple of 8");
    if (a.written) {
        RTX_CHECK(a.n_written && a.in.max_row_len > 0 && a.in.max_row_len < a.written_cap && a.Iin < a.ldx, RTX_EINVAL,
                  "gather: the scatter form needs the matrix's longest row (%d) below the list capacity (%d)", a.in.max_row_len, a.written_cap);
        if (is_bf16)
            hipLaunchKernelGGL(k_gather_scatter<bf16_t>, dim3(a.Bp), dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL(k_gather_scatter<float>, dim3(a.Bp), dim3(256), 0, stream, a);
        RTX_HIP(hipGetLastError());
        return RTX_OK;
    }
    if (is_bf16)
        hipLaunchKernelGGL(k_gather<bf16_t>, dim3(a.Bp), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(k_gather<float>, dim3(a.Bp), dim3(256), 0, stream, a);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// DataSampler densify (samplers.py:99-105): rows -> float32 [B][I], ld = I (arbitrary alignment)
__global__ __launch_bounds__(256) void k_csr_to_dense(const RtxCsrView v, int I, float* out)
{
    __shared__ float row[RTX_GATHER_CHUNK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t u = csr_row(v, b);
    const int64_t beg = v.indptr[u], end = v.indptr[u + 1];
    float* o = out + (size_t)b * I;
    for (int c0 = 0; c0 < I; c0 += RTX_GATHER_CHUNK) {
        const int cn = min(RTX_GATHER_CHUNK, I - c0);
        for (int i = tid; i < cn; i += 256) row[i] = 0.f;
        __syncthreads();
        for (int64_t k = beg + tid; k < end; k += 256) {
            const int i = v.indices[k];
            if (i >= c0 && i < c0 + cn) row[i - c0] = v.values ? v.values[k] : 1.f;
        }
        __syncthreads();
        for (int i = tid; i < cn; i += 256) o[c0 + i] = row[i];
        __syncthreads();
    }
}

int rtx_launch_csr_to_dense(const RtxCsrView& v, int B, int I, float* out, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    hipLaunchKernelGGL(k_csr_to_dense, dim3(B), dim3(256), 0, stream, v, I, out);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// ------------------------------------------------------------------------------------------------
// dense [B][I] float32 -> CSR (stored entries = non-zeros, column order preserved)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_count(const float* X, int I, int32_t* counts)
{
    __shared__ float red[4];
    const int b = blockIdx.x;
    float c = 0.f;
    for (int i = threadIdx.x; i < I; i += 256) c += (X[(size_t)b * I + i] != 0.f) ? 1.f : 0.f;
    c = block_sum(c, red);
    if (threadIdx.x == 0) counts[b] = (int32_t)c;
}

__global__ void k_scan_counts(const int32_t* counts, int B, int64_t* indptr)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int64_t acc = 0;
        indptr[0] = 0;
        for (int b = 0; b < B; ++b) {
            acc += counts[b];
            indptr[b + 1] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void k_dense_fill(const float* X, int I, const int64_t* indptr, int32_t* indices, float* values)
{
    __shared__ int wave_cnt[4];
    __shared__ int base_sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base_sh = 0;
    __syncthreads();
    const int64_t out0 = indptr[b];
    for (int c0 = 0; c0 < I; c0 += 256) {
        const int i = c0 + tid;
        const float v = (i < I) ? X[(size_t)b * I + i] : 0.f;
        const bool nz = v != 0.f;
        const unsigned long long bal = __ballot(nz);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wave_cnt[w];
        const int base = base_sh;
        if (nz) {
            const int64_t o = out0 + base + woff + before;
            indices[o] = i;
            values[o] = v;
        }
        __syncthreads();
        if (tid == 0) base_sh = base + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
}

int rtx_launch_dense_count(const float* X, int B, int I, int32_t* counts, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    hipLaunchKernelGGL(k_dense_count, dim3(B), dim3(256), 0, stream, X, I, counts);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
int rtx_launch_scan_counts(const int32_t* counts, int B, int64_t* indptr, hipStream_t stream)
{
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(64), 0, stream, counts, B, indptr);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
int rtx_launch_dense_fill(const float* X, int B, int I, const int64_t* indptr, int32_t* indices, float* values, hipStream_t stream)
{
    if (B <= 0) return RTX_OK;
    hipLaunchKernelGGL(k_dense_fill, dim3(B), dim3(256), 0, stream, X, I, indptr, indices, values);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
