// opr.hip -- one-plus-random evaluation (rectorch/evaluation.py:113-178), device half: the place of every held-out positive among
// its r + 1 scores.
//
// The reference gathers scores[u][[i] + negatives] for every contest, stacks them into a [contests, r + 1] host array and runs the
// top-k metrics on it, the positive being column 0.  With a single relevant column every metric is a function of the positive's
// rank alone, so the kernel returns that rank and the host evaluates the metrics from it (evaluation.py: _opr_metrics).
//
// One wavefront per contest: its r negatives' item ids are read once (coalesced, 64 per load), the scores they point at are
// gathered from the batch's score row -- 80 KB at ml-20m width, L2-resident across the contests of a user -- and counted against the
// positive's score.  The positive wins ties (strict >): the lower-column rule of the top-k kernel, column 0 being the positive.
// 4 bytes per contest go back to the host.
#include "../../include/rectorch_hip.h"
#include "rtx_common.h"

// T: the score type -- float (the autoencoders' predict) or double (EASE, ADMM_Slim); the comparison is made in T
template <typename T>
__global__ __launch_bounds__(256) void k_opr_rank(const T* __restrict__ scores, long ld, int n_rows, int n_items,
                                                  const int32_t* __restrict__ crow, const int32_t* __restrict__ citem,
                                                  const int32_t* __restrict__ draws, long n_contests, int r, int32_t* __restrict__ rank)
{
    const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= n_contests) return;
    const int u = crow[c], pi = citem[c];
    if (u < 0 || u >= n_rows || pi < 0 || pi >= n_items) {        // (never from rtx_opr_draw: a guard, not a route)
        if (lane == 0) rank[c] = -1;
        return;
    }
    const T* __restrict__ row = scores + (size_t)u * ld;
    const T s0 = row[pi];
    const int32_t* __restrict__ d = draws + (size_t)c * r;
    int cnt = 0, bad = 0;
    for (int j = lane; j < r; j += 64) {
        const int it = d[j];
        if (it < 0 || it >= n_items) { bad = 1; continue; }
        cnt += row[it] > s0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); bad |= __shfl_xor(bad, o, 64); }
    if (lane == 0) rank[c] = bad ? -1 : cnt;
}

template <typename T>
static int opr_rank_launch(const T* scores, int64_t ld, int32_t n_rows, int32_t n_items, const int32_t* contest_row,
                           const int32_t* contest_item, const int32_t* draws, int64_t n_contests, int32_t r, int32_t* rank, void* stream)
{
    RTX_CHECK(n_contests >= 0 && r >= 0 && n_rows >= 0 && n_items >= 0 && ld >= n_items, RTX_EINVAL, "opr_rank: bad sizes");
    if (n_contests == 0) return RTX_OK;
    RTX_CHECK(scores && contest_row && contest_item && rank && (draws || r == 0), RTX_EINVAL, "opr_rank: NULL argument");
    const int64_t blocks = (n_contests + 3) / 4;
    RTX_CHECK(blocks <= 0x7fffffff, RTX_EINVAL, "opr_rank: %lld contests in one call", (long long)n_contests);
    hipLaunchKernelGGL(k_opr_rank<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, scores, (long)ld, n_rows, n_items,
                       contest_row, contest_item, draws, (long)n_contests, r, rank);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

extern "C" int rtx_opr_rank(const float* scores, int64_t ld, int32_t n_rows, int32_t n_items, const int32_t* contest_row,
                            const int32_t* contest_item, const int32_t* draws, int64_t n_contests, int32_t r, int32_t* rank, void* stream)
{
    return opr_rank_launch<float>(scores, ld, n_rows, n_items, contest_row, contest_item, draws, n_contests, r, rank, stream);
}

extern "C" int rtx_opr_rank_f64(const double* scores, int64_t ld, int32_t n_rows, int32_t n_items, const int32_t* contest_row,
                                const int32_t* contest_item, const int32_t* draws, int64_t n_contests, int32_t r, int32_t* rank, void* stream)
{
    return opr_rank_launch<double>(scores, ld, n_rows, n_items, contest_row, contest_item, draws, n_contests, r, rank, stream);
}
