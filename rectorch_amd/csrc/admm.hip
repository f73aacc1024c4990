// admm.hip -- ADMM SLIM (rectorch/models.py:1389-1577) on MI355X, in float64.
//
// Reference (numpy float64 on the host), X = train.toarray():
//     [item_bias: b = X.sum(0); X = X - 1 b^T]   XtX = X^T X;  P = inv(XtX + (lam2 + rho) I)
//     neither nn_constr nor l1_penalty:  C = I - P * diag(1 / diag(P))                 (element-wise *: C ~ 0)
//     otherwise:  B_aux = P XtX;  Gamma = C = 0;  num_iter times:
//         B~ = B_aux + P (rho C - Gamma);  B = B~ - P * diag(diag(B~) / diag(P))     (element-wise: only the diagonal moves)
//         C = soft(B + Gamma / rho, lam1 / rho)  [then max(C, 0) | max(B, 0)];  Gamma += rho (B - C)
//     model = X C [+ b]
// Here:
//   1. G and P by EASE's pipeline (rtx_gram_inverse, ease.hip), with the item-bias term in the Gram matrix:
//      (X - 1 b^T)^T (X - 1 b^T) = X^T X + (n_users - 2) b b^T, so X is never densified.  P comes back full (mirrored).
//   2. B_aux^T = G P: one f64 NT GEMM.  The factorisation workspace is freed first.
//   3. The iterate is held TRANSPOSED (M^T = rho C^T - Gamma^T, Gamma^T, B_aux^T): with P symmetric, (P M)^T = M^T P is the
//      NT product A = M^T, B = P, so each iteration is ONE launch of rtx_dgemm_nt<4, RTX_DEPI_ADMM>, whose epilogue does all
//      the element-wise work and writes the next M^T into the other buffer of a ping-pong pair (other tiles still read the
//      current one).  The first iteration has M = 0, so B~ = B_aux exactly: it runs with K = 0.  The last writes C, in the
//      original orientation, through the transposed-store path.
//   4. Scores (X C)[ids] by EASE's sparse-row x dense kernel; with item_bias the row r = b - C^T b is added
//      ((X - 1 b^T) C + 1 b^T = X C + 1 r^T).
#include "../../include/rectorch_hip.h"
#include "rtx_dgemm.h"
#include "rtx_kernels.h"
#include "solver_common.h"

#include <memory>
#include <vector>

struct rtx_admm {
    int n = 0, np = 0;
    double* P = nullptr;       // [np][np], full symmetric
    double* C = nullptr;       // [np][np], original orientation
    double* Gamma = nullptr;   // [np][np], TRANSPOSED; nullptr for the closed-form variant (Gamma = 0)
    double* r = nullptr;       // [n] score bias row b - C^T b (item_bias), else nullptr
    double fit_ms = 0, factor_ms = 0, baux_ms = 0, iter_ms = 0;
};

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_admm_diag(const double* P, long ld, int np, double* d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < np) d[i] = P[(size_t)i * ld + i];
}

// closed-form variant: C = I - P * diag(1 / diag(P)) -- zero off the diagonal, 1 - P_ii (1 / P_ii) on it (C zero-filled before)
__global__ __launch_bounds__(256) void k_admm_closed_form(const double* P, long ld, int n, double* C)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const double p = P[(size_t)i * ld + i];
        C[(size_t)i * ld + i] = 1.0 - p * (1.0 / p);
    }
}

// r[j] = b[j] - sum_i C[i][j] b[i]
__global__ __launch_bounds__(256) void k_admm_bias_row(const double* C, long ld, const double* b, int n, double* r)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += C[(size_t)i * ld + j] * b[i];
    r[j] = b[j] - s;
}

// dst[i][j] (ld n) = src[j][i] (ld lds), i, j < n: 64x64 tiles through LDS
__global__ __launch_bounds__(256) void k_admm_transpose(const double* src, long lds, int n, double* dst)
{
    __shared__ double tile[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64, tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int idx = k * 256 + tid, rr = idx >> 6, cc = idx & 63;
        if (r0 + rr < n && c0 + cc < n) tile[rr][cc] = src[(size_t)(r0 + rr) * lds + c0 + cc];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int idx = k * 256 + tid, cc = idx >> 6, rr = idx & 63;
        if (r0 + rr < n && c0 + cc < n) dst[(size_t)(c0 + cc) * n + r0 + rr] = tile[rr][cc];
    }
}

// ------------------------------------------------------------------------------------------------ host side
static void admm_free(rtx_admm* h)
{
    for (double* p : {h->P, h->C, h->Gamma, h->r})
        if (p) (void)hipFree(p);
    delete h;
}

extern "C" {

int rtx_admm_fit(const rtx_csr* X, double lambda1, double lambda2, double rho, int32_t nn_constr, int32_t l1_penalty, int32_t item_bias,
                 int32_t num_iter, rtx_admm** out, void* stream)
{
    RTX_CHECK(X && out, RTX_EINVAL, "admm_fit: NULL argument");
    RTX_CHECK(X->n_rows > 0 && X->n_cols > 0, RTX_EINVAL, "admm_fit: empty matrix");
    RTX_CHECK(num_iter >= 0, RTX_EINVAL, "admm_fit: num_iter = %d < 0", num_iter);
    hipStream_t st = (hipStream_t)stream;
    const int n = X->n_cols;
    const bool iterate = nn_constr || l1_penalty;
    // fs.pool: the bias and the buffers of the iterations; events: start, Gram, factor, P | B_aux, iterations begin, iterations end, end
    RtxFitScope<8> fs;
    RtxFitScope<0> gram, work;   // pools alone: P / G of rtx_gram_inverse, its factorisation workspace
    std::unique_ptr<rtx_admm, decltype(&admm_free)> h(new rtx_admm(), admm_free);
    h->n = n;
    const int rc = [&]() -> int {
        hipEvent_t* ev = fs.ev;
        RTX_TRY(fs.create_events());
        // ---- item bias b = column sums of X, in row order on the host (the order of numpy's X.sum(axis=0))
        double* bias = nullptr;
        if (item_bias) {
            const int64_t U = X->n_rows;
            std::vector<int64_t> ip((size_t)U + 1);
            RTX_HIP(hipMemcpy(ip.data(), X->indptr, sizeof(int64_t) * (U + 1), hipMemcpyDeviceToHost));
            const int64_t nnz = ip[U];
            std::vector<int32_t> ix((size_t)nnz);
            std::vector<float> vx(X->values ? (size_t)nnz : 0);
            if (nnz) RTX_HIP(hipMemcpy(ix.data(), X->indices, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost));
            if (nnz && X->values) RTX_HIP(hipMemcpy(vx.data(), X->values, sizeof(float) * nnz, hipMemcpyDeviceToHost));
            std::vector<double> hb((size_t)n, 0.0);
            for (int64_t k = 0; k < nnz; ++k) hb[ix[k]] += X->values ? (double)vx[k] : 1.0;
            RTX_TRY(rtx_pool_alloc("admm", (void**)&bias, sizeof(double) * n, fs.pool));
            RTX_HIP(hipMemcpy(bias, hb.data(), sizeof(double) * n, hipMemcpyHostToDevice));
        }
        // ---- 1. G (+ (n_users - 2) b b^T), P = (G + (lam2 + rho) I)^-1
        RtxGramInverse gi;
        RTX_TRY(rtx_gram_inverse(X, lambda2 + rho, bias, (double)(X->n_rows - 2), iterate ? 1 : 0, 1, &gi, gram.pool, work.pool, ev, st));
        const int np = gi.np, KB = np / 128;
        h->np = np;
        h->P = gi.P;   // the handle's from here on; G (with iterate) stays in the pool until B_aux is done
        gram.pool.clear();
        if (gi.G) gram.pool.push_back(gi.G);
        RTX_HIP(hipStreamSynchronize(st));
        int status = 0;
        RTX_HIP(hipMemcpy(&status, gi.status, sizeof(int), hipMemcpyDeviceToHost));
        RTX_CHECK(status == 0, RTX_EINVAL, "admm_fit: X^T X + (lambda2 + rho) I is not positive definite (lambda2 + rho = %g)", lambda2 + rho);
        rtx_free_all(work.pool);
        const size_t nn2 = (size_t)np * np;
        RTX_TRY(rtx_dev_alloc("admm", (void**)&h->C, sizeof(double) * nn2));
        if (!iterate) {
            RTX_HIP(hipMemsetAsync(h->C, 0, sizeof(double) * nn2, st));
            hipLaunchKernelGGL(k_admm_closed_form, dim3((n + 255) / 256), dim3(256), 0, st, h->P, (long)np, n, h->C);
            RTX_HIP(hipGetLastError());
            RTX_HIP(hipEventRecord(ev[4], st));
            RTX_HIP(hipEventRecord(ev[5], st));
            RTX_HIP(hipEventRecord(ev[6], st));
        } else {
            // ---- 2. B_aux^T = G P  (= (P G)^T: both symmetric); then G is not needed any more
            double *Baux = nullptr, *M0 = nullptr, *M1 = nullptr, *pdiag = nullptr;
            RTX_TRY(rtx_pool_alloc("admm", (void**)&Baux, sizeof(double) * nn2, fs.pool));
            {
                RtxDgemm g = {};
                g.A = gi.G; g.B = h->P; g.lda = np; g.ldb = np; g.m_tiles = KB; g.n_tiles = KB; g.k_slices = np / 16;
                g.C = Baux; g.ldc = np; g.alpha = 1.0; g.beta = 0.0; g.k_lo = RTX_DK_ALL; g.k_hi = RTX_DK_ALL;
                RTX_TRY(rtx_dgemm_launch(g, st));
            }
            RTX_HIP(hipEventRecord(ev[4], st));
            RTX_HIP(hipStreamSynchronize(st));
            rtx_free_all(gram.pool);
            RTX_TRY(rtx_dev_alloc("admm", (void**)&h->Gamma, sizeof(double) * nn2));
            RTX_TRY(rtx_pool_alloc("admm", (void**)&M0, sizeof(double) * nn2, fs.pool));
            RTX_TRY(rtx_pool_alloc("admm", (void**)&M1, sizeof(double) * nn2, fs.pool));
            RTX_TRY(rtx_pool_alloc("admm", (void**)&pdiag, sizeof(double) * np, fs.pool));
            RTX_HIP(hipMemsetAsync(h->Gamma, 0, sizeof(double) * nn2, st));
            RTX_HIP(hipMemsetAsync(h->C, 0, sizeof(double) * nn2, st));   // num_iter = 0: C = 0
            hipLaunchKernelGGL(k_admm_diag, dim3((np + 255) / 256), dim3(256), 0, st, h->P, (long)np, np, pdiag);
            RTX_HIP(hipGetLastError());
            RTX_HIP(hipEventRecord(ev[5], st));
            // ---- 3. the iterations: one fused launch each
            double* M[2] = {M0, M1};
            RtxDgemm g = {};
            g.B = h->P; g.lda = np; g.ldb = np; g.m_tiles = KB; g.n_tiles = KB;
            g.ldc = np; g.ldct = np; g.k_lo = RTX_DK_ALL; g.k_hi = RTX_DK_ALL;
            g.e_add = Baux; g.e_pdiag = pdiag; g.e_gamma = h->Gamma; g.e_rho = rho; g.e_thr = lambda1 / rho; g.e_n = n;
            g.e_variant = (nn_constr && l1_penalty) ? RTX_ADMM_SOFT_NN : nn_constr ? RTX_ADMM_B_NN : RTX_ADMM_SOFT;
            for (int t = 0; t < num_iter; ++t) {
                g.A = M[t & 1];
                g.k_slices = t == 0 ? 0 : np / 16;   // M_0 = 0: B~_1 = B_aux
                g.e_mnext = M[(t + 1) & 1];
                g.CT = (t == num_iter - 1) ? h->C : nullptr;
                RTX_TRY(rtx_dgemm_admm_launch(g, st));
            }
            RTX_HIP(hipEventRecord(ev[6], st));
        }
        // ---- 4. score bias row
        if (item_bias) {
            RTX_TRY(rtx_dev_alloc("admm", (void**)&h->r, sizeof(double) * n));
            hipLaunchKernelGGL(k_admm_bias_row, dim3((n + 255) / 256), dim3(256), 0, st, h->C, (long)np, bias, n, h->r);
            RTX_HIP(hipGetLastError());
        }
        RTX_HIP(hipEventRecord(ev[7], st));
        RTX_HIP(hipStreamSynchronize(st));
        h->factor_ms = rtx_elapsed_ms(ev[0], ev[3]);
        h->baux_ms = iterate ? rtx_elapsed_ms(ev[3], ev[4]) : 0.0;
        h->iter_ms = rtx_elapsed_ms(ev[5], ev[6]);
        h->fit_ms = rtx_elapsed_ms(ev[0], ev[7]);
        return RTX_OK;
    }();
    if (rc) {
        (void)hipStreamSynchronize(st);   // launches already queued may use the pools, which are freed on return
        return rc;
    }
    *out = h.release();
    return RTX_OK;
}

int rtx_admm_destroy(rtx_admm* h)
{
    if (h) admm_free(h);
    return RTX_OK;
}

int rtx_admm_copy(const rtx_admm* h, int32_t what, double* dst_dev, void* stream)
{
    RTX_CHECK(h && dst_dev, RTX_EINVAL, "admm_copy: NULL argument");
    RTX_CHECK(what == RTX_ADMM_P || what == RTX_ADMM_C || what == RTX_ADMM_GAMMA, RTX_EINVAL, "admm_copy: unknown matrix %d", what);
    hipStream_t st = (hipStream_t)stream;
    const int n = h->n;
    const size_t row = sizeof(double) * n, ld = sizeof(double) * h->np;
    if (what == RTX_ADMM_GAMMA) {
        if (!h->Gamma) {
            RTX_HIP(hipMemsetAsync(dst_dev, 0, row * n, st));
            return RTX_OK;
        }
        hipLaunchKernelGGL(k_admm_transpose, dim3((n + 63) / 64, (n + 63) / 64), dim3(256), 0, st, h->Gamma, (long)h->np, n, dst_dev);
        RTX_HIP(hipGetLastError());
        return RTX_OK;
    }
    RTX_HIP(hipMemcpy2DAsync(dst_dev, row, what == RTX_ADMM_P ? h->P : h->C, ld, row, n, hipMemcpyDeviceToDevice, st));
    return RTX_OK;
}

int rtx_admm_timings(const rtx_admm* h, double* fit_ms, double* factor_ms, double* baux_ms, double* iter_ms)
{
    RTX_CHECK(h, RTX_EINVAL, "admm: NULL handle");
    if (fit_ms) *fit_ms = h->fit_ms;
    if (factor_ms) *factor_ms = h->factor_ms;
    if (baux_ms) *baux_ms = h->baux_ms;
    if (iter_ms) *iter_ms = h->iter_ms;
    return RTX_OK;
}

int rtx_admm_scores(const rtx_admm* h, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const rtx_csr* mask,
                    const int32_t* mask_row_ids, double* out, void* stream)
{
    RTX_CHECK(h && X && out, RTX_EINVAL, "admm_scores: NULL argument");
    RtxCsrView v, mv;
    RTX_TRY(rtx_scores_args("admm_scores", h->n, X, row_ids, batch, mask, mask_row_ids, &v, &mv));
    if (batch == 0) return RTX_OK;
    return rtx_dense_scores_launch(v, mv, h->C, h->np, h->r, h->n, batch, out, (hipStream_t)stream);
}

}  // extern "C"
