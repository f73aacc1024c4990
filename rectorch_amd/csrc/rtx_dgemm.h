// rtx_dgemm.h -- f64 MFMA NT GEMM used by the EASE closed-form solver (ease.hip) and ADMM SLIM (admm.hip):
//
//   C[m][n] = beta * C[m][n] + alpha * sum_{k0(m,n) <= k < k1(m,n)} A[m][k] * B[n][k]
//
// v_mfma_f64_16x16x4_f64; 128x128 tile (or 64x64 for the small nodes), 4 waves, 64x64 of C per wave as 4x4 blocks of 16x16; K consumed in
// 128-byte slices (16 doubles) through the same global->VGPR->LDS staging as the bf16/f32 GEMM (144-B padded rows,
// conflict-free ds_read_b64 fragment reads).  All dimensions are multiples of 128 (the solver pads the Gram matrix
// with an identity block), so there are no bounds checks.
#pragma once
#include "rtx_common.h"

enum { RTX_DK_ALL = 0, RTX_DK_TM = 1, RTX_DK_TN = 2, RTX_DK_MAX = 3 };

struct RtxDgemm {
    const double* A;   // [M][lda]
    const double* B;   // [N][ldb]
    long lda, ldb;
    int m_tiles, n_tiles;
    int k_slices;      // K / 16
    double* C;
    long ldc;
    double* CT;        // nullable: the result is also stored transposed, CT[n][m] (ldct)
    long ldct;
    double alpha, beta;
    int lower_only;    // skip tiles strictly above the diagonal (tn > tm)
    // triangular operands: the K range of tile (tm, tn) starts at 128 * {0, tm, tn, max(tm, tn)}  (k_lo) and ends
    // at 128 * ({tm, tn} + 1) (k_hi: RTX_DK_TM / RTX_DK_TN) instead of covering all of K
    int k_lo, k_hi;
    int small_tile;    // 1: 64x64 workgroup tiles (m_tiles / n_tiles and the tile-relative K ranges count 64s)
    // fused ADMM SLIM epilogue (rtx_dgemm_admm_launch only; admm.hip).  The iterate is held transposed, so with A = M^T and
    // B = P the accumulator is (P M)^T and every array below is [M][ldc] in that orientation.  Per element (r, c):
    //   bt = add + acc;  b = bt, or bt - pd (bt / pd) with pd = pdiag[r] when r == c;  C = soft(b + gamma / rho, thr) and the
    //   projection of `variant`;  gamma += rho (b - C);  mnext = rho C - gamma;  C^T to CT when CT != NULL (alpha / beta unused).
    // Rows and columns >= n are written as exact zeros.
    const double* e_add;     // B_aux^T
    const double* e_pdiag;   // diag(P)
    double* e_gamma;         // Gamma^T, read and updated in place
    double* e_mnext;         // the other buffer of the M^T pair (A is the current one)
    double e_rho, e_thr;     // rho, lambda1 / rho
    int e_n;
    int e_variant;           // RTX_ADMM_SOFT, RTX_ADMM_SOFT_NN, RTX_ADMM_B_NN
};

enum { RTX_ADMM_SOFT = 0, RTX_ADMM_SOFT_NN = 1, RTX_ADMM_B_NN = 2 };

int rtx_dgemm_launch(const RtxDgemm& g, hipStream_t stream);
// one ADMM SLIM iteration: C = A B^T (128x128 tiles, all of K) with the fused epilogue above
int rtx_dgemm_admm_launch(const RtxDgemm& g, hipStream_t stream);

// leaf of the recursive Cholesky: W = inv(chol(Akk)) of one 128x128 block into Wkk (lower) and WTkk (upper), both with
// leading dimension ldw; *status = 1 if the block is not positive definite (potf2.hip)
int rtx_potf2_inv_launch(const double* Akk, long ld, double* Wkk, double* WTkk, long ldw, int* status, hipStream_t stream);
// measurement knob: 1 (default) = the blocked leaf (four 32-column panels, ~30 barriers), 0 = one barrier per column (round 1)
void rtx_potf2_set_blocked(int on);
void rtx_potf2_set_stamps(unsigned long long* dev);   // measurement: >= 16 device entries receive 100-MHz clock stamps of the blocked leaf's phases

// ---- shared by the EASE and ADMM SLIM solvers (ease.hip) ------------------------------------------------------------
// rtx_gram_inverse: G = X^T X (+ bias_scale b b^T when bias, a device vector of n doubles) and P = (G + shift I)^-1 by the
// EASE pipeline (MFMA Gram matrix, recursive Cholesky with the inverse of the factor, P = W^T W), padded to np = a multiple
// of 128 with an identity block (so P's pad block is the identity).  P holds its lower tiles only, or the full symmetric
// matrix with full_P.  want_G: G (unshifted, full, zero in the pad) is returned as well.  P and G are allocated into
// `keep`, the factorisation workspace into `work` (the caller frees both; work may go as soon as the stream has run).
// Everything is queued on st; ev[0..3] are recorded at the start, after the Gram matrix, after the factorisation and
// after P.  *status (device int, in `work`) is non-zero after the stream has run if G + shift I is not positive definite.
#include <vector>
struct rtx_csr;
struct RtxCsrView;
struct RtxGramInverse {
    double* P = nullptr;
    double* G = nullptr;
    int np = 0;
    int* status = nullptr;
};
int rtx_gram_inverse(const rtx_csr* X, double shift, const double* bias, double bias_scale, int want_G, int full_P, RtxGramInverse* out,
                     std::vector<void*>& keep, std::vector<void*>& work, const hipEvent_t ev[4], hipStream_t st);
// Step 1 of rtx_gram_inverse on its own (the item-kNN fit, knn.hip): Gf (device double [np][np], np = n_cols rounded up to 128) =
// the full symmetric X^T X, zero in the pad -- the same exactness test, scatter, SYRK / f64 product and mirror launches, so the
// same bits.  Operands and the lower-triangle result go into `work`; everything is queued on st.
int rtx_gram_full(const rtx_csr* X, double* Gf, int np, std::vector<void*>& work, hipStream_t st);
// out[b][j] = sum over the stored entries (i, v) of row b of x of v * B[i][j] (+ bias[j]) for j < n, -inf at the non-zero
// entries of mask's row b (mask.indptr nullable)
int rtx_dense_scores_launch(const RtxCsrView& x, const RtxCsrView& mask, const double* B, long ldb, const double* bias, int n, int batch,
                            double* out, hipStream_t st);
