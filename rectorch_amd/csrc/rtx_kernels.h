// rtx_kernels.h -- launchers of the non-GEMM kernels of the Mult-VAE/DAE step: the boundary the engine sees.  One file per role:
//   batch_rows.hip   batch formation: gather (K1), CSR -> dense, dense -> CSR   (row arithmetic: batch_rows.h, shared with spmm_in.hip)
//   spmm_in.hip      the first encoder layer as a sparse product;  small_layers.hip  the one-launch hidden layers
//   post_layers.hip  post kernels and the VAE head of the generic / float32 layer chain
//   loss.hip         losses, their gradients w.r.t. the logits, the loss sum, the -inf mask of predict()
//   adam.hip         fused multi-tensor Adam, squared norms, bf16 cast, split-K slab sum of a weight gradient
//   topk.hip         ranking metrics of evaluate();  recommend.hip  top-N item lists of recommend()
//   list_metrics.hip ranking metrics of ready-made item lists (any score type, any list length)
// Device helpers they share (reductions, csr_row): rtx_device.h.
// All pointers are device pointers; every launcher enqueues on `stream` and returns RTX_OK / RTX_E*.
#pragma once
#include "rtx_common.h"

// A batch of users as rows of a CSR matrix resident in HBM.  Batch row b is CSR row
// (row_ids ? row_ids[b] : b).  values == NULL means every stored entry is 1.0 (implicit feedback).
struct RtxCsrView {
    const int64_t* indptr;
    const int32_t* indices;
    const float* values;
    const int32_t* row_ids;
    int32_t max_row_len;   // longest row of the matrix the view comes from (0 = unknown: a densified batch)
    int32_t avg_row_len;   // its mean row length, rounded up
};

// the opaque rtx_csr of include/rectorch_hip.h: a scipy-style CSR matrix resident in HBM
struct rtx_csr {
    int64_t* indptr = nullptr;
    int32_t* indices = nullptr;
    float* values = nullptr;  // nullptr -> all ones
    int64_t n_rows = 0, nnz = 0;
    int32_t n_cols = 0;
    int32_t max_row_len = 0;
    // wmf.hip: 0 = not looked at yet, 1 = every stored value is > 0, -1 = one is not (the matrix never changes after the upload, so
    // the one host pass over the values that the WMF entry points need is made once per matrix)
    mutable int32_t values_positive = 0;
};

// elements per LDS chunk of a dense row (16 KB fp32): k_csr_to_dense, and the target image / row-loss partials of the loss kernels
#define RTX_GATHER_CHUNK 4096

// ---- K1: sparse user rows -> dense normalised (+dropout) input ---------------------------------------
//   X  [Bp][ldx]  row-major: forward A operand and (read K-major) weight-gradient B operand; rows >= B are
//                 written as zeros; column Iin holds ONES for b < B, so the weight-gradient product emits the
//                 bias gradient as one extra output column (the forward weight copy has a zero column there)
//   tsum[b] = sum of the TARGET row's values (s_b of the multinomial likelihood)
struct RtxGatherArgs {
    RtxCsrView in, target;
    int B, Bp, I, ldx;
    int Iin;              // input columns (= I, or I + cond_dim: trailing condition columns stay raw)
    int raw;              // 1: every column as stored, no normalisation (VAE_net, RTX_GVAE: nets.py:287)
    void* X;
    float* tsum;
    int training;
    float dropout_p;
    const uint8_t* mask;  // [B][I] injected keep-mask (nullable -> Philox)
    uint64_t seed, offset;
    // Scatter form (round 4, nullable): the image is ALL ZERO except the columns the previous launch wrote, which it listed per row
    // slot (written[b * written_cap ..], n_written[b]).  The launch clears those, writes this batch's stored entries and the ones
    // column (2- / 4-byte scattered stores) and lists them again: ~150 stores per user instead of a 40-KB row of zeros.  The
    // caller guarantees the invariant (engine.hip: any other writer of the image, or a row longer than written_cap - 1, makes the
    // next launch a full rewrite) and in.max_row_len < written_cap.
    int32_t* written;
    int32_t* n_written;
    int written_cap;
};
int rtx_launch_gather(const RtxGatherArgs& a, int is_bf16, hipStream_t stream);

// ---- first encoder layer as a sparse product (spmm_in.hip; bf16 numerics) -----------------------------------------
// k_in_chunks: the batch's stored entries, normalised / dropped out exactly as k_gather does, as ONE stream of 64-entry
// chunks (item | bf16 value << 16), users back to back; desc[chunk] = user (desc[n_chunks] = -1); wsplit[0..16] = a split
// of the stream at user boundaries.  Capacity: sum_b max(1, ceil(len_b / 64)) chunks + 64 chunks of read-ahead slack.
#define RTX_SPMM_WAVES 16
struct RtxInChunksArgs {
    RtxCsrView in;
    int B, I, Iin;
    int training;
    float dropout_p;
    const uint8_t* mask;
    uint64_t seed, offset;
    uint32_t* ent;
    int32_t* desc;
    int32_t* wsplit;
    int64_t cap_chunks;  // capacity of ent / desc in chunks: a user whose chunks would not fit writes nothing (0 = unchecked)
    // optional: what k_gather<bf16> writes, from the same pass over the entries (training step)
    RtxCsrView target;   // rows whose sums go to tsum (read only if tsum != NULL)
    float* tsum;         // [Bp] nullable
    bf16_t* X;           // [Bp][ldx] nullable: dense image, rows >= B zero, column Iin = 1 for b < B
    int ldx, Bp;
};
int rtx_launch_in_chunks(const RtxInChunksArgs& a, hipStream_t stream);
// k_spmm_in: O32 / R [Bp][Np] = act(chunks x W^T + bias) with the padding and ones-column conventions of k_post (forward)
struct RtxSpmmInArgs {
    const uint32_t* ent;
    const int32_t* desc;
    const int32_t* wsplit;
    int B, Bp;
    const bf16_t* W;   // [>= N_real][ldw] compute copy of the first layer's weight matrix
    int ldw, Kin;      // Kin = input columns an entry may name (n_items + cond_dim)
    const float* bias;
    int N_real, Np, tanh_act;
    float* O32;        // nullable
    bf16_t* R;         // nullable
    int ones_col;
    uint64_t* stamps;  // nullable measurement hook: [workgroups][2 waves][4] shader-clock stamps (start, staged, summed, end)
};
size_t rtx_spmm_in_lds_bytes(int Kin);   // <= 160 KB or the launch is refused
int rtx_launch_spmm_in(const RtxSpmmInArgs& a, hipStream_t stream);

// ---- hidden layers of the forward pass in one launch each (small_layers.hip; bf16 numerics, padded input width <= 1024) ----
// Z == 0: R / O32 [Bp][Np] = act(A W^T + bias) with the conventions of k_post (forward).  Z > 0: the VAE head with the
// conventions of k_vae_fwd (W rows [0, Z) = mu, [Z, 2Z) = logvar; R = the next operand [Bp][Np = Zp]).
struct RtxSmallFwdArgs {
    const bf16_t* A;   // [Bp][lda]
    const bf16_t* W;   // [w_rows][ldw]
    int lda, ldw, w_rows;
    int B, Bp, N_real, Np, tanh_act;
    const float* bias;
    float* O32;        // hidden: nullable
    bf16_t* R;
    // VAE head
    int Z, training;
    float *mu32, *lv32, *eps32, *mu_out, *lv_out;
    const float* eps_in;
    uint64_t seed, offset;
};
bool rtx_small_fwd_ok(int K);
void rtx_small_set_kw(int kw);      // measurement knob: waves that share the K range of a 16-row block (1, 2 or 4)
void rtx_small_set_waves(int w);   // measurement knob: 16-row waves per workgroup of the one-launch hidden layers (1, 2 or 4)
int rtx_launch_small_fwd(const RtxSmallFwdArgs& a, hipStream_t stream);
// backward through a hidden layer (Z == 0: conventions of k_post backward) or the VAE head (Z > 0: of k_vae_bwd):
// Dout [Bp][Np] from D [Bp][ld] (the layer's output gradient) and W^T [wt_rows][ld] (row n = input feature n)
struct RtxSmallBwdArgs {
    const bf16_t* D;
    const bf16_t* WT;
    int ld, wt_rows;
    int B, Bp, N_real, Np, tanh_act;
    const float* O32;  // hidden: the saved activation of the layer below [Bp][Np] (read if tanh_act)
    bf16_t* Dout;
    // VAE head
    int Z, training;
    const float *mu32, *lv32, *eps32;
    float beta, inv_batch;
    const float *g_mu, *g_lv;   // see RtxVaeBwdArgs
};
int rtx_launch_small_bwd(const RtxSmallBwdArgs& a, hipStream_t stream);

// DataSampler densify: rows -> float32 [B][I] (ld = I), optional second matrix
int rtx_launch_csr_to_dense(const RtxCsrView& v, int B, int I, float* out, hipStream_t stream);

// ---- post kernels: fp32 GEMM output (possibly split-K slabs) -> the next GEMM's operand (row-major) -----
enum { RTX_POST_FWD = 0, RTX_POST_BWD = 1 };
struct RtxPostArgs {
    const float* C;     // [splits][Bp][ldc]
    int splits;
    long slab_stride;
    int ldc;
    int B, Bp;          // valid / padded batch rows processed by this call
    int N_real, Np;     // valid / padded feature columns
    int tanh_act;
    const float* bias;  // FWD
    float* O32;         // FWD: post-activation fp32 [Bp][Np] (nullable); BWD: input (the saved activation)
    void* R;            // row-major output  T [Bp][Np]   (nullable)
    int ones_col;       // FWD: R[b][N_real] = 1 for b < B (bias-gradient column of the next layer's weight gradient)
};
int rtx_launch_post(const RtxPostArgs& a, int mode, int is_bf16, hipStream_t stream);

// ---- the user node of CDAE (include/rectorch_hip.h: "CDAE"): one row of V per batch row, in the epilogues of k_post ----
//   FWD: x = (c + bias) + V[uid[b]][n]   before the activation, for b < B, n < N_real, 0 <= uid[b] < n_users
//   BWD: g = c (1 - o^2) is d loss / d V[uid[b]][n]: the rows' lazy Adam update (rtx_user_adam1, post_layers.hip) in the epilogue
// A kernel argument of its own beside RtxPostArgs: the instantiations without a table keep their argument block and their code.
struct RtxPostUsers {
    const int32_t* uid;   // [B] device ids, -1 (or anything outside [0, n_users)) = no user term
    int n_users;
    float* V;             // [n_users][ld]
    float* m;             // BWD: exp_avg    [n_users][ld]
    float* v;             // BWD: exp_avg_sq [n_users][ld]
    long ld;
    int vec;              // rows may be read as float4: ld % 4 == 0, ld >= roundup(N_real, 4), all bases 16-byte aligned
    float omb1, omb2;     // BWD: (float)(1 - beta1), (float)(1 - beta2)
    float eps, step_size; // BWD: eps, (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t))
};
// the scalars of torch.optim.SparseAdam's update number `step`, computed in double as torch does on the host
void rtx_user_adam_scalars(float lr, float beta1, float beta2, float eps, int step, RtxPostUsers& u);
bool rtx_user_rows_vec(const float* V, const float* m, const float* v, long ld, int latent);
int rtx_launch_post_users(const RtxPostArgs& a, const RtxPostUsers& u, int mode, int is_bf16, hipStream_t stream);
// the same update outside a step (rtx_user_rows_adam): g float32 [batch][ldg], thread (b, n .. n + 3) as in k_post
int rtx_launch_user_rows_adam(const RtxPostUsers& u, const float* g, long ldg, int batch, int latent, hipStream_t stream);

// ---- VAE head -------------------------------------------------------------------------------------
struct RtxVaeFwdArgs {
    const float* C;  // [splits][Bp][ldc], columns [0,Z) = mu, [Z,2Z) = logvar (pre-bias)
    int splits;
    long slab_stride;
    int ldc;
    int B, Bp, Z, Zp;
    const float* bias;   // [2Z]
    float* mu32;         // [Bp][Z] engine copies for the backward
    float* lv32;
    float* eps32;
    float* mu_out;       // [B][Z] user outputs (nullable)
    float* lv_out;
    void* Zr;            // T [Bp][Zp], column Z = ones (b < B)
    int training;
    const float* eps_in; // [B][Z] injected (nullable -> Philox)
    uint64_t seed, offset;
};
int rtx_launch_vae_fwd(const RtxVaeFwdArgs& a, int is_bf16, hipStream_t stream);

struct RtxVaeBwdArgs {
    const float* C;  // dz [splits][Bp][ldc]
    int splits;
    long slab_stride;
    int ldc;
    int B, Bp, Z, Np;  // Np = P(2Z)
    const float* mu32;
    const float* lv32;
    const float* eps32;
    int training;
    float beta, inv_batch;
    void* D;   // T [Bp][Np]
    // gradients of a loss computed outside the engine w.r.t. mu and logvar, float32 [B][Z] (both or neither; nullable).  Set, they
    // REPLACE the built-in KL terms (beta and inv_batch are not read): dmu = dz + g_mu, dlogvar = dz eps exp(logvar / 2) / 2 + g_lv.
    const float *g_mu, *g_lv;
};
int rtx_launch_vae_bwd(const RtxVaeBwdArgs& a, int is_bf16, hipStream_t stream);

// ---- the cut between the encoder and the decoder half (post_layers.hip) ------------------------------
// The head's sampling step on its own, float32 [n][Z] contiguous: z = mu + eps exp(logvar / 2) through the helper the two head kernels
// call (rtx_device.h: rtx_reparam_z); eps = eps_in[b][j] (nullable) or rtx_normal(seed, offset, b Z + j); eps_out (nullable) keeps the draws.
int rtx_launch_reparam(const float* mu, const float* logvar, long n, int Z, const float* eps_in, uint64_t seed, uint64_t offset, float* z,
                       float* eps_out, hipStream_t stream);
// its derivative: d_mu = d_z, d_logvar = d_z eps exp(logvar / 2) / 2 (either output nullable; logvar / eps read for d_logvar only)
int rtx_launch_reparam_grad(const float* d_z, const float* logvar, const float* eps, long n, int Z, float* d_mu, float* d_logvar,
                            hipStream_t stream);
// d loss / d h enters the encoder's chain with no decoder behind it: D [Bp][Np] (T) = dh[b][n] (1 - O32[b][n]^2) (tanh_act; else dh)
// for b < B, n < N_real, zeros in the padding.  dh: the caller's UNPADDED float32 [B][N_real], read under the mask only.
int rtx_launch_import_dh(const float* dh, int B, int N_real, int Bp, int Np, int tanh_act, const float* O32, void* D, int is_bf16,
                         hipStream_t stream);
// d loss / d z leaves the decoder's chain: d_z [n][Z] (unpadded float32) = the split-K slabs C [splits][>= n][ldc] summed in slab order
int rtx_launch_export_dz(const float* C, int splits, long slab_stride, int ldc, int n, int Z, float* d_z, hipStream_t stream);

// ---- loss ------------------------------------------------------------------------------------------
struct RtxLossArgs {
    const float* Y;  // logits [Bp][ldy]
    int ldy, B, I;
    const float2* part;  // per-row, per-strip (max, sumexp) partials from the logits GEMM epilogue (nullable)
    int n_strips, part_ld;
    RtxCsrView target;
    const float* tsum;
    float* lse;       // [Bp] out
    float* row_loss;  // [Bp] out
    float inv_batch;
    // VAE KL term
    const float* mu32;
    const float* lv32;
    int Z;
    float beta;
};
// loss_out[0] = sum(row_loss[0..B)) + lam * sum_t sqrt(sumsq[t]);  loss_accum[0] += the same (nullable)
int rtx_launch_reduce_loss(const float* row_loss, int B, float lam, const float* sumsq, int n_tensors,
                           float* loss_out, float* loss_accum, hipStream_t stream, uint32_t* mailbox = nullptr, uint32_t seq = 0, uint32_t tag = 0);
// Loss AND its gradient w.r.t. the logits in one pass over Y (reference models.py:813-815 + autograd of log_softmax):
//   lse_b from the strip partials the logits GEMM left (or, without them, a first pass over the row),
//   row-loss partials (their fixed-order sum is the loss),  D[b][i] = (s_b * softmax(Y_b)_i - t_bi) * inv_batch  (T = bf16 / f32, zero padding)
struct RtxDlogitsArgs {
    RtxLossArgs loss;   // Y, target, tsum, part..., outputs lse / row_loss, KL inputs
    int Bp;             // rows [B, Bp) of D are written as zeros
    void* D;            // T [Bp][ldd]
    int ldd;            // >= I, multiple of 8; columns [I, ldd) are written as zeros
    const void* Y16;    // T = bf16 only (nullable): the logits as IEEE half [Bp][ldd] INSTEAD of loss.Y (rtx_gemm_launch's C16);
                        //   may be the same buffer as D -- every thread reads its 16 bytes before it writes them
};
int rtx_launch_dlogits(const RtxDlogitsArgs& a, int is_bf16, hipStream_t stream);
// d loss / d output computed OUTSIDE the engine (rtx_engine_backward) into the same D, under the same layout contract (T [Bp][ldd],
// rows >= B and columns >= I zero): g float32 [B][>= I] with row stride ld >= I, any alignment (16-byte loads when base and stride
// allow them).  sigmoid == 0: D = g.  sigmoid != 0 (RTX_GVAE, whose public output is p = sigmoid(y)): D = g (1 - p) p with p from the
// float32 logits a.loss.Y [B][ldy] -- torch's sigmoid_backward in float32.  Of a.loss only B, I, Y and ldy are read; no loss is written.
int rtx_launch_import_dout(const RtxDlogitsArgs& a, const float* g, long ld, int sigmoid, int is_bf16, hipStream_t stream);
// one workgroup per (user, 4096-column chunk): loss.row_loss receives [B][rtx_dlogits_chunks(ldd)] partial sums
int rtx_dlogits_chunks(int ldd);
// VAE_net's loss (RTX_GVAE; reference models.py:581-583) and its gradient w.r.t. the logits in one pass over Y, with the layout
// contract of rtx_launch_dlogits (D [Bp][ldd], rows >= B and columns >= I zero; loss.row_loss [B][rtx_dlogits_chunks(ldd)]):
//   p = sigmoid(y) (float32),  row_part += ((x - 1) max(log1p(-p), -100) - x max(log p, -100)) * inv_elems,
//   D = (p - x) / max(p (1 - p), 1e-12) * inv_elems * p (1 - p)   (autograd of F.binary_cross_entropy + torch.sigmoid),
//   chunk 0 adds beta * KL_b * inv_batch.  x from the target CSR row (0 off its stored entries); loss.part / tsum / lse unused.
int rtx_launch_bce_dlogits(const RtxDlogitsArgs& a, float inv_elems, int is_bf16, hipStream_t stream);
// predict() of RTX_GVAE: logits[b][i] = sigmoid(logits[b][i]) for i < n_items (in place, before rtx_launch_neg_inf)
int rtx_launch_sigmoid_rows(float* logits, int B, long ld, int n_items, hipStream_t stream);
// public VAE.loss_function on dense tensors: row_loss[b] = sum_i bce(p_bi, x_bi) * inv_elems + KL_b * inv_batch
int rtx_launch_dense_bce_kl(const float* P, const float* X, int B, int I, const float* mu, const float* lv, int Z,
                            float inv_elems, float inv_batch, float* row_loss, hipStream_t stream);
// AETrainer's loss (RTX_AE; reference models.py:377, 441-447: torch.nn.MSELoss against the target rows as stored) and its
// gradient w.r.t. the raw outputs in one pass over Y, with the layout contract of rtx_launch_dlogits (D [Bp][ldd], rows >= B and
// columns >= I zero; loss.row_loss [B][rtx_dlogits_chunks(ldd)]):
//   e = y - x,  row_part += e e * inv_elems,  D = 2 inv_elems e   (inv_elems = 1 / (B I)).
// x from the target CSR row (0 off its stored entries); loss.part / tsum / lse / mu32 / beta unused.
int rtx_launch_mse_dlogits(const RtxDlogitsArgs& a, float inv_elems, int is_bf16, hipStream_t stream);
// public AETrainer.loss_function on dense tensors: row_loss[b] = sum_i (x_bi - y_bi)^2 * inv_elems
int rtx_launch_dense_mse(const float* Y, const float* X, int B, int I, float inv_elems, float* row_loss, hipStream_t stream);
// predict(): logits[b][i] = -inf where the input has a stored non-zero
int rtx_launch_neg_inf(const RtxCsrView& in, int B, float* logits, long ld, int n_items, hipStream_t stream);
// public loss_function on dense tensors: row_loss[b] = s*lse - <x,y>  (+ beta * KL_b)
int rtx_launch_dense_loss(const float* Y, const float* X, int B, int I, const float* mu, const float* lv, int Z,
                          float beta, float inv_batch, float* row_loss, hipStream_t stream);
// The three dense loss functions with their gradients at unit upstream gradient (rtx_*_loss_grad): row_loss[b] as the launcher of the
// same name without _grad writes it, to the bit, and in the same launch
//   dense_loss_grad:    dY = (s_b softmax(y_b)_i - x_bi) * inv_batch,  dmu = beta inv_batch mu,  dlv = beta inv_batch (exp(lv) - 1) / 2
//   dense_bce_kl_grad:  dP = (p - x) / max(p (1 - p), 1e-12) * inv_elems,  dmu = inv_batch mu,  dlv = inv_batch (exp(lv) - 1) / 2
//   dense_mse_grad:     dY = 2 inv_elems (y - x)
// Y / P, X, dY / dP: float32 [B][I], row stride I, any alignment (16-byte accesses when all three bases are 16-byte aligned and
// I % 4 == 0); mu, lv, dmu, dlv: [B][Z], all four or none.
int rtx_launch_dense_loss_grad(const float* Y, const float* X, int B, int I, const float* mu, const float* lv, int Z, float beta,
                               float inv_batch, float* row_loss, float* dY, float* dmu, float* dlv, hipStream_t stream);
int rtx_launch_dense_bce_kl_grad(const float* P, const float* X, int B, int I, const float* mu, const float* lv, int Z, float inv_elems,
                                 float inv_batch, float* row_loss, float* dP, float* dmu, float* dlv, hipStream_t stream);
int rtx_launch_dense_mse_grad(const float* Y, const float* X, int B, int I, float inv_elems, float* row_loss, float* dY, hipStream_t stream);
// grads[t][i] = tensors[t][i] / sqrt(sumsq[t]), zeros where sumsq[t] == 0: the gradient of sum_t ||tensor_t||_2 from the squared norms
// sumsq (a device array); tensors_host / grads_host / sizes are HOST arrays of n <= 32 entries.  rtx_launch_sumsq_ordered fills sumsq
// in a fixed order (bit-equal between calls; rtx_launch_sumsq's value to the bit for a tensor of <= 4096 elements) through
// `part`, rtx_sumsq_ordered_scratch(n) floats of device scratch.
struct RtxNormGradArgs {
    const float* w[32];
    float* g[32];
    long n[32];
};
int rtx_launch_norm_grad(const float* const* tensors_host, float* const* grads_host, const long* sizes, int n, const float* sumsq,
                         hipStream_t stream);
int rtx_sumsq_ordered_scratch(int n);
int rtx_launch_sumsq_ordered(const float* const* tensors_host, const long* sizes, int n, float* sumsq, float* part, hipStream_t stream);

// ---- dense batch -> CSR (drop-in train_batch(tr_batch, te_batch) / predict(x) with dense tensors) --
int rtx_launch_dense_count(const float* X, int B, int I, int32_t* counts, hipStream_t stream);
int rtx_launch_scan_counts(const int32_t* counts, int B, int64_t* indptr, hipStream_t stream);
int rtx_launch_dense_fill(const float* X, int B, int I, const int64_t* indptr, int32_t* indices, float* values,
                          hipStream_t stream);

// ---- fused multi-tensor Adam (+ shadow refresh) ------------------------------------------------------
#define RTX_MAX_TENSORS 32
struct RtxAdamTensor {
    float* p;
    const float* g;
    const bf16_t* g16;   // nullable: read the gradient from this bf16 image instead of g
    float* m;
    float* v;
    void* sh;    // T [rows_p][ld_sh]   compute copy, same orientation   (nullable)
    void* shT;   // T [cols_p][ld_shT]  compute copy, transposed          (nullable; the engine passes the hidden layers' W^T here)
    const float* sumsq;  // DAE: this tensor's squared norm (g += lam * p / ||p||), nullable
    int rows, cols, ld_sh, ld_shT;
    int tile_start;  // first tile of this tensor in the launch
    int flat;        // filled by rtx_launch_adam: walked as one contiguous array in chunks of 4096 elements (see k_adam)
};
struct RtxAdamArgs {
    RtxAdamTensor t[RTX_MAX_TENSORS];
    int n;
    int total_tiles;   // filled by rtx_launch_adam
    int update;        // 0: only refresh the shadows from the master parameters
    float step_size;   // lr / (1 - beta1^t)
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    float beta1, beta2, eps, weight_decay;
    float lam;         // DAE: g += lam * p / ||p||  (per-tensor norms in t[k].sumsq)
    float grad_scale;  // multiplies g before use (1.0; data-parallel averaging hooks)
    // the update rule of the launch (adam.hip: k_optim<T, Rule>); all zero = Adam with coupled decay, what the fields above describe
    int rule;          // RTX_RULE_*
    int first;         // SGD with momentum: the parameters' first update, buf = g
    int nesterov;      // SGD
    float lr;          // SGD, RMSprop: lr; Adagrad: clr = lr / (1 + (t - 1) lr_decay)
    float momentum;    // SGD, RMSprop
    float damp1;       // SGD: 1 - dampening
    float alpha, alpha1;   // RMSprop: alpha, 1 - alpha
    float decay;       // decoupled Adam: 1 - lr weight_decay
    // gradient clipping (k_optim<T, Rule, Clip>; all zero = none, the kernels of every release so far): what is clipped is
    // G = g grad_scale + lam p / ||p||, before the weight decay is added (torch clips p.grad, optimizer.step() adds the decay)
    int clip;                // RTX_CLIPK_*
    float clip_value;        // RTX_CLIPK_VALUE: G <- clamp(G, -clip_value, +clip_value)
    const float* clip_coef;  // RTX_CLIPK_COEF: device pair {total norm, coefficient} of rtx_launch_grad_norm; G <- G * clip_coef[1]
};
enum { RTX_CLIPK_NONE = 0, RTX_CLIPK_COEF = 1, RTX_CLIPK_VALUE = 2 };
enum { RTX_RULE_ADAM = 0, RTX_RULE_ADAMW, RTX_RULE_SGD, RTX_RULE_SGD_MOM, RTX_RULE_ADAGRAD, RTX_RULE_RMSPROP, RTX_RULE_RMSPROP_MOM, RTX_RULE_COUNT };
// the optimizer of an engine handle: rtx_optim of include/rectorch_hip.h, field by field (RTX_OPTIM_* values there and here)
enum { RTX_OPT_ADAM = 0, RTX_OPT_SGD = 1, RTX_OPT_ADAGRAD = 2, RTX_OPT_RMSPROP = 3 };
enum { RTX_OPTF_DECOUPLED = 1, RTX_OPTF_NESTEROV = 2, RTX_OPTF_FIRST = 4 };
struct RtxOptim {
    int kind = RTX_OPT_ADAM, flags = 0;
    double momentum = 0, dampening = 0, alpha = 0.99, lr_decay = 0;      // doubles, as torch holds them: 1 - alpha is rounded to float32 once
    bool plain_adam() const { return kind == RTX_OPT_ADAM && !(flags & RTX_OPTF_DECOUPLED); }
};
int rtx_optim_validate(const RtxOptim& o);
int rtx_optim_scalars(const RtxOptim& o, float lr, float beta1, float beta2, float eps, float weight_decay, int step, RtxAdamArgs& a);
// rtx_launch_adam runs a.rule (0: Adam, every caller that leaves the rule fields zero)
int rtx_launch_adam(RtxAdamArgs& a, int is_bf16, hipStream_t stream);
// ---- gradient clipping (adam.hip) ---------------------------------------------------------------------------------------------------
// The global norm of G over the tensor table of an optimizer launch (p, g / g16, sumsq, rows, cols, lam, grad_scale of `a`; nothing else
// is read): k_grad_norm_part writes one double per 4096-element chunk into `part` (rtx_grad_norm_parts(a) doubles), k_grad_norm_finish
// sums them in a fixed order and writes pair = {total, coef = min(1, max_norm / (total + 1e-6))} (NaN stays NaN) as float32 -- and, with
// `mailbox` (three 32-bit words of coherent host memory), {total bits, coef bits, seq, tag}, seq released at system scope.  norm_inf: max |G|.
// No atomics: two launches on the same data give the same bits.
long rtx_grad_norm_parts(const RtxAdamArgs& a);
int rtx_launch_grad_norm(const RtxAdamArgs& a, int norm_inf, float max_norm, double* part, float* pair, uint32_t* mailbox, uint32_t seq,
                         uint32_t tag, hipStream_t stream);
// the clip setting of an engine handle and the device memory behind it (rtx_engine_set_grad_clip / rtx_svae_set_grad_clip)
enum { RTX_CLIPM_NONE = 0, RTX_CLIPM_NORM2 = 1, RTX_CLIPM_NORMINF = 2, RTX_CLIPM_VALUE = 3 };
struct RtxClipState {
    int mode = RTX_CLIPM_NONE;
    double bound = 0;
    double* part = nullptr;       // device scratch of the partial sums
    long part_cap = 0;
    float* pair = nullptr;        // device {total, coef}
    uint32_t* mailbox = nullptr;  // coherent host memory {total bits, coef bits, ticket, tag}
    uint32_t ticket = 0;          // ticket of the last norm enqueued (monotonic)
    bool last_has_norm = false;   // the last optimizer launch computed a norm
};
int rtx_clip_validate(int mode, double bound, const char* who);
void rtx_clip_release(RtxClipState& cs);
// the optimizer launch of a handle: with a norm mode the norm pass and its finish in front of it, on the same stream; `tag`: the
// caller's step count for the mailbox.  rtx_clip_prepare is the part in front of rtx_launch_adam on its own: it enqueues the norm (if
// the mode has one) and fills a.clip / a.clip_value / a.clip_coef
int rtx_clip_prepare(RtxAdamArgs& a, RtxClipState& cs, uint32_t tag, hipStream_t stream);
int rtx_launch_clipped_adam(RtxAdamArgs& a, int is_bf16, RtxClipState& cs, uint32_t tag, hipStream_t stream);
int rtx_clip_wait_norm(RtxClipState& cs, const char* who, float* host2, double timeout_s, uint32_t* tag_out);
int rtx_launch_cast_f32_bf16(const float* src, bf16_t* dst, long n, hipStream_t stream);
// float32 parity mode: split-K slabs [splits][M_pad][ldc] of a small weight-gradient product -> gW [M_real][N_real], gbias [M_real] (column N_real)
int rtx_launch_dw_slab_reduce(const float* C, int splits, long slab_stride, long ldc, int M_real, int N_real, float* gW, float* gbias, hipStream_t stream);
// gradient accumulation: the same sum into accumulators -- add = 0: gW = scale * sum; add = 1: gW = fmaf(scale, sum, gW); gbias alike (required)
int rtx_launch_dw_slab_reduce_acc(const float* C, int splits, long slab_stride, long ldc, int M_real, int N_real, float* gW, float* gbias, int add,
                                  float scale, hipStream_t stream);
int rtx_launch_sumsq(const float* const* params_host, const long* sizes, int n, float* sumsq, hipStream_t stream);

// evaluate() on the device: exact top-kmax per score row + nDCG@k / Recall@k (+ hit@k / mrr@k when either pointer is given) for
// each cut-off in ks (host array)
int rtx_launch_topk_metrics(const float* scores, long ld, int B, int n_items, const RtxCsrView& held, const int* ks, int n_k,
                            int kmax, double* ndcg, double* recall, int32_t* topk, hipStream_t stream, long out_ld = 0, const RtxCsrView* excl = nullptr,
                            double* hit = nullptr, double* mrr = nullptr);
// recommend(): per score row (float32, or float64 with is_f64) the min(k, n_items) best items, score descending, item id ascending among
// equal scores (items [B][K], item_scores T [B][K] nullable); excl (nullable): batch row b's stored non-zero entries rank as -inf
int rtx_launch_topk_items(const void* scores, int is_f64, long ld, int B, int n_items, const RtxCsrView* excl, int k, int32_t* items,
                          void* item_scores, hipStream_t stream);
// metrics of ranked lists: items [n][ld], the first K of a row best first, against batch row b of `held` (a row id outside
// [0, held_rows) reads as an empty row); nDCG / Recall / hit / mrr @ ks[q] with kk = min(ks[q], K) into double [n_k][out_ld], each nullable
int rtx_launch_list_metrics(const int32_t* items, long ld, int n, int K, const RtxCsrView& held, long held_rows, const int* ks, int n_k,
                            double* ndcg, double* recall, double* hit, double* mrr, long out_ld, hipStream_t stream);
