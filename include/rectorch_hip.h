/*
 * rectorch_hip.h -- C ABI of librectorch_hip.so: the MI355X (gfx950) implementation of rectorch's
 * Mult-VAE / Mult-DAE training and scoring path.
 *
 * The reference (makgyver/rectorch) is pure Python and has no FFI; its boundary for this path is the
 * Python class API.  Each entry point below names the reference code it replaces.  The Python mirror
 * of that API (rectorch_amd/{nets,models,samplers}.py) binds these symbols with ctypes and exposes
 * them as torch.library ops; INTEGRATION.md shows the binding a rectorch maintainer would add.
 *
 * Conventions
 *   - plain C, no torch types.  Pointers are HIP DEVICE pointers unless the name ends in _host.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls only enqueue work.
 *   - return 0 on success, <0 (RTX_E*) on failure; rtx_last_error() gives the message (thread local).
 *   - the caller owns every buffer it passes.  An rtx_engine owns its compute-precision weight copies
 *     ("shadows"), activations and workspaces.  One engine per device, externally serialised.
 *   - parameter tensors are float32, [out,in] row-major, in the order of net.parameters():
 *     enc W0,b0,W1,b1,... then dec W0,b0,...   (reference rectorch/nets.py:260-270, 208-217)
 */
#ifndef RECTORCH_HIP_H
#define RECTORCH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_MAX_LAYERS 8

#define RTX_VAE 0 /* MultiVAE_net: last encoder layer emits mu|logvar, reparameterised z        */
#define RTX_DAE 1 /* MultiDAE_net: tanh on every encoder layer                                  */
#define RTX_GVAE 2 /* VAE_net (nets.py:250-353): the RTX_VAE layer layout on the RAW input rows (no normalisation, no
                    * dropout), z sampled in every mode (eval too), sigmoid output; training loss BCE + KL
                    * (models.py:581-583, no beta).  rtx_engine_forward returns the sigmoid probabilities            */
#define RTX_AE 3 /* AETrainer(MultiDAE_net) (models.py:325-516): the RTX_DAE layer layout and forward (normalised input,
                  * dropout in training, tanh on every layer but the decoder's last, raw outputs); training loss
                  * torch.nn.MSELoss against the target rows AS STORED (models.py:377, 441-447).  lam and beta of
                  * rtx_step are ignored; cond_dim must be 0; no data-parallel step                              */

#define RTX_FP32 0 /* parity mode: v_mfma_f32_32x32x2_f32, exact f32 products and sums           */
#define RTX_BF16 1 /* throughput mode: v_mfma_f32_32x32x16_bf16, f32 accumulate, f32 master params */

typedef struct rtx_engine rtx_engine;
typedef struct rtx_csr rtx_csr;

typedef struct {
    int32_t n_enc;                        /* Linear layers in the encoder                          */
    int32_t n_dec;                        /* Linear layers in the decoder                          */
    int32_t enc_dims[RTX_MAX_LAYERS + 1]; /* enc_dims[0] = n_items ... enc_dims[n_enc] = latent    */
    int32_t dec_dims[RTX_MAX_LAYERS + 1]; /* dec_dims[0] = latent  ... dec_dims[n_dec] = n_items   */
    int32_t variant;                      /* RTX_VAE | RTX_DAE | RTX_GVAE | RTX_AE                 */
    int32_t numerics;                     /* RTX_FP32 | RTX_BF16                                   */
    float dropout_p;                      /* nn.Dropout(p) on the normalised input (nets.py:392)   */
    int32_t max_batch;                    /* largest batch this engine will be given               */
    int32_t splitk;                       /* split-K factor for the two K = n_items GEMMs, 0 = auto */
    int32_t cond_dim;                     /* CMultiVAE_net (nets.py:455-480): the input rows carry cond_dim extra
                                           * columns after the n_items item columns; they enter the first encoder
                                           * layer raw (no normalisation, no dropout).  0 = MultiVAE / MultiDAE   */
} rtx_cfg;

/* A batch of users.  Either rows of a resident CSR matrix (fast path: nothing dense crosses the API)
 * or dense [batch][n_items] float32 device tensors.  With cfg.cond_dim > 0 the INPUT (csr / x_dense) has
 * n_items + cond_dim columns, the target keeps n_items and must be given (the conditioned samplers always do) (drop-in for train_batch(tr_batch, te_batch) /
 * predict(x), reference models.py:817-822, 619-624). */
typedef struct {
    const rtx_csr* csr;          /* input rows (NULL -> use x_dense)                                 */
    const int32_t* row_ids;      /* device int32 [batch] row numbers (NULL -> rows 0..batch-1)       */
    const rtx_csr* target_csr;   /* loss target rows, same row ids (NULL -> target = input)          */
    const float* x_dense;        /* device [batch][n_items]                                          */
    const float* target_dense;   /* device [batch][n_items] (NULL -> target = input)                 */
    int32_t batch;
} rtx_batch;

/* Per-step scalars: what MultiVAE.train_batch / MultiDAE + torch.optim.Adam hold (models.py:817-835,
 * 768-770, 657-659). */
typedef struct {
    float beta;                  /* VAE: KL weight after annealing (models.py:824-827)               */
    float lam;                   /* DAE: weight of sum_W ||W||_2   (models.py:702-706)               */
    float inv_batch;             /* scale of the batch mean: 1/B, or 1/B_global under data parallel  */
    float lr, beta1, beta2, eps, weight_decay; /* Adam hyper-parameters                              */
    int32_t step;                /* Adam step count t of THIS update (1-based)                       */
    int32_t flags;               /* RTX_STEP_* bits                                                   */
    uint64_t seed, offset;       /* Philox stream for dropout and the reparameterisation noise       */
    const uint8_t* dropout_mask; /* injected keep-mask [batch][n_items] (NULL -> Philox)             */
    const float* eps_noise;      /* injected N(0,1) draws [batch][latent]  (NULL -> Philox)          */
} rtx_step;
/* The draw contract of (seed, offset) -- every device path (dense or CSR batch, scatter image, sparse first layer, prefetched
 * batch, either VAE head) takes the same draws, so a seed reproduces a run whatever the knobs; tests/test_philox_draws.py pins it
 * to oracle/philox_oracle.py.  Philox4x32-10, counter = (index lo, index hi, offset lo, offset hi), key = (seed lo, seed hi),
 * words x y z w:
 *   dropout  element (b, i) of the batch -- b = POSITION in the batch (not the CSR row id), i < n_items -- has
 *            index = b * n_items + i (the real width: not the padded one, not n_items + cond_dim) and is kept iff
 *            float32((x >> 8) * 2^-24) >= dropout_p, kept values scaled by 1 / (1 - p).  Only stored item entries are decided:
 *            the cond_dim condition columns pass raw, never dropped.
 *   noise    element (b, j), j < latent: index = b * latent + j on the stream offset ^ 0x5851F42D4C957F2D (dropout and noise never
 *            share a stream), eps = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((x >> 8) + 0.5) * 2^-24, u2 = (y >> 8) * 2^-24, in float32.
 *   offset   distinguishes the calls that share a seed: under data parallelism it is the rank, so that the ranks drop different
 *            entries.  seed, offset and index are used as full 64-bit numbers.
 * An injected dropout_mask / eps_noise replaces the corresponding draws element for element (same layout). */

/* In bf16 numerics rtx_engine_train_step runs the Adam update of every weight matrix inside its weight-gradient
 * kernel (dw_adam.hip), so those gradients are never written to HBM; set this bit to ALSO store them in the bound
 * gradient buffers (p.grad in the Python mirror).  float32 numerics and rtx_engine_loss_grads always store them. */
#define RTX_STEP_KEEP_GRADS 1
/* Mult-DAE under data parallelism: the regulariser lam * sum ||W||_2 is the same on every rank, so only ONE rank may add
 * it to the loss it reports before the ranks' losses are summed; the others set this bit (the update itself is unchanged) */
#define RTX_STEP_NO_REG_IN_LOSS 2
/* rtx_engine_loss_grads in bf16 numerics with rtx_engine_bind_grads16 done: every gradient is written ONLY as the bf16 image the
 * data-parallel exchange sends (the float32 gradient buffers are not touched, no cast pass follows); the optimizer then reads
 * the reduced bf16 gradients (rtx_engine_apply_adam_layers / _rows with their grads_bf16 arguments) */
#define RTX_STEP_GRADS_BF16 8
/* ABI 7 -- rtx_engine_train_step (bf16, single GPU): do NOT make the caller's stream wait for the engine's side stream at the end
 * of the step.  The caller promises not to touch anything the step produces outside the engine (parameters, optimizer state, the
 * loss buffers) on any stream before its next call into this engine or rtx_engine_join(e, stream) -- every engine entry point
 * that takes a stream resolves the open join first; a following training step that starts from a prefetched batch
 * (rtx_engine_set_next_batch) resolves it INSIDE its first kernel, so two steps follow each other on the caller's stream without
 * a wait packet between them.  What an epoch loop wants (rectorch/models.py:409-419); train_batch's float (rtx_engine_wait_loss)
 * needs no join.
 * The same promise covers where the optimizer state LIVES (option "state_tiles", default 1).  Between two deferred fused steps -- plain
 * Adam, no clipping, no accumulation -- the exp_avg and exp_avg_sq of the large fused layers (weight matrices of at least
 * "state_tiles_min_elems" elements, default 2^20, whose rows hold at least 4 floats) live in an engine-owned image in the order the
 * weight-gradient + Adam kernel walks them, one contiguous 32-KB chunk per 64 x 128 tile and array; the bound exp_avg / exp_avg_sq
 * tensors of those layers are STALE meanwhile.  A deferred fused step is the only thing that leaves them so.  Every other entry point
 * -- a step without this flag, the unfused / clipped / accumulating / data-parallel steps, rtx_engine_loss_grads, the custom-loss
 * routes, forward / encode / decode / evaluate / recommend, rtx_engine_sync_shadows, rtx_engine_apply_adam*, rtx_engine_join, a second
 * rtx_engine_bind, rtx_engine_destroy -- first resolves the join and then writes the image back into the bound tensors, bit for bit
 * what the row-major kernel would have left there; the first deferred fused step behind a write-back imports the bound tensors again,
 * always (the caller may have changed them: load_state_dict, a checkpoint).  Parameters, biases and their moments never move.
 * rtx_engine_get_option "state_imports" / "state_writebacks" count the layers copied each way. */
#define RTX_STEP_DEFER_JOIN 16

/* called on the host right after the kernels producing the gradients of layer `layer` (its W and b)
 * have been enqueued; layers complete in reverse order (last decoder layer first).  A data-parallel
 * caller records an event here and starts the RCCL all-reduce of that bucket on a side stream. */
typedef void (*rtx_layer_cb)(int32_t layer, void* user);

const char* rtx_last_error(void);
int32_t rtx_abi_version(void);

/* ---- resident CSR matrices: replaces DataSampler's per-batch scipy row gather + toarray()
 *      (rectorch/samplers.py:97-105).  Column ids must be unique within a row. -------------------- */
int rtx_csr_upload(const int64_t* indptr_host, const int32_t* indices_host, const float* values_host,
                   int64_t n_rows, int32_t n_cols, rtx_csr** out); /* values_host NULL -> all 1.0 */
int rtx_csr_destroy(rtx_csr* m);
int rtx_csr_shape(const rtx_csr* m, int64_t* n_rows, int32_t* n_cols, int64_t* nnz);
/* dense float32 [batch][n_cols] image of the given rows: what DataSampler.__iter__ yields */
int rtx_csr_gather_dense(const rtx_csr* m, const int32_t* row_ids, int32_t batch, float* out, void* stream);

/* ---- conditioned batches built on the device (CMultiVAE; rectorch/samplers.py:108-419: ConditionedDataSampler,
 *      BalancedConditionedDataSampler, EmptyConditionedDataSampler) -- additive to ABI 8 ---------------------------------------
 * An EXAMPLE is (row r, condition c), c = -1 for "unconditioned".  Its input row is row r of `tr` with one entry 1.0 appended at
 * column n_items + c when c >= 0 (n_items + n_cond columns, ids sorted); its target row is row r of `te` (NULL = tr) restricted to
 * the items whose condition list holds c -- for c = -1 the items with at least one condition -- values as stored.
 * rtx_cond_create keeps REFERENCES to the two resident matrices (same shape; they must outlive the object), uploads the
 * item -> condition bitmap (HOST uint32 [n_items][W], W = ceil(n_cond / 32), bit c % 32 of word c / 32; any_host: HOST uint32
 * [ceil(n_items / 32)], bit i = item i has a condition; both NULL = targets are not filtered, the Empty sampler) and the example
 * table (HOST int32 [n_ex] each), counts every example's lengths on the device once, and allocates n_slots (3..64) pairs of CSR
 * matrices of up to max_batch rows: input [n_items + n_cond columns] and target [n_items columns], `values` NULL (implicit ones)
 * where the source matrix has none.  A slot's max_row_len is the source matrix's (+ 1 for the input): an upper bound.
 * rtx_cond_lengths: per example the input length (stored entries + the condition entry) and the filtered target length, into HOST
 * buffers of n_ex int32 (either nullable); an example whose target length is 0 is one the samplers drop.
 * rtx_cond_build enqueues on `stream` the two kernels that write slot `slot` from the examples ex_ids[0 .. batch) (device int32;
 * batch <= max_batch; an id outside [0, n_ex) gives an empty row): row b of both matrices belongs to example ex_ids[b].  nnz_in /
 * nnz_target: the batch's entry counts when the caller knows them (sums of rtx_cond_lengths), -1 = unknown (an upper bound is
 * recorded).  Nothing is copied or computed on the host per batch.  The slot's earlier content is overwritten WITHOUT waiting for
 * its readers: with one batch of look-ahead in front of rtx_engine_train_step (RTX_STEP_DEFER_JOIN + rtx_engine_set_next_batch)
 * the two batches before the one being built can still be read from the engine's side stream, so consecutive batches must go to
 * at least 3 slots in turn (csrc/cond_rows.hip has the argument); other consumers on `stream` itself are ordered by the stream.
 * rtx_cond_slot: the slot's two handles.  Their addresses never change; they belong to the rtx_cond (never rtx_csr_destroy them)
 * and are consumed like uploaded matrices: rtx_batch.csr / target_csr with row ids 0 .. batch-1, rtx_csr_gather_dense,
 * rtx_topk_metrics, rtx_topk_items. */
typedef struct rtx_cond rtx_cond;
int rtx_cond_create(const rtx_csr* tr, const rtx_csr* te, int32_t n_cond, const uint32_t* bitmap_host, const uint32_t* any_host,
                    const int32_t* ex_row_host, const int32_t* ex_cond_host, int64_t n_ex, int32_t max_batch, int32_t n_slots,
                    rtx_cond** out);
int rtx_cond_destroy(rtx_cond* c);
int rtx_cond_lengths(const rtx_cond* c, int32_t* in_len_host, int32_t* target_len_host);
int rtx_cond_build(rtx_cond* c, int32_t slot, const int32_t* ex_ids, int32_t batch, int64_t nnz_in, int64_t nnz_target, void* stream);
int rtx_cond_slot(const rtx_cond* c, int32_t slot, const rtx_csr** in, const rtx_csr** target);

/* ---- engine ------------------------------------------------------------------------------------ */
int rtx_engine_create(const rtx_cfg* cfg, rtx_engine** out);
int rtx_engine_destroy(rtx_engine* e);
int32_t rtx_engine_n_tensors(const rtx_engine* e);
/* shape of parameter tensor t: rows = out features, cols = in features (1 for a bias) */
int rtx_engine_tensor_shape(const rtx_engine* e, int32_t t, int32_t* rows, int32_t* cols);
/* bind the float32 master parameters, gradient buffers and Adam moments (exp_avg / exp_avg_sq of
 * torch.optim.Adam's state) -- one device pointer per tensor.  grads/moments may be NULL for an
 * inference-only engine. */
int rtx_engine_bind(rtx_engine* e, float* const* params, float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq);
/* refresh the compute-precision copies after the master parameters were changed from outside
 * (load_state_dict, reference models.py:513) */
/* bf16 gradient images, one per tensor in parameter order, same shapes as the float32 gradients (weights [out][in] row-major);
 * NULL unbinds.  Used by steps flagged RTX_STEP_GRADS_BF16. */
int rtx_engine_bind_grads16(rtx_engine* e, uint16_t* const* grads_bf16);
int rtx_engine_sync_shadows(rtx_engine* e, void* stream);

/* VAE_net.forward / AE_net.forward (nets.py:322-339, 82-91) and VAE.predict / AETrainer.predict
 * (models.py:619-625, 467-473).  logits [batch][n_items]; mu/logvar [batch][latent] (VAE, nullable).
 * training != 0 applies dropout and samples z (uses step->seed/offset or the injected draws). */
int rtx_engine_forward(rtx_engine* e, const rtx_batch* batch, int32_t training, const rtx_step* step,
                       int32_t remove_train, float* logits, float* mu, float* logvar, void* stream);
/* MultiVAE_net.encode / MultiDAE_net.encode (nets.py:394-405, 219-225):
 * VAE: out0 = mu, out1 = logvar; DAE: out0 = h, out1 unused.  [batch][latent] */
int rtx_engine_encode(rtx_engine* e, const rtx_batch* batch, int32_t training, const rtx_step* step, float* out0,
                      float* out1, void* stream);
/* MultiVAE_net.decode / MultiDAE_net.decode (nets.py:413-417, 227-233): z [batch][latent] -> logits */
int rtx_engine_decode(rtx_engine* e, const float* z, int32_t batch, float* logits, void* stream);

/* forward + loss_function + backward of train_batch (models.py:829-832): gradients land in the bound
 * grad buffers; loss_out[0] = loss (device float, nullable); loss_accum[0] += loss (nullable). */
int rtx_engine_loss_grads(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* loss_out,
                          float* loss_accum, rtx_layer_cb cb, void* user, void* stream);
/* ---- a loss computed OUTSIDE the engine (additive to ABI 8): train_batch's  forward -> loss_function -> loss.backward()
 *      (models.py:829-832) with a loss_function the engine does not know.  Single GPU only: RTX_EINVAL while a data-parallel
 *      plan is attached (the route has no exchange).
 * rtx_engine_forward_train: the TRAINING-mode forward of rtx_engine_loss_grads / rtx_engine_train_step -- dropout and the sampled
 * z from step->seed / offset or the injected dropout_mask / eps_noise, the draws of the fused step under the contract above -- that
 * leaves every activation the backward needs in the engine and writes the public outputs: out [batch][n_items] float32 (the logits;
 * RTX_GVAE: their sigmoid, as VAE_net.decode returns it) and, for the VAE variants, mu / logvar [batch][latent] (nullable).
 * The batch needs no target.  *ticket names the activations: every engine entry point that overwrites them (another forward of any
 * kind, encode, decode, evaluate / recommend, a training step) makes it stale; tickets of different engines never coincide.
 * rtx_engine_backward: the backward chain of rtx_engine_loss_grads on ONE stream, started from the caller's gradient instead of a
 * built-in loss: d_out float32 [batch][ld >= n_items] = d loss / d out (RTX_GVAE: w.r.t. the sigmoid outputs; the engine applies
 * p (1 - p) from its logits), d_mu / d_logvar float32 [batch][latent] = d loss / d mu, d loss / d logvar (VAE variants; both NULL =
 * the loss does not depend on them; the chain through z = mu + eps exp(logvar / 2) is the engine's).  `batch` and `step` are those
 * of the forward.  Gradients land in the bound gradient buffers (overwritten, not accumulated); cb as in rtx_engine_loss_grads.
 * The caller's gradient carries its own scale: step->inv_batch, beta and lam are not read.  RTX_ESTATE, with nothing enqueued, when
 * the ticket is stale.  The optimizer is the caller's, or rtx_engine_apply_adam with lam = 0 (a regulariser is part of the caller's
 * loss, and its gradient of the caller's backward). */
int rtx_engine_forward_train(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* out, float* mu, float* logvar,
                             uint64_t* ticket, void* stream);
int rtx_engine_backward(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, uint64_t ticket, const float* d_out, int64_t ld,
                        const float* d_mu, const float* d_logvar, rtx_layer_cb cb, void* user, void* stream);
/* ---- the same route cut in two at z (additive to ABI 8): a forward composed by the caller from the reference's three pieces,
 *      mu, logvar = encode(x); z = sampling(mu, logvar); out = decode(z)   (nets.py:394-417), with any sampling in between.
 *      Single GPU only, gradient buffers bound (RTX_EINVAL / RTX_ESTATE otherwise, as above).
 * rtx_engine_encode_train: layers [0, n_enc) in training mode (dropout from step->seed / offset or the injected mask; the batch needs
 * no target); out0 / out1 as rtx_engine_encode writes them (VAE variants: mu, logvar; RTX_DAE / RTX_AE: h, out1 unused).  The
 * activations stay in the engine under *ticket.
 * rtx_engine_encode_backward: layers n_enc-1 .. 0 of the backward chain from d_out0 / d_out1 float32 [batch][latent] UNPADDED =
 * d loss / d mu, d loss / d logvar (VAE variants: both; no d z enters here -- the chain through a sampled z is the caller's,
 * rtx_reparam_grad) or d loss / d h (RTX_DAE / RTX_AE: d_out1 NULL; the engine applies 1 - h^2).  Weight and bias gradients of the
 * encoder layers land in the bound buffers; the decoder layers' buffers are not touched.
 * rtx_engine_decode_train: z float32 [n][latent] -> out [n][n_items] (RTX_GVAE: the sigmoid of the logits, which stay in the engine)
 * through layers [n_enc, n_layers), activations kept under *ticket.  n is any batch in [1, max_batch], independent of the
 * encoder's: K samples per user are ONE decode of K * batch rows.
 * rtx_engine_decode_backward: layers n_layers-1 .. n_enc from d_out [n][ld >= n_items] (as rtx_engine_backward takes it): the
 * decoder layers' gradients into the bound buffers, and d_z float32 [n][latent] UNPADDED = d loss / d z (nullable: NULL skips its
 * product).  `step` as in rtx_engine_backward (no field of it scales anything).
 * Tickets, one per half: a run of the encoder layers makes the encoder ticket stale AND the decoder ticket (the encoder's last layer
 * writes the decoder's input operand); a run of the decoder layers makes the decoder ticket stale.  So encode -> decode ->
 * decode_backward -> encode_backward is valid, and a second encode (or decode) before the backward makes the first ticket stale:
 * stack several views or samples as ONE batch.  Every other forward, prediction, evaluation or training step makes both stale, and
 * either of these forwards makes the ticket of rtx_engine_forward_train stale.  A stale ticket: RTX_ESTATE, nothing enqueued. */
int rtx_engine_encode_train(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* out0, float* out1, uint64_t* ticket,
                            void* stream);
int rtx_engine_encode_backward(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, uint64_t ticket, const float* d_out0,
                               const float* d_out1, rtx_layer_cb cb, void* user, void* stream);
int rtx_engine_decode_train(rtx_engine* e, const float* z, int32_t n, float* out, uint64_t* ticket, void* stream);
int rtx_engine_decode_backward(rtx_engine* e, int32_t n, const rtx_step* step, uint64_t ticket, const float* d_out, int64_t ld,
                               float* d_z, rtx_layer_cb cb, void* user, void* stream);
/* The VAE head's sampling step as an operator of its own, on any float32 [n][latent] (contiguous): z = mu + eps exp(logvar / 2) --
 * the head's own expression, compiled from the same helper -- with eps = eps_in[b][j] (nullable) or the fused head's draw for
 * (seed, offset) at index b * latent + j; eps_out (nullable) receives the draws for rtx_reparam_grad:
 * d_mu = d_z, d_logvar = d_z eps exp(logvar / 2) / 2 (either nullable). */
int rtx_reparam(const float* mu, const float* logvar, int32_t n, int32_t latent, const float* eps_in, uint64_t seed, uint64_t offset,
                float* z, float* eps_out, void* stream);
int rtx_reparam_grad(const float* d_z, const float* logvar, const float* eps, int32_t n, int32_t latent, float* d_mu, float* d_logvar,
                     void* stream);
/* optimizer.step() (models.py:833): the fused multi-tensor update of the engine's optimizer over the bound tensors + shadow refresh */
int rtx_engine_apply_adam(rtx_engine* e, const rtx_step* step, void* stream);
/* The optimizer of a handle (torch 2.10 torch.optim, single-tensor form; default: Adam with coupled weight decay, which is what an
 * engine nobody sets an optimizer on runs, bit for bit as before).  lr, eps, weight_decay, beta1 / beta2 and the 1-based step keep
 * coming from rtx_step.  The two state tensors per parameter are the `m` / `v` buffers of rtx_engine_bind / rtx_svae_bind:
 *   RTX_OPTIM_ADAM     m = exp_avg, v = exp_avg_sq; RTX_OPTIM_DECOUPLED (AdamW): p <- p (1 - lr wd) first, no decay in the gradient
 *   RTX_OPTIM_SGD      m = momentum_buffer (momentum != 0; untouched otherwise), v untouched.  RTX_OPTIM_NESTEROV; RTX_OPTIM_FIRST:
 *                      the parameters' first update, buf = g without dampening (torch clones the gradient there) -- the caller
 *                      clears the bit before the second update
 *   RTX_OPTIM_ADAGRAD  v = sum, m untouched; clr = lr / (1 + (step - 1) lr_decay)
 *   RTX_OPTIM_RMSPROP  v = square_avg, m = momentum_buffer (momentum != 0), centered off
 * A buffer named "untouched" is neither read nor written, but must still be bound.  With anything but plain Adam,
 * rtx_engine_train_step runs the schedule of the knob "fuse_adam" = 0 (gradients stored, one optimizer launch behind them), in bf16
 * too; rtx_engine_apply_adam and rtx_svae_apply_adam run the rule; the data-parallel entry points (rtx_engine_dp_attach,
 * rtx_engine_train_step_dp, rtx_engine_apply_adam_layers / _rows) return RTX_EINVAL. */
#define RTX_OPTIM_ADAM 0
#define RTX_OPTIM_SGD 1
#define RTX_OPTIM_ADAGRAD 2
#define RTX_OPTIM_RMSPROP 3
#define RTX_OPTIM_DECOUPLED 1
#define RTX_OPTIM_NESTEROV 2
#define RTX_OPTIM_FIRST 4
typedef struct {
    int32_t kind;                /* RTX_OPTIM_ADAM / _SGD / _ADAGRAD / _RMSPROP                       */
    int32_t flags;               /* RTX_OPTIM_DECOUPLED | RTX_OPTIM_NESTEROV | RTX_OPTIM_FIRST        */
    double momentum, dampening;  /* SGD (momentum: RMSprop too).  Doubles, as torch holds them: 1 - dampening and 1 - alpha are  */
    double alpha;                /* RMSprop                        formed in double and rounded to float32 once, as torch does  */
    double lr_decay;             /* Adagrad                                                           */
} rtx_optim;
int rtx_engine_set_optimizer(rtx_engine* e, const rtx_optim* optim);
/* Gradient clipping on the device (additive to ABI 8): torch 2.10 torch.nn.utils.clip_grad_norm_ (norm_type 2 or inf) and
 * clip_grad_value_ in front of the optimizer launch of rtx_engine_train_step and rtx_engine_apply_adam.  What is clipped is the
 * gradient G of the loss: the stored gradient (times the launch's gradient scale) PLUS Mult-DAE's regulariser term lam p / ||p||,
 * which the optimizer kernel forms itself; weight decay, coupled or decoupled, is added after the clip, as torch adds it inside
 * optimizer.step().
 *   RTX_CLIP_NORM2    total = sqrt(sum over all tensors of G^2), accumulated in double in a fixed order (bit-equal between runs);
 *                     coef = bound / (total + 1e-6) in float32, clamped above at 1 (a NaN stays a NaN); G <- G coef, always
 *   RTX_CLIP_NORMINF  total = max |G| (NaN-propagating); the rest as above
 *   RTX_CLIP_VALUE    G <- clamp(G, -bound, +bound), a NaN stays a NaN; no reduction
 * bound: >= 0; inf with a norm mode computes and reports the norm and clips nothing.  The bound gradient buffers keep the UNCLIPPED
 * gradient, without the regulariser term.  With a mode set rtx_engine_train_step runs the schedule of the knob "fuse_adam" = 0
 * (gradients stored; norm pass, its one-workgroup finish and the optimizer launch behind them on the caller's stream), in bf16 too;
 * the coefficient stays on the device.  May be called between any two steps.  The data-parallel entry points (rtx_engine_dp_attach,
 * rtx_engine_train_step_dp, rtx_engine_apply_adam_layers / _rows) return RTX_EINVAL with a mode set, and this call does under an
 * attached plan: the norm of the reduced gradient needs every bucket before the first optimizer pass.
 * rtx_engine_wait_grad_norm: host[0] = total, host[1] = coef of the LAST optimizer step enqueued (`step`: its count, checked), read
 * from coherent host memory like rtx_engine_wait_loss -- the stream is not drained; RTX_ESTATE when that step had no norm mode. */
#define RTX_CLIP_NONE 0
#define RTX_CLIP_NORM2 1
#define RTX_CLIP_NORMINF 2
#define RTX_CLIP_VALUE 3
int rtx_engine_set_grad_clip(rtx_engine* e, int32_t mode, double bound);
int rtx_engine_wait_grad_norm(rtx_engine* e, int32_t step, float* host, double timeout_s);
/* Gradient accumulation on the device (additive to ABI 8): several micro-batches per optimizer update, torch's
 * `(loss / k).backward()` k times in front of one `optimizer.step()`.  The accumulators are the bound gradient buffers.  With a mode
 * set, every weight-gradient product of rtx_engine_loss_grads, rtx_engine_train_step and of the external-loss route
 * (rtx_engine_backward / _encode_backward / _decode_backward) weights its gradient g into them instead of storing over them:
 *   RTX_ACCUM_FIRST   acc = scale * g               (opens a window: what the buffers held is overwritten)
 *   RTX_ACCUM_ADD     acc = fmaf(scale, g, acc)     (one rounding per element and micro-step; RTX_ESTATE when no RTX_ACCUM_FIRST pass
 *                                                    has run since the last optimizer launch or since the handle was created)
 *   RTX_ACCUM_OFF     the plain store, bit for bit the code path of a handle this was never called on
 * scale: finite, typically 1 / k.  A window: rtx_engine_loss_grads for every micro-batch but the last (forward, loss, backward on the
 * caller's stream, no optimizer), then rtx_engine_train_step, which with a mode set runs the schedule of the knob "fuse_adam" = 0 --
 * gradients into the accumulators, then norm / clip if set and ONE optimizer launch reading them -- in bf16 too; or
 * rtx_engine_apply_adam for a window that ends early.  Mult-DAE's regulariser term and the weight decay are formed by the optimizer
 * launch, once per window.  The mode holds for ONE backward pass: rtx_engine_loss_grads and the optimizer launch set it back to
 * RTX_ACCUM_OFF (the window stays open until the optimizer launch); behind the external-loss entries, where one pass may be two calls
 * (decode then encode), the caller sets RTX_ACCUM_OFF.  What a window holds is tracked per layer: RTX_ACCUM_ADD on a layer that no
 * pass of this window has written yet stores scale * g, so a backward of one half never adds into stale data of the other.
 * Every loss reduction takes a mailbox ticket of
 * its own, so rtx_engine_wait_loss returns the LAST micro-batch's loss although a window's micro-steps share step->step.
 * RTX_EINVAL under an attached data-parallel plan (and rtx_engine_dp_attach / rtx_engine_train_step_dp with a mode set). */
#define RTX_ACCUM_OFF 0
#define RTX_ACCUM_FIRST 1
#define RTX_ACCUM_ADD 2
int rtx_engine_set_grad_accum(rtx_engine* e, int32_t mode, float scale);
/* the global norm of n <= 32 float32 device tensors (sizes: HOST array, elements, each < 2^31) as an operator of its own: norm_type 2
 * or inf, one float32 into out_dev (device); the clipping norm's kernels, so the same bits on every call */
int rtx_grad_norm(const float* const* tensors, const int64_t* sizes, int32_t n, double norm_type, float* out_dev, void* stream);
/* the same update restricted to layers [layer_lo, layer_hi) (network order, encoder first).  A data-parallel caller
 * applies it bucket by bucket, each as soon as that bucket's gradient all-reduce has landed, on its own stream, so the
 * optimizer pass of the decoder matrix hides under the exchange of the encoder matrix.  grads_bf16 (nullable): one
 * pointer per bound tensor (2 per layer, ALL layers, W then b) to a bf16 image of the reduced gradient, read instead
 * of the float32 gradient buffers (bf16 gradient exchange halves the bytes on xGMI and the Adam read). */
int rtx_engine_apply_adam_layers(rtx_engine* e, const rtx_step* step, int32_t layer_lo, int32_t layer_hi,
                                 const uint16_t* const* grads_bf16, void* stream);
/* Sharded optimizer for data parallelism (reduce-scatter -> Adam on the local rows -> all-gather of the compute copy):
 * the update of rows [row_lo, row_hi) of layer `layer`'s weight matrix (row_hi may reach into the row padding) and,
 * with with_bias, of its whole (replicated) bias.  w_grad_bf16 / b_grad_bf16 (nullable): bf16 images of the reduced
 * gradients of the weight matrix (element 0 = row 0) and of the bias, read instead of the bound float32 buffers. */
int rtx_engine_apply_adam_rows(rtx_engine* e, const rtx_step* step, int32_t layer, int32_t row_lo, int32_t row_hi,
                               int32_t with_bias, const uint16_t* w_grad_bf16, const uint16_t* b_grad_bf16, void* stream);
/* the compute copy of layer `layer`'s weight matrix in HBM: [padded_rows][ld] elements of elem_bytes bytes (bf16 or
 * float32), padded_rows a multiple of 128; valid until the next rtx_engine_train_step (which may swap buffers) */
int rtx_engine_shadow_region(rtx_engine* e, int32_t layer, void** base, int32_t* padded_rows, int32_t* ld, int32_t* elem_bytes);
/* ---- RCCL hooks: what a host that is not Python needs for the data-parallel step.  One communicator
 * per process / GPU; RCCL (librccl.so) is bound at run time on first use.  Rank 0 creates the id, the host distributes
 * its RTX_COMM_ID_BYTES bytes out of band, every rank calls rtx_comm_init.  All collectives are IN PLACE and enqueue on
 * `stream`: a step is  rtx_engine_loss_grads -> rtx_comm_allreduce[_many] of the gradient buffers (or
 * rtx_comm_reduce_scatter of a weight matrix's padded region) -> rtx_engine_apply_adam[_layers|_rows] ->
 * rtx_comm_allgather of rtx_engine_shadow_region when the optimizer is sharded. */
#define RTX_COMM_ID_BYTES 128
typedef struct rtx_comm rtx_comm;
int rtx_comm_unique_id(uint8_t* id_out /* [RTX_COMM_ID_BYTES], host */);
int rtx_comm_init(const uint8_t* id /* host */, int32_t rank, int32_t world, rtx_comm** out);
int rtx_comm_destroy(rtx_comm* c);
int rtx_comm_rank(const rtx_comm* c, int32_t* rank, int32_t* world);
/* sum over the ranks of n elements (dtype RTX_FP32 or RTX_BF16) */
int rtx_comm_allreduce(rtx_comm* c, void* buf, int64_t n, int32_t dtype, void* stream);
/* the same for several buffers in one RCCL group (the per-tensor gradient buffers of an engine); bufs / counts: HOST arrays */
int rtx_comm_allreduce_many(rtx_comm* c, void* const* bufs, const int64_t* counts, int32_t n_bufs, int32_t dtype, void* stream);
/* n_total elements = world equal blocks; afterwards block `rank` holds the sum of that block over the ranks */
int rtx_comm_reduce_scatter(rtx_comm* c, void* buf, int64_t n_total, int32_t dtype, void* stream);
/* bytes_total = world equal blocks; block r is replaced by rank r's block on every rank */
int rtx_comm_allgather(rtx_comm* c, void* buf, int64_t bytes_total, void* stream);

/* several collectives issued between start and end go to RCCL as one group (ncclGroupStart / ncclGroupEnd) */
int rtx_comm_group_start(rtx_comm* c);
int rtx_comm_group_end(rtx_comm* c);

/* ---- the data-parallel step scheduled by the ENGINE (round 3; the reference has no counterpart) ----------------
 * rtx_engine_train_step_dp is train_batch for one rank of a data-parallel job: forward + loss + backward on this rank's
 * users (step->inv_batch = 1 / GLOBAL batch), the gradient exchange and the optimizer, all enqueued by ONE call -- no host
 * callback, no per-bucket event created per step.  The gradients leave the weight-gradient kernels as the images the
 * collectives send (engine-owned exchange buffer, comm_dtype), in two buckets: the decoder matrix (+ its bias) on the engine's
 * side stream beside the data-gradient chain, everything else behind the chain on the caller's stream.
 *   sharded = 0: all-reduce, then Adam on every rank (replicated weights stay bit-identical);
 *   sharded = 1: a big weight matrix's region (rows padded to a multiple of 128: equal blocks) is reduce-scattered, Adam runs
 *                on this rank's rows only -- the optimizer's 28 B/param of HBM traffic shrink by the number of ranks -- and the
 *                compute copy is all-gathered in place; biases and small layers are all-reduced and replicated.  The float32
 *                master rows / Adam moments of the OTHER ranks' rows go stale on this rank (rtx_engine_dp_owned_rows says which
 *                rows are current); gather them before reading parameters from the host side.
 * Collectives: an RCCL communicator (rtx_comm_init), or caller-supplied functions (any transport: the tests use
 * torch.distributed/gloo), or -- emulate = 1 -- none at all: every collective is replaced by device copies of the bytes one
 * rank of `world` would move and Adam runs on 1/world of the rows: the HBM cost of rank 0's step on ONE GPU (timing only: the
 * other ranks' rows are never updated). */
typedef struct {
    /* all IN PLACE on `buf`, enqueued on `stream`; dtype RTX_FP32 | RTX_BF16; return 0 on success.
     * reduce_scatter: n_total = world equal blocks, block `rank` receives the sum; all_gather: bytes_total = world equal
     * blocks, block r is replaced by rank r's */
    int (*all_reduce)(void* ctx, void* buf, int64_t n, int32_t dtype, void* stream);
    int (*reduce_scatter)(void* ctx, void* buf, int64_t n_total, int32_t dtype, void* stream);
    int (*all_gather)(void* ctx, void* buf, int64_t bytes_total, void* stream);
    int (*group_start)(void* ctx); /* nullable */
    int (*group_end)(void* ctx);   /* nullable */
    void* ctx;
} rtx_dp_ops;
typedef struct {
    int32_t rank, world;
    int32_t sharded;       /* 0 | 1 (above) */
    int32_t comm_dtype;    /* RTX_FP32 (exact sums: parity) | RTX_BF16 (half the bytes on xGMI) */
    int32_t emulate;       /* 1: no communicator, device copies of the same size (timing of rank 0's step on one GPU) */
    rtx_comm* comm;        /* RCCL communicator, or NULL when ops / emulate is given */
    const rtx_dp_ops* ops; /* caller-supplied collectives (copied), or NULL */
    /* ABI 7: the collectives of bucket A (the decoder matrix, issued on the engine's SIDE stream beside the data-gradient
     * chain) go through a communicator / function table of their own, so that RCCL's per-communicator serialisation cannot
     * couple them with bucket B's collectives on the caller's stream (with ONE communicator used from two streams RCCL runs
     * the operations in issue order: bucket B's reduce would wait for bucket A's all-gather).  NULL = bucket A shares
     * comm / ops (the single-communicator schedule of ABI 5-6).  Every rank must make the same choice. */
    rtx_comm* comm_side;        /* second RCCL communicator of the same ranks (rtx_comm_init with a second id), or NULL */
    const rtx_dp_ops* ops_side; /* caller-supplied collectives for the side stream (copied), or NULL */
    int32_t shard_min_elems;    /* sharded = 1: weight matrices of at least this many elements are sharded; 0 = the engine's
                                 * default (2^20, or what the option "dp_shard_min_elems" says) */
} rtx_dp_cfg;
int rtx_engine_dp_attach(rtx_engine* e, const rtx_dp_cfg* cfg /* NULL detaches */);
int rtx_engine_train_step_dp(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* loss_out, float* loss_accum,
                             void* stream);
/* rows [row_lo, row_hi) of layer `layer`'s weight matrix whose float32 master / Adam state this rank keeps current
 * (everything when the layer is not sharded); sharded_out: 1 if the layer is sharded */
int rtx_engine_dp_owned_rows(const rtx_engine* e, int32_t layer, int32_t* row_lo, int32_t* row_hi, int32_t* sharded_out);

/* float32 -> bfloat16 (round to nearest even) of n contiguous elements: stages a gradient bucket for a bf16 all-reduce */
int rtx_cast_f32_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);
/* ABI 7 -- THIS step's loss without draining the stream (the reference's train_batch ends in `return loss.item()`,
 * models.py:835).  With the mailbox enabled the loss reduction of every training step ALSO stores {loss, ticket, step->step} into
 * coherent host memory owned by the engine (the ticket is the engine's own monotonic count of reductions: a step count that restarts
 * or repeats cannot match a stale entry); rtx_engine_wait_loss(step) spins on the host until the mailbox carries the ticket of the
 * LAST step enqueued, checks that this is step `step` (RTX_ESTATE otherwise) and returns its loss: the kernels behind the loss
 * (weight gradients, Adam) keep running and the host can enqueue the next step under them.  timeout_s <= 0: 60 s.  Steps are
 * waited for in order, each before the next is enqueued (the mailbox holds the LAST step's loss). */
int rtx_engine_loss_mailbox(rtx_engine* e, int32_t enable);
int rtx_engine_wait_loss(rtx_engine* e, int32_t step, float* loss_host, double timeout_s);
/* ABI 7 -- announce the batch of the training step AFTER the next rtx_engine_train_step call (and its dropout stream: seed /
 * offset / dropout_mask of next_step; the other fields are ignored).  That call then also gathers the announced batch, on the
 * engine's side stream under its last weight-gradient + Adam launch, into a second batch image; the step that is then given
 * exactly this batch (same csr / target_csr / row_ids pointers, batch, seed, offset, mask) starts with the first-layer product.
 * A hint only: any other batch is gathered by its own step.  The announced row ids must stay unchanged until that step.  NULL
 * cancels.  bf16 numerics, resident CSR batches; the single-GPU fused step gathers under its last weight kernel, the data-parallel
 * step (rtx_engine_train_step_dp, since round 6) behind bucket A on its side stream.  The reference densifies every batch on the
 * host (samplers.py:99-100). */
int rtx_engine_set_next_batch(rtx_engine* e, const rtx_batch* next, const rtx_step* next_step);
/* resolves a join left open by a step flagged RTX_STEP_DEFER_JOIN: `stream` continues only after everything that step put on
 * the engine's side stream, and after the tile-major optimizer state such steps keep (see RTX_STEP_DEFER_JOIN) has been written back
 * into the bound exp_avg / exp_avg_sq tensors (no-op when nothing is open) */
int rtx_engine_join(rtx_engine* e, void* stream);
/* both of the above: one full train_batch */
int rtx_engine_train_step(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* loss_out,
                          float* loss_accum, void* stream);

/* MultiVAE.loss_function / MultiDAE's likelihood term on dense tensors (models.py:813-815):
 * loss_out[0] = mean_b(s_b*LSE_b - <x_b, y_b>) + beta * KLD   (mu/logvar NULL -> no KL term) */
int rtx_multinomial_loss(const float* recon, const float* x, int32_t batch, int32_t n_items, const float* mu,
                         const float* logvar, int32_t latent, float beta, float* loss_out, void* stream);

/* VAE.loss_function (models.py:581-583) on dense tensors: recon = the sigmoid probabilities p, x = the target.
 * loss_out[0] = mean over all batch * n_items elements of (x - 1) max(log1p(-p), -100) - x max(log p, -100)
 *               - 0.5 mean_b sum_z (1 + logvar - mu^2 - exp(logvar))   (mu/logvar NULL -> no KL term) */
int rtx_bce_kl_loss(const float* recon, const float* x, int32_t batch, int32_t n_items, const float* mu, const float* logvar,
                    int32_t latent, float* loss_out, void* stream);

/* AETrainer.loss_function (models.py:377: torch.nn.MSELoss()(ground_truth, prediction)) on dense [batch][n_items] tensors, rows
 * of any alignment: loss_out[0] = mean over all batch * n_items elements of (ground_truth - prediction)^2.
 * RTX_EINVAL when batch * n_items == 0. */
int rtx_mse_loss(const float* prediction, const float* ground_truth, int32_t batch, int32_t n_items, float* loss_out, void* stream);

/* the regulariser of MultiDAE.loss_function (models.py:702-706): out[0] = sum_t ||tensor_t||_2.
 * `tensors` is a HOST array of n device pointers, `sizes` a HOST array of element counts. */
int rtx_sum_l2_norms(const float* const* tensors, const int64_t* sizes, int32_t n, float* out, void* stream);

/* The four operators above with their gradients (additive to ABI 8): loss_out[0] / out[0] is the value of the entry of the same
 * name without _grad, to the bit, and the same launch writes the gradients at UNIT upstream gradient (a caller multiplies by its own):
 *   multinomial:  d_recon = (s_b softmax(recon_b)_i - x_bi) / batch, s_b = sum_i x_bi (a row without a target: zeros);
 *                 d_mu = beta mu / batch;  d_logvar = beta (exp(logvar) - 1) / (2 batch)
 *   bce_kl:       d_recon = (p - x) / max(p (1 - p), 1e-12) / (batch n_items)  (F.binary_cross_entropy's backward: finite at p = 0, 1);
 *                 d_mu = mu / batch;  d_logvar = (exp(logvar) - 1) / (2 batch)
 *   mse:          d_prediction = 2 (prediction - ground_truth) / (batch n_items)
 *   sum_l2_norms: grads[t] = tensors[t] / ||tensors[t]||_2, zeros where the norm is zero (torch's norm backward); `grads` is a HOST
 *                 array of n device pointers, grads[t] as large as tensors[t]
 * No gradient w.r.t. the targets.  d_recon / d_prediction: device float32 [batch][n_items] like their operand, rows of any alignment
 * (16-byte accesses when operand, target and gradient bases are 16-byte aligned and n_items % 4 == 0).  d_mu and d_logvar are NULL
 * exactly when mu and logvar are (RTX_EINVAL otherwise); every other check is that of the entry without _grad. */
int rtx_multinomial_loss_grad(const float* recon, const float* x, int32_t batch, int32_t n_items, const float* mu,
                              const float* logvar, int32_t latent, float beta, float* loss_out, float* d_recon, float* d_mu,
                              float* d_logvar, void* stream);
int rtx_bce_kl_loss_grad(const float* recon, const float* x, int32_t batch, int32_t n_items, const float* mu, const float* logvar,
                         int32_t latent, float* loss_out, float* d_recon, float* d_mu, float* d_logvar, void* stream);
int rtx_mse_loss_grad(const float* prediction, const float* ground_truth, int32_t batch, int32_t n_items, float* loss_out,
                      float* d_prediction, void* stream);
int rtx_sum_l2_norms_grad(const float* const* tensors, const int64_t* sizes, int32_t n, float* out, float* const* grads, void* stream);

/* Device-side consumer of predict() for evaluation.evaluate (rectorch/evaluation.py:100-106 + rectorch/metrics.py:
 * 136-147, 187-196): per user the exact top-max(ks) of the score row, then nDCG@k and Recall@k for every cut-off
 * against that user's held-out CSR row (column ids sorted).  ndcg / recall: device double [n_k][batch] (nullable);
 * topk_idx: device int32 [batch][max(ks, kmax)] sorted by descending score (nullable).  ks_host is a HOST array. */
/* evaluation.evaluate's whole loop (rectorch/evaluation.py:100-106) in ONE call: for every batch i, the users
 * row_ids[batch_offsets[i] .. batch_offsets[i + 1]) (device int32; batch_offsets is a HOST array of n_batches + 1 entries) are scored
 * in eval mode from their rows of `train`, their train items set to -inf (predict(remove_train=True)), and reduced to nDCG@k /
 * Recall@k against their rows of `heldout`.  scores_scratch: device float32 [max batch][n_items], overwritten batch after batch.
 * ndcg / recall: device double [n_k][total users] (nullable), user j of the loader in column j.  ks_host is a HOST array. */
int rtx_engine_evaluate_topk(rtx_engine* e, const rtx_csr* train, const rtx_csr* heldout, const int32_t* row_ids,
                             const int64_t* batch_offsets, int32_t n_batches, const int32_t* ks_host, int32_t n_k,
                             float* scores_scratch, double* ndcg, double* recall, void* stream);

int rtx_topk_metrics(const float* scores, int64_t ld, int32_t batch, int32_t n_items, const rtx_csr* heldout,
                     const int32_t* row_ids, const int32_t* ks_host, int32_t n_k, double* ndcg, double* recall,
                     int32_t* topk_idx, int32_t kmax, void* stream);

/* The two calls above with hit@k and mrr@k as well (rectorch/metrics.py:231-238, 272-285): hit / mrr are device double
 * [n_k][batch] (rtx_topk_metrics_ex) or [n_k][total users] (rtx_engine_evaluate_topk_ex), nullable.  hit holds 1.0 / 0.0:
 * some rank < min(k, n_items) has relevance > 0.  mrr: 1 / (1 + r) for the first rank r < min(k, n_items) whose relevance
 * is != 0, else 0.  The calls without _ex are these with hit = mrr = NULL. */
int rtx_topk_metrics_ex(const float* scores, int64_t ld, int32_t batch, int32_t n_items, const rtx_csr* heldout,
                        const int32_t* row_ids, const int32_t* ks_host, int32_t n_k, double* ndcg, double* recall,
                        double* hit, double* mrr, int32_t* topk_idx, int32_t kmax, void* stream);
int rtx_engine_evaluate_topk_ex(rtx_engine* e, const rtx_csr* train, const rtx_csr* heldout, const int32_t* row_ids,
                                const int64_t* batch_offsets, int32_t n_batches, const int32_t* ks_host, int32_t n_k,
                                float* scores_scratch, double* ndcg, double* recall, double* hit, double* mrr, void* stream);

/* ---- top-N recommendation lists (the lists the reference gets from predict() + a host sort; metrics.py:136-147 ranks the same
 * way for its metrics) -------------------------------------------------------------------------------------------------
 * rtx_topk_items: per row of `scores` (device, dtype RTX_F32 = float32 or RTX_F64 = float64, `ld` elements between two rows)
 * the K = min(k, n_items) best items, 1 <= k <= 1024.  Order: score descending, item id ascending among equal scores; equal
 * means equal as floating-point values (-0.0 and +0.0 tie), float64 rows are compared as full doubles, -inf is a legal score
 * and ranks last.  NaN scores are out of contract.  excl (nullable): the stored non-zero entries of its row b -- or row
 * excl_row_ids[b] (device int32, nullable) -- rank as -inf and report the score -inf if they reach the list; the scores are not
 * written to.  When fewer than K items are left, the tail of the list holds excluded items by ascending id (what writing -inf
 * and sorting gives).  With an exclusion, n_items <= 393 216 (the row's bitmap lives in LDS).  items: device int32 [batch][K];
 * item_scores (nullable): device [batch][K] of the dtype of `scores`, copies of the input elements. */
#define RTX_F32 0
#define RTX_F64 2
int rtx_topk_items(const void* scores, int32_t dtype, int64_t ld, int32_t batch, int32_t n_items, const rtx_csr* excl,
                   const int32_t* excl_row_ids, int32_t k, int32_t* items, void* item_scores, void* stream);
/* rtx_list_metrics: the ranking metrics of READY-MADE lists -- what rtx_topk_items / rtx_engine_recommend write -- against the
 * users' held-out rows, so that any model's lists (float64 scores included) are evaluated without their scores leaving the device.
 * items: device int32 [n][ld], the first K >= 1 entries of a row ranked best first (any K: no 1024 cap; an id no held-out row
 * stores, negative or >= n_cols included, has relevance 0).  List b belongs to row b -- or row row_ids[b] (device int32, nullable)
 * -- of `heldout` (column ids sorted within a row, as rtx_csr_upload's callers store them; a row id outside the matrix reads as an
 * empty row).  Per cut-off k = ks_host[q] (HOST array, 1 <= n_k <= 16, k >= 1), with kk = min(k, K) and rel_r = the row's stored
 * value at items[r] (0 when absent):
 *   ndcg   = sum_{r < kk} rel_r / log2(r + 2)  /  sum_{j < min(int(sum of the row's values), kk)} 1 / log2(j + 2)
 *   recall = float32(#{r < kk : rel_r > 0}) / min(kk, #{row values > 0})
 *   hit    = 1.0 / 0.0: some rel_r > 0 with r < kk;      mrr = 1 / (1 + first r < kk with rel_r != 0), else 0
 * (rectorch/metrics.py:136-147, 187-196, 231-238, 272-285 with the list in the place of the sort).  An empty held-out row gives
 * what rtx_topk_metrics_ex gives: ndcg = recall = NaN (0 / 0), hit = mrr = 0.  Outputs: device double [n_k][out_ld], out_ld >= n,
 * list b in column b, each nullable -- the layout of rtx_topk_metrics_ex.  RTX_EINVAL for bad sizes or a NULL items / heldout /
 * ks_host; n == 0 is a no-op. */
int rtx_list_metrics(const int32_t* items, int64_t ld, int32_t n, int32_t K, const rtx_csr* heldout, const int32_t* row_ids,
                     const int32_t* ks_host, int32_t n_k, double* ndcg, double* recall, double* hit, double* mrr,
                     int64_t out_ld, void* stream);
/* recommend() for a whole loader in ONE call (the list-producing twin of rtx_engine_evaluate_topk; RTX_VAE, RTX_DAE and RTX_AE
 * engines, RTX_EINVAL for RTX_GVAE): for every batch i, the users row_ids[batch_offsets[i] .. batch_offsets[i + 1]) (device int32;
 * batch_offsets is a HOST array of n_batches + 1 entries) are scored in eval mode from their rows of `train` and reduced to their
 * K = min(k, n_items) best items, their train items excluded when remove_train != 0.  scores_scratch: device float32
 * [max batch][n_items], overwritten batch after batch.  items: device int32 [total users][K], item_scores (nullable): device
 * float32 [total users][K]; user j of the loader in row j. */
int rtx_engine_recommend(rtx_engine* e, const rtx_csr* train, const int32_t* row_ids, const int64_t* batch_offsets,
                         int32_t n_batches, int32_t k, int32_t remove_train, float* scores_scratch, int32_t* items,
                         float* item_scores, void* stream);

/* ---- one-plus-random evaluation (rectorch/evaluation.py:113-178) ------------------------------------------------
 * rtx_opr_draw: the negatives Python's random.sample(negatives, r) draws for every held-out positive, reproduced index for
 * index on the HOST (no device work).  mt_state: 625 words in/out, the 624 MT19937 words and the position of
 * random.getstate()[1].  The held-out CSR (HOST arrays, values nullable = ones) is read at the rows row_ids[0 .. n_rows)
 * (nullable = 0 .. n_rows); a row's positives are its stored entries with value != 0, any order, duplicates allowed.  The
 * contests are row-major, positives ascending within a row; the j-th negative is the j-th item of [0, n_items) that is not a
 * positive.  Per contest c: contest_row[c] = index into row_ids, contest_item[c] = the positive, draws[c * r .. c * r + r) =
 * the drawn negatives' item ids.  At most max_contests are written; *n_contests = how many.  *short_row = the index of the
 * first row with fewer than r negatives (-1: none): drawing stops at its first contest, with the state as it was then (where
 * random.sample raises ValueError).  RTX_EINVAL when max_contests is too small (nothing is consumed then). */
int rtx_opr_draw(uint32_t* mt_state, const int64_t* indptr, const int32_t* indices, const float* values,
                 const int32_t* row_ids, int32_t n_rows, int32_t n_items, int32_t r, int64_t max_contests,
                 int32_t* contest_row, int32_t* contest_item, int32_t* draws, int64_t* n_contests, int32_t* short_row);

/* rank[c] = #{j < r : scores[contest_row[c]][draws[c][j]] > scores[contest_row[c]][contest_item[c]]} for c < n_contests: the
 * positive's 0-based place among its r + 1 scores, ties won by the positive (column 0).  All pointers are device memory;
 * scores is float32 [n_rows][ld].  A contest whose row or item ids fall outside [0, n_rows) x [0, n_items) gets rank -1. */
int rtx_opr_rank(const float* scores, int64_t ld, int32_t n_rows, int32_t n_items, const int32_t* contest_row,
                 const int32_t* contest_item, const int32_t* draws, int64_t n_contests, int32_t r, int32_t* rank, void* stream);
/* the same on float64 score rows (EASE, ADMM_Slim): the comparison is made in double */
int rtx_opr_rank_f64(const double* scores, int64_t ld, int32_t n_rows, int32_t n_items, const int32_t* contest_row,
                     const int32_t* contest_item, const int32_t* draws, int64_t n_contests, int32_t r, int32_t* rank, void* stream);

/* ---- EASE closed-form model (rectorch/models.py:1003-1069) ------------------------------------------
 * rtx_ease_fit replaces EASE.train (models.py:1015-1025: G = X^T X; G[diag] += lam; P = inv(G); B = P / (-diag P);
 * B[diag] = 0) with the Gram matrix, a blocked f64 Cholesky, the triangular inverse and P = W^T W all on f64 MFMA
 * (Gram matrix on fp8 / bf16 MFMA when that is exact: data that are integers after a power-of-two scale <= 8, with
 * max|s x|^2 * n_users < 2^24; float64 MFMA otherwise).  The item-item
 * matrix B stays in HBM as double [n_items][n_items]; rtx_ease_scores replaces `model = X.dot(B)` + the look-up of
 * EASE.predict (models.py:1025, 1054-1057): rows `row_ids` (nullable = 0..batch-1) of X times B into out (device
 * double [batch][n_items]), with -inf at the non-zero entries of row b (or mask_row_ids[b]) of `mask` when given.
 * Returns RTX_EINVAL when X^T X + lam I is not positive definite (lam <= 0 on rank-deficient data). */
typedef struct rtx_ease rtx_ease;
int rtx_ease_fit(const rtx_csr* X, double lam, rtx_ease** out, void* stream);
int rtx_ease_destroy(rtx_ease* h);
int rtx_ease_weights(const rtx_ease* h, double** B_dev, int32_t* n_items);
/* device-to-device copy of B into a caller buffer of n_items * n_items doubles */
int rtx_ease_copy_weights(const rtx_ease* h, double* dst_dev, void* stream);
int rtx_ease_scores(const rtx_ease* h, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const rtx_csr* mask,
                    const int32_t* mask_row_ids, double* out, void* stream);
/* HIP-event durations of the last fit (ms; any pointer nullable): whole fit, Gram matrix, chol_ms = Cholesky +
 * inverse of the factor, inv_ms = P = W^T W */
int rtx_ease_timings(const rtx_ease* h, double* fit_ms, double* gram_ms, double* chol_ms, double* inv_ms);

/* ---- ADMM SLIM (rectorch/models.py:1389-1577) ------------------------------------------------------------------------
 * rtx_admm_fit replaces ADMM_Slim.train in float64: the Gram matrix of X (with item_bias: of X - 1 b^T, b = column sums,
 * as X^T X + (n_users - 2) b b^T) and P = inv(G + (lambda2 + rho) I) by the EASE pipeline; then, unless both nn_constr and
 * l1_penalty are 0 (closed form C = I - P * diag(1 / diag P), element-wise), B_aux = P G and num_iter ADMM iterations, each
 * ONE f64 MFMA GEMM launch with the element-wise update fused into its epilogue.  C stays in HBM; rtx_admm_scores replaces
 * `model = X.dot(C) [+ b]` + the look-up of ADMM_Slim.predict, with the same arguments as rtx_ease_scores.
 * Returns RTX_EINVAL when num_iter < 0 or when the shifted Gram matrix is not positive definite (lambda2 + rho <= 0). */
typedef struct rtx_admm rtx_admm;
#define RTX_ADMM_P 0
#define RTX_ADMM_C 1
#define RTX_ADMM_GAMMA 2
int rtx_admm_fit(const rtx_csr* X, double lambda1, double lambda2, double rho, int32_t nn_constr, int32_t l1_penalty,
                 int32_t item_bias, int32_t num_iter, rtx_admm** out, void* stream);
int rtx_admm_destroy(rtx_admm* h);
int rtx_admm_scores(const rtx_admm* h, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const rtx_csr* mask,
                    const int32_t* mask_row_ids, double* out, void* stream);
/* device-to-device copy of P, C or Gamma (what = RTX_ADMM_*) after the fit into a caller buffer of n_items * n_items
 * doubles, row-major; Gamma is 0 for the closed-form variant */
int rtx_admm_copy(const rtx_admm* h, int32_t what, double* dst_dev, void* stream);
/* HIP-event durations of the fit (ms; any pointer nullable): whole fit, factor_ms = Gram matrix + Cholesky + P,
 * baux_ms = B_aux = P G, iter_ms = all iterations (the launches only: not the allocation of their buffers) */
int rtx_admm_timings(const rtx_admm* h, double* fit_ms, double* factor_ms, double* baux_ms, double* iter_ms);

/* ---- ItemKNN: item-based k-nearest-neighbour model (additive to ABI 8; the reference has none -- this text is the definition) ----
 * In float64 throughout.  G = X^T X, by the Gram step of the EASE pipeline (exact on fp8 / bf16 MFMA under the rule above, f64 MFMA
 * otherwise).  For i != j with G_ij > 0:
 *     RTX_KNN_COSINE   S_ij = G_ij / (sqrt(G_ii) * sqrt(G_jj) + shrink)         (this operation order: S_ij and S_ji are the same bits)
 *     RTX_KNN_JACCARD  S_ij = G_ij / (G_ii + G_jj - G_ij + shrink)              (binary data only: values NULL or every value 1)
 * S_ii and every entry with G_ij <= 0 are "no neighbour", carried as -inf.  N_k(j) = the k best i of row j of S -- similarity
 * descending, item id ascending among equal similarities (the order of rtx_topk_items), entries above -inf only, so an item may have
 * fewer than k neighbours or none.  The model is the sparse matrix W:  W_ij = S_ij if i is in N_k(j), else absent;  with normalize,
 * W_ij = S_ij / d_j, d_j = the similarities of N_k(j) added in list order (best first).  It is kept in HBM as CSR BY SOURCE ITEM i:
 * int64 indptr [n_items + 1], int32 indices (the j, ascending within a row), double values.
 * rtx_knn_similarity: S alone, into S_dev (device double [n_items][n_items], row-major); synchronises the stream.
 * rtx_knn_fit: the model; the work buffers (G and S, 8 n_items^2 bytes each, and the lists) are freed before it returns.
 * rtx_knn_load: a model from HOST CSR arrays of the layout above (what rtx_knn_copy hands out) -- no device work but the upload.
 * rtx_knn_copy: device-to-device copy of the three arrays into caller buffers sized by rtx_knn_shape (each nullable).
 * rtx_knn_scores: out[b][j] = sum over the stored entries (i, v) of the user's row, IN STORED ORDER, of v * W_ij, each term added as
 * fma(v, W_ij, acc) -- no atomics, so two calls agree to the bit and a host loop with std::fma reproduces them; arguments as
 * rtx_ease_scores.  A user with no entries gets a row of zeros.
 * RTX_EINVAL, before anything is launched: k < 1 or k > 1024 (the selection kernel's limit); shrink < 0 or not finite; an unknown
 * similarity; jaccard on data that store a value other than 1 (binarise first); rtx_knn_load with unsorted or out-of-range indices. */
typedef struct rtx_knn rtx_knn;
#define RTX_KNN_COSINE 0
#define RTX_KNN_JACCARD 1
int rtx_knn_similarity(const rtx_csr* X, double shrink, int32_t similarity, double* S_dev, void* stream);
int rtx_knn_fit(const rtx_csr* X, int32_t k, double shrink, int32_t similarity, int32_t normalize, rtx_knn** out, void* stream);
int rtx_knn_load(int32_t n_items, const int64_t* indptr_host, const int32_t* indices_host, const double* values_host, rtx_knn** out);
int rtx_knn_destroy(rtx_knn* h);
int rtx_knn_shape(const rtx_knn* h, int32_t* n_items, int64_t* nnz);
int rtx_knn_copy(const rtx_knn* h, int64_t* indptr_dev, int32_t* indices_dev, double* values_dev, void* stream);
int rtx_knn_scores(const rtx_knn* h, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const rtx_csr* mask,
                   const int32_t* mask_row_ids, double* out, void* stream);
/* HIP-event durations of the fit (ms; any pointer nullable): whole fit, Gram matrix, sim_ms = diagonal + similarity,
 * select_ms = ranked lists + thresholds (the CSR build is the rest of fit_ms) */
int rtx_knn_timings(const rtx_knn* h, double* fit_ms, double* gram_ms, double* sim_ms, double* select_ms);

/* ---- WMF: weighted matrix factorisation for implicit feedback by alternating least squares (Hu, Koren, Volinsky 2008; additive to
 *      ABI 8; the reference has none -- this text is the definition) --------------------------------------------------------------
 * In float64 throughout.  X is a resident CSR matrix, users x items, with stored values r_ui > 0; f = the number of factors.  The
 * confidence is c_ui = 1 + alpha r_ui, the preference 1 on stored entries and 0 elsewhere.  With item factors Y [n_items][f]
 * (row-major, unpadded) and G = Y^T Y, the vector of a row u with stored entries I_u solves
 *     A_u x_u = b_u,   A_u = G + sum_{i in I_u} (alpha r_ui) y_i y_i^T + lam I,   b_u = sum_{i in I_u} (1 + alpha r_ui) y_i.
 * The item half-sweep is the same formula on X^T (a second rtx_csr, which the caller uploads) with the user factors in the place
 * of Y.  One iteration = a user half-sweep, then an item half-sweep.  A row without entries gets the zero vector.
 * Operation order.  w = alpha * (double)r.  The entries are walked in stored order; S_u = sum w y_i y_i^T is accumulated on
 * v_mfma_f64_16x16x4_f64 over the 16 x 16 tiles of the lower triangle, left operand w * y_i[r] (rounded), right operand y_i[c];
 * A_u[r][c] = (G[r][c] + S_u[r][c]) + (r == c ? lam : 0) for c <= r, the upper triangle is its mirror image (symmetric to the bit);
 * b_u[c] = fma(1 + w, y_i[c], b_u[c]) entry by entry.  A row longer than RTX_WMF_SEGMENT entries is cut into segments of that
 * length (the last one ragged): each segment's S and b are accumulated from zero as above, and the segments are added in
 * ascending order, ((s_0 + s_1) + s_2) ... -- no floating-point atomics anywhere, so the result does not depend on scheduling and
 * two calls agree to the bit.  G is a two-stage sum: chunks of RTX_WMF_GRAM_ROWS rows of the table on the same MFMA tiles, the
 * chunks added in ascending order.  The system is solved by a Cholesky factorisation in LDS (16-column panels) and two
 * triangular solves.
 * rtx_wmf_systems: the systems alone: A_out device double [batch][f][f] (full, symmetric), b_out [batch][f], of the rows row_ids
 *     (device int32, NULL = rows 0 .. batch-1) of X against the factor table Y (device double [X.n_cols][f]); synchronises.
 * rtx_wmf_solve_rows: one half-sweep over the given rows: out device double [batch][f].  n_src = the rows of Y, which must equal
 *     X.n_cols.  This is also the fold-in of users the fit never saw.  Synchronises (it reads the status word).
 * rtx_wmf_fit: n_iter iterations from the item factors Y0_host (HOST double [n_items][f]; the C layer draws no random numbers).
 *     XT must be the transpose of X (shape and nnz are checked).  n_iter = 0 keeps Y0 and leaves the user factors zero.
 * rtx_wmf_load: a model from HOST item factors; it holds no user factors (rtx_wmf_shape reports n_users = 0).
 * rtx_wmf_copy: device-to-device copy of the item factors (RTX_WMF_ITEMS, [n_items][f]) or of the user factors of the last user
 *     half-sweep (RTX_WMF_USERS, [n_users][f]).
 * rtx_wmf_scores: fold-in and scores in one call: x_b = the solve of row b of X against the model's item factors, then
 *     out[b * ld + j] = x_b . y_j -- fma(x_b[k], y_j[k], acc) for k = 0 .. f-1 from acc = 0 -- for j < n_items, with -inf at the
 *     non-zero entries of the mask row; the other arguments are those of rtx_ease_scores; ld >= n_items.
 * rtx_wmf_timings: HIP-event durations of the fit (ms; any pointer nullable): the whole fit, and summed over the iterations the
 *     Gram matrices, the user half-sweeps and the item half-sweeps.
 * RTX_EINVAL with a message, before anything is launched: lam <= 0 or not finite; alpha < 0 or not finite; f outside
 * 1 .. RTX_WMF_MAX_FACTORS; a stored value <= 0 (looked for once per matrix, on the host); n_iter < 0.  RTX_EINVAL after the
 * launches: a pivot of some system was not positive ("not positive definite" -- factors that are not finite). */
typedef struct rtx_wmf rtx_wmf;
#define RTX_WMF_MAX_FACTORS 128
#define RTX_WMF_SEGMENT 4096      /* entries of a row per workgroup: longer rows are cut into segments */
#define RTX_WMF_GRAM_ROWS 512     /* rows of a factor table per partial Gram matrix */
#define RTX_WMF_ITEMS 0
#define RTX_WMF_USERS 1
int rtx_wmf_systems(const rtx_csr* X, const int32_t* row_ids, int32_t batch, const double* Y, int32_t f, double alpha, double lam,
                    double* A_out, double* b_out, void* stream);
int rtx_wmf_solve_rows(const rtx_csr* X, const int32_t* row_ids, int32_t batch, const double* Y, int32_t n_src, int32_t f, double alpha,
                       double lam, double* out, void* stream);
int rtx_wmf_fit(const rtx_csr* X, const rtx_csr* XT, int32_t f, double alpha, double lam, int32_t n_iter, const double* Y0_host,
                rtx_wmf** out, void* stream);
int rtx_wmf_load(int32_t n_items, int32_t f, double alpha, double lam, const double* Y_host, rtx_wmf** out);
int rtx_wmf_destroy(rtx_wmf* h);
int rtx_wmf_shape(const rtx_wmf* h, int32_t* n_users, int32_t* n_items, int32_t* f);
int rtx_wmf_copy(const rtx_wmf* h, int32_t what, double* dst_dev, void* stream);
int rtx_wmf_scores(rtx_wmf* h, const rtx_csr* X, const int32_t* row_ids, int32_t batch, const rtx_csr* mask,
                   const int32_t* mask_row_ids, double* out, int64_t ld, void* stream);
int rtx_wmf_timings(const rtx_wmf* h, double* fit_ms, double* gram_ms, double* user_ms, double* item_ms);

/* ---- BPR triples: the sampled (user, positive, negative) triples of pairwise-ranking matrix factorisation (Bayesian Personalised
 *      Ranking: Rendle, Freudenthaler, Gantner, Schmidt-Thieme, UAI 2009), host half (additive to ABI 8; plain host code, no HIP call;
 *      the reference has no BPR -- this text is the definition, and a device sampler has to give the same numbers) -----------------
 * Integers only, a pure function of (seed, epoch, sample).  The matrix is CSR in HOST memory, users x items, column ids sorted and
 * unique within a row (rtx_bpr_check_rows_host checks it); only the pattern is read; nnz, n_rows and n_items are below 2^31.  An epoch is nnz samples.  Sample s
 * of epoch e reads
 *     r0 = philox4x32_10(seed, RTX_BPR_FIT_STREAM + e, 2 s)   and, only if r0 yields no negative,   r1 = (..., 2 s + 1)
 * (the Philox4x32-10 of the draw contract at rtx_step).  p = mulhi32(r0.x, nnz) -- the high word of the 64-bit product -- is a
 * position in `indices`: the positive is i = indices[p], the user u is the row with indptr[u] <= p < indptr[u + 1] (binary search).
 * The RTX_BPR_NEG_TRIES = 7 candidates are c = mulhi32(w, n_items) for w = r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w in this order;
 * the first one not stored in row u (binary search in the sorted row) is the negative j.  If all seven are stored the sample is
 * SKIPPED: j = -1.  No loop is unbounded.  A row without entries is never drawn; every sample of a row that stores all items is skipped.
 * rtx_bpr_check_rows_host: the one pass over a matrix that the draws rely on: indptr ascending from 0 to nnz, every row's column ids
 *     sorted, unique and inside [0, n_items).  O(nnz); a caller makes it once per matrix.
 * rtx_bpr_draw_host: u_out / i_out / j_out HOST int32 [count], the samples lo .. lo + count - 1 of epoch `epoch`.  O(count log): it does
 *     not walk the matrix.  On a matrix that rtx_bpr_check_rows_host refuses it reads nothing outside the arrays (a drawn row whose
 *     range is not inside [0, nnz] or does not hold p is refused), but unsorted rows give wrong negatives.
 * RTX_EINVAL with a message: a NULL argument; a matrix without entries; nnz, n_rows or n_items outside [1, 2^31); epoch < 0; samples
 * outside the epoch -- all before anything is written; check_rows: a row whose column ids are not sorted, unique and inside the matrix.
 * What this section does NOT define: the batch update and the fold-in of BPRMF -- the next section ("BPRMF rule") does, again on the
 * host.  The library has no device trainer for the triples yet.  The fold-in draws on the second stream below, which no other draw of
 * the library takes. */
#define RTX_BPR_NEG_TRIES 7
#define RTX_BPR_FIT_STREAM 0x1B504D4600000000ULL    /* Philox offset of epoch e: this + e */
#define RTX_BPR_FOLD_STREAM 0x2B504D4600000000ULL   /* Philox offset of every fold-in (reserved: see above) */
int rtx_bpr_check_rows_host(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int32_t n_items);
int rtx_bpr_draw_host(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int32_t n_items, uint64_t seed, int32_t epoch,
                      int64_t lo, int64_t count, int32_t* u_out, int32_t* i_out, int32_t* j_out);

/* ---- BPRMF rule: the batch update and the fold-in of BPRMF on the triples above, host half (additive to ABI 8; plain host code, no
 *      HIP call; the reference has no BPR -- this text is the definition, tests/bpr_ref64.py restates it in numpy, and a device trainer
 *      has to give the same tables) ---------------------------------------------------------------------------------------------------
 * In float64 throughout.  U [n_users][f] and Y [n_items][f] in HOST memory, row-major, unpadded; the score of item j for user u is
 * u . y_j.  One batch = `count` triples (u_t, i_t, j_t), every gradient taken at the tables as they were at the batch's start:
 *     d_t = y_i - y_j (element by element, rounded),   x_t = u_t . d_t,   s_t = 1 / (1 + exp(x_t)),
 *     g_t = s_t * d_t for row u_t of U,   s_t * u_t for row i_t of Y,   -(s_t * u_t) for row j_t of Y           (each product rounded),
 *     acc = acc + g_t from acc = 0.0 over the c > 0 non-skipped samples that touch the row, in ascending t (an item's positive and
 *           negative roles interleaved by sample: sample t's positive before its negative),
 *     theta' = theta + lr * (acc - ((double)c * reg) * theta)        -- these five roundings; no fused multiply-add anywhere.
 * A skipped sample (j = -1) contributes to nothing; a row nobody touches keeps its bits.  What the definition leaves open is the
 * summation tree of x_t and the rounding of exp (here: the products added in ascending k from 0.0; libm's exp); everything after s_t
 * is fixed operation by operation, so two implementations fed the same s_t give the same bits.
 * rtx_bpr_update_host: one batch, the tables updated in place.  s_in (nullable, [count]): the coefficients to use instead of this
 *     file's own -- the hook by which another implementation's s_t is held to the rule bit for bit; s_out (nullable, [count]): the
 *     coefficients used (0 for a skipped sample).  O(count f + (n_users + n_items) f).
 * rtx_bpr_fold_in_host: the vector of every row of a HOST CSR matrix (the layout and the row rule of the section above) against Y:
 *     out HOST double [n_rows][f].  A row with n stored entries: x = 0, then fold_in_epochs * n sequential steps on x alone; step t
 *     reads r0 = philox4x32_10(seed, RTX_BPR_FOLD_STREAM, 2 t) [and r1 at 2 t + 1, only if r0 yields no negative], its positive is the
 *     row's entry number mulhi32(r0.x, n), its negative the first of the seven candidates the row does not store (a step without one
 *     changes nothing), and x = x + lr * (s * d - reg * x) with s from x . d as above, every operation rounded.  The vector is a
 *     function of the row's content alone; n = 0 and n = n_items give the zero vector.  The one exception to the row rule: a matrix
 *     without entries (indptr all 0), which rtx_bpr_check_rows_host refuses as nothing to sample, is taken and gives zeros.
 * RTX_EINVAL with a message, before anything is written: a NULL argument; f outside 1 .. RTX_BPR_MAX_FACTORS; lr not finite or <= 0;
 * reg not finite or < 0; count or fold_in_epochs < 0; a triple that names a row outside the tables (u, i outside their table, j
 * outside [-1, n_items)); a matrix that rtx_bpr_check_rows_host refuses. */
#define RTX_BPR_MAX_FACTORS 128   /* what a device trainer will hold as two doubles per lane of a wavefront */
int rtx_bpr_update_host(double* U, double* Y, int32_t n_users, int32_t n_items, int32_t f, const int32_t* u, const int32_t* i,
                        const int32_t* j, int64_t count, double lr, double reg, const double* s_in, double* s_out);
int rtx_bpr_fold_in_host(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int32_t n_items, const double* Y, int32_t f,
                         double lr, double reg, int32_t fold_in_epochs, uint64_t seed, double* out);

/* ---- CDAE: Collaborative Denoising Auto-Encoder (Wu, DuBois, Zheng, Ester, WSDM 2016; additive to ABI 8).  The reference's
 * CDAE_net is not exported and marked unchecked, so it defines no behaviour to be equal to -- this text is the definition.
 *
 * CDAE is the one-layer denoising autoencoder plus one vector per training user in front of the hidden activation.  For batch row b
 * with user id u = user_ids[b]:
 *     h   = tanh( W0 . dropout(normalize(x_b)) + b0 + [u >= 0] . V[u] )        V: float32 [n_users][latent]
 *     out = W1 . h + b1
 * Everything but the V[u] term is the RTX_DAE / RTX_AE engine with n_enc = n_dec = 1 (MultiDAE_net with enc_dims = [n_items, latent],
 * dec_dims = [latent, n_items]): the row normalisation, the Philox dropout draws, the loss of the variant (RTX_DAE: multinomial
 * likelihood + lam sum ||W||_2; RTX_AE: MSE).  An id of -1, or no ids at all, gives that engine's forward exactly.  V is not part of
 * the regulariser.  In float32 the user term is added after the bias: (sum + b0) + V[u].
 *
 * Training.  d loss / d V[u] is the float32 pre-activation gradient of the hidden layer, row b (in bf16 numerics too: it is taken
 * before the cast to the compute type).  W0, b0, W1, b1 follow the step's optimizer as ever.  V follows torch.optim.SparseAdam's rule
 * (torch.optim._functional.sparse_adam) on the rows the batch names, and no others -- rows outside the batch keep V, exp_avg and
 * exp_avg_sq to the bit.  Per element, float32, in this order, every operation rounded once (NO fma anywhere; IEEE division and
 * square root):
 *     um = (g - m) * (float)(1 - beta1)        m' = m + um
 *     uv = (g * g - v) * (float)(1 - beta2)    v' = v + uv
 *     p' = p - step_size * (m' / (sqrt(v') + eps))          step_size = (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t)), t = step
 * (1 - beta, the bias corrections and step_size in double on the host, as torch computes them).  The update runs in the epilogue of
 * the kernel that produces the hidden layer's gradient: there is no gradient buffer for V and no launch of its own.  The ids of one
 * batch must be DISTINCT (apart from -1): no two rows of a launch write the same row of V, there are no atomics, two runs are
 * bit-equal.  (Not checked on the device; rectorch_amd.samplers.DataSampler checks its ids once on the host.)
 *
 * rtx_engine_bind_users: the table and its moments (exp_avg / exp_avg_sq NULL: inference only), float32 [n_users][latent] contiguous.
 *   Only RTX_DAE / RTX_AE engines with n_enc == 1, n_dec == 1 and cond_dim == 0; anything else is RTX_EINVAL.  V == NULL unbinds.
 *   With a table bound the first layer always takes the dense product (one forward site, one backward site, both numerics), and
 *   RTX_EINVAL before any launch answers: a data-parallel plan (rtx_engine_dp_attach, rtx_engine_train_step_dp),
 *   rtx_engine_set_grad_clip with a mode, rtx_engine_set_grad_accum with a mode, rtx_engine_forward_train / rtx_engine_backward and the
 *   two halves (encode_train / decode_train and their backward calls), and the one-call loops rtx_engine_evaluate_topk*,
 *   rtx_engine_recommend (score per batch: rtx_engine_forward -> rtx_topk_metrics / rtx_topk_items).
 * rtx_engine_set_users: user_ids is device int32, parallel to the batch rows of the NEXT call into this engine that runs the first
 *   layer -- rtx_engine_forward, rtx_engine_encode, rtx_engine_train_step, rtx_engine_loss_grads -- and is consumed by that call
 *   (rtx_engine_set_next_batch announces item rows only and consumes nothing: a step adds ITS batch's users, never the announced
 *   batch's).  NULL: no user term.  An id outside [-1, n_users) is treated as -1.  lr, beta1, beta2, eps, step: SparseAdam's
 *   scalars for a training call (step >= 1 there; ignored by forward / encode).  A training call without ids leaves V untouched.
 * rtx_user_rows_adam: the same update outside a step, one small kernel: rows user_ids[b] of V / exp_avg / exp_avg_sq
 *   ([n_users][ld], ld >= latent) from g float32 [batch][ldg]; ids outside [0, n_users) are skipped. */
int rtx_engine_bind_users(rtx_engine* e, float* V, float* exp_avg, float* exp_avg_sq, int32_t n_users);
int rtx_engine_set_users(rtx_engine* e, const int32_t* user_ids, float lr, float beta1, float beta2, float eps, int32_t step);
int rtx_user_rows_adam(float* V, float* exp_avg, float* exp_avg_sq, int64_t ld, int32_t n_users, const int32_t* user_ids, const float* g,
                       int64_t ldg, int32_t batch, int32_t latent, float lr, float beta1, float beta2, float eps, int32_t step, void* stream);

/* ---- SVAE: sequential VAE, one user sequence per optimizer step (rectorch/nets.py:624-693,
 * rectorch/models.py:1581-1635) ---------------------------------------------------------------------------------------
 * Parameter tensors in the order of SVAE_net.parameters(): enc W,b ... dec W,b ..., item_embed.weight [n_items][embed],
 * gru.weight_ih_l0 [3R][embed], gru.weight_hh_l0 [3R][R], gru.bias_ih_l0 [3R], gru.bias_hh_l0 [3R] (gate order r|z|n). */
typedef struct rtx_svae rtx_svae;
typedef struct {
    int32_t n_items, embed_size, rnn_size;
    int32_t n_enc, n_dec;
    int32_t enc_dims[RTX_MAX_LAYERS + 1]; /* enc_dims[0] = rnn_size ... enc_dims[n_enc] = latent */
    int32_t dec_dims[RTX_MAX_LAYERS + 1]; /* dec_dims[0] = latent   ... dec_dims[n_dec] = n_items */
    int32_t max_len;                      /* longest input sequence (time steps) */
} rtx_svae_cfg;
int rtx_svae_create(const rtx_svae_cfg* cfg, rtx_svae** out);
int rtx_svae_destroy(rtx_svae* s);
/* "gemm_bf16" (0 / 1, default 0): every matrix product of the model (input projection, encoder / decoder layers, their data and
 * weight gradients) takes its operands rounded to bf16 and accumulates in float32 on the bf16 MFMA -- the dtype BASELINE.json
 * configs[4] names; the GRU recurrences, the losses, the master weights and Adam stay float32.  Default: float32 products (the
 * reference's arithmetic, ~1e-6 parity). */
/* ABI 8 -- THIS step's loss without draining the stream (rtx_engine_loss_mailbox / rtx_engine_wait_loss for the sequence model):
 * once enabled, every rtx_svae_train_step / rtx_svae_train_pack also stores its loss into coherent host memory as soon as it is
 * final -- before the backward recurrence -- and rtx_svae_wait_loss returns the loss of the LAST step enqueued (steps are waited
 * for in order).  Reference: `return loss.item()` at the end of train_batch (rectorch/models.py:835). */
int rtx_svae_loss_mailbox(rtx_svae* s, int32_t enable);
int rtx_svae_wait_loss(rtx_svae* s, float* loss_host, double timeout_s);
int rtx_svae_set_option(rtx_svae* s, const char* key, int32_t value);
/* the current value of "gemm_bf16", or which GRU recurrence kernel the handle launches (read-only; fixed at rtx_svae_create from
 * rnn_size, the LDS budgets and the RTX_SVAE_GRU_ROWS / RTX_SVAE_GRU_KS / RTX_SVAE_GRU_BWD_KS measurement switches): "gru_fwd" and
 * "gru_bwd" -- 0 generic (W_hh streamed every step), 1 weight-resident on 1024 threads (reported for the backward only), 2 whole
 * rows on 512 threads (forward only), 3 K-sliced on 512 threads */
int rtx_svae_get_option(const rtx_svae* s, const char* key, int32_t* value);
int32_t rtx_svae_n_tensors(const rtx_svae* s);
int rtx_svae_tensor_shape(const rtx_svae* s, int32_t t, int32_t* rows, int32_t* cols);
int rtx_svae_bind(rtx_svae* s, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq);
/* SVAE_net.forward (nets.py:666-676) on one sequence `items` (device int32 [T]); z is always sampled (eps_noise: injected
 * N(0,1) draws [T][latent], NULL -> Philox(seed, offset)).  Any output may be NULL: logits_all [T][n_items], logits_last
 * [n_items] = recon_x[:, -1, :] with -inf at the items of the sequence when remove_train (SVAE.predict,
 * models.py:1628-1635), mu / logvar [T][latent].
 * Draw contract (rtx_step above; there is no dropout here): step t, latent j takes the noise draw of index = t * latent + j on the
 * stream offset ^ 0x5851F42D4C957F2D of (seed, offset); rtx_svae_train_step / _pack take the same draws from step->seed / offset,
 * t counting the rows of the concatenation. */
int rtx_svae_forward(rtx_svae* s, const int32_t* items, int32_t T, const float* eps_noise, uint64_t seed, uint64_t offset,
                     int32_t remove_train, float* logits_all, float* logits_last, float* mu, float* logvar, void* stream);
/* MultiVAE.train_batch with SVAE.loss_function and the SVAE optimizer (models.py:817-835, 1622-1626, 1618-1620):
 * forward, loss = sum_t NLL_t * step->inv_batch + step->beta * mean_t KL_t (inv_batch = 1 / number of ones in the
 * target), backward (decoder, encoder head, GRU through time, embedding), Adam with step->weight_decay.  The target is
 * either a CSR over the T steps (device int64 indptr [T+1], int32 indices, implicit ones) or a dense device [T][n_items]. */
int rtx_svae_train_step(rtx_svae* s, const int32_t* items, int32_t T, const int64_t* target_indptr, const int32_t* target_indices,
                        const float* target_dense, const rtx_step* step, float* loss_out, float* loss_accum, void* stream);
/* NOT in the reference (which takes one Adam step per user; samplers.py:517-571, models.py:1609-1635): `n_seq` user sequences
 * in ONE optimizer step.  The sequences are concatenated -- items [total_steps], rows [seq_ptr[u], seq_ptr[u+1]) belong to
 * sequence u (device int32 [n_seq+1]; max_len of the handle bounds total_steps) -- and the step minimises
 * sum_t nll_scale[t] * NLL_t + sum_t kl_scale[t] * KL_t (device float [total_steps] each): with nll_scale = 1 / (d_u * n_seq) and
 * kl_scale = beta / (T_u * n_seq) that is the mean over the pack of the reference's per-user loss -- gradient accumulation
 * over the pack, then one Adam step.  The products become [total_steps, .] GEMMs, the recurrences run one workgroup per
 * sequence side by side.  With n_seq = 1 it computes what rtx_svae_train_step computes.  step->inv_batch / beta are ignored. */
int rtx_svae_train_pack(rtx_svae* s, const int32_t* items, int32_t total_steps, const int32_t* seq_ptr, int32_t n_seq, const float* nll_scale,
                        const float* kl_scale, const int64_t* target_indptr, const int32_t* target_indices, const rtx_step* step, float* loss_out,
                        float* loss_accum, void* stream);
/* NOT in the reference: SVAE.predict for n_seq users at once.  items/seq_ptr as rtx_svae_train_pack.  Only each user's
 * LAST time step is encoded, sampled and decoded.  eps_noise: NULL -> Philox(seed, offset), else [total_steps][latent],
 * of which the row of each user's last step is read (so per-user noise arrays concatenate); the Philox draws follow the same rule:
 * user u, latent j takes index = (seq_ptr[u + 1] - 1) * latent + j, the draw rtx_svae_forward of the concatenation gives that row
 * (and of user 0 alone; a later user scored alone starts again at row 0).  scores [n_seq][n_items],
 * -inf at the user's own input items when remove_train; mu / logvar [n_seq][latent], nullable. */
int rtx_svae_predict_pack(rtx_svae* s, const int32_t* items, int32_t total_steps, const int32_t* seq_ptr, int32_t n_seq,
                          const float* eps_noise, uint64_t seed, uint64_t offset, int32_t remove_train,
                          float* scores, float* mu, float* logvar, void* stream);
/* ---- a loss computed OUTSIDE the handle (additive to ABI 8; rtx_engine_forward_train / rtx_engine_backward for the sequence model):
 *      MultiVAE.train_batch's  forward -> loss_function -> loss.backward() -> optimizer.step()  (models.py:829-833) with a
 *      loss_function the handle does not know.  Needs bound gradient buffers.
 * rtx_svae_forward_train: the forward of rtx_svae_train_step / _pack (seq_ptr NULL, n_seq = 1: one sequence; else as
 * rtx_svae_train_pack) that keeps its activations in the handle and writes the logits of ALL rows into logits_out
 * [total_steps][n_items] float32 and, nullable, mu / logvar [total_steps][latent].  It draws what rtx_svae_forward draws for the
 * same seed / offset or injected eps_noise.  *ticket names the activations: every entry point that overwrites them
 * (rtx_svae_forward, rtx_svae_predict_pack, both training calls, another rtx_svae_forward_train) makes it stale; tickets of
 * different handles never coincide.
 * rtx_svae_backward: the backward chain of the training step -- decoder, encoder head, GRU through time, the embedding's
 * scatter-add, every weight and bias gradient -- into the bound gradient buffers (overwritten, not accumulated), started from
 * d_logits float32 [total_steps][ld >= n_items] = d loss / d logits (a contiguous one, ld = n_items, is read in place; NULL = the
 * loss does not depend on the logits: the decoder's gradients are written as zeros) and d_mu / d_logvar float32
 * [total_steps][latent] = d loss / d mu, d loss / d logvar (either NULL = zero).  The chain through z = mu + eps exp(logvar / 2) is
 * the handle's; it adds no KL term and no scale of its own.  items / total_steps / seq_ptr / n_seq are those of the forward.
 * RTX_ESTATE, with nothing enqueued, when the ticket is stale.
 * rtx_svae_apply_adam: the optimizer of rtx_svae_train_step on its own, over the bound tensors (step->lr, beta1, beta2, eps,
 * weight_decay, step): a fused step and forward_train / backward / apply_adam are interchangeable in the middle of training. */
int rtx_svae_forward_train(rtx_svae* s, const int32_t* items, int32_t total_steps, const int32_t* seq_ptr, int32_t n_seq,
                           const float* eps_noise, uint64_t seed, uint64_t offset, float* logits_out, float* mu, float* logvar,
                           uint64_t* ticket, void* stream);
int rtx_svae_backward(rtx_svae* s, const int32_t* items, int32_t total_steps, const int32_t* seq_ptr, int32_t n_seq, uint64_t ticket,
                      const float* d_logits, int64_t ld, const float* d_mu, const float* d_logvar, void* stream);
int rtx_svae_apply_adam(rtx_svae* s, const rtx_step* step, void* stream);
/* the optimizer of rtx_svae_train_step / _train_pack / rtx_svae_apply_adam: rtx_optim as for rtx_engine_set_optimizer */
int rtx_svae_set_optimizer(rtx_svae* s, const rtx_optim* optim);
/* gradient clipping of the same three calls (RTX_CLIP_*, as rtx_engine_set_grad_clip); rtx_svae_wait_grad_norm: {total, coef} of the
 * LAST optimizer step enqueued */
int rtx_svae_set_grad_clip(rtx_svae* s, int32_t mode, double bound);
int rtx_svae_wait_grad_norm(rtx_svae* s, float* host, double timeout_s);

/* measurement knobs of one engine (the defaults are the shipped configuration): key "fuse_adam" (0/1, bf16 step:
 * Adam inside the weight-gradient kernels), "two_stream" (0/1: the two big ones on a second stream beside the
 * data-gradient chain), "lse_fuse" (0/1:
 * log-sum-exp partials from the logits GEMM epilogue), "nt_regstage" (0/1: the big NT contractions on the register-staged GEMM
 * instead of the LDS-DMA one), "dw_cfg" (0..8: tile configuration of the weight-gradient kernel, RtxDwCfg in csrc/rtx_gemm.h; 0 = 64 x 128, the default), "splitk" (split factor of the K = n_items GEMMs, 0 = automatic), "in_on_main" (0/1: the encoder matrix's weight kernel on
 * the caller's stream behind the chain), "sparse_in" (0/1, default 0 since round 4, bf16: the first encoder layer as a sparse VALU
 * product over the batch's stored entries -- spmm_in.hip -- instead of the dense MFMA split-K GEMM; needs a CSR batch,
 * n_items + cond_dim <= 20 480 and at most ~4000 expected 64-entry chunks per batch), "small_fwd" / "small_bwd" (0/1, bf16: hidden
 * layers and the VAE head of the forward pass / of the data-gradient chain as one register-resident launch each --
 * small_layers.hip -- for padded widths <= 1024), "logits16" (0/1, bf16 training step: the logits leave their product as IEEE half
 * in the buffer of d loss / d logits and the loss kernel converts them in place), "gather_scatter" (0/1: the dense batch image stays
 * all-zero between batches and only the stored entries are cleared / written -- resident CSR batches), "dp_shard_min_elems" (>= 1, before
 * rtx_engine_dp_attach: smallest weight matrix the sharded optimizer shards; default 2^20 elements), "hop_values" (0/1: the step's
 * two cross-stream dependencies as hipStreamWriteValue32 / hipStreamWaitValue32 pairs on signal memory instead of events; falls
 * back to events where the device cannot wait on a value), "hop_wrap" (>= 2: the sequence number at which both streams drain and
 * the signal words restart from zero; default 2^31 - 16, tests lower it).
 * Further keys (csrc/engine_api.hip holds the one table of all of them; an unknown key's error message lists it): "hop_kernels",
 * "hop_fold", "dw_side_pad", "prefetch", "big_batch_tiles", "f32_dw_split", "splitk_fwd", "splitk_bwd", "dp_one_comm" (before
 * rtx_engine_dp_attach), "timing_calibrate", and the process-wide "small_kw" / "small_waves".  Any other key: RTX_EINVAL.
 * Replaces round 1's RTX_* environment switches. */
int rtx_engine_set_option(rtx_engine* e, const char* key, int32_t value);
/* the current value of a knob; also "last_sparse_in": 1 when the last forward pass ran the first layer as the sparse product;
 * "side_concurrent": 1 when the step's second stream was seen to run beside the caller's; data parallel, the LAST step's exchange
 * per rank: "dp_bytes_all_reduce", "dp_bytes_reduce_scatter", "dp_bytes_all_gather" (buffer bytes handed to the collectives,
 * saturating at INT32_MAX) and "dp_collectives" (their number) */
int rtx_engine_get_option(const rtx_engine* e, const char* key, int32_t* value);

/* ---- instrumentation: per-kernel HIP-event timing on the engine's stream ------------------------- */
/* enable: 0 = off, 1 = every launch of the site, N > 1 = every N-th launch (two event records cost a few microseconds of the
 * stream they are recorded on: a sampled site perturbs a timed loop N times less) */
int rtx_engine_set_timing(rtx_engine* e, const char* site /* NULL = every launch site */, int32_t enable);
/* synchronises, returns up to `cap` entries (name, total ms, launches) and clears the counters */
int rtx_engine_get_timings(rtx_engine* e, int32_t cap, char (*names)[48], float* total_ms, int32_t* launches,
                           int32_t* n_out);
/* algorithmic HBM bytes / MFMA flops of one train step at batch B (DESIGN.md derivation) */
int rtx_engine_step_cost(const rtx_engine* e, int32_t batch, double* hbm_bytes, double* flops);

#ifdef __cplusplus
}
#endif
#endif
