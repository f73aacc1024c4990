// engine_api.hip -- the parts of the C ABI that are not the step: measurement knobs (rtx_engine_set_option / get_option), the
// stand-alone operators (loss, norms, top-k metrics) and the instrumentation (event-timed sites, algorithmic cost of a step).
#include "engine_internal.h"

// The sequence of every stand-alone loss / norm operator, all on `stream`: n floats of scratch, the launch that fills them (fill returns
// its status), the fixed-order sum into *out -- of n row losses, or (roots) of the roots of n sums of squares -- and the release.
// `extra`: further floats of scratch behind the n, for the fill's own use.
template <typename Fill>
static int reduce_through_scratch(int n, bool roots, float* out, void* stream, Fill fill, int extra = 0)
{
    hipStream_t st = (hipStream_t)stream;
    float* scratch = nullptr;
    RTX_HIP(hipMallocAsync((void**)&scratch, sizeof(float) * ((size_t)n + extra), st));
    int rc = fill(scratch, st);
    if (!rc)
        rc = roots ? rtx_launch_reduce_loss(nullptr, 0, 1.f, scratch, n, out, nullptr, st)
                   : rtx_launch_reduce_loss(scratch, n, 0.f, nullptr, 0, out, nullptr, st);
    (void)hipFreeAsync(scratch, st);
    return rc;
}

extern "C" {

// measurement knobs: one entry point instead of environment variables scattered over the kernels' launchers.  ONE table of the
// keys that are a plain member of the engine (or of its data-parallel state); rtx_engine_set_option and rtx_engine_get_option both
// walk it.  Keys with a check or a side effect are handled by name in front of it (set_checked / get_computed).
enum OptKind {
    OPT_BOOL,      // stored as value != 0
    OPT_INT,       // stored as given
    OPT_CHECKED,   // read from the table, written by set_checked
    OPT_COUNTER,   // read-only
};
struct OptEntry {
    const char* key;
    OptKind kind;
    int rtx_engine::*member;
    int DpState::*dp_member;      // (when `member` is null) a member of rtx_engine::dp
};
static const OptEntry OPTIONS[] = {
    {"fuse_adam", OPT_BOOL, &rtx_engine::opt_fuse_adam},
    {"lse_fuse", OPT_BOOL, &rtx_engine::opt_lse_fuse},
    {"logits16", OPT_BOOL, &rtx_engine::opt_logits16},
    {"hop_values", OPT_BOOL, &rtx_engine::opt_hop_values},
    {"hop_kernels", OPT_BOOL, &rtx_engine::opt_hop_kernels},
    {"hop_fold", OPT_BOOL, &rtx_engine::opt_hop_fold},
    {"timing_calibrate", OPT_BOOL, &rtx_engine::opt_timing_calibrate},
    {"f32_dw_split", OPT_BOOL, &rtx_engine::opt_f32_dw_split},
    {"splitk_fwd", OPT_INT, &rtx_engine::opt_splitk_fwd},
    {"splitk_bwd", OPT_INT, &rtx_engine::opt_splitk_bwd},
    {"gather_scatter", OPT_BOOL, &rtx_engine::opt_gather_scatter},
    {"prefetch", OPT_BOOL, &rtx_engine::opt_prefetch},
    {"two_stream", OPT_BOOL, &rtx_engine::opt_two_stream},
    {"nt_regstage", OPT_BOOL, &rtx_engine::opt_nt_regstage},
    {"in_on_main", OPT_BOOL, &rtx_engine::opt_in_on_main},
    {"sparse_in", OPT_BOOL, &rtx_engine::opt_sparse_in},
    {"small_fwd", OPT_BOOL, &rtx_engine::opt_small_fwd},
    {"small_bwd", OPT_BOOL, &rtx_engine::opt_small_bwd},
    {"big_batch_tiles", OPT_BOOL, &rtx_engine::opt_big_batch_tiles},
    {"dw_side_pad", OPT_CHECKED, &rtx_engine::opt_dw_side_pad},
    {"dp_shard_min_elems", OPT_CHECKED, &rtx_engine::opt_dp_shard_min_elems},
    {"dp_one_comm", OPT_CHECKED, &rtx_engine::opt_dp_one_comm},
    {"dw_cfg", OPT_CHECKED, &rtx_engine::opt_dw_cfg},
    {"state_tiles", OPT_BOOL, &rtx_engine::opt_state_tiles},             // deferred fused steps keep the big layers' exp_avg / exp_avg_sq tile-major (0: row-major)
    {"state_tiles_min_elems", OPT_CHECKED, &rtx_engine::opt_state_tiles_min_elems},
    {"state_imports", OPT_COUNTER, &rtx_engine::st_state_imports},       // layers whose moments were copied into their tile-major image
    {"state_writebacks", OPT_COUNTER, &rtx_engine::st_state_writebacks}, // ... and back into the bound tensors
    {"join_folds", OPT_COUNTER, &rtx_engine::st_join_folds},            // deferred joins that rode on a first-layer product
    {"prefetch_hits", OPT_COUNTER, &rtx_engine::st_prefetch_hits},       // steps that started from a prefetched batch image
    {"prefetch_issued", OPT_COUNTER, &rtx_engine::st_prefetch_issued},
    {"last_sparse_in", OPT_COUNTER, &rtx_engine::last_sparse_in},        // 1: the last forward pass ran the first layer as the sparse product
    {"side_concurrent", OPT_COUNTER, &rtx_engine::side_concurrent},      // 1: the step's second stream was seen to run beside the caller's
    {"dp_collectives", OPT_COUNTER, nullptr, &DpState::st_collectives},
};
// keys outside the table: written only (process-wide knobs of small_layers.hip), or computed on reading
static const char* const OPTIONS_SET_ONLY = "hop_wrap, splitk, small_kw, small_waves";
static const char* const OPTIONS_GET_ONLY = "splitk, dp_bytes_all_reduce, dp_bytes_reduce_scatter, dp_bytes_all_gather, dp_two_comms";

static std::string option_keys(bool writable)
{
    std::string out;
    for (const OptEntry& o : OPTIONS)
        if (!writable || o.kind != OPT_COUNTER) out += std::string(o.key) + ", ";
    return out + (writable ? OPTIONS_SET_ONLY : OPTIONS_GET_ONLY);
}

// the keys with a check or a side effect; *handled = false: not one of them
static int set_checked(rtx_engine* e, const std::string& k, int32_t value, bool* handled)
{
    *handled = true;
    if (k == "dw_side_pad") e->opt_dw_side_pad = value > 0 ? value : 0;
    else if (k == "small_kw") rtx_small_set_kw(value);         // (process-wide: K split of small_layers.hip's kernels over waves)
    else if (k == "small_waves") rtx_small_set_waves(value);   // (process-wide: a launch-shape knob of small_layers.hip)
    else if (k == "hop_wrap") {
        RTX_CHECK(value >= 2, RTX_EINVAL, "set_option: hop_wrap must be >= 2");
        e->hop_wrap = (uint32_t)value;
    } else if (k == "dp_shard_min_elems") {
        RTX_CHECK(!e->dp.on && value >= 1, RTX_ESTATE, "set_option: dp_shard_min_elems (>= 1) must be set before rtx_engine_dp_attach");
        e->opt_dp_shard_min_elems = value;
    } else if (k == "state_tiles_min_elems") {   // (tests lower it so that small layers take the tile-major state, as dp_shard_min_elems)
        RTX_CHECK(value >= 0, RTX_EINVAL, "set_option: state_tiles_min_elems must be >= 0");
        e->opt_state_tiles_min_elems = value;
    } else if (k == "dp_one_comm") {
        RTX_CHECK(!e->dp.on, RTX_ESTATE, "set_option: dp_one_comm must be set before rtx_engine_dp_attach");
        e->opt_dp_one_comm = value != 0;
    } else if (k == "dw_cfg") {
        RTX_CHECK(value >= 0 && value < RTX_DW_CFG_COUNT, RTX_EINVAL, "set_option: dw_cfg must be 0..%d", RTX_DW_CFG_COUNT - 1);
        e->opt_dw_cfg = value;
        e->opt_dw_cfg_set = 1;
    } else if (k == "splitk") {
        RTX_CHECK(value >= 0, RTX_EINVAL, "set_option: splitk must be >= 0");
        // the scratch was sized for the automatic choice: only accept factors it can hold
        const int old = e->cfg.splitk;
        e->cfg.splitk = value;
        size_t need = 0;
        for (int li = 0; li < e->NL; ++li) {
            if (li < e->NL - 1) need = std::max(need, plan_cacc_elems(e, e->L[li].outp, e->L[li].inp));
            if (li > 0) need = std::max(need, plan_cacc_elems(e, e->L[li].inp, e->L[li].outp));
        }
        if (need > e->cacc_elems) {
            e->cfg.splitk = old;
            rtx_set_error("set_option: split factor %d needs %zu scratch floats, the engine holds %zu", value, need, e->cacc_elems);
            return RTX_EINVAL;
        }
    } else {
        *handled = false;
    }
    return RTX_OK;
}

int rtx_engine_set_option(rtx_engine* e, const char* key, int32_t value)
{
    RTX_CHECK(e && key, RTX_EINVAL, "set_option: NULL argument");
    const std::string k(key);
    bool handled = false;
    const int rc = set_checked(e, k, value, &handled);
    if (handled) return rc;
    for (const OptEntry& o : OPTIONS)
        if (k == o.key && (o.kind == OPT_BOOL || o.kind == OPT_INT)) {
            e->*o.member = o.kind == OPT_BOOL ? (value != 0) : value;
            return RTX_OK;
        }
    rtx_set_error("set_option: unknown key '%s' (%s)", key, option_keys(true).c_str());
    return RTX_EINVAL;
}

int rtx_engine_get_option(const rtx_engine* e, const char* key, int32_t* value)
{
    RTX_CHECK(e && key && value, RTX_EINVAL, "get_option: NULL argument");
    const std::string k(key);
    for (const OptEntry& o : OPTIONS)
        if (k == o.key) {
            *value = o.member ? e->*o.member : e->dp.*o.dp_member;
            return RTX_OK;
        }
    if (k == "splitk") *value = e->cfg.splitk;
    else if (k == "dp_bytes_all_reduce") *value = (int32_t)std::min<int64_t>(e->dp.st_all_reduce, INT32_MAX);       // per rank, last step
    else if (k == "dp_bytes_reduce_scatter") *value = (int32_t)std::min<int64_t>(e->dp.st_reduce_scatter, INT32_MAX);
    else if (k == "dp_bytes_all_gather") *value = (int32_t)std::min<int64_t>(e->dp.st_all_gather, INT32_MAX);
    else if (k == "dp_two_comms") *value = e->dp.on && e->dp.two_comms;   // bucket A's collectives have a communicator of their own
    else {
        rtx_set_error("get_option: unknown key '%s' (%s)", key, option_keys(false).c_str());
        return RTX_EINVAL;
    }
    return RTX_OK;
}

int rtx_multinomial_loss(const float* recon, const float* x, int32_t batch, int32_t n_items, const float* mu, const float* logvar,
                         int32_t latent, float beta, float* loss_out, void* stream)
{
    RTX_CHECK(recon && x && loss_out && batch >= 1 && n_items >= 1, RTX_EINVAL, "multinomial_loss: bad arguments");
    return reduce_through_scratch(batch, false, loss_out, stream, [&](float* row_loss, hipStream_t st) {
        return rtx_launch_dense_loss(recon, x, batch, n_items, (mu && logvar) ? mu : nullptr, logvar, latent, beta, 1.f / (float)batch,
                                     row_loss, st);
    });
}

int rtx_bce_kl_loss(const float* recon, const float* x, int32_t batch, int32_t n_items, const float* mu, const float* logvar,
                    int32_t latent, float* loss_out, void* stream)
{
    RTX_CHECK(recon && x && loss_out && batch >= 1 && n_items >= 1, RTX_EINVAL, "bce_kl_loss: bad arguments");
    // F.binary_cross_entropy's mean over every element; the KL term's mean over the rows
    const float inv_elems = (float)(1.0 / ((double)batch * (double)n_items));
    return reduce_through_scratch(batch, false, loss_out, stream, [&](float* row_loss, hipStream_t st) {
        return rtx_launch_dense_bce_kl(recon, x, batch, n_items, (mu && logvar) ? mu : nullptr, logvar, latent, inv_elems,
                                       1.f / (float)batch, row_loss, st);
    });
}

int rtx_mse_loss(const float* prediction, const float* ground_truth, int32_t batch, int32_t n_items, float* loss_out, void* stream)
{
    RTX_CHECK(prediction && ground_truth && loss_out && batch >= 1 && n_items >= 1, RTX_EINVAL, "mse_loss: bad arguments");
    // torch.nn.MSELoss's mean over every element
    const float inv_elems = (float)(1.0 / ((double)batch * (double)n_items));
    return reduce_through_scratch(batch, false, loss_out, stream, [&](float* row_loss, hipStream_t st) {
        return rtx_launch_dense_mse(prediction, ground_truth, batch, n_items, inv_elems, row_loss, st);
    });
}

int rtx_sum_l2_norms(const float* const* tensors, const int64_t* sizes, int32_t n, float* out, void* stream)
{
    RTX_CHECK(tensors && sizes && out && n >= 1 && n <= RTX_MAX_TENSORS, RTX_EINVAL, "sum_l2_norms: bad arguments");
    std::vector<long> sz(sizes, sizes + n);
    return reduce_through_scratch(n, true, out, stream,
                                  [&](float* sumsq, hipStream_t st) { return rtx_launch_sumsq(tensors, sz.data(), n, sumsq, st); });
}

// The deterministic global norm of n float32 device tensors (norm_type 2 or inf; the norm kernels of gradient clipping, adam.hip, as
// an operator of its own): one float into out_dev.  Bit-equal between calls on the same data.
int rtx_grad_norm(const float* const* tensors, const int64_t* sizes, int32_t n, double norm_type, float* out_dev, void* stream)
{
    RTX_CHECK(tensors && sizes && out_dev && n >= 1 && n <= RTX_MAX_TENSORS, RTX_EINVAL, "grad_norm: bad arguments (1 to %d tensors)", RTX_MAX_TENSORS);
    RTX_CHECK(norm_type == 2.0 || (std::isinf(norm_type) && norm_type > 0), RTX_EINVAL, "grad_norm: norm_type %g (supported: 2 and inf)", norm_type);
    RtxAdamArgs a = {};
    a.n = n;
    a.grad_scale = 1.f;
    for (int k = 0; k < n; ++k) {
        RTX_CHECK(sizes[k] >= 0 && sizes[k] < (1LL << 31) && (tensors[k] || sizes[k] == 0), RTX_EINVAL, "grad_norm: tensor %d: %lld elements at %p", k,
                  (long long)sizes[k], (const void*)tensors[k]);
        a.t[k].g = tensors[k] ? tensors[k] : out_dev;     // (an empty tensor: any pointer, never followed)
        a.t[k].rows = 1;
        a.t[k].cols = (int)sizes[k];
    }
    hipStream_t st = (hipStream_t)stream;
    const long parts = rtx_grad_norm_parts(a);
    double* scratch = nullptr;      // the partial sums, and behind them the pair {total, coef}
    RTX_HIP(hipMallocAsync((void**)&scratch, sizeof(double) * ((size_t)parts + 1), st));
    float* pair = (float*)(scratch + parts);
    int rc = rtx_launch_grad_norm(a, norm_type != 2.0, INFINITY, scratch, pair, nullptr, 0, 0, st);
    if (!rc && hipMemcpyAsync(out_dev, pair, sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
        rtx_set_error("grad_norm: copy of the result failed");
        rc = RTX_EHIP;
    }
    (void)hipFreeAsync(scratch, st);
    return rc;
}

// ---- the VAE head's sampling step and its derivative as operators of their own (kernels: post_layers.hip) ---------------------------
int rtx_reparam(const float* mu, const float* logvar, int32_t n, int32_t latent, const float* eps_in, uint64_t seed, uint64_t offset,
                float* z, float* eps_out, void* stream)
{
    return rtx_launch_reparam(mu, logvar, n, latent, eps_in, seed, offset, z, eps_out, (hipStream_t)stream);
}

int rtx_reparam_grad(const float* d_z, const float* logvar, const float* eps, int32_t n, int32_t latent, float* d_mu, float* d_logvar,
                     void* stream)
{
    return rtx_launch_reparam_grad(d_z, logvar, eps, n, latent, d_mu, d_logvar, (hipStream_t)stream);
}

// ---- CDAE's lazy row update outside a step (include/rectorch_hip.h "CDAE"; kernel and rule: post_layers.hip) -------------------------
int rtx_user_rows_adam(float* V, float* exp_avg, float* exp_avg_sq, int64_t ld, int32_t n_users, const int32_t* user_ids, const float* g,
                       int64_t ldg, int32_t batch, int32_t latent, float lr, float beta1, float beta2, float eps, int32_t step, void* stream)
{
    RTX_CHECK(V && exp_avg && exp_avg_sq && user_ids && g, RTX_EINVAL, "user_rows_adam: NULL argument");
    RTX_CHECK(step >= 1, RTX_EINVAL, "user_rows_adam: step count must be >= 1, got %d", step);
    RTX_CHECK(latent >= 1 && ld >= latent && ldg >= latent && n_users >= 1 && batch >= 1, RTX_EINVAL,
              "user_rows_adam: need latent >= 1, ld >= latent, ldg >= latent, n_users >= 1, batch >= 1");
    RtxPostUsers u = {};
    u.uid = user_ids; u.n_users = n_users; u.V = V; u.m = exp_avg; u.v = exp_avg_sq; u.ld = (long)ld;
    u.vec = rtx_user_rows_vec(V, exp_avg, exp_avg_sq, (long)ld, latent);
    rtx_user_adam_scalars(lr, beta1, beta2, eps, step, u);
    return rtx_launch_user_rows_adam(u, g, (long)ldg, batch, latent, (hipStream_t)stream);
}

// ---- the same four with their gradients at unit upstream gradient: the argument checks of the four above, the gradient outputs, and
// d_mu / d_logvar NULL exactly when mu / logvar are ----
static bool kl_grads_match(const float* mu, const float* logvar, const float* d_mu, const float* d_logvar)
{
    return (mu != nullptr) == (d_mu != nullptr) && (logvar != nullptr) == (d_logvar != nullptr);
}

int rtx_multinomial_loss_grad(const float* recon, const float* x, int32_t batch, int32_t n_items, const float* mu, const float* logvar,
                              int32_t latent, float beta, float* loss_out, float* d_recon, float* d_mu, float* d_logvar, void* stream)
{
    RTX_CHECK(recon && x && loss_out && d_recon && batch >= 1 && n_items >= 1, RTX_EINVAL, "multinomial_loss_grad: bad arguments");
    RTX_CHECK(kl_grads_match(mu, logvar, d_mu, d_logvar), RTX_EINVAL,
              "multinomial_loss_grad: d_mu / d_logvar must be NULL exactly when mu / logvar are");
    const bool kl = mu && logvar;
    return reduce_through_scratch(batch, false, loss_out, stream, [&](float* row_loss, hipStream_t st) {
        return rtx_launch_dense_loss_grad(recon, x, batch, n_items, kl ? mu : nullptr, logvar, latent, beta, 1.f / (float)batch, row_loss,
                                          d_recon, d_mu, d_logvar, st);
    });
}

int rtx_bce_kl_loss_grad(const float* recon, const float* x, int32_t batch, int32_t n_items, const float* mu, const float* logvar,
                         int32_t latent, float* loss_out, float* d_recon, float* d_mu, float* d_logvar, void* stream)
{
    RTX_CHECK(recon && x && loss_out && d_recon && batch >= 1 && n_items >= 1, RTX_EINVAL, "bce_kl_loss_grad: bad arguments");
    RTX_CHECK(kl_grads_match(mu, logvar, d_mu, d_logvar), RTX_EINVAL,
              "bce_kl_loss_grad: d_mu / d_logvar must be NULL exactly when mu / logvar are");
    const bool kl = mu && logvar;
    const float inv_elems = (float)(1.0 / ((double)batch * (double)n_items));
    return reduce_through_scratch(batch, false, loss_out, stream, [&](float* row_loss, hipStream_t st) {
        return rtx_launch_dense_bce_kl_grad(recon, x, batch, n_items, kl ? mu : nullptr, logvar, latent, inv_elems, 1.f / (float)batch,
                                            row_loss, d_recon, d_mu, d_logvar, st);
    });
}

int rtx_mse_loss_grad(const float* prediction, const float* ground_truth, int32_t batch, int32_t n_items, float* loss_out,
                      float* d_prediction, void* stream)
{
    RTX_CHECK(prediction && ground_truth && loss_out && d_prediction && batch >= 1 && n_items >= 1, RTX_EINVAL,
              "mse_loss_grad: bad arguments");
    const float inv_elems = (float)(1.0 / ((double)batch * (double)n_items));
    return reduce_through_scratch(batch, false, loss_out, stream, [&](float* row_loss, hipStream_t st) {
        return rtx_launch_dense_mse_grad(prediction, ground_truth, batch, n_items, inv_elems, row_loss, d_prediction, st);
    });
}

int rtx_sum_l2_norms_grad(const float* const* tensors, const int64_t* sizes, int32_t n, float* out, float* const* grads, void* stream)
{
    RTX_CHECK(tensors && sizes && out && grads && n >= 1 && n <= RTX_MAX_TENSORS, RTX_EINVAL, "sum_l2_norms_grad: bad arguments");
    std::vector<long> sz(sizes, sizes + n);
    // the squared norms stay in the scratch until the sum has read them: the gradient launch reads them there too; behind them the
    // block sums of the fixed-order squared norms
    return reduce_through_scratch(n, true, out, stream, [&](float* sumsq, hipStream_t st) {
        RTX_TRY(rtx_launch_sumsq_ordered(tensors, sz.data(), n, sumsq, sumsq + n, st));
        return rtx_launch_norm_grad(tensors, grads, sz.data(), n, sumsq, st);
    }, rtx_sumsq_ordered_scratch(n));
}

int rtx_topk_metrics(const float* scores, int64_t ld, int32_t batch, int32_t n_items, const rtx_csr* heldout,
                     const int32_t* row_ids, const int32_t* ks_host, int32_t n_k, double* ndcg, double* recall,
                     int32_t* topk_idx, int32_t kmax, void* stream)
{
    return rtx_topk_metrics_ex(scores, ld, batch, n_items, heldout, row_ids, ks_host, n_k, ndcg, recall, nullptr, nullptr, topk_idx,
                               kmax, stream);
}

int rtx_topk_metrics_ex(const float* scores, int64_t ld, int32_t batch, int32_t n_items, const rtx_csr* heldout,
                        const int32_t* row_ids, const int32_t* ks_host, int32_t n_k, double* ndcg, double* recall,
                        double* hit, double* mrr, int32_t* topk_idx, int32_t kmax, void* stream)
{
    RTX_CHECK(scores && heldout && ks_host, RTX_EINVAL, "topk_metrics: NULL argument");
    RTX_CHECK(heldout->n_cols == n_items, RTX_EINVAL, "topk_metrics: held-out matrix has %d columns, scores have %d", heldout->n_cols, n_items);
    RTX_CHECK(row_ids || batch <= heldout->n_rows, RTX_EINVAL, "topk_metrics: batch larger than the held-out matrix");
    int km = kmax;
    for (int q = 0; q < n_k; ++q) km = std::max(km, (int)ks_host[q]);
    RtxCsrView v = {heldout->indptr, heldout->indices, heldout->values, row_ids};
    return rtx_launch_topk_metrics(scores, (long)ld, batch, n_items, v, ks_host, n_k, km, ndcg, recall, topk_idx, (hipStream_t)stream,
                                   0, nullptr, hit, mrr);
}

int rtx_topk_items(const void* scores, int32_t dtype, int64_t ld, int32_t batch, int32_t n_items, const rtx_csr* excl,
                   const int32_t* excl_row_ids, int32_t k, int32_t* items, void* item_scores, void* stream)
{
    RTX_CHECK(scores && items, RTX_EINVAL, "topk_items: %s is NULL", scores ? "items" : "scores");
    RTX_CHECK(dtype == RTX_F32 || dtype == RTX_F64, RTX_EINVAL, "topk_items: dtype must be RTX_F32 (%d) or RTX_F64 (%d), got %d", RTX_F32, RTX_F64, dtype);
    RTX_CHECK(k >= 1 && k <= 1024, RTX_EINVAL, "topk_items: k must be in [1, 1024], got %d", k);
    RTX_CHECK(batch >= 0 && n_items >= 1 && ld >= n_items, RTX_EINVAL, "topk_items: batch = %d, n_items = %d, ld = %lld", batch, n_items, (long long)ld);
    RtxCsrView v = {};
    if (excl) {
        RTX_CHECK(excl_row_ids || batch <= excl->n_rows, RTX_EINVAL, "topk_items: batch larger than the exclusion matrix");
        v.indptr = excl->indptr; v.indices = excl->indices; v.values = excl->values; v.row_ids = excl_row_ids;
    }
    return rtx_launch_topk_items(scores, dtype == RTX_F64, (long)ld, batch, n_items, excl ? &v : nullptr, k, items, item_scores,
                                 (hipStream_t)stream);
}

// ---- instrumentation -------------------------------------------------------------------------------
int rtx_engine_set_timing(rtx_engine* e, const char* site, int32_t enable)
{
    RTX_CHECK(e, RTX_EINVAL, "engine is NULL");
    if (!site) {
        e->timing_all = enable != 0;
        if (!enable) e->timing_sites.clear();
    } else if (enable) {
        e->timing_sites[site] = enable;
        e->timing_seen[site] = 0;
    } else {
        e->timing_sites.erase(site);
    }
    return RTX_OK;
}

int rtx_engine_get_timings(rtx_engine* e, int32_t cap, char (*names)[48], float* total_ms, int32_t* launches, int32_t* n_out)
{
    RTX_CHECK(e && n_out, RTX_EINVAL, "get_timings: NULL argument");
    RTX_HIP(hipDeviceSynchronize());
    int n = 0;
    for (auto& kv : e->sites) {
        TimingSite& s = kv.second;
        for (auto& pr : s.pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                s.total_ms += ms;
                s.launches += 1;
            }
            e->event_pool.push_back(pr.first);
            e->event_pool.push_back(pr.second);
        }
        s.pending.clear();
        if (n < cap && names && total_ms && launches) {
            strncpy(names[n], kv.first.c_str(), 47);
            names[n][47] = 0;
            total_ms[n] = (float)s.total_ms;
            launches[n] = s.launches;
            ++n;
        }
        s.total_ms = 0;
        s.launches = 0;
    }
    *n_out = n;
    return RTX_OK;
}

int rtx_engine_step_cost(const rtx_engine* e, int32_t batch, double* hbm_bytes, double* flops)
{
    RTX_CHECK(e, RTX_EINVAL, "engine is NULL");
    // bytes = 38*P + 12*B*I  (fp32 master params + Adam state, logits written once and read twice)
    //               flops = forward 2*sum(in*out) + weight grads 2*sum(in*out) + data grads 2*sum_{l>0}(in*out), per user
    double P = 0, f_all = 0, f_rest = 0;
    for (int li = 0; li < e->NL; ++li) {
        const double w = (double)e->L[li].in * e->L[li].out;
        P += w + e->L[li].out;
        f_all += w;
        if (li > 0) f_rest += w;
    }
    if (hbm_bytes) *hbm_bytes = 38.0 * P + 12.0 * (double)batch * e->I;
    if (flops) *flops = (double)batch * 2.0 * (2.0 * f_all + f_rest);
    return RTX_OK;
}

}  // extern "C"
