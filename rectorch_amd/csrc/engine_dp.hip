// engine_dp.hip -- the data-parallel plan of the engine (rtx_engine_dp_attach): the exchange buffer's layout, which matrices are
// sharded, and the transports the step's collectives go through (the engine's own RCCL communicators, caller-supplied operations,
// same-size device copies for one-GPU emulation), and the exchange + optimizer pass of one bucket of that plan (dp_bucket), which
// the step calls (rtx_engine_train_step_dp -> run_step in engine_step.hip).
// (The reference has no collective code: rectorch/models.py:409-419 is a single-device loop.)
#include "engine_internal.h"

// tensors of the exchange buffer in layout order (DpState): W[NL-1], b[NL-1], ..., W[1], b[1], b[0], W[0]
static int dp_layout_order(const rtx_engine* e, int* order)
{
    int n = 0;
    for (int li = e->NL - 1; li >= 1; --li) { order[n++] = 2 * li; order[n++] = 2 * li + 1; }
    order[n++] = 1;
    order[n++] = 0;
    return n;
}
static size_t dp_region_elems(const rtx_engine* e, const DpState& d, int t)
{
    const Layer& l = e->L[t / 2];
    if (t & 1) return (size_t)l.out;
    return (size_t)(d.shard[t / 2] ? l.outp : l.out) * l.in;
}

extern "C" {

// ---- data parallel: attach / step --------------------------------------------------------------------------------
static int dp_rccl_all_reduce(void* c, void* buf, int64_t n, int32_t dt, void* st) { return rtx_comm_allreduce((rtx_comm*)c, buf, n, dt, st); }
static int dp_rccl_reduce_scatter(void* c, void* buf, int64_t n, int32_t dt, void* st) { return rtx_comm_reduce_scatter((rtx_comm*)c, buf, n, dt, st); }
static int dp_rccl_all_gather(void* c, void* buf, int64_t bytes, void* st) { return rtx_comm_allgather((rtx_comm*)c, buf, bytes, st); }
static int dp_rccl_group_start(void* c) { return rtx_comm_group_start((rtx_comm*)c); }
static int dp_rccl_group_end(void* c) { return rtx_comm_group_end((rtx_comm*)c); }

// emulate: the bytes one rank of `world` sends + receives in a ring collective, as device copies through a scratch buffer
// (reduce-scatter / all-gather: (world - 1) / world of the buffer read and written once; all-reduce: twice -- there and back,
// numerically a no-op).  One launch per collective, or per group of collectives, like RCCL's own kernels.
struct EmuCopyArgs {
    struct { const uint4* src; uint4* dst; unsigned long n16; int back; } p[8];
    int n;
};
__global__ __launch_bounds__(256) void k_emu_copy(const EmuCopyArgs a)
{
    for (int k = 0; k < a.n; ++k) {
        const uint4* __restrict__ src = a.p[k].src;
        uint4* __restrict__ dst = a.p[k].dst;
        for (unsigned long i = (unsigned long)blockIdx.x * 256 + threadIdx.x; i < a.p[k].n16; i += (unsigned long)gridDim.x * 256) {
            const uint4 v = src[i];
            dst[i] = v;
            if (a.p[k].back) ((uint4*)src)[i] = v;   // the all-gather half of an all-reduce writes the block back
        }
    }
}
static int dp_emu_flush(DpState* d)
{
    if (d->emu_n == 0) return RTX_OK;
    EmuCopyArgs a = {};
    size_t used = 0;
    for (int k = 0; k < d->emu_n; ++k) {
        const size_t w = (size_t)d->cfg.world, bytes = d->emu_q[k].bytes;
        size_t s = (bytes / w * (w - 1)) & ~(size_t)15;
        s = std::min(s, d->emu_bytes - used);
        if (s == 0) continue;
        a.p[a.n].src = (const uint4*)((char*)d->emu_q[k].buf + ((bytes - s) & ~(size_t)15));   // "the other ranks' blocks"
        a.p[a.n].dst = (uint4*)((char*)d->emu_scratch + used);
        a.p[a.n].n16 = s / 16;
        a.p[a.n].back = d->emu_q[k].back;
        used += s;
        ++a.n;
    }
    d->emu_n = 0;
    if (a.n == 0) return RTX_OK;
    hipLaunchKernelGGL(k_emu_copy, dim3(2048), dim3(256), 0, d->emu_stream, a);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
static int dp_emu_move(DpState* d, void* buf, size_t bytes, bool back, hipStream_t st)
{
    if (d->emu_n == 8) RTX_TRY(dp_emu_flush(d));
    d->emu_stream = st;
    d->emu_q[d->emu_n++] = DpState::EmuPiece{buf, bytes, back ? 1 : 0};
    return d->emu_grouped ? RTX_OK : dp_emu_flush(d);
}
static int dp_emu_group_start(void* c) { ((DpState*)c)->emu_grouped = 1; return RTX_OK; }
static int dp_emu_group_end(void* c) { ((DpState*)c)->emu_grouped = 0; return dp_emu_flush((DpState*)c); }
static int dp_emu_all_reduce(void* c, void* buf, int64_t n, int32_t dt, void* st)
{
    return dp_emu_move((DpState*)c, buf, (size_t)n * (dt == RTX_BF16 ? 2 : 4), true, (hipStream_t)st);
}
static int dp_emu_reduce_scatter(void* c, void* buf, int64_t n, int32_t dt, void* st)
{
    return dp_emu_move((DpState*)c, buf, (size_t)n * (dt == RTX_BF16 ? 2 : 4), false, (hipStream_t)st);
}
static int dp_emu_all_gather(void* c, void* buf, int64_t bytes, void* st) { return dp_emu_move((DpState*)c, buf, (size_t)bytes, false, (hipStream_t)st); }

}  // extern "C"
void dp_release(rtx_engine* e)
{
    DpState& d = e->dp;
    dev_free(e, d.xg);
    dev_free(e, d.emu_scratch);
    d = DpState();
}

// ---- one bucket of the step: layers [l_lo, l_hi) on stream ws ----------------------------------------------------------------
struct DpBucket {
    const StepCtx& c;
    int l_lo, l_hi;
    hipStream_t ws;
    bool side;               // bucket A on the side stream of a two-stream step
    const rtx_dp_ops& O;
    bool has(int t) const { return t / 2 >= l_lo && t / 2 < l_hi; }
};

// (1) staging: float32 numerics with a bf16 exchange cast their gradients; a float32 exchange hands the caller its copy
static int dp_stage(const DpBucket& b, const int* order, int n_order)
{
    rtx_engine* e = b.c.e;
    const DpState& d = *b.c.dp;
    const int cdt = d.cfg.comm_dtype;
    for (int q = 0; q < n_order; ++q) {
        const int t = order[q];
        if (!b.has(t)) continue;
        const Layer& l = e->L[t / 2];
        const size_t n = (t & 1) ? (size_t)l.out : (size_t)l.out * l.in;
        if (!e->bf16 && cdt == RTX_BF16) RTX_TRY(rtx_launch_cast_f32_bf16(e->grads[t], d.xg16(t), (long)n, b.ws));
        else if (b.c.keep_grads && cdt == RTX_FP32) RTX_HIP(hipMemcpyAsync(e->grads[t], d.xg32(t), n * sizeof(float), hipMemcpyDeviceToDevice, b.ws));
    }
    return RTX_OK;
}

// the collectives of one group: reduce-scatter of every sharded matrix, one all-reduce per contiguous run of replicated tensors
static int dp_all_reduce_run(const DpBucket& b, long* run_lo, long* run_hi)
{
    DpState& d = *b.c.dp;
    if (*run_lo >= 0 && *run_hi > *run_lo) {
        RTX_CHECK(b.O.all_reduce(b.O.ctx, (char*)d.xg + (size_t)*run_lo * d.xesz, *run_hi - *run_lo, d.cfg.comm_dtype, b.ws) == 0, RTX_EHIP,
                  "data parallel: all_reduce failed: %s", rtx_last_error_str());
        d.st_all_reduce += (int64_t)(*run_hi - *run_lo) * (int64_t)d.xesz;
        d.st_collectives += 1;
    }
    *run_lo = *run_hi = -1;
    return RTX_OK;
}
static int dp_exchange_group(const DpBucket& b, const int* order, int n_order)
{
    rtx_engine* e = b.c.e;
    DpState& d = *b.c.dp;
    long run_lo = -1, run_hi = -1;
    for (int q = 0; q < n_order; ++q) {
        const int t = order[q];
        const bool sharded_w = !(t & 1) && d.shard[t / 2];
        if (!b.has(t) || sharded_w) {
            RTX_TRY(dp_all_reduce_run(b, &run_lo, &run_hi));
            if (b.has(t)) {
                RTX_CHECK(b.O.reduce_scatter(b.O.ctx, (char*)d.xg + d.xoff[t] * d.xesz, (int64_t)dp_region_elems(e, d, t), d.cfg.comm_dtype, b.ws) == 0,
                          RTX_EHIP, "data parallel: reduce_scatter failed: %s", rtx_last_error_str());
                d.st_reduce_scatter += (int64_t)dp_region_elems(e, d, t) * (int64_t)d.xesz;
                d.st_collectives += 1;
            }
            continue;
        }
        if (run_lo < 0) run_lo = (long)d.xoff[t];
        run_hi = (long)(d.xoff[t] + dp_region_elems(e, d, t));
    }
    return dp_all_reduce_run(b, &run_lo, &run_hi);
}

// (2) exchange.  A failure between group_start and group_end still closes the group (an open RCCL group would swallow every later
//     collective of the communicator) and marks the plan unusable until it is attached again.
static int dp_exchange(const DpBucket& b, const int* order, int n_order)
{
    DpState& d = *b.c.dp;
    const rtx_dp_ops& O = b.O;
    ScopedTimer tm(b.c.e, b.side ? "dp_exchange_side" : "dp_exchange_main", b.ws);
    if (O.group_start) RTX_CHECK(O.group_start(O.ctx) == 0, RTX_EHIP, "data parallel: group_start failed: %s", rtx_last_error_str());
    const int rc = dp_exchange_group(b, order, n_order);
    if (rc != RTX_OK) {
        d.broken = true;
        std::string msg = rtx_last_error_str();           // group_end may overwrite the thread's error slot
        if (O.group_end) (void)O.group_end(O.ctx);
        RTX_CHECK(false, rc, "%s", msg.c_str());
    }
    if (O.group_end && O.group_end(O.ctx) != 0) {
        d.broken = true;
        RTX_CHECK(false, RTX_EHIP, "data parallel: group_end failed: %s", rtx_last_error_str());
    }
    return RTX_OK;
}

// (3) Adam: replicated tensors in full, a sharded matrix on this rank's rows
static int dp_adam(const DpBucket& b, bool alt)
{
    rtx_engine* e = b.c.e;
    const DpState& d = *b.c.dp;
    RtxAdamArgs a = {};
    int ids[RTX_MAX_TENSORS];
    for (int li = b.l_lo; li < b.l_hi; ++li) {
        Layer& l = e->L[li];
        RtxAdamArgs one = {};
        fill_adam_tensors(e, one, li, li + 1);
        RtxAdamTensor w = one.t[0], bias = one.t[1];
        if (d.cfg.comm_dtype == RTX_BF16) { w.g16 = d.xg16(2 * li); bias.g16 = d.xg16(2 * li + 1); }
        else { w.g = d.xg32(2 * li); bias.g = d.xg32(2 * li + 1); }
        if (alt && l.Wsh_alt) w.sh = l.Wsh_alt;
        bool any_w = true;
        if (d.shard[li]) {
            const int per = l.outp / d.cfg.world;
            const int lo = d.cfg.rank * per, hi = std::min((d.cfg.rank + 1) * per, l.out);   // padding rows hold no parameters
            any_w = lo < hi;
            const size_t off = (size_t)lo * l.in;
            w.p += off; w.m += off; w.v += off;
            if (w.g16) w.g16 += off; else w.g += off;
            w.sh = (char*)w.sh + (size_t)lo * l.inp * e->esz;
            w.rows = any_w ? hi - lo : 0;
        }
        if (any_w) { ids[a.n] = 2 * li; a.t[a.n++] = w; }
        ids[a.n] = 2 * li + 1; a.t[a.n++] = bias;
    }
    fill_adam_scalars(e, b.c.step, a, 0, ids);
    ScopedTimer tm(e, "adam", b.ws);
    return rtx_launch_adam(a, e->bf16, b.ws);
}

// (4) the other ranks' rows of the compute copy
static int dp_all_gather(const DpBucket& b, bool alt)
{
    rtx_engine* e = b.c.e;
    DpState& d = *b.c.dp;
    for (int li = b.l_lo; li < b.l_hi; ++li)
        if (d.shard[li]) {
            Layer& l = e->L[li];
            ScopedTimer tm(e, b.side ? "dp_allgather_side" : "dp_allgather_main", b.ws);
            if (b.O.all_gather(b.O.ctx, (alt && l.Wsh_alt) ? l.Wsh_alt : l.Wsh, (int64_t)((size_t)l.outp * l.inp * e->esz), b.ws) != 0) {
                d.broken = true;
                RTX_CHECK(false, RTX_EHIP, "data parallel: all_gather failed: %s", rtx_last_error_str());
            }
            d.st_all_gather += (int64_t)((size_t)l.outp * l.inp * e->esz);
            d.st_collectives += 1;
        }
    return RTX_OK;
}

int dp_bucket(const StepCtx& c, int l_lo, int l_hi, hipStream_t ws, bool alt)
{
    const bool side = ws == c.e->side && c.two;
    // the side stream's bucket talks through its own communicator: RCCL orders the operations of ONE communicator in issue
    // order across streams, which would make bucket B's reduce (caller's stream) wait for bucket A's all-gather
    const DpBucket b = {c, l_lo, l_hi, ws, side, side ? c.dp->ops_side : c.dp->ops};
    int order[2 * 2 * RTX_MAX_LAYERS];
    const int n_order = dp_layout_order(c.e, order);
    RTX_TRY(dp_stage(b, order, n_order));
    RTX_TRY(dp_exchange(b, order, n_order));
    RTX_TRY(dp_adam(b, alt));
    return dp_all_gather(b, alt);
}

extern "C" {

int rtx_engine_dp_attach(rtx_engine* e, const rtx_dp_cfg* cfg)
{
    RTX_CHECK(e, RTX_EINVAL, "engine is NULL");
    RTX_HIP(hipDeviceSynchronize());
    e->join_pending = e->join_fold = false;   // (every stream has drained)
    dp_release(e);
    if (!cfg) return RTX_OK;
    RTX_CHECK(!e->gvae, RTX_EINVAL, "dp_attach: the VAE_net variant (RTX_GVAE) has no data-parallel step");
    RTX_CHECK(!e->ae, RTX_EINVAL, "dp_attach: the plain autoencoder variant (RTX_AE) has no data-parallel step");
    RTX_NO_USERS(e, "dp_attach", "the single-GPU step rtx_engine_train_step (the table's rows are updated in place, there is no gradient to exchange)");
    RTX_CHECK(e->optim.plain_adam(), RTX_EINVAL, "dp_attach: the data-parallel step runs Adam only; the engine's optimizer is kind %d flags %d", e->optim.kind, e->optim.flags);
    RTX_CHECK(e->clip.mode == RTX_CLIPM_NONE, RTX_EINVAL, "dp_attach: gradient clipping is set (mode %d); the bucketed exchange has no global gradient norm", e->clip.mode);
    RTX_CHECK(e->accum_mode == RTX_ACCUM_OFF && e->accum_layers == 0, RTX_EINVAL, "dp_attach: a gradient accumulation window is open (mode %d); the data-parallel step has none", e->accum_mode);
    RTX_CHECK(cfg->world >= 1 && cfg->rank >= 0 && cfg->rank < cfg->world, RTX_EINVAL, "dp_attach: rank %d of %d", cfg->rank, cfg->world);
    RTX_CHECK(cfg->comm_dtype == RTX_FP32 || cfg->comm_dtype == RTX_BF16, RTX_EINVAL, "dp_attach: comm_dtype must be RTX_FP32 or RTX_BF16");
    RTX_CHECK((cfg->emulate != 0) + (cfg->comm != nullptr) + (cfg->ops != nullptr) == 1, RTX_EINVAL,
              "dp_attach: give exactly one of comm (RCCL), ops (caller's collectives) or emulate");
    DpState& d = e->dp;
    d.cfg = *cfg;
    if (cfg->emulate) {
        d.ops = rtx_dp_ops{dp_emu_all_reduce, dp_emu_reduce_scatter, dp_emu_all_gather, dp_emu_group_start, dp_emu_group_end, &e->dp};
    } else if (cfg->comm) {
        int32_t r = -1, w = -1;
        RTX_TRY(rtx_comm_rank(cfg->comm, &r, &w));
        RTX_CHECK(r == cfg->rank && w == cfg->world, RTX_EINVAL, "dp_attach: the communicator is rank %d of %d, the plan says %d of %d", r, w, cfg->rank, cfg->world);
        d.ops = rtx_dp_ops{dp_rccl_all_reduce, dp_rccl_reduce_scatter, dp_rccl_all_gather, dp_rccl_group_start, dp_rccl_group_end, cfg->comm};
    } else {
        RTX_CHECK(cfg->ops->all_reduce && cfg->ops->reduce_scatter && cfg->ops->all_gather, RTX_EINVAL, "dp_attach: ops needs all_reduce, reduce_scatter and all_gather");
        d.ops = *cfg->ops;
    }
    d.cfg.ops = nullptr;
    // bucket A's table: a second communicator / function table when the plan brings one, else the same as bucket B's
    d.ops_side = d.ops;
    d.two_comms = false;
    if (!cfg->emulate && cfg->comm && cfg->comm_side && !e->opt_dp_one_comm) {
        int32_t r = -1, w = -1;
        RTX_TRY(rtx_comm_rank(cfg->comm_side, &r, &w));
        RTX_CHECK(r == cfg->rank && w == cfg->world, RTX_EINVAL, "dp_attach: comm_side is rank %d of %d, the plan says %d of %d", r, w, cfg->rank, cfg->world);
        RTX_CHECK(cfg->comm_side != cfg->comm, RTX_EINVAL, "dp_attach: comm_side must be a communicator of its own (or NULL)");
        d.ops_side.ctx = cfg->comm_side;
        d.two_comms = true;
    } else if (!cfg->emulate && cfg->ops && cfg->ops_side && !e->opt_dp_one_comm) {
        RTX_CHECK(cfg->ops_side->all_reduce && cfg->ops_side->reduce_scatter && cfg->ops_side->all_gather, RTX_EINVAL,
                  "dp_attach: ops_side needs all_reduce, reduce_scatter and all_gather");
        d.ops_side = *cfg->ops_side;
        d.two_comms = true;
    }
    d.cfg.ops_side = nullptr;
    d.xesz = cfg->comm_dtype == RTX_BF16 ? 2 : 4;
    size_t biggest = 0;
    for (int li = 0; li < e->NL; ++li) {
        const Layer& l = e->L[li];
        // a hidden layer that keeps a transposed compute copy (WshT) is never sharded: that copy is a column-block layout
        const long min_elems = cfg->shard_min_elems > 0 ? (long)cfg->shard_min_elems : (long)e->opt_dp_shard_min_elems;
        d.shard[li] = cfg->sharded && (long)l.out * l.in >= min_elems && !l.WshT && l.outp % cfg->world == 0;
        biggest = std::max(biggest, (size_t)l.outp * l.inp * std::max(e->esz, d.xesz));
    }
    int order[2 * 2 * RTX_MAX_LAYERS];
    const int n_order = dp_layout_order(e, order);
    size_t off = 0;
    for (int q = 0; q < n_order; ++q) {
        d.xoff[order[q]] = off;
        off += (dp_region_elems(e, d, order[q]) + 63) / 64 * 64;
    }
    d.xbytes = off * d.xesz;
    RTX_TRY(dev_alloc(e, &d.xg, d.xbytes));
    if (cfg->emulate) {
        d.emu_bytes = 2 * biggest;
        RTX_TRY(dev_alloc(e, &d.emu_scratch, d.emu_bytes, false));
        // rows no rank updates here keep their weights in BOTH compute copies (the step alternates between them)
        RTX_TRY(ensure_shadows(e, nullptr));
        for (auto& l : e->L)
            if (l.Wsh_alt) RTX_HIP(hipMemcpy(l.Wsh_alt, l.Wsh, (size_t)l.outp * l.inp * e->esz, hipMemcpyDeviceToDevice));
    }
    d.on = true;
    return RTX_OK;
}

int rtx_engine_dp_owned_rows(const rtx_engine* e, int32_t layer, int32_t* row_lo, int32_t* row_hi, int32_t* sharded_out)
{
    RTX_CHECK(e && layer >= 0 && layer < e->NL, RTX_EINVAL, "dp_owned_rows: bad arguments");
    const Layer& l = e->L[layer];
    int lo = 0, hi = l.out, sh = 0;
    if (e->dp.on && e->dp.shard[layer]) {
        const int per = l.outp / e->dp.cfg.world;
        lo = std::min(e->dp.cfg.rank * per, l.out);
        hi = std::min((e->dp.cfg.rank + 1) * per, l.out);
        sh = 1;
    }
    if (row_lo) *row_lo = lo;
    if (row_hi) *row_hi = hi;
    if (sharded_out) *sharded_out = sh;
    return RTX_OK;
}

}  // extern "C"
