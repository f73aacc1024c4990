// engine_step.hip -- the training step of the engine: forward + loss + backward (+ optimizer), in its four schedules (StepKind),
// and the second stream they share.  One short sequence (run_step) over plain functions that take the step's context (StepCtx);
// the data-parallel exchange of a bucket is dp_bucket in engine_dp.hip, beside the plan it executes.
#include "engine_internal.h"

// ---- training --------------------------------------------------------------------------------------
// forward + loss + backward.  With FUSED (single-GPU bf16 step) the Adam update of every weight matrix whose rows are
// a multiple of 4 floats runs INSIDE its weight-gradient kernel (dw_adam.hip: the gradient never reaches HBM and the
// optimizer's HBM traffic overlaps the matrix work); biases and the remaining tensors follow in one small launch.
// Otherwise the gradients land in the bound buffers (data-parallel exchange, p.grad, float32 parity mode).
// (the float32 parity mode stores its gradients and runs one multi-tensor k_adam launch.  Round 4 measured Adam as an epilogue of its
//  TN product too -- IEEE sqrt / divisions on 64 accumulators per lane, 4-byte accesses in the MFMA layout: 1.130 ms per ml-20m step
//  against 1.052 with the separate launch, whose 110 us of streaming it replaced by ~190 us of epilogues: dropped)
static bool layer_fusable(const rtx_engine* e, const Layer& l) { return e->bf16 && l.in >= 4; }   // (rows of in % 4 != 0 floats: the strided epilogue, dw_adam.hip)
static bool layer_is_big(const Layer& l) { return (long)l.out * l.in >= (1L << 20); }
// the layers whose exp_avg / exp_avg_sq a deferred fused step keeps tile-major (by default layer_is_big's bound)
static bool layer_takes_tiles(const rtx_engine* e, const Layer& l) { return layer_fusable(e, l) && (long)l.out * l.in >= (long)e->opt_state_tiles_min_elems; }

// Head of a deferred fused step, on the caller's stream behind the resolved join: the moments of every such layer that are current in
// the bound tensors go into the layer's image -- always from the tensors, whatever an earlier import left in the image: the caller may
// have changed them since the write-back (load_state_dict, a checkpoint restore).  Between two deferred fused steps nothing is copied.
static bool state_needs_import(const rtx_engine* e)
{
    for (int li = 0; li < e->NL; ++li)
        if (layer_takes_tiles(e, e->L[li]) && !(li < (int)e->state_tiled.size() && e->state_tiled[li])) return true;
    return false;
}
static int state_import(rtx_engine* e, hipStream_t st)
{
    if (e->state_tiled.empty()) { e->state_tiled.assign(e->NL, 0); e->m_img.assign(e->NL, nullptr); e->v_img.assign(e->NL, nullptr); }
    for (int li = 0; li < e->NL; ++li) {
        const Layer& l = e->L[li];
        if (e->state_tiled[li] || !layer_takes_tiles(e, l)) continue;
        const int m_tiles = l.outp / rtx_dw_tile_rows(RTX_DW_64x128), n_tiles = (l.inp + rtx_dw_tile_cols(RTX_DW_64x128) - 1) / rtx_dw_tile_cols(RTX_DW_64x128);
        const size_t bytes = rtx_dw_state_image_elems(m_tiles, n_tiles, RTX_DW_64x128) * sizeof(float);   // (the import writes every slot)
        if (!e->m_img[li]) RTX_TRY(dev_alloc(e, (void**)&e->m_img[li], bytes, false));
        if (!e->v_img[li]) RTX_TRY(dev_alloc(e, (void**)&e->v_img[li], bytes, false));
        TIMED("state_import");
        RTX_TRY(rtx_dw_state_relayout(e->m[2 * li], e->v[2 * li], e->m_img[li], e->v_img[li], l.out, l.in, m_tiles, n_tiles, RTX_DW_64x128, 1, st));
        e->state_tiled[li] = 1;
        ++e->st_state_imports;
    }
    return RTX_OK;
}

// A deferred join folded into the first-layer product (RtxGemm::wait_word) makes EVERY workgroup of that grid spin until the side
// stream has stored its number.  The side stream's remaining kernels (weight gradient + Adam, loss sum, the next batch's gather, the
// store itself) must therefore be able to make progress beside a grid that is entirely resident and spinning.  Occupancy argument: the
// register-staged 128 x 128 product takes 73 728 B of LDS per workgroup, i.e. at most TWO workgroups per CU whatever else limits it; a
// grid of G workgroups leaves at least 2 * n_cus - G of those slots empty, and a CU with an empty slot has >= 86 KB of LDS, >= 28 wave
// slots and >= 328 registers per lane and SIMD free -- room for a workgroup of any kernel the side stream runs (the largest, the 64 x 128
// weight-gradient tile: 72 KB, 8 waves, <= 128 registers).  With fewer than 16 empty slots, or any other product kernel, the join is
// the one-wave k_hop_wait in front of the step instead (resolve_join): a spinning wave that holds nothing.
static bool fold_has_room(const rtx_engine* e, int Mp, int Np, int Kp)
{
    const GemmPlan pl = plan_gemm(e, Mp, Np, Kp, RTX_FORM_NT);
    if (!pl.regstage || pl.cfg != RTX_TILE_128x128) return false;
    const long groups = pl.splits > 1 ? pl.splits : (pl.m_tiles <= pl.n_tiles ? pl.n_tiles : pl.m_tiles);
    const long gsize = pl.splits > 1 ? (long)pl.m_tiles * pl.n_tiles : (pl.m_tiles <= pl.n_tiles ? pl.m_tiles : pl.n_tiles);
    const long grid = 8 * ((groups + 7) / 8) * gsize;   // (rtx_gemm_launch's grid: idle workgroups of the XCD padding exit at once, counted anyway)
    return grid + 16 <= 2L * e->n_cus;
}

// ---- the second stream of the step ------------------------------------------------------------------------------------------
// HIP maps streams onto a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in creation order.  A process that also
// runs RCCL / torch.distributed has created a dozen streams before the engine's first step, and the engine's new stream can land
// on the SAME hardware queue as the caller's: its kernels then simply queue up behind / in front of the caller's and the step
// runs serially (rocprofv3 showed both streams on queue 1: 397 us/step against 343 -- profiles/r3_dp_priority_experiment.txt).
// So the stream is PROBED: a kernel that spins for ~150 us goes on the caller's stream, an empty kernel on the candidate; the
// candidate is kept if its kernel finishes while the spinner is still running.  Up to 8 candidates at normal priority, then
// one at the highest priority (a different queue pool); with none found the step falls back to one stream.
extern "C" {
__global__ void k_probe_spin(unsigned long long ticks, int* sink)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // constant 100 MHz counter
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) {}
    if (sink && ticks == 0xffffffffffffffffull) *sink = 1;
}
__global__ void k_probe_nop() {}
}

static int make_side_stream(rtx_engine* e, hipStream_t st)
{
    RTX_HIP(hipStreamSynchronize(st));
    if (e->side) RTX_HIP(hipStreamSynchronize(e->side));   // (the previous caller's stream keeps its side stream in the cache)
    e->side = nullptr;
    e->side_for = st;
    auto hit = e->side_cache.find(st);
    if (hit != e->side_cache.end()) {
        e->side = hit->second.first;
        e->side_concurrent = hit->second.second;
        return RTX_OK;
    }
    int prio_least = 0, prio_greatest = 0;
    RTX_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    hipEvent_t ev_spin = nullptr, ev_cand = nullptr;
    RTX_HIP(hipEventCreateWithFlags(&ev_spin, hipEventDisableTiming));
    RTX_HIP(hipEventCreateWithFlags(&ev_cand, hipEventDisableTiming));
    std::vector<hipStream_t> rejected;
    hipStream_t found = nullptr;
    for (int attempt = 0; attempt < 9 && !found; ++attempt) {
        hipStream_t cand = nullptr;
        if (hipStreamCreateWithPriority(&cand, hipStreamNonBlocking, attempt < 8 ? 0 : prio_greatest) != hipSuccess) break;
        hipLaunchKernelGGL(k_probe_spin, dim3(1), dim3(64), 0, st, 15000ull, (int*)nullptr);   // 150 us
        (void)hipEventRecord(ev_spin, st);
        hipLaunchKernelGGL(k_probe_nop, dim3(1), dim3(64), 0, cand);
        (void)hipEventRecord(ev_cand, cand);
        (void)hipEventSynchronize(ev_cand);
        const bool concurrent = hipEventQuery(ev_spin) == hipErrorNotReady;   // the spinner is still at it: different hardware queues
        (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        if (concurrent) found = cand;
        else rejected.push_back(cand);
    }
    for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
    (void)hipEventDestroy(ev_spin);
    (void)hipEventDestroy(ev_cand);
    e->side_concurrent = found != nullptr;
    if (!found) {
        static bool said = false;   // once per process: the step silently losing its second stream costs ~20 %
        if (!said) fprintf(stderr, "rectorch_hip: no HIP stream runs beside the caller's (all candidates share its hardware queue): the training step uses ONE stream\n");
        said = true;
        RTX_HIP(hipStreamCreateWithFlags(&found, hipStreamNonBlocking));   // (keeps the code paths alive; the step still orders everything by events)
    }
    e->side = found;
    e->side_cache[st] = {found, e->side_concurrent};
    return RTX_OK;
}

// the side stream that belongs to the caller's stream `st`, and the events of the two-stream step
static int ensure_side_stream(rtx_engine* e, hipStream_t st)
{
    if (e->side && e->side_for == st) return RTX_OK;
    RTX_TRY(make_side_stream(e, st));
    if (!e->ev_done) {
        // (events created with hipEventReleaseToDevice -- a device-scope release at the record -- measure the same: 328.0 vs 327.7 us)
        for (int l = 0; l < e->NL + 1; ++l) RTX_HIP(hipEventCreateWithFlags(&e->ev_d[l], hipEventDisableTiming));
        RTX_HIP(hipEventCreateWithFlags(&e->ev_done, hipEventDisableTiming));
    }
    return RTX_OK;
}

// `to` continues only after everything enqueued on `from` so far: a write / wait pair of stream memory operations on word `slot` of
// the engine's signal memory (monotonic sequence numbers, compare >=), or an event record + wait
static int stream_dependency(rtx_engine* e, hipStream_t from, hipStream_t to, hipEvent_t ev, int slot)
{
    if (e->opt_hop_kernels) {
        RTX_TRY(ensure_hopk(e));
        const uint32_t v = ++e->hopk_seq;       // (compared as a signed difference: wraps after 2^31 hops without any reset)
        RTX_TRY(launch_hop_set(e, from, slot, v));
        return launch_hop_wait(e, to, slot, v);
    }
    if (e->opt_hop_values) {
        if (!e->hop_mem) {
            int dev = 0, ok = 0;
            RTX_HIP(hipGetDevice(&dev));
            if (hipDeviceGetAttribute(&ok, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess || !ok ||
                hipExtMallocWithFlags((void**)&e->hop_mem, 64, hipMallocSignalMemory) != hipSuccess) {
                (void)hipGetLastError();
                e->hop_mem = nullptr;
                e->opt_hop_values = 0;   // not available here: events
            } else {
                RTX_HIP(hipMemset(e->hop_mem, 0, 64));
                RTX_HIP(hipStreamSynchronize(nullptr));   // (the NULL stream's memset must not land after a write of `from`, see dev_alloc)
            }
        }
        if (e->hop_mem) {
            // two numbers per step: 2^31 is reached after ~80 hours of 270-us steps.  Before the sequence gets there (whether the
            // device compares signed or unsigned) both streams drain and the words start again from zero.
            if (e->hop_seq >= e->hop_wrap) {
                RTX_HIP(hipStreamSynchronize(from));
                RTX_HIP(hipStreamSynchronize(to));
                RTX_HIP(hipMemset(e->hop_mem, 0, 64));
                RTX_HIP(hipStreamSynchronize(nullptr));   // (the NULL stream's memset must not land after a write of `from`, see dev_alloc)
                e->hop_seq = 0;
            }
            const uint32_t v = ++e->hop_seq;
            RTX_HIP(hipStreamWriteValue32(from, e->hop_mem + slot, v, 0));
            RTX_HIP(hipStreamWaitValue32(to, e->hop_mem + slot, v, hipStreamWaitValueGte, 0xffffffffu));
            return RTX_OK;
        }
    }
    RTX_HIP(hipEventRecord(ev, from));
    RTX_HIP(hipStreamWaitEvent(to, ev, 0));
    return RTX_OK;
}

static void swap_img_sets(rtx_engine* e)
{
    std::swap(e->L[0].A, e->A0_alt);
    std::swap(e->tsum, e->tsum_alt);
    std::swap(e->img_written, e->img_written_alt);
    std::swap(e->img_nwritten, e->img_nwritten_alt);
    std::swap(e->img_cap, e->img_cap_alt);
    std::swap(e->img_exact, e->img_exact_alt);
}

// The batch announced for the NEXT step (rtx_engine_set_next_batch): its gather on the side stream, into the other image set.
// A hint: whatever keeps it from being issued is not an error (the next step then gathers for itself).
static int prefetch_next(rtx_engine* e)
{
    const rtx_batch& nb = e->next.b;
    if (!e->opt_prefetch || !e->bf16 || !e->side || !nb.csr || !nb.row_ids || nb.x_dense || nb.target_dense) return RTX_OK;
    if (nb.batch < 1 || nb.batch > e->cfg.max_batch || nb.csr->n_cols != e->Iin || nb.csr->max_row_len <= 0) return RTX_OK;
    if (nb.target_csr ? nb.target_csr->n_cols != e->I : e->Iin != e->I) return RTX_OK;
    RtxCsrView in = {}, tg = {};
    RTX_TRY(resolve_batch(e, &nb, &in, &tg, e->side));       // (a CSR batch: views only, nothing is enqueued)
    int64_t chunks = 0;
    if (sparse_in_ok(e, &in, rtx_pad_batch(nb.batch), &chunks)) return RTX_OK;   // the sparse first layer builds its own stream
    if (!e->A0_alt) {
        RTX_TRY(dev_alloc(e, &e->A0_alt, (size_t)e->Bp_alloc * e->L[0].inp * e->esz));
        RTX_TRY(dev_alloc(e, (void**)&e->tsum_alt, (size_t)e->Bp_alloc * sizeof(float)));
        e->img_exact_alt = false;
    }
    swap_img_sets(e);
    const int rc = gather_batch(e, &in, &tg, nb.batch, 1, &e->next.s, e->side);
    swap_img_sets(e);
    RTX_TRY(rc);
    e->pre.valid = true;
    e->pre.b = nb;
    e->pre.seed = e->next.s.seed; e->pre.offset = e->next.s.offset; e->pre.mask = e->next.s.dropout_mask;
    ++e->st_prefetch_issued;
    return RTX_OK;
}

// The end of a two-stream step.  With RTX_STEP_DEFER_JOIN the caller will not touch parameters / losses outside the engine before
// its next engine call (or rtx_engine_join): the side stream stores a number behind its last kernel, and whoever uses the engine
// next waits for it -- the next training step inside its first kernel (no packet, no gap between two steps on the caller's stream).
// Otherwise everything the step did is ordered on the caller's stream when the call returns (the same form of dependency as the
// step's fork: stream values where the device has them, else the event).
static int close_side_stream(StepCtx& c)
{
    rtx_engine* e = c.e;
    if ((c.step->flags & RTX_STEP_DEFER_JOIN) && e->opt_hop_fold && e->bf16) {
        RTX_TRY(ensure_hopk(e));
        e->join_seq = ++e->hopk_seq;
        RTX_TRY(launch_hop_set(e, e->side, 3, e->join_seq));
        e->join_pending = true;
        return RTX_OK;
    }
    return stream_dependency(e, e->side, c.st, e->ev_done, 1);
}

// ---- the pieces of the step ----------------------------------------------------------------------------------------------------
// Fused step, two streams.  After the loss kernel the critical path would be
//     dX chain (short latency-bound launches)  ->  every weight-gradient + Adam kernel (long streaming launches).
// The weight kernel of layer l needs only D[l] and A[l], so the two BIG ones run on a side stream: the decoder matrix
// beside the whole chain, the encoder matrix as soon as the chain has produced D[0]; the small layers' kernels follow
// the chain on the caller's stream, beside the encoder matrix.  A big layer's fused optimizer writes the NEXT step's
// compute copy (Wsh_alt; swapped at the end), because the chain still reads this step's.
// The encoder matrix's kernel is the END of the step's critical path (it needs D[0], the last thing the chain produces, and
// the next step's first product needs its result).  A cross-stream dependency costs about 18 us from the event's record to
// the first workgroup of the waiting stream and a record about 7 us on the recording stream (profiles/r2_step_timeline.txt),
// so that kernel stays on the CALLER's stream right behind the chain -- no hop before it, none after it -- and takes the small
// layers' weight kernels with it in the same launch (as launches of their own beside it they crawl: 53 + 33 us).
// (a hidden layer keeps ONE transposed compute copy, WshT, which its fused optimizer epilogue overwrites and the chain's
// k_bwd_hidden reads: such a layer's weight kernel must stay behind the chain on the caller's stream)
static bool on_side(const StepCtx& c, int li)
{
    const rtx_engine* e = c.e;
    const int NL = e->NL;
    if (c.dp) return c.two && NL >= 2 && li == NL - 1 && layer_is_big(e->L[li]) && !e->L[li].WshT;   // bucket A of the exchange
    return c.two && layer_is_big(e->L[li]) && li != c.main_li && !e->L[li].WshT;
}

static int reduce_loss(StepCtx& c, hipStream_t ws)
{
    rtx_engine* e = c.e;
    const rtx_step* step = c.step;
    ScopedTimer tm(e, "reduce_loss", ws);
    const bool reg_in_loss = c.dae_reg && !(step->flags & RTX_STEP_NO_REG_IN_LOSS);
    return rtx_launch_reduce_loss(e->row_loss, c.B * rtx_dlogits_chunks(e->Ip), step->lam, reg_in_loss ? e->sumsq : nullptr, 2 * e->NL, c.loss_out,
                                  c.loss_accum, ws, e->loss_mailbox, e->loss_mailbox ? ++e->loss_ticket : 0u, (uint32_t)step->step);
}

// weight + bias gradient of layer li on stream ws: gW[out][in] = D[Bp][outp]^T x A[Bp][inp] (both read K-major); column
// `in` of the product (the ones column of A) is the bias gradient
// bf16: the weight-gradient problem of layer li (fused with Adam where the layer allows it)
static bool make_dw(StepCtx& c, int li, RtxDw& d)
{
    rtx_engine* e = c.e;
    const rtx_step* step = c.step;
    const DpState* dp = c.dp;
    Layer& l = e->L[li];
    const bool fused = c.kind == STEP_FUSED && layer_fusable(e, l);
    d = RtxDw{};
    d.A = l.D; d.lda = l.outp; d.B = l.A; d.ldb = l.inp;
    d.m_tiles = l.outp / rtx_dw_tile_rows(c.dw_cfg); d.n_tiles = (l.inp + rtx_dw_tile_cols(c.dw_cfg) - 1) / rtx_dw_tile_cols(c.dw_cfg); d.k_slices = c.Bp / 64;
    d.M_real = l.out; d.N_real = l.in;
    if (fused) {
        RtxAdamArgs sc = {};
        fill_adam_scalars(e, step, sc, 2 * li);
        d.adam.p = e->params[2 * li]; d.adam.m = e->m[2 * li]; d.adam.v = e->v[2 * li];
        if (c.tiles && li < (int)e->state_tiled.size() && e->state_tiled[li]) { d.adam.m_img = e->m_img[li]; d.adam.v_img = e->v_img[li]; }
        d.adam.gkeep = c.keep_grads ? e->grads[2 * li] : nullptr;
        d.gbias = c.keep_grads ? e->grads[2 * li + 1] : nullptr;
        d.adam.sh = on_side(c, li) ? l.Wsh_alt : l.Wsh; d.adam.shT = l.WshT; d.adam.ld_sh = l.inp; d.adam.ld_shT = l.WshT ? l.outp : 0;
        d.adam.step_size = sc.step_size; d.adam.bc2_sqrt = sc.bc2_sqrt; d.adam.beta1 = sc.beta1; d.adam.beta2 = sc.beta2;
        d.adam.eps = sc.eps; d.adam.weight_decay = sc.weight_decay; d.adam.lam = sc.lam;
        d.adam.sumsq = c.dae_reg ? e->sumsq + 2 * li : nullptr;
        d.bias_p = e->params[2 * li + 1]; d.bias_m = e->m[2 * li + 1]; d.bias_v = e->v[2 * li + 1];
        d.bias_sumsq = c.dae_reg ? e->sumsq + 2 * li + 1 : nullptr;
    } else if (dp) {
        // the gradient leaves the kernel as the image the exchange sends; RTX_STEP_KEEP_GRADS also stores this rank's own
        // (unreduced) float32 gradient in the bound buffers
        if (dp->cfg.comm_dtype == RTX_BF16) {
            d.g16 = dp->xg16(2 * li); d.gbias16 = dp->xg16(2 * li + 1);
            if (c.keep_grads) { d.gW = e->grads[2 * li]; d.gbias = e->grads[2 * li + 1]; }
        } else {
            d.gW = dp->xg32(2 * li); d.gbias = dp->xg32(2 * li + 1);
        }
    } else if ((step->flags & RTX_STEP_GRADS_BF16) && !e->grads16.empty()) {
        // data-parallel bf16 exchange: the gradient leaves the kernel as the bf16 image the all-reduce sends (no float32
        // store, no cast pass)
        d.g16 = (bf16_t*)e->grads16[2 * li]; d.gbias16 = (bf16_t*)e->grads16[2 * li + 1];
    } else {
        d.gW = e->grads[2 * li]; d.gbias = e->grads[2 * li + 1];
    }
    return fused;
}

// gradient accumulation: layer li's product adds (its accumulators hold a term of this window) or stores the window's first term
static bool accum_adds(const rtx_engine* e, int li) { return e->accum_mode == RTX_ACCUM_ADD && (e->accum_layers >> li & 1u); }

static int weight_grad_bf16(StepCtx& c, int li, hipStream_t ws)
{
    rtx_engine* e = c.e;
    RtxDw d;
    const bool fused = make_dw(c, li, d);
    // the fused step's side-stream launch runs beside the data-gradient chain: one workgroup per CU leaves the chain room (RtxDw::lds_pad)
    if (fused && !c.dp && c.two && ws == e->side && ws != c.st && c.dw_cfg == RTX_DW_64x128) d.lds_pad = e->opt_dw_side_pad;
    if (e->accum_mode != RTX_ACCUM_OFF) {   // (never fused, never data parallel: run_step and the setter see to it) -- into the accumulators
        d.acc_scale = e->accum_scale;
        return rtx_dw_launch(d, accum_adds(e, li) ? RTX_DW_GRAD_ADD : RTX_DW_GRAD_FIRST, c.dw_cfg, ws);
    }
    return rtx_dw_launch(d, fused ? RTX_DW_ADAM : RTX_DW_GRAD, c.dw_cfg, ws);
}

static int weight_grad_f32(StepCtx& c, int li, hipStream_t ws)
{
    rtx_engine* e = c.e;
    const DpState* dp = c.dp;
    Layer& l = e->L[li];
    RtxGemm g = {};
    g.form = RTX_FORM_TN;
    g.A = l.D; g.lda = l.outp; g.B = l.A; g.ldb = l.inp;
    g.k_slices = c.Bp / 32; g.tile_shape = RTX_TILE_128x128; g.m_tiles = l.outp / 128; g.n_tiles = l.inp / 128;
    g.splits = 1; g.C = e->grads[2 * li]; g.gbias = e->grads[2 * li + 1];
    if (dp && dp->cfg.comm_dtype == RTX_FP32) { g.C = dp->xg32(2 * li); g.gbias = dp->xg32(2 * li + 1); }
    g.M_real = l.out; g.N_real = l.in;
    // A hidden layer's gradient is 10-20 tiles of 128 x 128 with K = the batch: one workgroup per tile walks 16 K slices at the
    // f32 MFMA rate of ONE CU (1.7 us per slice) while 240 CUs idle -- 40 us per launch, 80 us of the 1.05-ms float32 step
    // (profiles/r4_fp32_step_timeline.txt).  Such products are split over the batch into slabs and summed in a fixed order.
    const int tiles = g.m_tiles * g.n_tiles;
    int sp = std::min(8, g.k_slices / 2);
    while (sp > 1 && (sp - 1) * ((g.k_slices + sp - 1) / sp) >= g.k_slices) --sp;   // no empty split
    // (Cacc is shared with the data-gradient products: safe because the float32 step runs every kernel on the caller's stream)
    if (e->opt_f32_dw_split && tiles <= 64 && sp >= 2 && (size_t)sp * l.outp * l.inp <= e->cacc_elems) {
        float* gW = g.C;
        float* gb = g.gbias;
        g.splits = sp; g.C = e->Cacc; g.ldc = l.inp; g.slab_stride = (long)l.outp * l.inp; g.gbias = nullptr;
        RTX_TRY(rtx_gemm_f32_km_launch(g, RTX_EPI_STORE, ws));
        if (e->accum_mode != RTX_ACCUM_OFF)   // the slabs as ever; the reduce weights their sum into the accumulators
            return rtx_launch_dw_slab_reduce_acc(e->Cacc, sp, g.slab_stride, g.ldc, l.out, l.in, gW, gb, accum_adds(e, li), e->accum_scale, ws);
        return rtx_launch_dw_slab_reduce(e->Cacc, sp, g.slab_stride, g.ldc, l.out, l.in, gW, gb, ws);
    }
    if (e->accum_mode != RTX_ACCUM_OFF) {
        g.acc_scale = e->accum_scale;
        return rtx_gemm_f32_km_launch(g, accum_adds(e, li) ? RTX_EPI_GRAD_ADD : RTX_EPI_GRAD_FIRST, ws);
    }
    return rtx_gemm_f32_km_launch(g, RTX_EPI_GRAD, ws);
}

static int weight_grad(StepCtx& c, int li, hipStream_t ws)
{
    rtx_engine* e = c.e;
    const bool fused = c.kind == STEP_FUSED && layer_fusable(e, e->L[li]);
    const char* site = li == e->NL - 1 ? (fused ? "dW_adam_out" : "gemm_dW_out") : (li == 0 ? (fused ? "dW_adam_in" : "gemm_dW_in") : (fused ? "dW_adam_hidden" : "gemm_dW_hidden"));
    if (e->accum_mode != RTX_ACCUM_OFF)   // the accumulating instantiations are timed under names of their own, beside the plain-store ones
        site = li == e->NL - 1 ? "gemm_dW_out_acc" : (li == 0 ? "gemm_dW_in_acc" : "gemm_dW_hidden_acc");
    ScopedTimer tm(e, site, ws);
    RTX_TRY(e->bf16 ? weight_grad_bf16(c, li, ws) : weight_grad_f32(c, li, ws));
    if (e->accum_mode != RTX_ACCUM_OFF) e->accum_layers |= 1u << li;
    return RTX_OK;
}

// what the side stream does for layer li once D[li] is there: the long weight kernel, and under data parallelism bucket A
static int side_work(StepCtx& c, int li)
{
    rtx_engine* e = c.e;
    RTX_TRY(weight_grad(c, li, e->side));
    if (c.dp) {   // bucket A: the decoder matrix's exchange and optimizer pass run beside the chain; the loss sum rides along
        RTX_TRY(reduce_loss(c, e->side));
        RTX_TRY(dp_bucket(c, li, li + 1, e->side, true));
    }
    return RTX_OK;
}

// data gradient of layer li: dA[Bp][inp] = D[Bp][outp] x Wsh[outp][inp]   (Wsh read K-major).  On ONE stream it must come before
// the weight kernel of this layer, whose fused optimizer epilogue overwrites the compute copy.  With fold_hop the product also
// stores fold_seq for the side stream, whose wait and work are enqueued right behind it.
static int data_grad(StepCtx& c, int li, bool fold_hop, uint32_t fold_seq)
{
    rtx_engine* e = c.e;
    hipStream_t st = c.st;
    const rtx_step* step = c.step;
    const int NL = e->NL, B = c.B, Bp = c.Bp;
    Layer& l = e->L[li];
    if (li > 0 && li < NL - 1 && l.WshT && e->opt_small_bwd) {
        // a hidden layer: product with the transposed compute copy + the activation derivative (or the VAE head's
        // backward) + the bf16 gradient of the layer below in one launch (small_layers.hip)
        Layer& pv = e->L[li - 1];
        RtxSmallBwdArgs a = {};
        a.D = (const bf16_t*)l.D; a.WT = (const bf16_t*)l.WshT; a.ld = l.outp; a.wt_rows = l.inp;
        a.B = B; a.Bp = Bp; a.Np = pv.outp; a.Dout = (bf16_t*)pv.D;
        if (e->vae && li == e->cfg.n_enc) {
            a.Z = e->Z; a.training = 1; a.mu32 = e->mu32; a.lv32 = e->lv32; a.eps32 = e->eps32;
            a.beta = step->beta; a.inv_batch = step->inv_batch;
            a.g_mu = c.ext_mu; a.g_lv = c.ext_lv;
        } else {
            a.N_real = pv.out; a.tanh_act = pv.tanh_act; a.O32 = pv.O32;
        }
        TIMED(a.Z ? "bwd_head" : "bwd_hidden");
        return rtx_launch_small_bwd(a, st);
    }
    if (li == 0) return RTX_OK;
    int splits = 1;
    {
        TIMED(li == NL - 1 ? "gemm_dX_out" : "gemm_dX_hidden");
        RTX_TRY(gemm_to_cacc(e, RTX_FORM_NN, l.D, l.outp, l.Wsh, l.inp, Bp, l.inp, l.outp, &splits, st, fold_hop ? e->hopk_mem + 2 : nullptr, fold_seq));
        if (fold_hop) {   // the product that stores the number is enqueued: now the side stream's wait and its work
            RTX_TRY(launch_hop_wait(e, e->side, 2, fold_seq));
            RTX_TRY(side_work(c, li));
        }
    }
    Layer& pv = e->L[li - 1];
    if (e->vae && li == e->cfg.n_enc) {
        RtxVaeBwdArgs a = {};
        a.C = e->Cacc; a.splits = splits; a.slab_stride = (long)Bp * l.inp; a.ldc = l.inp;
        a.B = B; a.Bp = Bp; a.Z = e->Z; a.Np = pv.outp;
        a.mu32 = e->mu32; a.lv32 = e->lv32; a.eps32 = e->eps32; a.training = 1;
        a.beta = step->beta; a.inv_batch = step->inv_batch; a.D = pv.D;
        a.g_mu = c.ext_mu; a.g_lv = c.ext_lv;
        TIMED("vae_head_bwd");
        return rtx_launch_vae_bwd(a, e->bf16, st);
    }
    RtxPostArgs a = {};
    a.C = e->Cacc; a.splits = splits; a.slab_stride = (long)Bp * l.inp; a.ldc = l.inp;
    a.B = B; a.Bp = Bp; a.N_real = pv.out; a.Np = pv.outp;
    a.tanh_act = pv.tanh_act; a.O32 = pv.O32; a.R = pv.D;
    TIMED("post_bwd");
    // CDAE: layer 0's pre-activation gradient is the gradient of the batch's rows of V -- their update rides in this epilogue
    RtxPostUsers u;
    if (li == 1 && !c.ext && user_node_args(e, true, u)) return rtx_launch_post_users(a, u, RTX_POST_BWD, e->bf16, st);
    return rtx_launch_post(a, RTX_POST_BWD, e->bf16, st);
}

// ---- the step, in order ----------------------------------------------------------------------------------------------------------
// Prologue and forward pass: the join the previous step left open, the compute copies, the batch, the side stream, a prefetched
// batch image; then every layer's forward on the caller's stream.
static int begin_and_forward(StepCtx& c, const rtx_batch* batch)
{
    rtx_engine* e = c.e;
    hipStream_t st = c.st;
    const rtx_step* step = c.step;
    const bool two_kind = c.kind == STEP_FUSED || (c.dp && e->bf16);
    const int NL = e->NL;
    // a join the previous step left open (RTX_STEP_DEFER_JOIN): decided below, once it is known how this step starts
    // (a step that does not go on with the tile-major optimizer state writes it back first -- behind the join: ensure_shadows resolves
    //  it then and there)
    bool join_open = e->join_pending && e->shadows_valid && (c.tiles || !state_any_tiled(e));
    // Until the wait for that join has really been enqueued (the one-wave kernel, or the first-layer product that carries it), every
    // early return below -- a wrong batch size, a failed launch -- must leave the join OPEN: the next entry point (rtx_engine_join,
    // predict, apply_adam, the next step) still has to wait for the side stream's weight kernel before it reads what that writes.
    struct JoinGuard {
        rtx_engine* e; bool armed;
        ~JoinGuard() { if (armed) { e->join_pending = true; e->join_fold = false; } }
    } join_guard{e, join_open};
    if (join_open) e->join_pending = false;
    RTX_TRY(ensure_shadows(e, st, c.tiles));
    // layers to import: their copy reads what the side stream wrote, so the join cannot ride on the first-layer product
    const bool import = c.tiles && state_needs_import(e);
    RtxCsrView in = {};
    RTX_TRY(resolve_batch(e, batch, &in, &c.tg, st));
    c.B = batch->batch;
    c.Bp = rtx_pad_batch(c.B);
    // (see on_side for what the two streams do)
    // (data parallel: the second stream carries the decoder matrix's weight kernel, its exchange and its optimizer pass; the
    //  float32 parity mode keeps one compute copy per matrix and therefore one stream)
    c.two = two_kind && e->opt_two_stream;
    if (c.two) RTX_TRY(ensure_side_stream(e, st));
    if (c.two && !e->side_concurrent) c.two = false;   // no stream that really runs beside the caller's: one stream, no event traffic
    c.main_li = (c.two && c.kind == STEP_FUSED && e->opt_in_on_main && NL >= 2 && layer_is_big(e->L[0]) && layer_is_big(e->L[NL - 1]) && layer_fusable(e, e->L[0])) ? 0 : -1;
    if (e->pre.valid) {
        // the batch of this step was announced one step ago and gathered on the side stream under that step's last weight
        // kernel (the step's closing stream dependency ordered it before anything enqueued now): its image set becomes the
        // current one, the gather is skipped.  Anything else than exactly the announced batch / dropout stream: a normal step.
        const rtx_batch& pb = e->pre.b;
        const bool hit = two_kind && c.two && st == e->side_for && batch->csr && pb.csr == batch->csr && pb.row_ids == batch->row_ids &&
                         pb.target_csr == batch->target_csr && !batch->x_dense && !batch->target_dense && pb.batch == batch->batch &&
                         e->pre.seed == step->seed && e->pre.offset == step->offset && e->pre.mask == step->dropout_mask;
        e->pre.valid = false;
        if (hit) {
            swap_img_sets(e);
            e->gather_done = true;
            ++e->st_prefetch_hits;
            // this step starts with the first-layer product: the open join rides on it (run_forward; every workgroup checks the
            // number the side stream stored -- long ago -- before it touches the prefetched image)
            if (join_open && !import && e->opt_hop_fold && e->bf16 && fold_has_room(e, c.Bp, e->L[0].outp, e->L[0].inp)) { e->join_fold = true; join_open = false; ++e->st_join_folds; }
        }
    }
    if (join_open) {   // any other start: a one-wave kernel in front of the step
        e->join_pending = true;
        RTX_TRY(resolve_join(e, st, c.tiles));
    }
    if (import) RTX_TRY(state_import(e, st));
    // (RTX_GVAE, RTX_AE: no log-sum-exp partials and no half-precision logits -- their loss kernels read the float32 logits only)
    RTX_TRY(run_forward(e, &in, &c.tg, c.B, 1, step, (e->gvae || e->ae) ? 0 : 1, 0, NL, e->Y, e->Ip, nullptr, nullptr, st));
    join_guard.armed = false;   // the wait is on the stream (k_hop_wait above, or inside the first-layer product)
    return RTX_OK;
}

// loss and d loss / d logits in one pass over Y
static int loss_and_dlogits(StepCtx& c)
{
    rtx_engine* e = c.e;
    hipStream_t st = c.st;
    const rtx_step* step = c.step;
    if (c.dae_reg) {
        TIMED("sumsq");
        RTX_TRY(launch_sumsq(e, st));
    }
    RtxDlogitsArgs a = {};
    a.loss.Y = e->Y; a.loss.ldy = e->Ip; a.loss.B = c.B; a.loss.I = e->I; a.loss.target = c.tg; a.loss.tsum = e->tsum;
    a.loss.lse = e->lse; a.loss.row_loss = e->row_loss; a.loss.inv_batch = step->inv_batch;
    if (e->opt_lse_fuse) { a.loss.part = e->lse_part; a.loss.n_strips = e->lse_strips; a.loss.part_ld = e->lse_strips; }
    if (e->vae) { a.loss.mu32 = e->mu32; a.loss.lv32 = e->lv32; a.loss.Z = e->Z; a.loss.beta = step->beta; }
    a.Bp = c.Bp; a.D = e->L[e->NL - 1].D; a.ldd = e->Ip;
    if (e->gvae) {
        // binary cross-entropy: the mean over all B x n_items elements (1 / (B I), from the step's 1 / B)
        a.loss.part = nullptr;
        TIMED("bce_dlogits_loss");
        return rtx_launch_bce_dlogits(a, step->inv_batch / (float)e->I, e->bf16, st);
    }
    if (e->ae) {
        // mean squared error over all B x n_items elements (1 / (B I), from the step's 1 / B) against the stored target values
        a.loss.part = nullptr;
        TIMED("mse_dlogits_loss");
        return rtx_launch_mse_dlogits(a, step->inv_batch / (float)e->I, e->bf16, st);
    }
    if (logits16_on(e)) a.Y16 = a.D;   // run_forward left half-precision logits there
    TIMED("dlogits_loss");
    return rtx_launch_dlogits(a, e->bf16, st);
}

// the layer loop, last layer first: per layer the side stream's fork, the data gradient, on ONE stream the weight gradient.
// [l_lo, l_hi]: the layers of one half (rtx_engine_encode_backward / decode_backward; l_hi < 0: all of them).  A range that ends above
// layer 0 leaves out the data gradient of layer l_lo: what leaves the chain there is the caller's business (d loss / d z).
static int backward_layers(StepCtx& c, rtx_layer_cb cb, void* user, int l_hi = -1, int l_lo = 0)
{
    rtx_engine* e = c.e;
    hipStream_t st = c.st;
    const int NL = e->NL;
    if (l_hi < 0) l_hi = NL - 1;
    if (!c.two && !c.ext) RTX_TRY(reduce_loss(c, st));
    for (int li = l_hi; li >= l_lo; --li) {
        Layer& l = e->L[li];
        bool fold_hop = false;          // this layer's fork is folded into its data-gradient product
        uint32_t fold_seq = 0;
        if (on_side(c, li)) {   // the long kernel first: it only needs D[li], which exists now
            // The fork (round 5, "hop_fold"): the side stream waits in a one-wave kernel (k_hop_wait) for a number that the NEXT kernel
            // of the caller's stream -- this layer's data-gradient product, which follows the producers of D[li] in order -- stores as
            // its first instruction.  The caller's stream, which carries the step's critical path, gets no packet of its own: the
            // 6-9 us gap behind k_dlogits (profiles/r4_step_timeline.txt) goes.
            // The number is stored by a kernel that is enqueued AFTER this point, so the side stream's work is enqueued behind it
            // (side_work in data_grad): a host that blocks on the side stream in between -- the gloo test transport drains the device inside
            // its collectives -- would otherwise wait for a number nobody has been told to write yet.
            fold_hop = e->opt_hop_fold && e->bf16 && li > 0 && !(li < NL - 1 && l.WshT && e->opt_small_bwd) &&
                       !plan_gemm(e, c.Bp, l.inp, l.outp, RTX_FORM_NN).regstage;
            if (fold_hop) {
                RTX_TRY(ensure_hopk(e));
                fold_seq = ++e->hopk_seq;
            } else {
                RTX_TRY(stream_dependency(e, st, e->side, e->ev_d[li], 0));
                RTX_TRY(side_work(c, li));
            }
        }
        if (li > l_lo || l_lo == 0) RTX_TRY(data_grad(c, li, fold_hop, fold_seq));
        if (!c.two) RTX_TRY(weight_grad(c, li, st));
        if (c.kind == STEP_FUSED && !layer_fusable(e, l)) {   // what is left for the multi-tensor Adam launch at the end of the step
            RtxAdamArgs one = {};
            fill_adam_tensors(e, one, li, li + 1);
            c.rest_ids[c.rest.n] = 2 * li; c.rest.t[c.rest.n++] = one.t[0];
            c.rest_ids[c.rest.n] = 2 * li + 1; c.rest.t[c.rest.n++] = one.t[1];
        }
        if (cb) cb(li, user);
    }
    return RTX_OK;
}

// gradients from both streams feed the leftover Adam launch: the side stream waits for the caller's, then runs it
static int leftover_adam_to_side(StepCtx& c, hipStream_t* rs)
{
    rtx_engine* e = c.e;
    if (c.rest.n == 0) return RTX_OK;
    RTX_HIP(hipEventRecord(e->ev_d[e->NL], c.st));
    RTX_HIP(hipStreamWaitEvent(e->side, e->ev_d[e->NL], 0));
    *rs = e->side;
    return RTX_OK;
}

// fused step, two streams, the encoder matrix on the caller's stream ("in_on_main"): behind the chain, on this stream: the encoder
// matrix's kernel and the small layers' (their compute copies have no reader left) ...
static int finish_in_on_main(StepCtx& c, hipStream_t* rs)
{
    rtx_engine* e = c.e;
    hipStream_t st = c.st;
    // ... ONE launch for the encoder matrix and the small fusable layers (small problems first); small layers that are not
    // fusable store their gradients first, for the leftover Adam launch.  The loss reduction only needs what the loss kernel
    // wrote: it goes behind the decoder matrix's kernel on the side stream (no new event).
    RtxDw grp[RTX_DW_GROUP_MAX];
    int ng = 0;
    for (int li = e->NL - 1; li >= 1; --li) {
        if (on_side(c, li)) continue;
        if (layer_fusable(e, e->L[li]) && ng < RTX_DW_GROUP_MAX - 1) make_dw(c, li, grp[ng++]);
        else RTX_TRY(weight_grad(c, li, st));
    }
    make_dw(c, c.main_li, grp[ng++]);
    {
        ScopedTimer tm(e, "dW_adam_in", st);
        RTX_TRY(rtx_dw_launch_group(grp, ng, RTX_DW_ADAM, c.dw_cfg, st));
    }
    RTX_TRY(reduce_loss(c, e->side));
    // the side stream idles from here to the end of the step: the NEXT step's gather, when its batch was announced
    if (e->next.valid && !c.rest.n) RTX_TRY(prefetch_next(e));
    return leftover_adam_to_side(c, rs);
}

// fused step, two streams, both big matrices on the side stream: behind the chain, beside the encoder matrix's kernel: the small
// layers' weight kernels (their compute copies have no reader left on this stream) and the loss reduction
static int finish_two_stream(StepCtx& c, hipStream_t* rs)
{
    for (int li = c.e->NL - 1; li >= 0; --li)
        if (!on_side(c, li)) RTX_TRY(weight_grad(c, li, c.st));
    RTX_TRY(reduce_loss(c, c.st));
    return leftover_adam_to_side(c, rs);
}

// fused step: what the layer loop left (on one stream: nothing but the leftover Adam launch), the swap of the compute copies the
// side stream wrote, the join
static int finish_fused(StepCtx& c)
{
    rtx_engine* e = c.e;
    hipStream_t rs = c.st;    // the stream the leftover Adam launch runs on
    if (c.two && c.main_li >= 0) RTX_TRY(finish_in_on_main(c, &rs));
    else if (c.two) RTX_TRY(finish_two_stream(c, &rs));
    if (c.rest.n > 0) {
        fill_adam_scalars(e, c.step, c.rest, 0, c.rest_ids);
        ScopedTimer tm(e, "adam_small", rs);
        RTX_TRY(rtx_launch_adam(c.rest, e->bf16, rs));
    }
    if (c.two) {
        for (int li = 0; li < e->NL; ++li)
            if (on_side(c, li) && layer_fusable(e, e->L[li])) std::swap(e->L[li].Wsh, e->L[li].Wsh_alt);
        RTX_TRY(close_side_stream(c));
    }
    e->shadows_valid = true;
    return RTX_OK;
}

// float32, or bf16 with the fused optimizer switched off: every gradient is in its bound buffer on the caller's stream; one
// multi-tensor Adam launch behind them
static int finish_unfused_adam(StepCtx& c)
{
    rtx_engine* e = c.e;
    hipStream_t st = c.st;
    RtxAdamArgs a = {};
    fill_adam_tensors(e, a, 0, e->NL);
    fill_adam_scalars(e, c.step, a, 0);
    if (e->clip.mode != RTX_CLIPM_NONE) {   // the norm pass and its finish first, on this stream: every gradient is there, no parameter has moved
        TIMED("grad_norm");
        RTX_TRY(rtx_clip_prepare(a, e->clip, (uint32_t)c.step->step, st));
    }
    {
        TIMED("adam");
        RTX_TRY(rtx_launch_adam(a, e->bf16, st));
    }
    e->shadows_valid = true;
    e->accum_mode = RTX_ACCUM_OFF;   // an accumulation window ends with its optimizer launch
    e->accum_layers = 0;
    return RTX_OK;
}

// data parallel: bucket B behind the chain on the caller's stream: the remaining weight kernels (bf16: grouped launches), their
// exchange, their optimizer pass -- the END of the step's critical path, so no stream hop before or between them
static int finish_data_parallel(StepCtx& c)
{
    rtx_engine* e = c.e;
    hipStream_t st = c.st;
    const int NL = e->NL;
    const bool dp_side = on_side(c, NL - 1);
    const int b_hi = dp_side ? NL - 1 : NL;
    if (c.two) {
        RtxDw grp[RTX_DW_GROUP_MAX];
        int ng = 0;
        for (int li = b_hi - 1; li >= 0; --li) {
            make_dw(c, li, grp[ng++]);
            if (ng == RTX_DW_GROUP_MAX || li == 0) {
                ScopedTimer tm(e, "gemm_dW_in", st);
                RTX_TRY(rtx_dw_launch_group(grp, ng, RTX_DW_GRAD, c.dw_cfg, st));
                ng = 0;
            }
        }
        if (!dp_side) RTX_TRY(reduce_loss(c, st));
    }
    RTX_TRY(dp_bucket(c, 0, b_hi, st, false));
    if (dp_side) {
        std::swap(e->L[NL - 1].Wsh, e->L[NL - 1].Wsh_alt);
        // (round 6) the side stream has finished bucket A long before bucket B's exchange ends: the NEXT step's gather goes there,
        // behind bucket A and in front of the join -- the data-parallel step then starts with its first-layer product as well
        if (e->next.valid) RTX_TRY(prefetch_next(e));
        RTX_TRY(close_side_stream(c));
    }
    e->shadows_valid = true;
    return RTX_OK;
}

static int run_step(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* loss_out, float* loss_accum, rtx_layer_cb cb, void* user,
                    hipStream_t st, StepKind kind)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(step, RTX_EINVAL, "loss_grads: step is NULL");
    DpState* dp = kind == STEP_DATA_PARALLEL ? &e->dp : nullptr;
    RTX_CHECK(!(dp && e->gvae), RTX_EINVAL, "data parallel: the VAE_net variant (RTX_GVAE) has no data-parallel step");
    RTX_CHECK(!(dp && e->ae), RTX_EINVAL, "data parallel: the plain autoencoder variant (RTX_AE) has no data-parallel step");
    rtx_step gstep;
    if (e->gvae) {   // VAE.loss_function: BCE + KLD, no beta and no annealing (reference models.py:581-583)
        gstep = *step;
        gstep.beta = 1.f;
        step = &gstep;
    }
    if (e->ae) {   // AETrainer.loss_function: the MSE alone, no regulariser and no KL term (reference models.py:377)
        gstep = *step;
        gstep.lam = 0.f;
        gstep.beta = 0.f;
        step = &gstep;
    }
    if (e->users.bound()) {   // CDAE (include/rectorch_hip.h): before anything is enqueued
        RTX_CHECK(!dp && !e->dp.on, RTX_EINVAL, "user table (CDAE): a data-parallel plan is attached; supported: the single-GPU steps (rtx_engine_train_step, rtx_engine_loss_grads)");
        RTX_CHECK(e->clip.mode == RTX_CLIPM_NONE, RTX_EINVAL, "user table (CDAE): gradient clipping is set (mode %d); supported: RTX_CLIP_NONE", e->clip.mode);
        RTX_CHECK(e->accum_mode == RTX_ACCUM_OFF, RTX_EINVAL, "user table (CDAE): gradient accumulation is set (mode %d); supported: one batch per update (RTX_ACCUM_OFF)", e->accum_mode);
        if (e->users.next.ids) {
            RTX_CHECK(e->users.m && e->users.v, RTX_ESTATE, "user table (CDAE): the table was bound without exp_avg / exp_avg_sq (inference only); bind them to train");
            RTX_CHECK(e->users.next.step >= 1, RTX_EINVAL, "user table (CDAE): rtx_engine_set_users came with step %d; a training call needs step >= 1", e->users.next.step);
        }
    }
    struct ClearNext { rtx_engine* e; ~ClearNext() { e->next.valid = false; } } clear_next{e};   // an announcement is for ONE step
    if (dp) {
        RTX_CHECK(!dp->broken, RTX_ESTATE, "data parallel: a collective of an earlier step failed; attach the plan again (rtx_engine_dp_attach)");
        dp->st_all_reduce = dp->st_reduce_scatter = dp->st_all_gather = 0;
        dp->st_collectives = 0;
    }
    StepCtx c = {};
    c.e = e; c.step = step; c.st = st; c.kind = kind; c.dp = dp;
    c.loss_out = loss_out; c.loss_accum = loss_accum;
    c.dae_reg = !e->vae && step->lam != 0.f;
    if (dp && c.dae_reg)   // lam * W / ||W|| needs the norm of the WHOLE matrix; a rank of the sharded optimizer holds current rows of its shard only
        for (int li = 0; li < e->NL; ++li)
            RTX_CHECK(!dp->shard[li], RTX_EINVAL, "data parallel: Mult-DAE's norm regulariser (lam != 0) needs whole master matrices; attach with sharded = 0");
    c.keep_grads = (step->flags & RTX_STEP_KEEP_GRADS) != 0;
    if (e->accum_mode != RTX_ACCUM_OFF) {   // before anything is enqueued: the accumulators are the float32 buffers of ONE device
        RTX_CHECK(!dp && !e->dp.on, RTX_EINVAL, "gradient accumulation: a data-parallel plan is attached; supported: the single-GPU steps (rtx_engine_loss_grads, rtx_engine_train_step)");
        RTX_CHECK(kind != STEP_FUSED, RTX_ESTATE, "gradient accumulation: the fused step stores no gradient");
        RTX_CHECK(!(step->flags & RTX_STEP_GRADS_BF16), RTX_EINVAL, "gradient accumulation: RTX_STEP_GRADS_BF16 stores bf16 images for an exchange; the accumulators are float32");
    }
    // tile of the weight-gradient kernels: 64 x 128 for the fused Adam epilogue (an HBM streaming kernel: many small workgroups);
    // the data-parallel step stores bf16 gradient images instead and is bound by operand delivery: 128 x 128 tiles halve the
    // operand bytes per parameter (emulated 8-rank step 262.3 vs 268.8 us, one box)
    // (not so the fused epilogue, even at K = 4096 batch rows: configs[3] on one GPU 1343 us/step with 64 x 128, 1380 with 128 x 128)
    c.dw_cfg = (dp && !e->opt_dw_cfg_set) ? RTX_DW_128x128 : e->opt_dw_cfg;
    // the tile-major optimizer state: only where the caller has promised to leave the state alone until its next engine call
    c.tiles = kind == STEP_FUSED && (step->flags & RTX_STEP_DEFER_JOIN) && e->opt_state_tiles && c.dw_cfg == RTX_DW_64x128;

    RTX_TRY(begin_and_forward(c, batch));
    RTX_TRY(loss_and_dlogits(c));
    RTX_TRY(backward_layers(c, cb, user));
    switch (kind) {
    case STEP_DATA_PARALLEL: return finish_data_parallel(c);
    case STEP_FUSED: return finish_fused(c);
    case STEP_UNFUSED_ADAM: return finish_unfused_adam(c);
    case STEP_GRADS_ONLY: break;   // the caller runs the optimizer (rtx_engine_apply_adam*)
    }
    e->accum_mode = RTX_ACCUM_OFF;   // (rtx_engine_set_grad_accum) the mode was set for this backward pass; the window itself stays open
    return RTX_OK;
}

extern "C" {

int rtx_engine_loss_grads(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* loss_out, float* loss_accum,
                          rtx_layer_cb cb, void* user, void* stream)
{
    return run_step(e, batch, step, loss_out, loss_accum, cb, user, (hipStream_t)stream, STEP_GRADS_ONLY);
}

// ---- a loss computed outside the engine: the training forward on its own, then the backward chain from the caller's gradient ------
int rtx_engine_forward_train(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* out, float* mu, float* logvar,
                             uint64_t* ticket, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(batch && step && out && ticket, RTX_EINVAL, "forward_train: NULL argument");
    RTX_CHECK(!e->dp.on, RTX_EINVAL, "forward_train: a data-parallel plan is attached; the external-loss route has no gradient exchange");
    RTX_NO_USERS(e, "forward_train", "rtx_engine_train_step / rtx_engine_loss_grads with the engine's own loss");
    hipStream_t st = (hipStream_t)stream;
    *ticket = 0;
    RTX_TRY(ensure_shadows(e, st));     // (resolves a join the last fused step left open)
    e->next.valid = false;              // a batch announced to, or prefetched for, a fused step is not this forward's
    e->pre.valid = false;
    RtxCsrView in = {}, tg = {};
    RTX_TRY(resolve_batch(e, batch, &in, &tg, st, 0));
    const int B = batch->batch;
    // float32 logits, no log-sum-exp partials, no half-precision image: straight into the caller's tensor -- but for RTX_GVAE,
    // whose backward needs the logits themselves: they stay in Y and the caller gets their sigmoid
    if (e->gvae) {
        RTX_TRY(run_forward(e, &in, &in, B, 1, step, 0, 0, e->NL, e->Y, e->Ip, mu, logvar, st));
        RTX_HIP(hipMemcpy2DAsync(out, (size_t)e->I * sizeof(float), e->Y, (size_t)e->Ip * sizeof(float), (size_t)e->I * sizeof(float), B,
                                 hipMemcpyDeviceToDevice, st));
        TIMED("sigmoid");
        RTX_TRY(rtx_launch_sigmoid_rows(out, B, e->I, e->I, st));
    } else {
        RTX_TRY(run_forward(e, &in, &in, B, 1, step, 0, 0, e->NL, out, e->I, mu, logvar, st));
    }
    e->act_B = B;
    *ticket = e->act_ticket;
    return RTX_OK;
}

int rtx_engine_backward(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, uint64_t ticket, const float* d_out, int64_t ld,
                        const float* d_mu, const float* d_logvar, rtx_layer_cb cb, void* user, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(batch && step && d_out, RTX_EINVAL, "backward: NULL argument");
    RTX_CHECK(!e->dp.on, RTX_EINVAL, "backward: a data-parallel plan is attached; the external-loss route has no gradient exchange");
    RTX_NO_USERS(e, "backward", "rtx_engine_train_step / rtx_engine_loss_grads with the engine's own loss");
    RTX_CHECK(ld >= e->I, RTX_EINVAL, "backward: row stride %lld of d_out is below n_items = %d", (long long)ld, e->I);
    RTX_CHECK(!d_mu == !d_logvar && (e->vae || !d_mu), RTX_EINVAL, "backward: d_mu and d_logvar come together, for the VAE variants only");
    // on the host, before anything is enqueued: do the activations in the engine still belong to the caller's forward?
    RTX_CHECK(ticket != 0 && ticket == e->act_ticket && e->act_B == batch->batch, RTX_ESTATE,
              "backward: stale ticket %llu: the activations of that forward were overwritten by a later forward, prediction or training "
              "step of this engine (it now holds ticket %llu, batch %d); run rtx_engine_forward_train again",
              (unsigned long long)ticket, (unsigned long long)e->act_ticket, e->act_B);
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(resolve_join(e, st));
    rtx_step bstep = *step;     // the caller's gradient carries its own scale and every loss term: no KL, no regulariser, no flags
    bstep.beta = 0.f; bstep.lam = 0.f; bstep.flags = 0;
    StepCtx c = {};
    c.e = e; c.step = &bstep; c.st = st; c.kind = STEP_GRADS_ONLY;
    c.ext = true; c.ext_mu = d_mu; c.ext_lv = d_logvar;
    c.dw_cfg = e->opt_dw_cfg;
    c.B = batch->batch; c.Bp = rtx_pad_batch(c.B);
    c.main_li = -1;
    RtxDlogitsArgs a = {};
    a.loss.Y = e->Y; a.loss.ldy = e->Ip; a.loss.B = c.B; a.loss.I = e->I;
    a.Bp = c.Bp; a.D = e->L[e->NL - 1].D; a.ldd = e->Ip;
    {
        TIMED("import_dout");
        RTX_TRY(rtx_launch_import_dout(a, d_out, (long)ld, e->gvae, e->bf16, st));
    }
    return backward_layers(c, cb, user);
}

// ---- the same route cut in two at z (additive to ABI 8): the backward of each half on its own ----------------------------------------
// what the two calls share with rtx_engine_backward: one stream, gradients only, no loss term of the engine's
static void ext_ctx(rtx_engine* e, const rtx_step* bstep, hipStream_t st, int B, StepCtx& c)
{
    c = {};
    c.e = e; c.step = bstep; c.st = st; c.kind = STEP_GRADS_ONLY;
    c.ext = true;
    c.dw_cfg = e->opt_dw_cfg;
    c.B = B; c.Bp = rtx_pad_batch(B);
    c.main_li = -1;
}

int rtx_engine_encode_backward(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, uint64_t ticket, const float* d_out0,
                               const float* d_out1, rtx_layer_cb cb, void* user, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(batch && step, RTX_EINVAL, "encode_backward: NULL argument");
    RTX_CHECK(!e->dp.on, RTX_EINVAL, "encode_backward: a data-parallel plan is attached; the external-loss route has no gradient exchange");
    RTX_NO_USERS(e, "encode_backward", "rtx_engine_train_step / rtx_engine_loss_grads with the engine's own loss");
    RTX_CHECK(d_out0 || !d_out1, RTX_EINVAL, "encode_backward: d_out1 without d_out0");
    RTX_CHECK(d_out0 && (e->vae ? d_out1 != nullptr : d_out1 == nullptr), RTX_EINVAL,
              "encode_backward: d_out0 = d mu and d_out1 = d logvar for the VAE variants, d_out0 = d h alone for the others");
    RTX_CHECK(ticket != 0 && ticket == e->enc_ticket && e->enc_B == batch->batch, RTX_ESTATE,
              "encode_backward: stale ticket %llu: the activations of that encode were overwritten by a later encode, forward, prediction "
              "or training step of this engine (its encoder half now holds ticket %llu, batch %d); run rtx_engine_encode_train again",
              (unsigned long long)ticket, (unsigned long long)e->enc_ticket, e->enc_B);
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(resolve_join(e, st));
    rtx_step bstep = *step;
    bstep.beta = 0.f; bstep.lam = 0.f; bstep.flags = 0;
    StepCtx c;
    ext_ctx(e, &bstep, st, batch->batch, c);
    const int ne = e->cfg.n_enc;
    Layer& l = e->L[ne - 1];
    if (e->vae) {
        // no decoder behind this chain: an EMPTY slab sum (d z = 0; the chain through z is the caller's, rtx_reparam_grad) and the
        // eval form, so that D[n_enc - 1] = [d mu | d logvar] as given -- k_vae_bwd, whatever numerics: the one-launch head kernel of
        // small_layers.hip computes its d z itself
        RtxVaeBwdArgs a = {};
        a.C = e->Cacc; a.splits = 0; a.slab_stride = 0; a.ldc = l.outp;
        a.B = c.B; a.Bp = c.Bp; a.Z = e->Z; a.Np = l.outp;
        a.mu32 = e->mu32; a.lv32 = e->lv32; a.eps32 = e->eps32; a.training = 0;
        a.D = l.D; a.g_mu = d_out0; a.g_lv = d_out1;
        TIMED("vae_head_bwd");
        RTX_TRY(rtx_launch_vae_bwd(a, e->bf16, st));
    } else {
        TIMED("import_dh");
        RTX_TRY(rtx_launch_import_dh(d_out0, c.B, l.out, c.Bp, l.outp, l.tanh_act, l.O32, l.D, e->bf16, st));
    }
    return backward_layers(c, cb, user, ne - 1, 0);
}

int rtx_engine_decode_backward(rtx_engine* e, int32_t n, const rtx_step* step, uint64_t ticket, const float* d_out, int64_t ld, float* d_z,
                               rtx_layer_cb cb, void* user, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(step && d_out, RTX_EINVAL, "decode_backward: NULL argument");
    RTX_CHECK(!e->dp.on, RTX_EINVAL, "decode_backward: a data-parallel plan is attached; the external-loss route has no gradient exchange");
    RTX_NO_USERS(e, "decode_backward", "rtx_engine_train_step / rtx_engine_loss_grads with the engine's own loss");
    RTX_CHECK(ld >= e->I, RTX_EINVAL, "decode_backward: row stride %lld of d_out is below n_items = %d", (long long)ld, e->I);
    RTX_CHECK(ticket != 0 && ticket == e->dec_ticket && e->dec_B == n, RTX_ESTATE,
              "decode_backward: stale ticket %llu: the activations of that decode were overwritten by a later decode, encode, forward, "
              "prediction or training step of this engine (its decoder half now holds ticket %llu, batch %d); run rtx_engine_decode_train again",
              (unsigned long long)ticket, (unsigned long long)e->dec_ticket, e->dec_B);
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(resolve_join(e, st));
    rtx_step bstep = *step;
    bstep.beta = 0.f; bstep.lam = 0.f; bstep.flags = 0;
    StepCtx c;
    ext_ctx(e, &bstep, st, n, c);
    RtxDlogitsArgs a = {};
    a.loss.Y = e->Y; a.loss.ldy = e->Ip; a.loss.B = c.B; a.loss.I = e->I;
    a.Bp = c.Bp; a.D = e->L[e->NL - 1].D; a.ldd = e->Ip;
    {
        TIMED("import_dout");
        RTX_TRY(rtx_launch_import_dout(a, d_out, (long)ld, e->gvae, e->bf16, st));
    }
    const int ne = e->cfg.n_enc;
    RTX_TRY(backward_layers(c, cb, user, e->NL - 1, ne));
    if (!d_z) return RTX_OK;
    // instead of a head backward: the data-gradient product of layer n_enc, its slabs summed into the caller's unpadded tensor
    Layer& l = e->L[ne];
    int splits = 1;
    {
        TIMED(ne == e->NL - 1 ? "gemm_dX_out" : "gemm_dX_hidden");
        RTX_TRY(gemm_to_cacc(e, RTX_FORM_NN, l.D, l.outp, l.Wsh, l.inp, c.Bp, l.inp, l.outp, &splits, st));
    }
    TIMED("export_dz");
    return rtx_launch_export_dz(e->Cacc, splits, (long)c.Bp * l.inp, l.inp, n, e->Z, d_z, st);
}

int rtx_engine_train_step_dp(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* loss_out, float* loss_accum, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(step && step->step >= 1, RTX_EINVAL, "train_step_dp: step count must be >= 1");
    RTX_NO_USERS(e, "train_step_dp", "the single-GPU step rtx_engine_train_step");
    RTX_CHECK(!e->ae, RTX_EINVAL, "train_step_dp: the plain autoencoder variant (RTX_AE) has no data-parallel step");
    RTX_CHECK(e->dp.on, RTX_ESTATE, "train_step_dp: rtx_engine_dp_attach() has not been called");
    RTX_CHECK(e->optim.plain_adam(), RTX_EINVAL, "train_step_dp: the data-parallel step runs Adam only");
    RTX_CHECK(e->clip.mode == RTX_CLIPM_NONE, RTX_EINVAL, "train_step_dp: gradient clipping is set (mode %d); the bucketed exchange has no global gradient norm", e->clip.mode);
    RTX_CHECK(e->accum_mode == RTX_ACCUM_OFF, RTX_EINVAL, "train_step_dp: gradient accumulation is set (mode %d); the data-parallel step has none", e->accum_mode);
    return run_step(e, batch, step, loss_out, loss_accum, nullptr, nullptr, (hipStream_t)stream, STEP_DATA_PARALLEL);
}

int rtx_engine_train_step(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* loss_out, float* loss_accum,
                          void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(step && step->step >= 1, RTX_EINVAL, "train_step: step count must be >= 1");
    // (float32, or bf16 with the fused optimizer switched off: Adam as a launch of its own inside the same call)
    // (any optimizer but plain Adam too: the fused epilogue of dw_adam.hip is Adam's)
    // (a clip mode too: the global norm needs every gradient stored before any parameter moves)
    // (an accumulation window's last micro-step too: the optimizer reads the accumulators, which the fused epilogue does not)
    const StepKind kind = (e->bf16 && e->opt_fuse_adam && e->optim.plain_adam() && e->clip.mode == RTX_CLIPM_NONE && e->accum_mode == RTX_ACCUM_OFF) ? STEP_FUSED : STEP_UNFUSED_ADAM;
    if (e->clip.mode == RTX_CLIPM_NONE) e->clip.last_has_norm = false;   // (rtx_engine_wait_grad_norm: this step reports none)
    return run_step(e, batch, step, loss_out, loss_accum, nullptr, nullptr, (hipStream_t)stream, kind);
}

// Gradient accumulation (additive to ABI 8; include/rectorch_hip.h): how the weight-gradient products of the next backward passes
// write the bound gradient buffers.  Nothing is enqueued here.
int rtx_engine_set_grad_accum(rtx_engine* e, int32_t mode, float scale)
{
    RTX_CHECK(e, RTX_EINVAL, "set_grad_accum: engine is NULL");
    RTX_CHECK(mode == RTX_ACCUM_OFF || mode == RTX_ACCUM_FIRST || mode == RTX_ACCUM_ADD, RTX_EINVAL,
              "set_grad_accum: mode %d (supported: RTX_ACCUM_OFF, RTX_ACCUM_FIRST, RTX_ACCUM_ADD)", mode);
    if (mode == RTX_ACCUM_OFF) {
        e->accum_mode = RTX_ACCUM_OFF;
        return RTX_OK;
    }
    RTX_CHECK(!e->dp.on, RTX_EINVAL, "set_grad_accum: a data-parallel plan is attached; gradient accumulation is single-GPU (detach the plan)");
    RTX_CHECK(!e->users.bound(), RTX_EINVAL, "set_grad_accum: this engine has a user table bound (CDAE), whose rows are updated inside every backward pass; supported: RTX_ACCUM_OFF (one batch per update)");
    RTX_CHECK(scale - scale == 0.f, RTX_EINVAL, "set_grad_accum: scale must be finite");
    RTX_CHECK(mode != RTX_ACCUM_ADD || e->accum_layers != 0, RTX_ESTATE,
              "set_grad_accum: RTX_ACCUM_ADD without an RTX_ACCUM_FIRST pass since the last optimizer launch (or since this handle was created): the "
              "accumulators hold nothing to add to");
    if (mode == RTX_ACCUM_FIRST) e->accum_layers = 0;   // a new window: whatever the buffers hold is overwritten
    e->accum_mode = mode;
    e->accum_scale = scale;
    return RTX_OK;
}

}  // extern "C"
