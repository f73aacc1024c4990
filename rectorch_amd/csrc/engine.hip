// engine.hip -- host orchestration of the Mult-VAE / Mult-DAE engine on MI355X and the C ABI
// (include/rectorch_hip.h): life cycle, batch resolution, the forward pass and the small entry points (the training step is
// engine_step.hip).  One stream-ordered sequence of hand-written kernels per call; no host
// synchronisation on the CSR fast path.
//
// Data layout in HBM (T = bf16 or f32 by cfg.numerics; P(d) = roundup(d+1,128), Bp = roundup(B,128)):
//   layer l (in_l -> out_l), l = 0 .. NL-1 (encoder layers then decoder layers)
//     Wsh[l]   T [P(out)][P(in)]    compute copy of W_l, row-major like the master: the forward B operand (K = in
//                                   contiguous) AND, read K-major, the backward-data B operand
//     A[l]     T [Bp][P(in)]        input activation of layer l; column `in` = ones for b < B: the forward A operand and,
//                                   read K-major, the weight-gradient B operand (the ones column yields the bias gradient)
//     O32[l]   f32 [Bp][P(out)]     post-activation output (tanh layers)         (backward derivative)
//     D[l]     T [Bp][P(out)]       d loss / d pre-activation: backward-data A operand and, read K-major, the
//                                   weight-gradient A operand
//   Y  f32 [Bp][P(I)] logits;  Cacc f32 split-K slabs / small GEMM outputs.
//   No transposed copy of anything exists: the kernels that contract over the batch or over the output features read
//   the row-major matrices K-major (ds_read_b64_tr_b16 for bf16, plain 4-byte reads for f32).
//   All pads are zero (memset at creation; producers rewrite the batch padding every call), so no GEMM
//   needs a bounds check in its main loop.
#include "engine_internal.h"

// ------------------------------------------------------------------------------------------------
int dev_alloc(rtx_engine* e, void** p, size_t bytes, bool zero)
{
    if (bytes == 0) bytes = 16;
    hipError_t rc = hipMalloc(p, bytes);
    if (rc != hipSuccess) {
        rtx_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(rc));
        return RTX_ENOMEM;
    }
    if (e) e->allocs.push_back(*p);
    if (zero) {
        // hipMemset runs on the NULL stream, and neither the engine's side stream nor a caller's non-blocking stream (every
        // torch.cuda.Stream) waits for that one: without the synchronise below the zeroing can land AFTER the first kernels that
        // write the buffer.  Found by the stream-ordered multi-rank test and the batch prefetch (round 5): a data-parallel step on
        // a non-blocking stream lost its first gradient images to the late memset of the exchange buffer, a prefetched batch image
        // was zeroed after the gather had filled it.  Allocation is set-up time; the wait costs nothing per step.
        RTX_HIP(hipMemset(*p, 0, bytes));
        RTX_HIP(hipStreamSynchronize(nullptr));
    }
    return RTX_OK;
}

void dev_free(rtx_engine* e, void* p)
{
    if (!p) return;
    auto it = std::find(e->allocs.begin(), e->allocs.end(), p);
    if (it != e->allocs.end()) e->allocs.erase(it);
    (void)hipFree(p);
}

static int build_layers(const rtx_cfg& c, std::vector<Layer>& L)
{
    RTX_CHECK(c.n_enc >= 1 && c.n_dec >= 1 && c.n_enc <= RTX_MAX_LAYERS && c.n_dec <= RTX_MAX_LAYERS, RTX_EINVAL,
              "bad layer counts %d/%d", c.n_enc, c.n_dec);
    RTX_CHECK(c.enc_dims[c.n_enc] == c.dec_dims[0], RTX_EINVAL, "latent size mismatch: enc %d vs dec %d",
              c.enc_dims[c.n_enc], c.dec_dims[0]);
    RTX_CHECK(c.enc_dims[0] == c.dec_dims[c.n_dec], RTX_EINVAL, "n_items mismatch: enc %d vs dec %d", c.enc_dims[0],
              c.dec_dims[c.n_dec]);
    RTX_CHECK(c.cond_dim >= 0, RTX_EINVAL, "negative cond_dim %d", c.cond_dim);
    L.clear();
    for (int i = 0; i < c.n_enc; ++i) {
        Layer l;
        l.in = c.enc_dims[i] + (i == 0 ? c.cond_dim : 0);   // CMultiVAE_net: temp_dims[0] += cond_dim (nets.py:459-460)
        l.out = c.enc_dims[i + 1];
        l.tanh_act = true;
        if (i == c.n_enc - 1 && (c.variant == RTX_VAE || c.variant == RTX_GVAE)) {  // mu | logvar, linear (reference nets.py:262-265, 398-404)
            l.out = 2 * c.enc_dims[i + 1];
            l.tanh_act = false;
        }
        L.push_back(l);
    }
    for (int i = 0; i < c.n_dec; ++i) {
        Layer l;
        l.in = c.dec_dims[i];
        l.out = c.dec_dims[i + 1];
        l.tanh_act = (i != c.n_dec - 1);  // reference nets.py:413-417 / 227-233
        L.push_back(l);
    }
    for (auto& l : L) {
        RTX_CHECK(l.in > 0 && l.out > 0, RTX_EINVAL, "non-positive layer size");
        l.inp = rtx_pad(l.in);
        l.outp = rtx_pad(l.out);
    }
    return RTX_OK;
}

// ---- GEMM helpers -------------------------------------------------------------------------------------
GemmPlan plan_gemm(const rtx_engine* e, int Mp, int Np, int Kp, int form)
{
    GemmPlan pl = {};
    pl.k_slices = (int)((size_t)Kp * e->esz / 128);     // 64 bf16 or 32 f32 per slice
    pl.regstage = !e->bf16 || (form == RTX_FORM_NT && e->opt_nt_regstage && (long)Np * Kp >= (1L << 21));
    if (!pl.regstage) {
        // the 512-row tile covers every batch row of a B <= 512 step: each weight byte is read by one workgroup.  Small
        // problems (hidden layers) are latency-bound: 128x128 tiles give 4x the workgroups.
        const bool big = (Mp % 512 == 0) && ((long)Np * Kp >= (1L << 21));
        pl.cfg = big ? RTX_DMA_512x128 : RTX_DMA_128x128;
        // data-gradient chain beside the weight-gradient kernels (two streams): a 64-KB-LDS configuration, so that its
        // workgroups fit on a CU next to one of theirs (the 512-row tile takes the whole LDS of a CU)
        if (form == RTX_FORM_NN && e->opt_fuse_adam && e->opt_two_stream) pl.cfg = RTX_DMA_128x128_S2;
        // a batch of thousands of rows (configs[3] on one GPU: B = 4096): the product is no longer a skinny one hiding beside a
        // streaming kernel but 90 GFLOP of its own -- the 512-row tile needs a third of the operand bytes per flop of the 128 x 128 one
        if (big && e->opt_big_batch_tiles && Mp >= 1024) pl.cfg = RTX_DMA_512x128;
        rtx_gemm_dma_tile_dims(pl.cfg, &pl.bm, &pl.bn);
    } else {
        pl.cfg = RTX_TILE_128x128;
        pl.bm = pl.bn = 128;
    }
    pl.m_tiles = Mp / pl.bm;
    pl.n_tiles = Np / pl.bn;
    const int tiles = pl.m_tiles * pl.n_tiles;
    // split K so that one wave of workgroups fills the chip: 1 per CU for the LDS-DMA kernels (their stages fill the
    // LDS), 2 per CU for the register-staged f32 kernel; at least two K slices per workgroup
    const int resident = (pl.regstage || pl.cfg == RTX_DMA_128x128_S2) ? 512 : 256;
    int s = 1;
    if (tiles * 2 <= resident) {
        s = resident / tiles;
        if (pl.regstage && s >= 8) s &= ~7;   // register-staged kernel: every XCD owns whole splits
        // data-gradient products: the slabs are summed by a post kernel beside the streaming weight kernel, where every slab
        // costs: 16 slabs instead of 25 at the ml-20m shape is 5 us per step (286 vs 291; 12: 288, 8: 292)
        if (form == RTX_FORM_NN && s > 16 && e->bf16) s = 16;   // (float32: one stream, nothing beside the post kernel -- fill the chip)
        if (pl.k_slices >= 64 && e->cfg.splitk > 0) s = e->cfg.splitk;
        if (pl.k_slices >= 64 && form == RTX_FORM_NT && e->opt_splitk_fwd > 0) s = e->opt_splitk_fwd;
        if (pl.k_slices >= 64 && form == RTX_FORM_NN && e->opt_splitk_bwd > 0) s = e->opt_splitk_bwd;
        const int max_s = pl.k_slices / 2 > 0 ? pl.k_slices / 2 : 1;
        if (s > max_s) s = max_s;
        if (s < 1) s = 1;
    }
    // every split must own at least one slice: per = ceil(k / s) slices each -> ceil(k / per) non-empty splits
    const int per = (pl.k_slices + s - 1) / s;
    pl.splits = (pl.k_slices + per - 1) / per;
    return pl;
}

size_t plan_cacc_elems(rtx_engine* e, int Np, int Kp)
{
    size_t mx = 0;
    const int keep = e->opt_nt_regstage, keep2 = e->opt_two_stream;
    for (int rs = 0; rs < 4; ++rs) {     // whichever kernels the knobs select later
        e->opt_nt_regstage = rs & 1;
        e->opt_two_stream = rs >> 1;
        for (int form : {RTX_FORM_NT, RTX_FORM_NN})
            for (int Mp = 128; Mp <= e->Bp_alloc; Mp += 128) {
                const GemmPlan pl = plan_gemm(e, Mp, Np, Kp, form);
                mx = std::max(mx, (size_t)pl.splits * Mp * Np);
            }
    }
    e->opt_nt_regstage = keep;
    e->opt_two_stream = keep2;
    return mx;
}

int gemm_to_cacc(rtx_engine* e, int form, const void* A, long lda, const void* B, long ldb, int Mp, int Np, int Kp, int* splits_out,
                 hipStream_t st, uint32_t* hop_word, uint32_t hop_seq, const uint32_t* wait_word, uint32_t wait_seq)
{
    const GemmPlan pl = plan_gemm(e, Mp, Np, Kp, form);
    RtxGemm g = {};
    g.form = form;
    g.A = A; g.B = B; g.lda = lda; g.ldb = ldb;
    g.k_slices = pl.k_slices; g.tile_shape = pl.cfg; g.m_tiles = pl.m_tiles; g.n_tiles = pl.n_tiles; g.splits = pl.splits;
    g.C = e->Cacc; g.ldc = Np; g.slab_stride = (long)Mp * Np;
    RTX_CHECK((size_t)g.splits * Mp * Np <= e->cacc_elems, RTX_ESTATE, "internal: Cacc too small (%d x %d x %d)", g.splits, Mp, Np);
    *splits_out = g.splits;
    g.xcd_block = 1;   // (the launcher keeps the strip order for split-K and for grids under 8 x 4 tiles)
    RTX_CHECK(!hop_word || !pl.regstage, RTX_ESTATE, "internal: a folded stream hop needs the LDS-DMA product");
    g.hop_word = hop_word; g.hop_seq = hop_seq;
    RTX_CHECK(!wait_word || e->bf16, RTX_ESTATE, "internal: a folded join needs a bf16 product");
    g.wait_word = wait_word; g.wait_seq = wait_seq;
    if (!pl.regstage) return rtx_gemm_dma_launch(g, RTX_EPI_STORE, st);
    if (form == RTX_FORM_NT) return rtx_gemm_launch(g, e->bf16 ? RTX_DT_BF16 : RTX_DT_F32, RTX_EPI_STORE, st);
    return rtx_gemm_f32_km_launch(g, RTX_EPI_STORE, st);
}

// ---- batch resolution --------------------------------------------------------------------------------
static int ensure_tmp(rtx_engine* e, TempCsr& t, int64_t nnz)
{
    if (!t.indptr) {
        RTX_TRY(dev_alloc(e, (void**)&t.indptr, sizeof(int64_t) * (e->cfg.max_batch + 1)));
        RTX_TRY(dev_alloc(e, (void**)&t.counts, sizeof(int32_t) * (e->cfg.max_batch + 1)));
    }
    if (nnz > t.cap) {
        int64_t cap = nnz + nnz / 2 + 1024;
        // old buffers stay in e->allocs and are freed with the engine (growth is rare)
        RTX_TRY(dev_alloc(e, (void**)&t.indices, sizeof(int32_t) * cap, false));
        RTX_TRY(dev_alloc(e, (void**)&t.values, sizeof(float) * cap, false));
        t.cap = cap;
    }
    return RTX_OK;
}

static int dense_to_view(rtx_engine* e, TempCsr& t, const float* x, int B, int width, RtxCsrView* v, hipStream_t st)
{
    RTX_TRY(ensure_tmp(e, t, 0));
    RTX_TRY(rtx_launch_dense_count(x, B, width, t.counts, st));
    RTX_TRY(rtx_launch_scan_counts(t.counts, B, t.indptr, st));
    int64_t nnz = 0;
    RTX_HIP(hipMemcpyAsync(&nnz, t.indptr + B, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    RTX_HIP(hipStreamSynchronize(st));  // dense drop-in path only; the CSR path never synchronises
    RTX_TRY(ensure_tmp(e, t, nnz));
    RTX_TRY(rtx_launch_dense_fill(x, B, width, t.indptr, t.indices, t.values, st));
    v->indptr = t.indptr; v->indices = t.indices; v->values = t.values; v->row_ids = nullptr;
    v->max_row_len = 0; v->avg_row_len = 0;   // a densified batch: row lengths unknown -> the dense first layer (sparse_in_ok)
    return RTX_OK;
}

int resolve_batch(rtx_engine* e, const rtx_batch* b, RtxCsrView* in, RtxCsrView* tg, hipStream_t st, int need_target)
{
    RTX_CHECK(b, RTX_EINVAL, "batch is NULL");
    RTX_CHECK(b->batch >= 1 && b->batch <= e->cfg.max_batch, RTX_EINVAL, "batch %d outside [1, max_batch=%d]", b->batch,
              e->cfg.max_batch);
    if (b->csr) {
        RTX_CHECK(b->csr->n_cols == e->Iin, RTX_EINVAL, "CSR has %d columns, network expects %d (items + conditions)", b->csr->n_cols,
                  e->Iin);
        RTX_CHECK(b->row_ids || b->batch <= b->csr->n_rows, RTX_EINVAL, "batch larger than the matrix");
        in->indptr = b->csr->indptr; in->indices = b->csr->indices; in->values = b->csr->values; in->row_ids = b->row_ids;
        in->max_row_len = b->csr->max_row_len;
        in->avg_row_len = (int32_t)std::min<int64_t>((b->csr->nnz + std::max<int64_t>(b->csr->n_rows, 1) - 1) / std::max<int64_t>(b->csr->n_rows, 1), INT32_MAX);
    } else {
        RTX_CHECK(b->x_dense, RTX_EINVAL, "batch has neither csr nor x_dense");
        RTX_TRY(dense_to_view(e, e->tmp_in, b->x_dense, b->batch, e->Iin, in, st));
    }
    if (b->target_csr) {
        RTX_CHECK(b->target_csr->n_cols == e->I, RTX_EINVAL, "target CSR has %d columns, expected %d", b->target_csr->n_cols, e->I);
        tg->indptr = b->target_csr->indptr; tg->indices = b->target_csr->indices; tg->values = b->target_csr->values;
        tg->row_ids = b->row_ids;
        tg->max_row_len = b->target_csr->max_row_len;
    } else if (b->target_dense) {
        RTX_TRY(dense_to_view(e, e->tmp_tg, b->target_dense, b->batch, e->I, tg, st));
    } else {
        // a conditioned input has cond_dim extra columns: it cannot be its own target.  Scoring calls (need_target = 0)
        // never read the target beyond its row sums, which k_gather restricts to the item columns.
        RTX_CHECK(e->Iin == e->I || !need_target, RTX_EINVAL, "a conditioned network (cond_dim = %d) needs an explicit target", e->Iin - e->I);
        *tg = *in;
    }
    return RTX_OK;
}

// ---- forward ---------------------------------------------------------------------------------------
// Runs layers [l0, l1).  If l0 == 0 the gather kernel builds A[0] from `in`.  The last network layer
// writes logits to `logits` (ld = ldlog); with want_lse it also leaves the log-sum-exp partials (training).
// The first layer as a sparse product (spmm_in.hip): bf16 numerics, a batch that names rows of a resident CSR matrix (its
// longest row bounds the chunk stream), a first layer followed by an ordinary activation, weight rows that fit the LDS.
// the training step's logits as half precision in the delta buffer (opt_logits16): needs the epilogue's log-sum-exp partials and
// the register-staged product that writes them
bool logits16_on(const rtx_engine* e) { return e->bf16 && e->opt_logits16 && e->opt_lse_fuse && e->opt_nt_regstage; }

bool user_node_args(const rtx_engine* e, bool update, RtxPostUsers& u)
{
    const UserNode& n = e->users;
    if (!n.bound() || !n.cur.ids) return false;
    u = {};
    u.uid = n.cur.ids; u.n_users = n.n_users;
    u.V = n.V; u.m = update ? n.m : nullptr; u.v = update ? n.v : nullptr;
    u.ld = e->L[0].out;   // (the table is bound contiguous: [n_users][latent])
    u.vec = rtx_user_rows_vec(n.V, update ? n.m : n.V, update ? n.v : n.V, u.ld, e->L[0].out);
    if (update) rtx_user_adam_scalars(n.cur.lr, n.cur.beta1, n.cur.beta2, n.cur.eps, n.cur.step, u);
    return true;
}

bool sparse_in_ok(const rtx_engine* e, const RtxCsrView* in, int Bp, int64_t* chunks)
{
    // (VAE_net, RTX_GVAE: its raw input rows stay on the dense first layer -- k_in_chunks normalises the entries it streams)
    if (!e->bf16 || !e->opt_sparse_in || e->NL < 2 || (e->vae && e->cfg.n_enc == 1) || e->gvae) return false;
    if (e->users.bound()) return false;   // CDAE: the user term lives in k_post's epilogue, the one forward site of the first layer
    if (in->max_row_len <= 0 || e->Iin > 65536 || rtx_spmm_in_lds_bytes(e->Iin) > 160 * 1024) return false;
    *chunks = (int64_t)Bp * std::max(1, (in->max_row_len + 63) / 64) + 64;   // + the read-ahead of the last wave
    // every workgroup of k_spmm_in walks the whole chunk stream (~6 ns per chunk), the dense product re-reads the weights and
    // the dense batch image (~25 us + 8 us per 1000 rows): beyond ~4000 expected chunks (ml-20m at B = 500: ~1500; Netflix-
    // shaped rows at B = 4096: ~18 000) the dense product wins
    const int64_t expected = (int64_t)Bp * ((in->avg_row_len + 63) / 64 + 1);
    return *chunks * 256 <= ((int64_t)512 << 20) && expected <= 4096;
}
static int ensure_in_chunks(rtx_engine* e, int64_t chunks, hipStream_t st)
{
    if (chunks <= e->in_cap_chunks) return RTX_OK;
    if (e->in_ent) {   // a matrix with longer rows than the last one: rare, so simply wait and regrow
        RTX_HIP(hipStreamSynchronize(st));
        dev_free(e, e->in_ent);
        dev_free(e, e->in_desc);
        e->in_ent = nullptr; e->in_desc = nullptr;
    }
    RTX_TRY(dev_alloc(e, (void**)&e->in_ent, (size_t)chunks * 256));
    RTX_TRY(dev_alloc(e, (void**)&e->in_desc, (size_t)(chunks + 128) * sizeof(int32_t)));
    if (!e->in_wsplit) RTX_TRY(dev_alloc(e, (void**)&e->in_wsplit, (RTX_SPMM_WAVES + 1) * sizeof(int32_t)));
    e->in_cap_chunks = chunks;
    return RTX_OK;
}

// Third form (round 5, option "hop_kernels"): the dependency as two ONE-WAVE KERNELS -- k_hop_set on the producing stream stores a
// sequence number (agent-scope release) behind the kernels it follows, k_hop_wait on the consuming stream spins on it (acquire,
// s_sleep between polls, bounded) in front of the kernels that need the data.  A kernel boundary on each side: the producers'
// end-of-kernel release has completed before k_hop_set runs (in-order queue), the consumers' start-of-kernel acquire comes after
// k_hop_wait has seen the number.  No stream memory operation, no event: those are packets that make the command processor release
// to SYSTEM scope (the signal word is host-visible memory) and cost the stream 6-9 us each (profiles/r4_step_timeline.txt: the
// gaps behind k_dlogits and between two steps).
__global__ void k_hop_set(uint32_t* word, uint32_t v)
{
    if (threadIdx.x == 0) __hip_atomic_store(word, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void k_hop_wait(const uint32_t* word, uint32_t v, uint32_t* stuck)
{
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
    while ((int32_t)(__hip_atomic_load(word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - v) < 0) {
        __builtin_amdgcn_s_sleep(8);
        if (__builtin_amdgcn_s_memrealtime() - t0 > 2000000000ull) {   // 20 s: the producer is gone; do not hang the device
            if (stuck) *stuck = v;
            __builtin_trap();
        }
    }
}

int ensure_hopk(rtx_engine* e)
{
    if (!e->hopk_mem) {
        RTX_HIP(hipMalloc((void**)&e->hopk_mem, 64));
        RTX_HIP(hipMemset(e->hopk_mem, 0, 64));
        RTX_HIP(hipStreamSynchronize(nullptr));
    }
    return RTX_OK;
}

// the two kernels on word `slot` of hopk_mem (0 / 1: the step's fork and join as kernels, 2: the folded fork, 3: the deferred join);
// a wait that gives up leaves its number in word 8 + slot
int launch_hop_set(rtx_engine* e, hipStream_t st, int slot, uint32_t v)
{
    hipLaunchKernelGGL(k_hop_set, dim3(1), dim3(64), 0, st, e->hopk_mem + slot, v);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}
int launch_hop_wait(rtx_engine* e, hipStream_t st, int slot, uint32_t v)
{
    hipLaunchKernelGGL(k_hop_wait, dim3(1), dim3(64), 0, st, e->hopk_mem + slot, v, e->hopk_mem + 8 + slot);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// the join a step flagged RTX_STEP_DEFER_JOIN left open: `st` continues only after everything that step put on the side stream
int resolve_join(rtx_engine* e, hipStream_t st, bool keep_tiles)
{
    if (e->join_pending) {
        e->join_pending = false;
        e->join_fold = false;
        RTX_TRY(launch_hop_wait(e, st, 3, e->join_seq));
    }
    // behind the join: the weight kernels of the last deferred step have written their last moments into the images
    return keep_tiles ? RTX_OK : state_to_caller(e, st);
}

bool state_any_tiled(const rtx_engine* e)
{
    for (char t : e->state_tiled)
        if (t) return true;
    return false;
}

// the tile-major exp_avg / exp_avg_sq of every tiled layer back into the bound tensors, on `st`: bit for bit what the row-major kernel
// would have left there.  The images are always those of the 64 x 128 tile (StepCtx::tiles).
int state_to_caller(rtx_engine* e, hipStream_t st)
{
    for (int li = 0; li < (int)e->state_tiled.size(); ++li) {
        if (!e->state_tiled[li]) continue;
        const Layer& l = e->L[li];
        TIMED("state_writeback");
        RTX_TRY(rtx_dw_state_relayout(e->m[2 * li], e->v[2 * li], e->m_img[li], e->v_img[li], l.out, l.in, l.outp / rtx_dw_tile_rows(RTX_DW_64x128),
                                      (l.inp + rtx_dw_tile_cols(RTX_DW_64x128) - 1) / rtx_dw_tile_cols(RTX_DW_64x128), RTX_DW_64x128, 0, st));
        e->state_tiled[li] = 0;
        ++e->st_state_writebacks;
    }
    return RTX_OK;
}

// The batch image A[0] (+ target row sums, + the scatter lists) of one batch, on stream `st`, into the CURRENT image set.
int gather_batch(rtx_engine* e, const RtxCsrView* in, const RtxCsrView* tg, int B, int training, const rtx_step* step, hipStream_t st)
{
    const int Bp = rtx_pad_batch(B);
    Layer& l = e->L[0];
    RtxGatherArgs a = {};
    a.in = *in; a.target = *tg;
    a.B = B; a.Bp = Bp; a.I = e->I; a.Iin = e->Iin; a.ldx = l.inp; a.raw = e->gvae;
    a.X = l.A; a.tsum = e->tsum;
    a.training = training; a.dropout_p = e->cfg.dropout_p;
    a.mask = step->dropout_mask; a.seed = step->seed; a.offset = step->offset;
    // The image is all zeros but for ~75 entries per user: with a resident matrix (its longest row is known) only those are
    // touched -- cleared, rewritten, listed (k_gather_scatter).  First use, a longer matrix, or another writer of A[0] in
    // between (the sparse first layer's k_in_chunks, a densified batch through k_gather): one full reset of image and lists.
    if (e->opt_gather_scatter && in->max_row_len > 0 && ((int64_t)in->max_row_len + 66) * e->Bp_alloc * 4 <= ((int64_t)256 << 20)) {
        const int need = (in->max_row_len + 2 + 63) / 64 * 64;
        if (need > e->img_cap) {
            if (e->img_written) {
                RTX_HIP(hipStreamSynchronize(st));
                dev_free(e, e->img_written);
                dev_free(e, e->img_nwritten);
                e->img_written = nullptr; e->img_nwritten = nullptr;
            }
            RTX_TRY(dev_alloc(e, (void**)&e->img_written, (size_t)e->Bp_alloc * need * sizeof(int32_t), false));
            RTX_TRY(dev_alloc(e, (void**)&e->img_nwritten, (size_t)e->Bp_alloc * sizeof(int32_t)));
            e->img_cap = need;
            e->img_exact = false;
        }
        if (!e->img_exact) {
            RTX_HIP(hipMemsetAsync(l.A, 0, (size_t)e->Bp_alloc * l.inp * e->esz, st));
            RTX_HIP(hipMemsetAsync(e->img_nwritten, 0, (size_t)e->Bp_alloc * sizeof(int32_t), st));
            e->img_exact = true;
        }
        a.written = e->img_written; a.n_written = e->img_nwritten; a.written_cap = e->img_cap;
    } else {
        e->img_exact = false;
    }
    TIMED("gather");
    RTX_TRY(rtx_launch_gather(a, e->bf16, st));
    return RTX_OK;
}

static uint64_t next_act_ticket()
{
    static std::atomic<uint64_t> seq{0};
    return ++seq;
}

int run_forward(rtx_engine* e, const RtxCsrView* in, const RtxCsrView* tg, int B, int training, const rtx_step* step,
                int want_lse, int l0, int l1, float* logits, long ldlog, float* mu_out, float* lv_out, hipStream_t st)
{
    const int Bp = rtx_pad_batch(B);
    static const rtx_step zero_step = {};
    if (!step) step = &zero_step;
    e->act_ticket = next_act_ticket();   // whatever activations a training forward left are being overwritten (rtx_engine_backward)
    e->act_B = 0;
    // ... and the tickets of the halves whose layers this run writes (engine_internal.h: enc_ticket / dec_ticket)
    if (l0 < e->cfg.n_enc) { e->enc_ticket = e->act_ticket; e->enc_B = 0; }
    if (l0 < e->cfg.n_enc || l1 > e->cfg.n_enc) { e->dec_ticket = e->act_ticket; e->dec_B = 0; }
    if (l0 == 0) {   // CDAE: the ids announced for this call become the current batch's, and are consumed
        e->users.cur = e->users.next;
        e->users.next = UserNode::Ids();
    }
    // VAE_net (RTX_GVAE) samples z in every mode: its _reparameterize has no eval branch (reference nets.py:317-320)
    const int sample = training || e->gvae;
    int64_t in_chunks = 0;
    const bool sparse_in = l0 == 0 && l1 > 1 && sparse_in_ok(e, in, Bp, &in_chunks);
    if (l0 == 0) e->last_sparse_in = sparse_in;
    const bool gathered = e->gather_done;
    e->gather_done = false;
    if (e->join_fold && !(l0 == 0 && l1 > 1 && !sparse_in && gathered && e->bf16)) {
        // the deferred join cannot ride on the first-layer product after all (it is not this call's first kernel): a kernel of its own
        e->join_fold = false;
        RTX_TRY(launch_hop_wait(e, st, 3, e->join_seq));
    }
    if (l0 == 0 && !sparse_in && !gathered) RTX_TRY(gather_batch(e, in, tg, B, training, step, st));
    for (int li = l0; li < l1; ++li) {
        Layer& l = e->L[li];
        if (li == e->NL - 1) {
            // logits = A x Wsh^T + b, one launch; K = hidden (short), output [Bp][n_items] f32
            RtxGemm g = {};
            g.form = RTX_FORM_NT;
            g.A = l.A; g.B = l.Wsh; g.lda = l.inp; g.ldb = l.inp;
            g.k_slices = (int)((size_t)l.inp * e->esz / 128);
            g.splits = 1; g.C = logits; g.ldc = ldlog; g.bias = e->params[2 * li + 1];
            g.M_real = B; g.N_real = l.out;
            TIMED("gemm_logits");
            if (e->bf16 && !e->opt_nt_regstage) {
                g.tile_shape = (Bp % 512 == 0) ? RTX_DMA_512x128 : RTX_DMA_128x128;
                int bm, bn;
                rtx_gemm_dma_tile_dims(g.tile_shape, &bm, &bn);
                g.m_tiles = Bp / bm; g.n_tiles = l.outp / bn;
                if (want_lse && e->opt_lse_fuse) { g.lse_part = e->lse_part; g.lse_ld = e->lse_strips; }   // (see lse_fused)
                g.xcd_block = 1;
                RTX_TRY(rtx_gemm_dma_launch(g, RTX_EPI_BIAS_ROWS, st));
            } else {
                g.tile_shape = RTX_TILE_128x128;
                g.m_tiles = Bp / 128; g.n_tiles = l.outp / 128;
                if (want_lse && e->opt_lse_fuse) { g.lse_part = e->lse_part; g.lse_ld = e->lse_strips; }
                if (want_lse && logits16_on(e)) { g.C16 = l.D; g.ldc16 = l.outp; }
                RTX_TRY(rtx_gemm_launch(g, e->bf16 ? RTX_DT_BF16 : RTX_DT_F32, RTX_EPI_BIAS_ROWS, st));
            }
            break;
        }
        if (li == 0 && sparse_in) {
            // the batch's stored entries as a chunk stream; in a training step the same launch also leaves what the gather
            // kernel would (the dense image the weight-gradient kernel reads, the target row sums)
            RTX_TRY(ensure_in_chunks(e, in_chunks, st));
            RtxInChunksArgs c = {};
            c.in = *in; c.B = B; c.I = e->I; c.Iin = e->Iin;
            c.training = training; c.dropout_p = e->cfg.dropout_p;
            c.mask = step->dropout_mask; c.seed = step->seed; c.offset = step->offset;
            c.ent = e->in_ent; c.desc = e->in_desc; c.wsplit = e->in_wsplit; c.cap_chunks = e->in_cap_chunks;
            if (training) { c.target = *tg; c.tsum = e->tsum; c.X = (bf16_t*)l.A; c.ldx = l.inp; c.Bp = Bp; e->img_exact = false; }
            {
                TIMED("in_chunks");
                RTX_TRY(rtx_launch_in_chunks(c, st));
            }
            RtxSpmmInArgs a = {};
            a.ent = e->in_ent; a.desc = e->in_desc; a.wsplit = e->in_wsplit;
            a.B = B; a.Bp = Bp;
            a.W = (const bf16_t*)l.Wsh; a.ldw = l.inp; a.Kin = e->Iin;
            a.bias = e->params[2 * li + 1]; a.N_real = l.out; a.Np = l.outp; a.tanh_act = l.tanh_act;
            a.O32 = l.O32; a.R = (bf16_t*)e->L[li + 1].A; a.ones_col = 1;
            TIMED("spmm_in");
            RTX_TRY(rtx_launch_spmm_in(a, st));
            continue;
        }
        if (li > 0 && e->bf16 && e->opt_small_fwd && rtx_small_fwd_ok(l.inp)) {
            // a hidden layer (or the VAE head): product + bias + activation + the next operand in one launch (small_layers.hip)
            Layer& nx1 = e->L[li + 1];
            RtxSmallFwdArgs a = {};
            a.A = (const bf16_t*)l.A; a.W = (const bf16_t*)l.Wsh; a.lda = l.inp; a.ldw = l.inp; a.w_rows = l.outp;
            a.B = B; a.Bp = Bp; a.bias = e->params[2 * li + 1]; a.R = (bf16_t*)nx1.A;
            if (e->vae && li == e->cfg.n_enc - 1) {
                a.Z = e->Z; a.Np = e->Zp; a.N_real = e->Z; a.training = sample;
                a.mu32 = e->mu32; a.lv32 = e->lv32; a.eps32 = e->eps32; a.mu_out = mu_out; a.lv_out = lv_out;
                a.eps_in = step->eps_noise; a.seed = step->seed; a.offset = step->offset;
            } else {
                a.N_real = l.out; a.Np = l.outp; a.tanh_act = l.tanh_act; a.O32 = l.O32;
            }
            TIMED(a.Z ? "fwd_head" : "fwd_hidden");
            RTX_TRY(rtx_launch_small_fwd(a, st));
            continue;
        }
        int splits = 1;
        {
            TIMED(li == 0 ? "gemm_fwd_in" : "gemm_fwd_hidden");
            const bool fold = e->join_fold;      // (set only for a step whose FIRST kernel is this product)
            e->join_fold = false;
            RTX_TRY(gemm_to_cacc(e, RTX_FORM_NT, l.A, l.inp, l.Wsh, l.inp, Bp, l.outp, l.inp, &splits, st, nullptr, 0, fold ? e->hopk_mem + 3 : nullptr, e->join_seq));
        }
        Layer& nx = e->L[li + 1];
        if (e->vae && li == e->cfg.n_enc - 1) {
            RtxVaeFwdArgs a = {};
            a.C = e->Cacc; a.splits = splits; a.slab_stride = (long)Bp * l.outp; a.ldc = l.outp;
            a.B = B; a.Bp = Bp; a.Z = e->Z; a.Zp = e->Zp;
            a.bias = e->params[2 * li + 1];
            a.mu32 = e->mu32; a.lv32 = e->lv32; a.eps32 = e->eps32;
            a.mu_out = mu_out; a.lv_out = lv_out;
            a.Zr = nx.A;
            a.training = sample; a.eps_in = step->eps_noise; a.seed = step->seed; a.offset = step->offset;
            TIMED("vae_head_fwd");
            RTX_TRY(rtx_launch_vae_fwd(a, e->bf16, st));
        } else {
            RtxPostArgs a = {};
            a.C = e->Cacc; a.splits = splits; a.slab_stride = (long)Bp * l.outp; a.ldc = l.outp;
            a.B = B; a.Bp = Bp; a.N_real = l.out; a.Np = l.outp;
            a.tanh_act = l.tanh_act; a.bias = e->params[2 * li + 1];
            a.O32 = l.O32; a.R = nx.A; a.ones_col = 1;
            TIMED("post_fwd");
            RtxPostUsers u;
            if (li == 0 && user_node_args(e, false, u)) RTX_TRY(rtx_launch_post_users(a, u, RTX_POST_FWD, e->bf16, st));
            else RTX_TRY(rtx_launch_post(a, RTX_POST_FWD, e->bf16, st));
        }
    }
    return RTX_OK;
}

int check_ready(rtx_engine* e, bool train)
{
    RTX_CHECK(e, RTX_EINVAL, "engine is NULL");
    RTX_CHECK(e->bound, RTX_ESTATE, "rtx_engine_bind() has not been called");
    RTX_CHECK(!train || e->can_train, RTX_ESTATE, "engine was bound without gradient / Adam buffers");
    return RTX_OK;
}

int ensure_shadows(rtx_engine* e, hipStream_t st, bool keep_tiles)
{
    RTX_TRY(resolve_join(e, st, keep_tiles));   // (a join the last training step left open: before anything else of the engine runs on `st`)
    if (e->shadows_valid) return RTX_OK;
    return rtx_engine_sync_shadows(e, st);
}

// tensors of layers [l0, l1) into a (W and b per layer)
void fill_adam_tensors(rtx_engine* e, RtxAdamArgs& a, int l0, int l1)
{
    if (l1 < 0) l1 = e->NL;
    a.n = 0;
    for (int li = l0; li < l1; ++li) {
        Layer& l = e->L[li];
        RtxAdamTensor& w = a.t[a.n++];
        w.p = e->params[2 * li];
        w.g = e->can_train ? e->grads[2 * li] : nullptr;
        w.m = e->can_train ? e->m[2 * li] : nullptr;
        w.v = e->can_train ? e->v[2 * li] : nullptr;
        w.sh = l.Wsh; w.shT = l.WshT; w.rows = l.out; w.cols = l.in; w.ld_sh = l.inp; w.ld_shT = l.WshT ? l.outp : 0;
        w.sumsq = nullptr;
        RtxAdamTensor& b = a.t[a.n++];
        b.p = e->params[2 * li + 1];
        b.g = e->can_train ? e->grads[2 * li + 1] : nullptr;
        b.m = e->can_train ? e->m[2 * li + 1] : nullptr;
        b.v = e->can_train ? e->v[2 * li + 1] : nullptr;
        b.sh = nullptr; b.shT = nullptr; b.rows = 1; b.cols = l.out; b.ld_sh = 0; b.ld_shT = 0;
        b.sumsq = nullptr;
    }
}

// torch.optim.Adam's scalars for update `step` (computed in double like torch does on the host).  The tensors of `a`
// are tensors [t0, t0 + a.n) of the network unless `ids` names them one by one (DAE: per-tensor norms).
void fill_adam_scalars(rtx_engine* e, const rtx_step* step, RtxAdamArgs& a, int t0 /* first tensor index */, const int* ids)
{
    rtx_optim_scalars(e->optim, step->lr, step->beta1, step->beta2, step->eps, step->weight_decay, step->step, a);   // (the kind was checked when it was set)
    if (!e->vae && !e->ae && step->lam != 0.f) {   // (RTX_AE: the MSE loss has no regulariser)
        a.lam = step->lam;
        for (int k = 0; k < a.n; ++k) a.t[k].sumsq = e->sumsq + (ids ? ids[k] : t0 + k);
    }
}

int launch_sumsq(rtx_engine* e, hipStream_t st)
{
    std::vector<const float*> ps(2 * e->NL);
    std::vector<long> sz(2 * e->NL);
    for (int li = 0; li < e->NL; ++li) {
        ps[2 * li] = e->params[2 * li];
        sz[2 * li] = (long)e->L[li].out * e->L[li].in;
        ps[2 * li + 1] = e->params[2 * li + 1];
        sz[2 * li + 1] = e->L[li].out;
    }
    return rtx_launch_sumsq(ps.data(), sz.data(), 2 * e->NL, e->sumsq, st);
}

__global__ void k_unpad_copy(const float* src, int ld, int B, int n, float* dst)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long)B * n) dst[i] = src[(i / n) * ld + (i % n)];
}

// ones != 0: column n holds 1 for b < B, as the VAE head and k_post leave the operand of a layer whose bias gradient will be asked for
template <typename T>
__global__ void k_pad_convert(const float* src, int B, int n, T* dst, int ld, int Bp, int ones)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long)Bp * ld) {
        const int b = (int)(i / ld), j = (int)(i % ld);
        dst[i] = Elem<T>::from((b < B && j < n) ? src[(long)b * n + j] : (ones && b < B && j == n) ? 1.f : 0.f);
    }
}

// z float32 [batch][latent] (unpadded) -> the operand A[n_enc] of the first decoder layer
static int pad_convert_z(rtx_engine* e, const float* z, int batch, int ones, hipStream_t st)
{
    Layer& l = e->L[e->cfg.n_enc];
    const int Bp = rtx_pad_batch(batch);
    const long n = (long)Bp * l.inp;
    if (e->bf16)
        hipLaunchKernelGGL(k_pad_convert<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, z, batch, l.in, (bf16_t*)l.A, l.inp, Bp, ones);
    else
        hipLaunchKernelGGL(k_pad_convert<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, z, batch, l.in, (float*)l.A, l.inp, Bp, ones);
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// =================================================================================================
extern "C" {

const char* rtx_last_error(void) { return rtx_last_error_str(); }
// 2: rtx_cfg.cond_dim, rtx_ease_*; 3: rtx_engine_set_option, step fuses Adam by default; 4: rtx_comm_*, rtx_engine_apply_adam_rows /
// shadow_region; 5: rtx_engine_dp_attach / train_step_dp (the engine schedules the data-parallel step); 6: rtx_svae_set_option;
// 7: rtx_dp_cfg.comm_side / ops_side / shard_min_elems (bucket A's own communicator), rtx_engine_loss_mailbox / rtx_engine_wait_loss;
// 8: rtx_engine_evaluate_topk (additive since: *_ex with hit / mrr, rtx_opr_*, rtx_admm_*, rtx_topk_items / rtx_engine_recommend,
//    rtx_list_metrics, rtx_opr_rank_f64, rtx_engine_forward_train / backward, rtx_engine_encode_train / encode_backward /
//    decode_train / decode_backward, rtx_reparam / rtx_reparam_grad)
int32_t rtx_abi_version(void) { return 8; }

// ---- CSR -------------------------------------------------------------------------------------------
int rtx_csr_upload(const int64_t* indptr_host, const int32_t* indices_host, const float* values_host, int64_t n_rows,
                   int32_t n_cols, rtx_csr** out)
{
    RTX_CHECK(indptr_host && out && n_rows >= 0 && n_cols > 0, RTX_EINVAL, "csr_upload: bad arguments");
    const int64_t nnz = indptr_host[n_rows];
    RTX_CHECK(nnz == 0 || indices_host, RTX_EINVAL, "csr_upload: indices is NULL");
    rtx_csr* m = new rtx_csr();
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    int64_t longest = 0;
    for (int64_t r = 0; r < n_rows; ++r) longest = std::max<int64_t>(longest, indptr_host[r + 1] - indptr_host[r]);
    m->max_row_len = (int32_t)std::min<int64_t>(longest, INT32_MAX);
    int rc = dev_alloc(nullptr, (void**)&m->indptr, sizeof(int64_t) * (n_rows + 1), false);
    if (!rc) rc = dev_alloc(nullptr, (void**)&m->indices, sizeof(int32_t) * (nnz > 0 ? nnz : 1), false);
    if (!rc && values_host) rc = dev_alloc(nullptr, (void**)&m->values, sizeof(float) * (nnz > 0 ? nnz : 1), false);
    if (rc) { rtx_csr_destroy(m); return rc; }
    hipError_t h = hipMemcpy(m->indptr, indptr_host, sizeof(int64_t) * (n_rows + 1), hipMemcpyHostToDevice);
    if (h == hipSuccess && nnz) h = hipMemcpy(m->indices, indices_host, sizeof(int32_t) * nnz, hipMemcpyHostToDevice);
    if (h == hipSuccess && nnz && values_host) h = hipMemcpy(m->values, values_host, sizeof(float) * nnz, hipMemcpyHostToDevice);
    if (h != hipSuccess) {
        rtx_set_error("csr_upload: hipMemcpy failed: %s", hipGetErrorString(h));
        rtx_csr_destroy(m);
        return RTX_EHIP;
    }
    *out = m;
    return RTX_OK;
}

int rtx_csr_destroy(rtx_csr* m)
{
    if (!m) return RTX_OK;
    if (m->indptr) (void)hipFree(m->indptr);
    if (m->indices) (void)hipFree(m->indices);
    if (m->values) (void)hipFree(m->values);
    delete m;
    return RTX_OK;
}

int rtx_csr_shape(const rtx_csr* m, int64_t* n_rows, int32_t* n_cols, int64_t* nnz)
{
    RTX_CHECK(m, RTX_EINVAL, "csr is NULL");
    if (n_rows) *n_rows = m->n_rows;
    if (n_cols) *n_cols = m->n_cols;
    if (nnz) *nnz = m->nnz;
    return RTX_OK;
}

int rtx_csr_gather_dense(const rtx_csr* m, const int32_t* row_ids, int32_t batch, float* out, void* stream)
{
    RTX_CHECK(m && out, RTX_EINVAL, "csr_gather_dense: bad arguments");
    RTX_CHECK(batch >= 0 && (row_ids || batch <= m->n_rows), RTX_EINVAL, "csr_gather_dense: bad batch %d", batch);
    RtxCsrView v = {m->indptr, m->indices, m->values, row_ids};
    return rtx_launch_csr_to_dense(v, batch, m->n_cols, out, (hipStream_t)stream);
}

// ---- engine lifecycle ------------------------------------------------------------------------------
int rtx_engine_create(const rtx_cfg* cfg, rtx_engine** out)
{
    RTX_CHECK(cfg && out, RTX_EINVAL, "engine_create: NULL argument");
    RTX_CHECK(cfg->variant == RTX_VAE || cfg->variant == RTX_DAE || cfg->variant == RTX_GVAE || cfg->variant == RTX_AE, RTX_EINVAL,
              "bad variant %d", cfg->variant);
    RTX_CHECK(cfg->variant != RTX_AE || cfg->cond_dim == 0, RTX_EINVAL, "RTX_AE (AETrainer's MSE loss) has no condition columns");
    RTX_CHECK(cfg->variant != RTX_GVAE || (cfg->dropout_p == 0.f && cfg->cond_dim == 0), RTX_EINVAL,
              "RTX_GVAE (VAE_net) has no dropout and no condition columns");
    RTX_CHECK(cfg->numerics == RTX_FP32 || cfg->numerics == RTX_BF16, RTX_EINVAL, "bad numerics %d", cfg->numerics);
    RTX_CHECK(cfg->max_batch >= 1, RTX_EINVAL, "max_batch must be >= 1");
    RTX_CHECK(cfg->dropout_p >= 0.f && cfg->dropout_p <= 1.f, RTX_EINVAL, "dropout_p outside [0,1]");
    int ndev = 0;
    hipError_t h = hipGetDeviceCount(&ndev);
    RTX_CHECK(h == hipSuccess && ndev > 0, RTX_EHIP, "no HIP device available (%s): librectorch_hip has no CPU path",
              hipGetErrorString(h));
    rtx_engine* e = new rtx_engine();
    e->cfg = *cfg;
    {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) e->n_cus = cus;
        (void)hipGetLastError();
    }
    int rc = build_layers(*cfg, e->L);
    if (rc) { delete e; return rc; }
    e->NL = (int)e->L.size();
    e->I = cfg->enc_dims[0];
    e->Iin = e->I + cfg->cond_dim;
    e->Z = cfg->enc_dims[cfg->n_enc];
    e->Ip = rtx_pad(e->I);
    e->Zp = rtx_pad(e->Z);
    e->bf16 = cfg->numerics == RTX_BF16;
    e->vae = cfg->variant == RTX_VAE || cfg->variant == RTX_GVAE;
    e->gvae = cfg->variant == RTX_GVAE;
    e->ae = cfg->variant == RTX_AE;
    e->esz = e->bf16 ? 2 : 4;
    e->Bp_alloc = rtx_pad_batch(cfg->max_batch);
    const size_t Bp = e->Bp_alloc, es = e->esz;
    size_t cacc = 0;
#define ALLOC(ptr, bytes)                                  \
    do {                                                   \
        rc = dev_alloc(e, (void**)&(ptr), (bytes));        \
        if (rc) { rtx_engine_destroy(e); return rc; }      \
    } while (0)
    for (int li = 0; li < e->NL; ++li) {
        Layer& l = e->L[li];
        ALLOC(l.Wsh, (size_t)l.outp * l.inp * es);
        if (e->bf16) ALLOC(l.Wsh_alt, (size_t)l.outp * l.inp * es);
        if (e->bf16 && li > 0 && li < e->NL - 1 && rtx_small_fwd_ok(l.outp)) ALLOC(l.WshT, (size_t)l.inp * l.outp * es);
        ALLOC(l.A, Bp * l.inp * es);
        if (li < e->NL - 1) ALLOC(l.O32, Bp * l.outp * sizeof(float));
        ALLOC(l.D, Bp * l.outp * es);
        // scratch for the forward output and the backward-data output of this layer (with split-K slabs), at any batch
        if (li < e->NL - 1) cacc = std::max(cacc, plan_cacc_elems(e, l.outp, l.inp));
        if (li > 0) cacc = std::max(cacc, plan_cacc_elems(e, l.inp, l.outp));
    }
    e->cacc_elems = cacc;
    ALLOC(e->Cacc, cacc * sizeof(float));
    ALLOC(e->Y, Bp * e->Ip * sizeof(float));
    ALLOC(e->mu32, Bp * e->Z * sizeof(float));
    ALLOC(e->lv32, Bp * e->Z * sizeof(float));
    ALLOC(e->eps32, Bp * e->Z * sizeof(float));
    e->lse_strips = e->Ip / 64;
    ALLOC(e->lse_part, Bp * e->lse_strips * sizeof(float2));
    ALLOC(e->tsum, Bp * sizeof(float));
    ALLOC(e->lse, Bp * sizeof(float));
    ALLOC(e->row_loss, Bp * rtx_dlogits_chunks(e->Ip) * sizeof(float));
    ALLOC(e->sumsq, sizeof(float) * 2 * RTX_MAX_LAYERS * 2);
    ALLOC(e->scratch_loss, sizeof(float) * 4);
#undef ALLOC
    *out = e;
    return RTX_OK;
}

int rtx_engine_destroy(rtx_engine* e)
{
    if (!e) return RTX_OK;
    (void)hipDeviceSynchronize();
    if (state_any_tiled(e)) {   // the bound tensors outlive the handle: their moments go back into them first
        e->join_pending = false;   // (the device has drained)
        (void)state_to_caller(e, nullptr);
        (void)hipDeviceSynchronize();
    }
    for (void* p : e->allocs) (void)hipFree(p);
    for (auto& kv : e->sites)
        for (auto& pr : kv.second.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t ev : e->event_pool) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->ev_d)
        if (ev) (void)hipEventDestroy(ev);
    if (e->ev_done) (void)hipEventDestroy(e->ev_done);
    if (e->hop_mem) (void)hipFree(e->hop_mem);
    if (e->hopk_mem) (void)hipFree(e->hopk_mem);
    if (e->loss_mailbox) (void)hipHostFree(e->loss_mailbox);
    rtx_clip_release(e->clip);
    for (auto& kv : e->side_cache)
        if (kv.second.first) (void)hipStreamDestroy(kv.second.first);
    delete e;
    return RTX_OK;
}

int32_t rtx_engine_n_tensors(const rtx_engine* e) { return e ? 2 * e->NL : 0; }

int rtx_engine_tensor_shape(const rtx_engine* e, int32_t t, int32_t* rows, int32_t* cols)
{
    RTX_CHECK(e && t >= 0 && t < 2 * e->NL, RTX_EINVAL, "tensor index %d out of range", t);
    const Layer& l = e->L[t / 2];
    if (rows) *rows = l.out;
    if (cols) *cols = (t & 1) ? 1 : l.in;
    return RTX_OK;
}

int rtx_engine_bind(rtx_engine* e, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq)
{
    RTX_CHECK(e && params, RTX_EINVAL, "engine_bind: NULL argument");
    if (state_any_tiled(e)) {
        // a rebind under an open deferred step: the tensors bound so far get their moments back before they are let go (no stream comes
        // with this call: the device drains, the copy runs on the NULL stream, the host waits for it)
        RTX_HIP(hipDeviceSynchronize());
        RTX_TRY(resolve_join(e, nullptr));
        RTX_HIP(hipStreamSynchronize(nullptr));
    }
    const int n = 2 * e->NL;
    for (int t = 0; t < n; ++t) {
        RTX_CHECK(params[t], RTX_EINVAL, "engine_bind: params[%d] is NULL", t);
        RTX_CHECK(((uintptr_t)params[t] & 15) == 0, RTX_EINVAL, "engine_bind: params[%d] is not 16-byte aligned", t);
    }
    e->params.assign(params, params + n);
    e->can_train = grads && exp_avg && exp_avg_sq;
    if (e->can_train) {
        for (int t = 0; t < n; ++t) {
            RTX_CHECK(grads[t] && exp_avg[t] && exp_avg_sq[t], RTX_EINVAL, "engine_bind: NULL grad/moment pointer for tensor %d", t);
            RTX_CHECK((((uintptr_t)grads[t] | (uintptr_t)exp_avg[t] | (uintptr_t)exp_avg_sq[t]) & 15) == 0, RTX_EINVAL,
                      "engine_bind: tensor %d buffers are not 16-byte aligned", t);
        }
        e->grads.assign(grads, grads + n);
        e->m.assign(exp_avg, exp_avg + n);
        e->v.assign(exp_avg_sq, exp_avg_sq + n);
    }
    e->bound = true;
    e->shadows_valid = false;
    return RTX_OK;
}

int rtx_engine_bind_grads16(rtx_engine* e, uint16_t* const* grads_bf16)
{
    RTX_CHECK(e, RTX_EINVAL, "engine is NULL");
    if (!grads_bf16) { e->grads16.clear(); return RTX_OK; }
    const int n = 2 * e->NL;
    for (int t = 0; t < n; ++t) {
        RTX_CHECK(grads_bf16[t], RTX_EINVAL, "bind_grads16: tensor %d is NULL", t);
        RTX_CHECK(((uintptr_t)grads_bf16[t] & 7) == 0, RTX_EINVAL, "bind_grads16: tensor %d is not 8-byte aligned", t);
    }
    e->grads16.assign(grads_bf16, grads_bf16 + n);
    return RTX_OK;
}

// ---- CDAE's user node (additive to ABI 8; include/rectorch_hip.h "CDAE") -----------------------------------------------------------
int rtx_engine_bind_users(rtx_engine* e, float* V, float* exp_avg, float* exp_avg_sq, int32_t n_users)
{
    RTX_CHECK(e, RTX_EINVAL, "bind_users: engine is NULL");
    if (!V) {
        e->users = UserNode();
        return RTX_OK;
    }
    RTX_CHECK(!e->vae && !e->gvae && e->cfg.n_enc == 1 && e->cfg.n_dec == 1 && e->cfg.cond_dim == 0, RTX_EINVAL,
              "bind_users: a user table needs an RTX_DAE or RTX_AE engine with n_enc == 1, n_dec == 1 and cond_dim == 0 (this one: variant %d, "
              "n_enc %d, n_dec %d, cond_dim %d); deeper networks, the VAE variants and conditioned inputs have no user node",
              (int)e->cfg.variant, e->cfg.n_enc, e->cfg.n_dec, e->cfg.cond_dim);
    RTX_CHECK(n_users >= 1, RTX_EINVAL, "bind_users: n_users = %d", n_users);
    RTX_CHECK(!exp_avg == !exp_avg_sq, RTX_EINVAL, "bind_users: exp_avg and exp_avg_sq come together (both NULL: inference only)");
    RTX_CHECK(!e->dp.on, RTX_EINVAL, "bind_users: a data-parallel plan is attached; supported with a user table: the single-GPU step (rtx_engine_train_step, rtx_engine_loss_grads)");
    RTX_CHECK(e->clip.mode == RTX_CLIPM_NONE, RTX_EINVAL, "bind_users: gradient clipping is set (mode %d); supported with a user table: no clipping (the table's gradient is never stored)", e->clip.mode);
    RTX_CHECK(e->accum_mode == RTX_ACCUM_OFF, RTX_EINVAL, "bind_users: gradient accumulation is set (mode %d); supported with a user table: one batch per update", e->accum_mode);
    e->users = UserNode();
    e->users.V = V; e->users.m = exp_avg; e->users.v = exp_avg_sq; e->users.n_users = n_users;
    return RTX_OK;
}

int rtx_engine_set_users(rtx_engine* e, const int32_t* user_ids, float lr, float beta1, float beta2, float eps, int32_t step)
{
    RTX_CHECK(e, RTX_EINVAL, "set_users: engine is NULL");
    RTX_CHECK(e->users.bound() || !user_ids, RTX_ESTATE, "set_users: rtx_engine_bind_users() has not been called");
    e->users.next = UserNode::Ids();
    if (!user_ids) return RTX_OK;
    e->users.next.ids = user_ids;
    e->users.next.lr = lr; e->users.next.beta1 = beta1; e->users.next.beta2 = beta2; e->users.next.eps = eps; e->users.next.step = step;
    return RTX_OK;
}

int rtx_engine_join(rtx_engine* e, void* stream)
{
    RTX_CHECK(e, RTX_EINVAL, "engine is NULL");
    return resolve_join(e, (hipStream_t)stream);
}

int rtx_engine_sync_shadows(rtx_engine* e, void* stream)
{
    RTX_TRY(check_ready(e, false));
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(resolve_join(e, st));
    RtxAdamArgs a = {};
    fill_adam_tensors(e, a);
    a.update = 0;
    a.grad_scale = 1.f;
    TIMED("sync_shadows");
    RTX_TRY(rtx_launch_adam(a, e->bf16, st));
    e->shadows_valid = true;
    return RTX_OK;
}

// ---- forward family --------------------------------------------------------------------------------
int rtx_engine_forward(rtx_engine* e, const rtx_batch* batch, int32_t training, const rtx_step* step, int32_t remove_train,
                       float* logits, float* mu, float* logvar, void* stream)
{
    RTX_TRY(check_ready(e, false));
    RTX_CHECK(logits, RTX_EINVAL, "forward: logits is NULL");
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(ensure_shadows(e, st));
    RtxCsrView in = {}, tg = {};
    RTX_TRY(resolve_batch(e, batch, &in, &tg, st, 0));
    RTX_TRY(run_forward(e, &in, &in, batch->batch, training, step, 0, 0, e->NL, logits, e->I, mu, logvar, st));
    if (e->gvae) {   // VAE_net.decode ends in torch.sigmoid (reference nets.py:315); the -inf mask comes after it (models.py:622-624)
        TIMED("sigmoid");
        RTX_TRY(rtx_launch_sigmoid_rows(logits, batch->batch, e->I, e->I, st));
    }
    if (remove_train) {
        TIMED("neg_inf");
        RTX_TRY(rtx_launch_neg_inf(in, batch->batch, logits, e->I, e->I, st));
    }
    return RTX_OK;
}

int rtx_engine_encode(rtx_engine* e, const rtx_batch* batch, int32_t training, const rtx_step* step, float* out0, float* out1,
                      void* stream)
{
    RTX_TRY(check_ready(e, false));
    RTX_CHECK(out0, RTX_EINVAL, "encode: out0 is NULL");
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(ensure_shadows(e, st));
    RtxCsrView in = {}, tg = {};
    RTX_TRY(resolve_batch(e, batch, &in, &tg, st, 0));
    const int ne = e->cfg.n_enc;
    RTX_TRY(run_forward(e, &in, &in, batch->batch, training, step, 0, 0, ne, nullptr, 0, out0, out1, st));
    if (!e->vae) {
        const Layer& l = e->L[ne - 1];
        const long n = (long)batch->batch * l.out;
        hipLaunchKernelGGL(k_unpad_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, l.O32, l.outp, batch->batch, l.out, out0);
        RTX_HIP(hipGetLastError());
    }
    return RTX_OK;
}

int rtx_engine_decode(rtx_engine* e, const float* z, int32_t batch, float* logits, void* stream)
{
    RTX_TRY(check_ready(e, false));
    RTX_CHECK(z && logits, RTX_EINVAL, "decode: NULL argument");
    RTX_CHECK(batch >= 1 && batch <= e->cfg.max_batch, RTX_EINVAL, "decode: batch %d outside [1,%d]", batch, e->cfg.max_batch);
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(ensure_shadows(e, st));
    const int ne = e->cfg.n_enc;
    RTX_TRY(pad_convert_z(e, z, batch, 0, st));
    RTX_TRY(run_forward(e, nullptr, nullptr, batch, 0, nullptr, 0, ne, e->NL, logits, e->I, nullptr, nullptr, st));
    if (e->gvae) RTX_TRY(rtx_launch_sigmoid_rows(logits, batch, e->I, e->I, st));   // VAE_net.decode (reference nets.py:315)
    return RTX_OK;
}

// ---- the two halves of the training forward (their backward calls: engine_step.hip) --------------------------------------------
int rtx_engine_encode_train(rtx_engine* e, const rtx_batch* batch, const rtx_step* step, float* out0, float* out1, uint64_t* ticket,
                            void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(batch && step && out0 && ticket, RTX_EINVAL, "encode_train: NULL argument");
    RTX_CHECK(!e->dp.on, RTX_EINVAL, "encode_train: a data-parallel plan is attached; the external-loss route has no gradient exchange");
    RTX_NO_USERS(e, "encode_train", "rtx_engine_train_step / rtx_engine_loss_grads with the engine's own loss");
    hipStream_t st = (hipStream_t)stream;
    *ticket = 0;
    RTX_TRY(ensure_shadows(e, st));     // (resolves a join the last fused step left open)
    e->next.valid = false;              // a batch announced to, or prefetched for, a fused step is not this forward's
    e->pre.valid = false;
    RtxCsrView in = {}, tg = {};
    RTX_TRY(resolve_batch(e, batch, &in, &tg, st, 0));
    const int ne = e->cfg.n_enc, B = batch->batch;
    // (the VAE head also samples a z of its own into A[n_enc]: nobody reads it, rtx_engine_decode_train writes that operand again)
    RTX_TRY(run_forward(e, &in, &in, B, 1, step, 0, 0, ne, nullptr, 0, out0, out1, st));
    if (!e->vae) {
        const Layer& l = e->L[ne - 1];
        const long n = (long)B * l.out;
        hipLaunchKernelGGL(k_unpad_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, l.O32, l.outp, B, l.out, out0);
        RTX_HIP(hipGetLastError());
    }
    e->enc_B = B;
    *ticket = e->enc_ticket;
    return RTX_OK;
}

int rtx_engine_decode_train(rtx_engine* e, const float* z, int32_t n, float* out, uint64_t* ticket, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(z && out && ticket, RTX_EINVAL, "decode_train: NULL argument");
    RTX_CHECK(n >= 1 && n <= e->cfg.max_batch, RTX_EINVAL, "decode_train: batch %d outside [1,%d]", n, e->cfg.max_batch);
    RTX_CHECK(!e->dp.on, RTX_EINVAL, "decode_train: a data-parallel plan is attached; the external-loss route has no gradient exchange");
    RTX_NO_USERS(e, "decode_train", "rtx_engine_train_step / rtx_engine_loss_grads with the engine's own loss");
    hipStream_t st = (hipStream_t)stream;
    *ticket = 0;
    RTX_TRY(ensure_shadows(e, st));
    e->next.valid = false;
    e->pre.valid = false;
    const int ne = e->cfg.n_enc;
    RTX_TRY(pad_convert_z(e, z, n, 1, st));      // with the ones column: the weight gradient of layer n_enc emits its bias gradient from it
    // as rtx_engine_forward_train: float32 logits straight into the caller's tensor -- but for RTX_GVAE, whose backward needs the
    // logits themselves: they stay in Y and the caller gets their sigmoid
    if (e->gvae) {
        RTX_TRY(run_forward(e, nullptr, nullptr, n, 1, nullptr, 0, ne, e->NL, e->Y, e->Ip, nullptr, nullptr, st));
        RTX_HIP(hipMemcpy2DAsync(out, (size_t)e->I * sizeof(float), e->Y, (size_t)e->Ip * sizeof(float), (size_t)e->I * sizeof(float), n,
                                 hipMemcpyDeviceToDevice, st));
        TIMED("sigmoid");
        RTX_TRY(rtx_launch_sigmoid_rows(out, n, e->I, e->I, st));
    } else {
        RTX_TRY(run_forward(e, nullptr, nullptr, n, 1, nullptr, 0, ne, e->NL, out, e->I, nullptr, nullptr, st));
    }
    e->dec_B = n;
    *ticket = e->dec_ticket;
    return RTX_OK;
}

// ---- optimizer entry points (the step itself: engine_step.hip) ------------------------------------------------------------------
static_assert(RTX_OPT_ADAM == RTX_OPTIM_ADAM && RTX_OPT_SGD == RTX_OPTIM_SGD && RTX_OPT_ADAGRAD == RTX_OPTIM_ADAGRAD && RTX_OPT_RMSPROP == RTX_OPTIM_RMSPROP &&
              RTX_OPTF_DECOUPLED == RTX_OPTIM_DECOUPLED && RTX_OPTF_NESTEROV == RTX_OPTIM_NESTEROV && RTX_OPTF_FIRST == RTX_OPTIM_FIRST,
              "rtx_kernels.h and include/rectorch_hip.h name the same optimizer kinds and flags");
static RtxOptim optim_of(const rtx_optim* o)
{
    RtxOptim r;
    r.kind = o->kind; r.flags = o->flags; r.momentum = o->momentum; r.dampening = o->dampening; r.alpha = o->alpha; r.lr_decay = o->lr_decay;
    return r;
}

int rtx_engine_set_optimizer(rtx_engine* e, const rtx_optim* optim)
{
    RTX_CHECK(e && optim, RTX_EINVAL, "set_optimizer: NULL argument");
    const RtxOptim o = optim_of(optim);
    RTX_TRY(rtx_optim_validate(o));
    RTX_CHECK(o.plain_adam() || !e->dp.on, RTX_EINVAL, "set_optimizer: a data-parallel plan is attached; its optimizer passes run Adam only");
    e->optim = o;
    return RTX_OK;
}

int rtx_engine_apply_adam(rtx_engine* e, const rtx_step* step, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(step && step->step >= 1, RTX_EINVAL, "apply_adam: step count must be >= 1");
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(resolve_join(e, st));
    RtxAdamArgs a = {};
    fill_adam_tensors(e, a);
    fill_adam_scalars(e, step, a, 0);
    if (e->clip.mode != RTX_CLIPM_NONE) {
        TIMED("grad_norm");
        RTX_TRY(rtx_clip_prepare(a, e->clip, (uint32_t)step->step, st));
    } else {
        e->clip.last_has_norm = false;
    }
    TIMED("adam");
    RTX_TRY(rtx_launch_adam(a, e->bf16, st));
    e->shadows_valid = true;
    e->accum_mode = RTX_ACCUM_OFF;   // (rtx_engine_set_grad_accum) an accumulation window ends with its optimizer launch
    e->accum_layers = 0;
    return RTX_OK;
}

// Gradient clipping (additive to ABI 8): torch.nn.utils.clip_grad_norm_ (norm_type 2 or inf) / clip_grad_value_ in front of every
// optimizer launch of rtx_engine_train_step and rtx_engine_apply_adam, on the device: the coefficient never visits the host.  What is
// clipped is the gradient of the loss -- the stored gradient plus Mult-DAE's regulariser term -- before the weight decay.  May be
// called between any two steps.  The data-parallel entry points refuse a handle with a mode set: the norm of the reduced gradient
// needs every bucket before the first optimizer pass.
static_assert(RTX_CLIPM_NONE == RTX_CLIP_NONE && RTX_CLIPM_NORM2 == RTX_CLIP_NORM2 && RTX_CLIPM_NORMINF == RTX_CLIP_NORMINF && RTX_CLIPM_VALUE == RTX_CLIP_VALUE,
              "rtx_kernels.h and include/rectorch_hip.h name the same clip modes");
int rtx_engine_set_grad_clip(rtx_engine* e, int32_t mode, double bound)
{
    RTX_CHECK(e, RTX_EINVAL, "set_grad_clip: engine is NULL");
    RTX_TRY(rtx_clip_validate(mode, bound, "set_grad_clip"));
    RTX_CHECK(mode == RTX_CLIPM_NONE || !e->dp.on, RTX_EINVAL, "set_grad_clip: a data-parallel plan is attached; its bucketed exchange has no global gradient norm");
    RTX_CHECK(mode == RTX_CLIPM_NONE || !e->users.bound(), RTX_EINVAL, "set_grad_clip: this engine has a user table bound (CDAE), whose gradient is never stored and so cannot enter a norm; supported: RTX_CLIP_NONE");
    e->clip.mode = mode;
    e->clip.bound = mode == RTX_CLIPM_NONE ? 0.0 : bound;
    return RTX_OK;
}

// host[0] = the total norm, host[1] = the coefficient of the LAST optimizer step enqueued (`step`: its step count, checked), from
// coherent host memory as rtx_engine_wait_loss reads the loss: the stream is not drained.  RTX_ESTATE when that step computed no norm.
int rtx_engine_wait_grad_norm(rtx_engine* e, int32_t step, float* host, double timeout_s)
{
    RTX_CHECK(e, RTX_EINVAL, "wait_grad_norm: engine is NULL");
    uint32_t tag = 0;
    RTX_TRY(rtx_clip_wait_norm(e->clip, "wait_grad_norm", host, timeout_s, &tag));
    RTX_CHECK(tag == (uint32_t)step, RTX_ESTATE, "wait_grad_norm: the mailbox holds the LAST step enqueued (step %u), not step %d", (unsigned)tag, step);
    return RTX_OK;
}

int rtx_engine_apply_adam_layers(rtx_engine* e, const rtx_step* step, int32_t layer_lo, int32_t layer_hi,
                                 const uint16_t* const* grads_bf16, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(step && step->step >= 1, RTX_EINVAL, "apply_adam: step count must be >= 1");
    RTX_CHECK(layer_lo >= 0 && layer_lo < layer_hi && layer_hi <= e->NL, RTX_EINVAL, "apply_adam_layers: bad layer range [%d, %d) of %d",
              layer_lo, layer_hi, e->NL);
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(resolve_join(e, st));
    RTX_CHECK(e->optim.plain_adam(), RTX_EINVAL, "apply_adam_layers: the data-parallel optimizer passes run Adam only; the engine's optimizer is kind %d flags %d",
              e->optim.kind, e->optim.flags);
    RTX_CHECK(e->clip.mode == RTX_CLIPM_NONE, RTX_EINVAL, "apply_adam_layers: gradient clipping is set (mode %d); an optimizer pass per bucket has no global gradient norm", e->clip.mode);
    RtxAdamArgs a = {};
    fill_adam_tensors(e, a, layer_lo, layer_hi);
    if (grads_bf16)
        for (int t = 0; t < a.n; ++t) a.t[t].g16 = grads_bf16[2 * layer_lo + t];
    fill_adam_scalars(e, step, a, 2 * layer_lo);
    TIMED("adam");
    RTX_TRY(rtx_launch_adam(a, e->bf16, st));
    // the compute copies are whole again once every layer has been visited; callers cover [0, NL) each step
    e->shadows_valid = true;
    return RTX_OK;
}

// Sharded optimizer (data parallel, ZeRO-1 style): this rank owns rows [row_lo, row_hi) of layer `layer`'s weight matrix.
// After the reduce-scatter of the gradient it updates only those rows (p, exp_avg, exp_avg_sq and the rows of the compute
// copy) -- the optimizer's 28 B/param of HBM traffic shrink by the number of ranks -- and, with with_bias, the (replicated,
// all-reduced) bias in full.  The caller then all-gathers the compute copy (rtx_engine_shadow_region).
int rtx_engine_apply_adam_rows(rtx_engine* e, const rtx_step* step, int32_t layer, int32_t row_lo, int32_t row_hi, int32_t with_bias,
                               const uint16_t* w_grad_bf16, const uint16_t* b_grad_bf16, void* stream)
{
    RTX_TRY(check_ready(e, true));
    RTX_CHECK(step && step->step >= 1, RTX_EINVAL, "apply_adam_rows: step count must be >= 1");
    RTX_CHECK(layer >= 0 && layer < e->NL, RTX_EINVAL, "apply_adam_rows: layer %d out of range", layer);
    RTX_CHECK(e->optim.plain_adam(), RTX_EINVAL, "apply_adam_rows: the data-parallel optimizer passes run Adam only; the engine's optimizer is kind %d flags %d",
              e->optim.kind, e->optim.flags);
    RTX_CHECK(e->clip.mode == RTX_CLIPM_NONE, RTX_EINVAL, "apply_adam_rows: gradient clipping is set (mode %d); an optimizer pass per shard has no global gradient norm", e->clip.mode);
    const Layer& l = e->L[layer];
    RTX_CHECK(row_lo >= 0 && row_lo <= row_hi && row_hi <= l.outp, RTX_EINVAL, "apply_adam_rows: bad row range [%d, %d) of %d", row_lo, row_hi, l.outp);
    // a hidden layer keeps a transposed compute copy (WshT, a column-block layout the caller's row-block all-gather cannot
    // complete): its rows cannot be updated piecewise
    RTX_CHECK(!l.WshT || (row_lo == 0 && row_hi >= l.out), RTX_EINVAL,
              "apply_adam_rows: layer %d keeps a transposed compute copy and cannot be sharded by rows (shard the first / last layer only)", layer);
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(resolve_join(e, st));
    RtxAdamArgs full = {}, a = {};
    fill_adam_tensors(e, full, layer, layer + 1);
    int ids[2];
    const int hi = std::min(row_hi, l.out);     // padding rows hold no parameters
    if (row_lo < hi) {
        RtxAdamTensor w = full.t[0];
        const size_t off = (size_t)row_lo * l.in;
        w.p += off; w.g += off; w.m += off; w.v += off;
        if (w_grad_bf16) w.g16 = w_grad_bf16 + off;
        w.sh = (char*)l.Wsh + (size_t)row_lo * l.inp * e->esz;
        w.rows = hi - row_lo;
        ids[a.n] = 2 * layer;
        a.t[a.n++] = w;
    }
    if (with_bias) {
        RtxAdamTensor b = full.t[1];
        if (b_grad_bf16) b.g16 = b_grad_bf16;
        ids[a.n] = 2 * layer + 1;
        a.t[a.n++] = b;
    }
    if (a.n == 0) return RTX_OK;
    fill_adam_scalars(e, step, a, 0, ids);
    TIMED("adam");
    RTX_TRY(rtx_launch_adam(a, e->bf16, st));
    e->shadows_valid = true;    // (whole again once the caller has all-gathered the compute copies of this step)
    return RTX_OK;
}

// the compute copy of layer `layer`'s weight matrix: [padded_rows][ld] elements of `elem_bytes` bytes, padded_rows a multiple
// of 128 -- the buffer a sharded-optimizer caller all-gathers in place (equal row blocks per rank)
int rtx_engine_shadow_region(rtx_engine* e, int32_t layer, void** base, int32_t* padded_rows, int32_t* ld, int32_t* elem_bytes)
{
    RTX_CHECK(e && layer >= 0 && layer < e->NL, RTX_EINVAL, "shadow_region: bad arguments");
    const Layer& l = e->L[layer];
    if (base) *base = l.Wsh;
    if (padded_rows) *padded_rows = l.outp;
    if (ld) *ld = l.inp;
    if (elem_bytes) *elem_bytes = (int32_t)e->esz;
    return RTX_OK;
}

int rtx_cast_f32_bf16(const float* src, uint16_t* dst, int64_t n, void* stream)
{
    RTX_CHECK(src && dst && n >= 0, RTX_EINVAL, "cast_f32_bf16: bad arguments");
    return rtx_launch_cast_f32_bf16(src, dst, (long)n, (hipStream_t)stream);
}

// The reference's train_batch ends in `return loss.item()` (models.py:835): the host needs THIS step's loss.  Draining the stream
// for it also waits for the weight-gradient + Adam kernels behind the loss (a third of the step) and leaves the GPU idle while
// the host enqueues the next step.  With the mailbox on, the loss reduction of every training step also stores {loss, step count}
// into coherent host memory (system-scope release), and rtx_engine_wait_loss spins on the step count: the float it returns is
// this step's loss, the stream keeps running.
int rtx_engine_loss_mailbox(rtx_engine* e, int32_t enable)
{
    RTX_CHECK(e, RTX_EINVAL, "engine is NULL");
    if (enable && !e->loss_mailbox) {
        void* p = nullptr;
        RTX_HIP(hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped));
        memset(p, 0, 64);
        e->loss_mailbox = (uint32_t*)p;
        e->loss_ticket = 0;
    } else if (!enable && e->loss_mailbox) {
        RTX_HIP(hipDeviceSynchronize());
        (void)hipHostFree(e->loss_mailbox);
        e->loss_mailbox = nullptr;
    }
    return RTX_OK;
}

int rtx_engine_wait_loss(rtx_engine* e, int32_t step, float* loss_host, double timeout_s)
{
    RTX_CHECK(e && loss_host, RTX_EINVAL, "wait_loss: NULL argument");
    RTX_CHECK(e->loss_mailbox, RTX_ESTATE, "wait_loss: rtx_engine_loss_mailbox(e, 1) has not been called");
    volatile uint32_t* mb = e->loss_mailbox;
    const auto t0 = std::chrono::steady_clock::now();
    // the word waited for is the engine's own ticket of the LAST reduction it enqueued (monotonic), not the caller's step count: a
    // count that restarts (a reloaded checkpoint, a new optimizer on the same engine) or repeats (step 0 twice) cannot match an old entry
    RTX_CHECK(e->loss_ticket != 0, RTX_ESTATE, "wait_loss: no training step has reported to the mailbox yet");
    const uint32_t want = e->loss_ticket;
    for (unsigned spin = 0;; ++spin) {
        if (__atomic_load_n(&mb[1], __ATOMIC_ACQUIRE) == want) break;
        if ((spin & 0x3ff) == 0x3ff) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            RTX_CHECK(el < (timeout_s > 0 ? timeout_s : 60.0), RTX_EHIP, "wait_loss: step %d did not report its loss within %.1f s (mailbox holds ticket %u of %u, step %u)",
                      step, el, (unsigned)mb[1], (unsigned)want, (unsigned)mb[2]);
            if (el > 0.002) sched_yield();      // a long wait is a long kernel: stop burning the core
        }
    }
    RTX_CHECK(__atomic_load_n(&mb[2], __ATOMIC_RELAXED) == (uint32_t)step, RTX_ESTATE,
              "wait_loss: the mailbox holds the LAST step enqueued (step %u), not step %d -- steps are waited for in order", (unsigned)mb[2], step);
    const uint32_t bits = __atomic_load_n(&mb[0], __ATOMIC_RELAXED);
    memcpy(loss_host, &bits, 4);
    return RTX_OK;
}

// ABI 7: the batch (and the dropout stream: seed / offset / dropout_mask of `next_step`; its other fields are ignored) of the
// training step AFTER the next rtx_engine_train_step call.  That call then also gathers the announced batch -- on the engine's
// side stream, under its last weight-gradient + Adam launch, into a second batch image -- and the step that is then given exactly
// this batch (same csr / target_csr / row_ids pointers, batch size, seed, offset, mask) starts with the first-layer product.
// A hint: a step that gets anything else gathers for itself.  The row ids must not change between the announcement and that
// step.  NULL cancels.  (The reference has no counterpart: its sampler densifies on the host, samplers.py:99-100.)
int rtx_engine_set_next_batch(rtx_engine* e, const rtx_batch* next, const rtx_step* next_step)
{
    RTX_CHECK(e, RTX_EINVAL, "engine is NULL");
    e->next.valid = false;
    if (!next) return RTX_OK;
    RTX_CHECK(next_step, RTX_EINVAL, "set_next_batch: next_step is NULL");
    e->next.b = *next;
    e->next.s = *next_step;
    e->next.valid = true;
    return RTX_OK;
}

// The body of evaluation.evaluate's loop (rectorch/evaluation.py:100-106) for EVERY batch of a held-out loader in one call: the host
// enqueues batch after batch without returning to Python in between (round 6: the selection kernel's 20 us left the host's ~100 us of
// per-batch Python and ctypes work as the limit of evaluate_device).
int rtx_engine_evaluate_topk(rtx_engine* e, const rtx_csr* train, const rtx_csr* heldout, const int32_t* row_ids, const int64_t* batch_offsets,
                             int32_t n_batches, const int32_t* ks_host, int32_t n_k, float* scores_scratch, double* ndcg, double* recall,
                             void* stream)
{
    return rtx_engine_evaluate_topk_ex(e, train, heldout, row_ids, batch_offsets, n_batches, ks_host, n_k, scores_scratch, ndcg, recall,
                                       nullptr, nullptr, stream);
}

int rtx_engine_evaluate_topk_ex(rtx_engine* e, const rtx_csr* train, const rtx_csr* heldout, const int32_t* row_ids, const int64_t* batch_offsets,
                                int32_t n_batches, const int32_t* ks_host, int32_t n_k, float* scores_scratch, double* ndcg, double* recall,
                                double* hit, double* mrr, void* stream)
{
    RTX_TRY(check_ready(e, false));
    RTX_CHECK(train && heldout && row_ids && batch_offsets && ks_host && scores_scratch, RTX_EINVAL, "evaluate_topk: NULL argument");
    RTX_CHECK(n_batches >= 0 && n_k >= 1, RTX_EINVAL, "evaluate_topk: bad counts");
    RTX_CHECK(heldout->n_cols == e->I, RTX_EINVAL, "evaluate_topk: held-out matrix has %d columns, the network scores %d items", heldout->n_cols, e->I);
    RTX_CHECK(!e->gvae, RTX_EINVAL, "evaluate_topk: the VAE_net variant (RTX_GVAE) samples per batch; score it batch by batch "
              "(rtx_engine_forward + rtx_topk_metrics_ex)");
    RTX_NO_USERS(e, "evaluate_topk", "batch by batch, rtx_engine_set_users + rtx_engine_forward + rtx_topk_metrics_ex");
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(ensure_shadows(e, st));
    const int64_t total = batch_offsets[n_batches] - batch_offsets[0];
    int km = 0;
    for (int q = 0; q < n_k; ++q) km = std::max(km, (int)ks_host[q]);
    for (int32_t i = 0; i < n_batches; ++i) {
        const int64_t lo = batch_offsets[i], n = batch_offsets[i + 1] - lo;
        RTX_CHECK(n >= 1 && n <= e->cfg.max_batch, RTX_EINVAL, "evaluate_topk: batch %d has %lld rows (max_batch = %d)", i, (long long)n, e->cfg.max_batch);
        rtx_batch b = {};
        b.csr = train; b.row_ids = row_ids + lo; b.batch = (int32_t)n;
        RtxCsrView in = {}, tg = {};
        RTX_TRY(resolve_batch(e, &b, &in, &tg, st, 0));
        RTX_TRY(run_forward(e, &in, &in, (int)n, 0, nullptr, 0, 0, e->NL, scores_scratch, e->I, nullptr, nullptr, st));
        // (the train items' -inf: inside the selection kernel, which takes the train rows as an exclusion list)
        RtxCsrView hv = {heldout->indptr, heldout->indices, heldout->values, row_ids + lo};
        const int64_t col = lo - batch_offsets[0];
        RTX_TRY(rtx_launch_topk_metrics(scores_scratch, (long)e->I, (int)n, e->I, hv, ks_host, n_k, km, ndcg ? ndcg + col : nullptr,
                                        recall ? recall + col : nullptr, nullptr, st, (long)total, &in, hit ? hit + col : nullptr,
                                        mrr ? mrr + col : nullptr));
    }
    return RTX_OK;
}

// evaluation.recommend's loop for every batch of a loader in one call: rtx_engine_evaluate_topk_ex with the list kernel in the place
// of the metrics kernel (no held-out matrix; the lists, not their metrics, stay on the device).
int rtx_engine_recommend(rtx_engine* e, const rtx_csr* train, const int32_t* row_ids, const int64_t* batch_offsets, int32_t n_batches,
                         int32_t k, int32_t remove_train, float* scores_scratch, int32_t* items, float* item_scores, void* stream)
{
    RTX_TRY(check_ready(e, false));
    RTX_CHECK(train && row_ids && batch_offsets && scores_scratch, RTX_EINVAL, "recommend: NULL argument");
    RTX_CHECK(items, RTX_EINVAL, "recommend: items is NULL");
    RTX_CHECK(n_batches >= 0, RTX_EINVAL, "recommend: bad batch count");
    RTX_CHECK(k >= 1 && k <= 1024, RTX_EINVAL, "recommend: k must be in [1, 1024], got %d", k);
    RTX_CHECK(!e->gvae, RTX_EINVAL, "recommend: the VAE_net variant (RTX_GVAE) samples per batch; score it batch by batch "
              "(rtx_engine_forward + rtx_topk_items)");
    RTX_NO_USERS(e, "recommend", "batch by batch, rtx_engine_set_users + rtx_engine_forward + rtx_topk_items");
    hipStream_t st = (hipStream_t)stream;
    RTX_TRY(ensure_shadows(e, st));
    const int K = std::min((int)k, e->I);
    for (int32_t i = 0; i < n_batches; ++i) {
        const int64_t lo = batch_offsets[i], n = batch_offsets[i + 1] - lo;
        RTX_CHECK(n >= 1 && n <= e->cfg.max_batch, RTX_EINVAL, "recommend: batch %d has %lld rows (max_batch = %d)", i, (long long)n, e->cfg.max_batch);
        rtx_batch b = {};
        b.csr = train; b.row_ids = row_ids + lo; b.batch = (int32_t)n;
        RtxCsrView in = {}, tg = {};
        RTX_TRY(resolve_batch(e, &b, &in, &tg, st, 0));
        RTX_TRY(run_forward(e, &in, &in, (int)n, 0, nullptr, 0, 0, e->NL, scores_scratch, e->I, nullptr, nullptr, st));
        const size_t out = (size_t)(lo - batch_offsets[0]) * K;
        TIMED("topk_items");
        RTX_TRY(rtx_launch_topk_items(scores_scratch, 0, (long)e->I, (int)n, e->I, remove_train ? &in : nullptr, K, items + out,
                                      item_scores ? item_scores + out : nullptr, st));
    }
    return RTX_OK;
}

}  // extern "C"
