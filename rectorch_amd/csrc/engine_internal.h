// engine_internal.h -- what the translation units of the engine share (engine.hip: life cycle, batch resolution, forward, the small
// entry points; engine_step.hip: the training step and its second stream; engine_dp.hip: the data-parallel plan, its transports and
// the exchange of a bucket; engine_api.hip: options, stand-alone operators, instrumentation).
// Not part of the C ABI (include/rectorch_hip.h is).
#pragma once
#include "../../include/rectorch_hip.h"
#include "rtx_gemm.h"
#include "rtx_kernels.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <string>
#include <vector>

const char* rtx_last_error_str();

struct Layer {
    int in = 0, out = 0, inp = 0, outp = 0;
    bool tanh_act = false;
    void* Wsh = nullptr;      // the compute copy every reader of this step uses
    void* Wsh_alt = nullptr;  // the fused optimizer writes the NEXT step's copy here (they swap after the step), so the
                              // weight-gradient kernels may run beside the data-gradient chain that still reads Wsh
    void* WshT = nullptr;     // hidden layers, bf16: the transposed compute copy [inp][outp] the backward chain reads (small_layers.hip)
    void* A = nullptr;
    float* O32 = nullptr;
    void* D = nullptr;
};

struct TimingSite {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0;
    int launches = 0;
};

struct TempCsr {  // dense batch converted to CSR on the device
    int64_t* indptr = nullptr;
    int32_t* counts = nullptr;
    int32_t* indices = nullptr;
    float* values = nullptr;
    int64_t cap = 0;
};

// data-parallel step scheduled by the engine (rtx_engine_dp_attach): the exchange buffer every gradient is produced into, in
// comm dtype.  Layout (elements; every tensor starts at a multiple of 64): W[NL-1], b[NL-1], W[NL-2], b[NL-2], ..., W[1], b[1],
// b[0], W[0] -- bucket A (the decoder matrix, exchanged on the side stream beside the data-gradient chain) first, bucket B
// (everything else, behind the chain) after it, the sharded encoder matrix last so that the replicated tensors of a bucket
// form ONE contiguous all-reduce range.  A sharded matrix's region is rows padded to P(out) = roundup(out + 1, 128) (zeros):
// world equal row blocks.
struct DpState {
    bool on = false;
    rtx_dp_cfg cfg = {};
    rtx_dp_ops ops = {};                      // bucket B (and everything on ONE stream): the caller's stream
    rtx_dp_ops ops_side = {};                 // bucket A on the side stream: a communicator of its own when the plan brings one (ABI 7)
    bool two_comms = false;                   // ops_side is a different communicator / table than ops
    void* xg = nullptr;                       // exchange buffer, comm dtype
    size_t xbytes = 0, xesz = 4;
    size_t xoff[2 * 2 * RTX_MAX_LAYERS] = {};   // element offset of tensor t
    bool shard[2 * RTX_MAX_LAYERS] = {};        // per layer: weight matrix reduce-scattered / updated by rows / all-gathered
    bool broken = false;                      // a collective failed inside a group: no further step until the plan is attached again
    // what the LAST step's exchange moved, per rank (buffer bytes handed to the collectives; rtx_engine_get_option "dp_*")
    int64_t st_all_reduce = 0, st_reduce_scatter = 0, st_all_gather = 0;
    int st_collectives = 0;
    void* emu_scratch = nullptr;              // emulate: where the stand-in copies go
    size_t emu_bytes = 0;
    // emulate: the collectives of one group become ONE copy launch (as RCCL fuses a group into one kernel)
    struct EmuPiece { void* buf; size_t bytes; int back; };
    EmuPiece emu_q[8];
    int emu_n = 0, emu_grouped = 0;
    hipStream_t emu_stream = nullptr;
    // where tensor t's gradient is produced (the exchange buffer, in comm dtype)
    bf16_t* xg16(int t) const { return (bf16_t*)xg + xoff[t]; }
    float* xg32(int t) const { return (float*)xg + xoff[t]; }
};

// CDAE's user node (include/rectorch_hip.h "CDAE"): the bound table, the ids announced for the next call that runs the first layer
// (rtx_engine_set_users), and the ids of the batch whose activations the engine holds -- run_forward moves `next` to `cur` when it
// runs layer 0, the backward site of the same step (data_grad, engine_step.hip) reads `cur`.  A batch announced with
// rtx_engine_set_next_batch never touches either: a step adds its own batch's users.
struct UserNode {
    float *V = nullptr, *m = nullptr, *v = nullptr;
    int n_users = 0;
    struct Ids { const int32_t* ids = nullptr; float lr = 0, beta1 = 0, beta2 = 0, eps = 0; int step = 0; } next, cur;
    bool bound() const { return V != nullptr; }
};

// what has no user node, for an engine with a table bound: RTX_EINVAL before anything is enqueued
#define RTX_NO_USERS(e, who, instead) \
    RTX_CHECK(!(e)->users.bound(), RTX_EINVAL, who ": this engine has a user table bound (CDAE), which this entry point does not carry; supported: " instead)

struct rtx_engine {
    rtx_cfg cfg;
    UserNode users;
    int NL = 0, I = 0, Z = 0, Ip = 0, Zp = 0;
    int Iin = 0;   // input columns = I + cfg.cond_dim
    int Bp_alloc = 0;
    bool bf16 = false, vae = false;
    bool gvae = false;   // RTX_GVAE (VAE_net): vae is set too (same layer layout); raw input, z sampled in every mode, BCE loss
    bool ae = false;     // RTX_AE (AETrainer(MultiDAE_net)): the RTX_DAE layout and forward (vae is clear); MSE loss, no regulariser
    size_t esz = 4;
    std::vector<Layer> L;
    std::vector<void*> allocs;
    float* Y = nullptr;
    float* Cacc = nullptr;
    size_t cacc_elems = 0;
    float *mu32 = nullptr, *lv32 = nullptr, *eps32 = nullptr;
    float2* lse_part = nullptr;
    int lse_strips = 0;
    float *tsum = nullptr, *lse = nullptr, *row_loss = nullptr, *sumsq = nullptr, *scratch_loss = nullptr;
    // bound tensors
    std::vector<float*> params, grads, m, v;
    std::vector<uint16_t*> grads16;   // optional bf16 gradient images (rtx_engine_bind_grads16; RTX_STEP_GRADS_BF16)
    bool bound = false, can_train = false, shadows_valid = false;
    TempCsr tmp_in, tmp_tg;
    // chunk stream of the batch's stored entries for the sparse first layer (spmm_in.hip)
    uint32_t* in_ent = nullptr;
    int32_t *in_desc = nullptr, *in_wsplit = nullptr;
    int64_t in_cap_chunks = 0;
    // batch image A[0] written by scatter (k_gather_scatter): per row slot, the columns the last launch wrote
    int32_t *img_written = nullptr, *img_nwritten = nullptr;
    int img_cap = 0;
    bool img_exact = false;           // A[0] is zero except the listed columns (any other writer of A[0] clears this flag)
    // The OTHER batch image (round 5): the NEXT step's gather (rtx_engine_set_next_batch) runs on the side stream, which idles
    // under this step's last weight-gradient + Adam launch, into a second image with lists and target sums of its own; the step
    // that then gets the announced batch swaps the two sets and starts with the first-layer product (the gather -- 7-9 us of pure
    // latency at the head of every step -- leaves the critical path).  swap_img_sets() exchanges these with L[0].A, tsum, img_*.
    void* A0_alt = nullptr;
    float* tsum_alt = nullptr;
    int32_t *img_written_alt = nullptr, *img_nwritten_alt = nullptr;
    int img_cap_alt = 0;
    bool img_exact_alt = false;
    struct { bool valid = false; rtx_batch b = {}; rtx_step s = {}; } next;        // announced for the step after the next call
    struct { bool valid = false; rtx_batch b = {}; uint64_t seed = 0, offset = 0; const uint8_t* mask = nullptr; } pre;   // gathered
    bool gather_done = false;         // run_forward: A[0] / tsum already hold this batch (a prefetch hit)
    // rtx_engine_forward_train / rtx_engine_backward: the number of the activations the engine holds.  run_forward -- every forward,
    // encode, decode, evaluation and training step goes through it -- takes the next one of a process-wide sequence (so tickets of two
    // engines never coincide); act_B: the batch size of the training forward the ticket was handed out for (0: none)
    uint64_t act_ticket = 0;
    int act_B = 0;
    // rtx_engine_encode_train / decode_train and their backward calls: a ticket per half.  A run of layers [l0, l1) of run_forward
    // takes a new decoder ticket when l1 > n_enc, and a new encoder ticket when l0 < n_enc -- which takes a new decoder ticket too,
    // because the encoder's last layer writes the decoder's input operand A[n_enc]: encode -> decode -> backward(decode) ->
    // backward(encode) is valid, a second encode or decode (or anything else that runs layers) in between is not.  *_B as act_B.
    uint64_t enc_ticket = 0, dec_ticket = 0;
    int enc_B = 0, dec_B = 0;
    int opt_prefetch = 1;             // 0: announced batches are ignored (A/B knob)
    int st_prefetch_hits = 0, st_prefetch_issued = 0;
    int st_join_folds = 0;             // deferred joins resolved INSIDE a first-layer product (get_option "join_folds")
    int opt_gather_scatter = 1;       // 0: k_gather rewrites the whole image every batch (rounds 1-3)
    // the weight-gradient + Adam kernels of the fused step run on a second stream beside the data-gradient chain
    hipStream_t side = nullptr;
    hipStream_t side_for = nullptr;   // the caller's stream the side stream was probed against (make_side_stream)
    std::map<hipStream_t, std::pair<hipStream_t, int>> side_cache;   // caller's stream -> (probed side stream, concurrent): a caller that
                                      //   alternates streams pays the ~1.5 ms probe once per stream, not on every change
    int side_concurrent = 0;          // 1: the probe saw the two streams run at the same time
    hipEvent_t ev_d[2 * RTX_MAX_LAYERS + 1] = {};   // ev_d[l]: D[l] is complete on the caller's stream
    hipEvent_t ev_done = nullptr;      // everything the step put on the side stream is complete
    // the two cross-stream dependencies of the fused step as stream memory operations (hipStreamWriteValue32 on the producing
    // stream, hipStreamWaitValue32 on the consuming one; option "hop_values", default on since round 4) instead of an event
    // record / wait: -3 us per step in three alternating pairs (283.7 / 280.1 / 276.0 -> 280.1 / 276.8 / 273.2,
    // profiles/r4_hop_values.txt); where the device cannot wait on a value the events remain
    int opt_hop_values = 1;
    int n_cus = 256;                   // compute units of the device (hipDeviceAttributeMultiprocessorCount)
    int opt_f32_dw_split = 1;          // float32 parity mode: small weight-gradient products split over the batch (0: one workgroup per tile)
    int opt_splitk_bwd = 0;            // measurement: split factor of the K = n_items data-gradient product alone (0 = automatic)
    int opt_splitk_fwd = 0;            // measurement: split factor of the dense first-layer product alone (0 = automatic)
    uint32_t* hopk_mem = nullptr;      // the same two words in plain device memory, for the kernel form of the hop (k_hop_set / k_hop_wait)
    uint32_t hopk_seq = 0;
    // a step flagged RTX_STEP_DEFER_JOIN ends with a k_hop_set on the side stream instead of a wait on the caller's: the NEXT use of
    // the engine on a stream resolves it (resolve_join) -- folded into the first-layer product of the next training step when that
    // step starts from a prefetched batch image, as a one-wave k_hop_wait otherwise
    bool join_pending = false, join_fold = false;
    uint32_t join_seq = 0;
    // Tile-major optimizer state (option "state_tiles"; include/rectorch_hip.h at RTX_STEP_DEFER_JOIN).  Between two DEFERRED fused steps the
    // exp_avg / exp_avg_sq of the big fused layers live in engine-owned images in the order the weight kernel walks them (RtxAdamEpi::m_img):
    // state_tiled[l] says where layer l's moments are current -- 0: the bound tensors, 1: the images (the bound tensors are stale).  A deferred
    // fused step imports at its head (state_import) and is the only thing that leaves a layer tiled; every other entry point writes the images
    // back behind the resolved join (state_to_caller, inside resolve_join) before anything reads the bound tensors.
    std::vector<float*> m_img, v_img;     // per layer, allocated at the layer's first import (dev_alloc)
    std::vector<char> state_tiled;
    int opt_state_tiles = 1;
    int opt_state_tiles_min_elems = 1 << 20;   // layers of at least this many weights (layer_is_big's bound; tests lower it)
    int st_state_imports = 0, st_state_writebacks = 0;
    int opt_timing_calibrate = 0;      // every timed bracket is followed by an empty one (site "<name>#empty"): what the events themselves cost
    // unused LDS of the decoder matrix's side-stream launch (RtxDw::lds_pad; knob "dw_side_pad").  12288 = one workgroup per CU beside the chain:
    // the chain's kernels then find registers at once (chain 95 -> 74 us on the timeline) and the step gains 2.3-4.3 us on fast and slow boxes
    // alike (profiles/r6_ab_small_waves_side_pad.txt) -- but the throttled launch itself stretches from 90 to 126 us and runs into the
    // encoder matrix's launch (90 -> 101 us): the step's dominant kernel would be REPORTED at 0.32 of the HBM roof instead of 0.40 for a 1 %
    // faster step.  Default off: the roofline of the dominant kernel is quoted for an unthrottled launch.
    int opt_dw_side_pad = 0;
    int opt_hop_fold = 1;              // the step's fork (caller's stream -> side stream) folded into the data-gradient product (engine_step.hip: backward_layers)
    int opt_hop_kernels = 0;           // (measured: no gain, a one-wave kernel costs its stream 5-6 us like the packet it replaces) the two cross-stream dependencies of the step as one-wave kernels (stream_dependency)
    uint32_t* hop_mem = nullptr;       // [0]: caller's stream -> side stream, [1]: side stream -> caller's stream (signal memory)
    uint32_t hop_seq = 0;
    uint32_t hop_wrap = 0x7ffffff0u;   // the sequence restarts from zero here (option "hop_wrap": tests lower it)
    // measurement knobs (rtx_engine_set_option; defaults are the shipped configuration)
    int opt_fuse_adam = 1;      // bf16: Adam of every weight matrix inside its weight-gradient kernel (dw_adam.hip)
    RtxOptim optim;             // rtx_engine_set_optimizer: the update rule of every optimizer launch (default: Adam, coupled decay);
                                // anything but plain Adam takes the unfused schedule (the fused epilogue of dw_adam.hip is Adam's)
    RtxClipState clip;          // rtx_engine_set_grad_clip: with a mode set every step takes the unfused schedule (a global norm needs every
                                // gradient before any parameter moves), bf16 too; its optimizer launch is rtx_launch_clipped_adam
    // rtx_engine_set_grad_accum: the weight-gradient products add into the bound gradient buffers (weight_grad, engine_step.hip); any
    // mode but OFF keeps rtx_engine_train_step on the unfused schedule.  accum_layers: bit l = layer l's accumulators hold a term of
    // the open window (a backward of one half -- rtx_engine_encode_backward / _decode_backward -- fills its own layers only: ADD on a
    // layer that holds nothing yet stores like FIRST instead of adding into stale data).  The mode is set for ONE backward pass:
    // rtx_engine_loss_grads and the external-loss callers go back to OFF behind it; an optimizer launch closes the window.
    int accum_mode = RTX_ACCUM_OFF;
    float accum_scale = 1.f;
    uint32_t accum_layers = 0;
    int opt_dw_cfg = RTX_DW_64x128;
    int opt_dp_shard_min_elems = 1 << 20;   // sharded optimizer: weight matrices of at least this many elements are reduce-scattered /
                                //   updated by rows / all-gathered, smaller ones all-reduced and replicated (tests lower it so that
                                //   small golden networks exercise the sharded path with real data)
    uint32_t* loss_mailbox = nullptr;   // coherent host memory {loss bits, ticket, step}: rtx_engine_loss_mailbox / rtx_engine_wait_loss
    uint32_t loss_ticket = 0;           // ticket of the last loss reduction enqueued with the mailbox on (monotonic; never a step count)
    int opt_dp_one_comm = 0;    // 1: bucket A shares bucket B's communicator even when the plan brings a second one (ABI 5-6 schedule; A/B knob)
    int opt_dw_cfg_set = 0;     // 1: chosen through rtx_engine_set_option (the data-parallel step otherwise picks its own tile, see dw_cfg_of)
    int opt_lse_fuse = 1;       // log-sum-exp partials from the logits GEMM's epilogue (no separate pass over the logits)
    int opt_logits16 = 1;       // bf16 training step: the logits leave their product as IEEE half, written where d loss / d logits
                                //   (bf16, same size) goes, and the loss kernel turns them into it IN PLACE: 41 + 41 MB of float32
                                //   logits traffic per ml-20m step become 21 + 21 MB (the log-sum-exp still comes from the float32
                                //   accumulators; half keeps 11 significant bits -- the bf16 products' own error level)
    int opt_two_stream = 1;     // fused step: weight-gradient kernels on a side stream beside the data-gradient chain (-10 us)
    int opt_in_on_main = 1;     // ... and the encoder matrix's kernel on the caller's stream behind the chain (engine_step.hip: finish_in_on_main)
    int opt_sparse_in = 0;      // bf16, 1: the first encoder layer as a sparse VALU product over the stored entries (spmm_in.hip).
                                //   Default since round 4: the dense [batch, n_items] x [n_items, hidden] contraction on MFMA
                                //   (k_gather -> split-K rtx_gemm_nt -> k_post), the configuration BASELINE.json's north star names;
                                //   the sparse product is the measured alternative (2-6 us per ml-20m step faster at B = 500)
    int opt_small_fwd = 1;      // bf16: hidden layers / VAE head of the forward pass as one register-resident launch each (small_layers.hip)
    int opt_small_bwd = 1;      // ... and of the data-gradient chain (reads the transposed compute copies of the hidden layers)
    int opt_big_batch_tiles = 1;   // batches of >= 1024 rows: 512 x 128 data-gradient tiles (configs[3] on one GPU: 1486 -> 1343 us/step)
    int last_sparse_in = 0;     // what the last forward pass did with the first layer (rtx_engine_get_option "last_sparse_in")
    int opt_nt_regstage = 1;    // bf16: the K = n_items / N = n_items NT contractions on the register-staged kernel (gemm.hip):
                                //   33 + 30 us in the step against 41 + 40 us on the LDS-DMA kernel at B = 500 (1 workgroup / CU)
    // timing
    bool timing_all = false;
    std::map<std::string, int> timing_sites;   // site -> sampling period (every N-th launch of the site is bracketed by events)
    std::map<std::string, long> timing_seen;
    std::map<std::string, TimingSite> sites;
    std::vector<hipEvent_t> event_pool;
    DpState dp;
};

// ---- timing -------------------------------------------------------------------------------------
struct ScopedTimer {
    rtx_engine* e;
    hipStream_t s;
    TimingSite* site = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::string name;
    ScopedTimer(rtx_engine* eng, const char* nm, hipStream_t st) : e(eng), s(st), name(nm)
    {
        const char* name = nm;
        if (!e->timing_all && e->timing_sites.empty()) return;
        if (!e->timing_all) {
            auto it = e->timing_sites.find(name);
            if (it == e->timing_sites.end()) return;
            // an event record costs microseconds on the stream it is recorded on (two per timed launch): sample
            if (it->second > 1 && (e->timing_seen[name]++ % it->second) != 0) return;
        }
        site = &e->sites[name];
        auto get = [&]() {
            hipEvent_t ev;
            if (!e->event_pool.empty()) {
                ev = e->event_pool.back();
                e->event_pool.pop_back();
            } else if (hipEventCreate(&ev) != hipSuccess) {
                ev = nullptr;
            }
            return ev;
        };
        e0 = get();
        e1 = get();
        if (e0) (void)hipEventRecord(e0, s);
    }
    ~ScopedTimer()
    {
        if (!site) return;
        if (e1) (void)hipEventRecord(e1, s);
        if (e0 && e1) site->pending.push_back({e0, e1});
        if (e->opt_timing_calibrate && e1) {
            // an EMPTY bracket right behind the timed one, on the same stream at the same moment: the time between two event records
            // with nothing in between is what the bracket above contains besides its kernel (option "timing_calibrate";
            // reported as site "<name>#empty", the caller subtracts)
            hipEvent_t a = nullptr, b = nullptr;
            if (!e->event_pool.empty()) { a = e->event_pool.back(); e->event_pool.pop_back(); } else if (hipEventCreate(&a) != hipSuccess) a = nullptr;
            if (!e->event_pool.empty()) { b = e->event_pool.back(); e->event_pool.pop_back(); } else if (hipEventCreate(&b) != hipSuccess) b = nullptr;
            if (a && b) {
                (void)hipEventRecord(a, s);
                (void)hipEventRecord(b, s);
                e->sites[name + "#empty"].pending.push_back({a, b});
            }
        }
    }
};
#define RTX_CAT2(a, b) a##b
#define RTX_CAT(a, b) RTX_CAT2(a, b)
#define TIMED(name) ScopedTimer RTX_CAT(_timer_, __LINE__)(e, name, st)

// ---- the training step (engine_step.hip; dp_bucket in engine_dp.hip) -----------------------------------------------------------
// the four schedules of the step, chosen once by the public entry point
enum StepKind {
    STEP_GRADS_ONLY,      // rtx_engine_loss_grads: gradients into the bound buffers, the per-layer callback
    STEP_FUSED,           // rtx_engine_train_step, bf16: Adam inside the weight-gradient kernels (the benchmarked path)
    STEP_UNFUSED_ADAM,    // rtx_engine_train_step, float32 or fuse_adam = 0: Adam as a launch of its own behind the gradients
    STEP_DATA_PARALLEL,   // rtx_engine_train_step_dp: gradients into the exchange buffer, the buckets of the attached plan
};
// what the functions of one step share
struct StepCtx {
    rtx_engine* e;
    const rtx_step* step;
    hipStream_t st;          // the caller's stream
    StepKind kind;
    DpState* dp;             // STEP_DATA_PARALLEL: the attached plan, else null
    float *loss_out, *loss_accum;
    bool dae_reg;            // Mult-DAE's norm regulariser is on (lam != 0)
    bool keep_grads;         // RTX_STEP_KEEP_GRADS
    // rtx_engine_backward: d loss / d output comes from the caller (no loss kernel ran, there is no loss to sum); ext_mu / ext_lv
    // (nullable): its d loss / d mu, d loss / d logvar for the VAE head's backward
    bool ext;
    const float *ext_mu, *ext_lv;
    int dw_cfg;              // tile of the weight-gradient kernels
    int B, Bp;
    RtxCsrView tg;           // the batch's target rows
    bool tiles;              // a deferred fused step on 64 x 128 tiles with "state_tiles" on: the big layers' moments are / stay tile-major
    bool two;                // the big weight kernels run on the side stream
    int main_li;             // the layer whose weight kernel closes the step on the caller's stream ("in_on_main"), or -1
    RtxAdamArgs rest;        // STEP_FUSED: tensors whose Adam is NOT fused into a weight-gradient kernel (odd-width matrices + their biases)
    int rest_ids[RTX_MAX_TENSORS];
};

// A contraction whose output goes to the fp32 scratch Cacc (possibly as split-K slabs):
//   form NT: C[Mp][Np] = A[Mp][Kp] x B[Np][Kp]^T      (forward)
//   form NN: C[Mp][Np] = A[Mp][Kp] x B[Kp][Np]        (backward-data: B = the weight copy itself)
struct GemmPlan {
    int cfg;        // LDS-DMA kernel: RtxDmaCfg; register-staged kernels (f32, optionally bf16 NT): 128x128 tiles
    int regstage;
    int bm, bn;
    int m_tiles, n_tiles, k_slices, splits;
};

// ---- helpers shared by the translation units (hidden: not exported from librectorch_hip.so); defined in engine.hip unless noted
#define RTX_INTERNAL __attribute__((visibility("hidden")))
RTX_INTERNAL int dev_alloc(rtx_engine* e, void** p, size_t bytes, bool zero = true);
RTX_INTERNAL void dev_free(rtx_engine* e, void* p);   // a tracked allocation nobody on the device uses any more (the caller has drained its readers)
RTX_INTERNAL int ensure_shadows(rtx_engine* e, hipStream_t st, bool keep_tiles = false);
RTX_INTERNAL int check_ready(rtx_engine* e, bool train);
RTX_INTERNAL size_t plan_cacc_elems(rtx_engine* e, int Np, int Kp);      // split-K scratch a product of this shape needs (set_option "splitk" re-sizes it)
RTX_INTERNAL GemmPlan plan_gemm(const rtx_engine* e, int Mp, int Np, int Kp, int form = RTX_FORM_NT);
RTX_INTERNAL int gemm_to_cacc(rtx_engine* e, int form, const void* A, long lda, const void* B, long ldb, int Mp, int Np, int Kp, int* splits_out,
                              hipStream_t st, uint32_t* hop_word = nullptr, uint32_t hop_seq = 0, const uint32_t* wait_word = nullptr, uint32_t wait_seq = 0);
RTX_INTERNAL int resolve_batch(rtx_engine* e, const rtx_batch* b, RtxCsrView* in, RtxCsrView* tg, hipStream_t st, int need_target = 1);
RTX_INTERNAL bool logits16_on(const rtx_engine* e);
RTX_INTERNAL bool sparse_in_ok(const rtx_engine* e, const RtxCsrView* in, int Bp, int64_t* chunks);
RTX_INTERNAL int gather_batch(rtx_engine* e, const RtxCsrView* in, const RtxCsrView* tg, int B, int training, const rtx_step* step, hipStream_t st);
RTX_INTERNAL int run_forward(rtx_engine* e, const RtxCsrView* in, const RtxCsrView* tg, int B, int training, const rtx_step* step,
                             int want_lse, int l0, int l1, float* logits, long ldlog, float* mu_out, float* lv_out, hipStream_t st);
// the user table of the current batch as a kernel argument (false: no table bound, or the batch came without ids)
RTX_INTERNAL bool user_node_args(const rtx_engine* e, bool update, RtxPostUsers& u);
RTX_INTERNAL int ensure_hopk(rtx_engine* e);
RTX_INTERNAL int launch_hop_set(rtx_engine* e, hipStream_t st, int slot, uint32_t v);    // k_hop_set / k_hop_wait on word `slot` of hopk_mem
RTX_INTERNAL int launch_hop_wait(rtx_engine* e, hipStream_t st, int slot, uint32_t v);
// keep_tiles: the caller is a deferred fused step, which goes on with the tile-major optimizer state; everybody else gets it written back
RTX_INTERNAL int resolve_join(rtx_engine* e, hipStream_t st, bool keep_tiles = false);
RTX_INTERNAL bool state_any_tiled(const rtx_engine* e);
RTX_INTERNAL int state_to_caller(rtx_engine* e, hipStream_t st);
RTX_INTERNAL void fill_adam_tensors(rtx_engine* e, RtxAdamArgs& a, int l0 = 0, int l1 = -1);
RTX_INTERNAL void fill_adam_scalars(rtx_engine* e, const rtx_step* step, RtxAdamArgs& a, int t0 /* first tensor index */, const int* ids = nullptr);
RTX_INTERNAL int launch_sumsq(rtx_engine* e, hipStream_t st);
RTX_INTERNAL void dp_release(rtx_engine* e);          // engine_dp.hip
// engine_dp.hip: exchange + optimizer of layers [l_lo, l_hi) on stream ws; `alt`: the big matrices' Adam writes the NEXT step's
// compute copy (the chain on the other stream still reads this step's)
RTX_INTERNAL int dp_bucket(const StepCtx& c, int l_lo, int l_hi, hipStream_t ws, bool alt);
