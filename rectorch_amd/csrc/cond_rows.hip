// cond_rows.hip -- conditioned batches for CMultiVAE built on the device (gfx950): what ConditionedDataSampler / Balanced... / Empty...
// (reference rectorch/samplers.py:108-419) assemble per batch on the host with scipy -- row slicing, hstack of the condition one-hot,
// a sparse product against the item-condition matrix, a multiply, a row filter -- as two small CSR matrices written by three
// kernels into buffers allocated once.  An EXAMPLE is (row r, condition c), c = -1 for "unconditioned":
//   input  row = row r of `tr` + one entry 1.0 at column n_items + c when c >= 0          [n_items + n_cond columns, ids sorted]
//   target row = row r of `te` restricted to the items whose condition list holds c (c = -1: the items with any condition)
// The engine consumes a slot's pair exactly as it consumes two uploaded matrices (rtx_batch.csr / target_csr + row ids 0..batch-1).
#include "rtx_common.h"
#include "rtx_kernels.h"
#include "../../include/rectorch_hip.h"

#include <algorithm>
#include <vector>

namespace {

struct CondSrc {
    const int64_t* tr_indptr; const int32_t* tr_indices; const float* tr_values;
    const int64_t* te_indptr; const int32_t* te_indices; const float* te_values;
    const uint32_t* bits;     // [n_items][W]: bit c of item i = condition c is in the item's list; nullptr = no filter
    const uint32_t* any;      // [ceil(n_items / 32)]: bit i = item i has at least one condition
    const int32_t* ex_row;    // [n_ex]
    const int32_t* ex_cond;   // [n_ex], -1 = unconditioned
    int64_t n_ex;
    int32_t n_items, W;
};

// does `item` of a target row survive under condition c?
__device__ __forceinline__ bool cond_keeps(const CondSrc& s, int item, int c)
{
    if (!s.bits) return true;
    if ((unsigned)item >= (unsigned)s.n_items) return false;
    if (c < 0) return (s.any[item >> 5] >> (item & 31)) & 1u;
    return (s.bits[(size_t)item * s.W + (c >> 5)] >> (c & 31)) & 1u;
}

// Counting kernel (creation time, all examples): one 64-lane wave per example; the fill kernel's target half without the stores.
__global__ __launch_bounds__(256) void k_cond_count(const CondSrc s, int32_t* ilen, int32_t* tlen)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= s.n_ex) return;
    const int r = s.ex_row[e], c = s.ex_cond[e];
    const int64_t beg = s.te_indptr[r];
    const int n = (int)(s.te_indptr[r + 1] - beg);
    int kept = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool ok = k < n && cond_keeps(s, s.te_indices[beg + k], c);
        kept += __popcll(__ballot(ok));
    }
    if (lane == 0) {
        tlen[e] = kept;
        ilen[e] = (int)(s.tr_indptr[r + 1] - s.tr_indptr[r]) + (c >= 0 ? 1 : 0);
    }
}

// Scan kernel: ONE workgroup.  Exclusive sums of the batch's input and target lengths -> the two int64 indptr arrays; a batch
// larger than the workgroup is walked in rounds of 256 with a running carry.  An example id outside [0, n_ex) counts as empty.
__global__ __launch_bounds__(256) void k_cond_scan(const int32_t* ex_ids, int batch, int64_t n_ex, const int32_t* ilen, const int32_t* tlen,
                                                   int64_t* in_indptr, int64_t* tg_indptr)
{
    __shared__ int wsum[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry_in = 0, carry_tg = 0;
    for (int base = 0; base < batch; base += 256) {
        const int i = base + tid;
        const int64_t e = i < batch ? (int64_t)ex_ids[i] : -1;
        const bool valid = e >= 0 && e < n_ex;
        const int a = valid ? ilen[e] : 0, t = valid ? tlen[e] : 0;
        int sa = a, stg = t;      // inclusive sums inside the wave (a round's total stays below 2^31: checked at creation)
        for (int d = 1; d < 64; d <<= 1) {
            const int ua = __shfl_up(sa, d), ut = __shfl_up(stg, d);
            if (lane >= d) { sa += ua; stg += ut; }
        }
        if (lane == 63) { wsum[0][wave] = sa; wsum[1][wave] = stg; }
        __syncthreads();
        int off_a = 0, off_t = 0, tot_a = 0, tot_t = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) { off_a += wsum[0][w]; off_t += wsum[1][w]; }
            tot_a += wsum[0][w]; tot_t += wsum[1][w];
        }
        if (i < batch) {
            in_indptr[i] = carry_in + off_a + sa - a;
            tg_indptr[i] = carry_tg + off_t + stg - t;
        }
        carry_in += tot_a; carry_tg += tot_t;
        __syncthreads();          // the round's totals are read: the next round may overwrite them
    }
    if (tid == 0) { in_indptr[batch] = carry_in; tg_indptr[batch] = carry_tg; }
}

struct CondDst {
    const int64_t* in_indptr; int32_t* in_indices; float* in_values; int64_t in_cap;
    const int64_t* tg_indptr; int32_t* tg_indices; float* tg_values; int64_t tg_cap;
};

// Fill kernel: one 64-lane wave per example of the batch.  The input row is copied 64 entries a pass and the condition entry
// appended (column ids stay sorted: n_items + c is beyond every item).  The target row is walked 64 entries a pass, every item
// tested against the bitmap, and the survivors written IN ORDER: ballot + population count of the lower lanes is the offset inside
// the pass, a running base carries across passes (the top-k and list-metrics kernels binary-search held-out rows).
// Every store is checked against the slot's capacity: lengths and offsets come from device arrays.
__global__ __launch_bounds__(256) void k_cond_fill(const CondSrc s, const int32_t* ex_ids, int batch, const CondDst d)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    const int64_t e = ex_ids[b];
    if (e < 0 || e >= s.n_ex) return;
    const int r = s.ex_row[e], c = s.ex_cond[e];
    {
        const int64_t beg = s.tr_indptr[r];
        const int n = (int)(s.tr_indptr[r + 1] - beg);
        const int64_t o = d.in_indptr[b];
        for (int k = lane; k < n; k += 64) {
            if (o + k < d.in_cap) {
                d.in_indices[o + k] = s.tr_indices[beg + k];
                if (d.in_values) d.in_values[o + k] = s.tr_values[beg + k];
            }
        }
        if (lane == 0 && c >= 0 && o + n < d.in_cap) {
            d.in_indices[o + n] = s.n_items + c;
            if (d.in_values) d.in_values[o + n] = 1.0f;
        }
    }
    const int64_t beg = s.te_indptr[r];
    const int n = (int)(s.te_indptr[r + 1] - beg);
    int64_t o = d.tg_indptr[b];
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const int item = k < n ? s.te_indices[beg + k] : 0;
        const bool ok = k < n && cond_keeps(s, item, c);
        const unsigned long long bal = __ballot(ok);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (ok && o + before < d.tg_cap) {
            d.tg_indices[o + before] = item;
            if (d.tg_values) d.tg_values[o + before] = s.te_values[beg + k];
        }
        o += __popcll(bal);
    }
}

}  // namespace

// Slot reuse without a wait (rtx_cond_build overwrites a slot that an earlier batch lived in):
// a trainer builds batch j on the caller's stream BEFORE it enqueues step j-1 (one batch of look-ahead for
// rtx_engine_set_next_batch).  Everything earlier on the caller's stream is ordered before the build; what is NOT is the engine's
// side stream as far as no join has been resolved yet.  engine_step.hip: step j-2 (the last one enqueued) ended with
// RTX_STEP_DEFER_JOIN (close_side_stream stores a number, nobody has waited for it), and its side stream carries that step's weight
// kernels and prefetch_next's gather of batch j-1 (finish_in_on_main / finish_data_parallel), which reads the CSR arrays of batch
// j-1's slot.  Step j-2's own batch was read by its gather -- on the caller's stream, or prefetched under step j-3 on the side
// stream, and step j-3's deferred join was resolved by step j-2's first kernel (begin_and_forward: resolve_join or the folded wait),
// which is on the caller's stream in front of this build.  So when batch j is built only the slots of batches j-1 (side stream,
// unordered) and j-2 (counted conservatively: its step is the newest one enqueued) can still have readers the build is not ordered
// behind: three distinct slots are needed, RTX_COND_SLOTS_DEFAULT = 4 leaves one spare.  rtx_cond_create refuses fewer than 3.
#define RTX_COND_SLOTS_MIN 3
#define RTX_COND_SLOTS_MAX 64

struct rtx_cond {
    const rtx_csr* tr = nullptr;      // resident source matrices: referenced, not owned
    const rtx_csr* te = nullptr;
    CondSrc src = {};
    uint32_t* bits = nullptr;
    uint32_t* any = nullptr;
    int32_t* ex_row = nullptr;
    int32_t* ex_cond = nullptr;
    int32_t* ilen = nullptr;          // [n_ex] input length  = len tr(row) + (cond >= 0)
    int32_t* tlen = nullptr;          // [n_ex] filtered target length
    int64_t n_ex = 0;
    int32_t n_items = 0, n_cond = 0, max_batch = 0;
    int64_t in_cap = 0, tg_cap = 0;   // entries per slot
    // a slot's handles are heap objects of their own: their addresses never change (the engine's prefetch matches the
    // announced batch by pointer); their arrays belong to this object, rtx_csr_destroy must not be called on them
    std::vector<rtx_csr*> in, tg;
};

static void cond_free(rtx_cond* c)
{
    if (!c) return;
    for (size_t s = 0; s < c->in.size(); ++s) {
        for (rtx_csr* m : {c->in[s], c->tg[s]}) {
            if (!m) continue;
            if (m->indptr) (void)hipFree(m->indptr);
            if (m->indices) (void)hipFree(m->indices);
            if (m->values) (void)hipFree(m->values);
            delete m;
        }
    }
    for (void* p : {(void*)c->bits, (void*)c->any, (void*)c->ex_row, (void*)c->ex_cond, (void*)c->ilen, (void*)c->tlen})
        if (p) (void)hipFree(p);
    delete c;
}

static int cond_alloc(void** p, size_t bytes)
{
    hipError_t rc = hipMalloc(p, bytes ? bytes : 16);
    if (rc != hipSuccess) {
        rtx_set_error("cond: hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(rc));
        return RTX_ENOMEM;
    }
    return RTX_OK;
}

static int cond_upload(void** p, const void* host, size_t bytes)
{
    RTX_TRY(cond_alloc(p, bytes));
    if (bytes) RTX_HIP(hipMemcpy(*p, host, bytes, hipMemcpyHostToDevice));
    return RTX_OK;
}

static int cond_setup(rtx_cond* c, const uint32_t* bits_host, const uint32_t* any_host, const int32_t* ex_row_host,
                      const int32_t* ex_cond_host, int32_t n_slots)
{
    const int W = (c->n_cond + 31) / 32;
    if (bits_host) {
        RTX_TRY(cond_upload((void**)&c->bits, bits_host, sizeof(uint32_t) * (size_t)c->n_items * W));
        RTX_TRY(cond_upload((void**)&c->any, any_host, sizeof(uint32_t) * (size_t)((c->n_items + 31) / 32)));
    }
    RTX_TRY(cond_upload((void**)&c->ex_row, ex_row_host, sizeof(int32_t) * (size_t)c->n_ex));
    RTX_TRY(cond_upload((void**)&c->ex_cond, ex_cond_host, sizeof(int32_t) * (size_t)c->n_ex));
    RTX_TRY(cond_alloc((void**)&c->ilen, sizeof(int32_t) * (size_t)c->n_ex));
    RTX_TRY(cond_alloc((void**)&c->tlen, sizeof(int32_t) * (size_t)c->n_ex));
    c->src = CondSrc{c->tr->indptr, c->tr->indices, c->tr->values, c->te->indptr, c->te->indices, c->te->values,
                     c->bits, c->any, c->ex_row, c->ex_cond, c->n_ex, c->n_items, W};
    c->in_cap = std::max<int64_t>((int64_t)c->max_batch * ((int64_t)c->tr->max_row_len + 1), 1);
    c->tg_cap = std::max<int64_t>((int64_t)c->max_batch * (int64_t)c->te->max_row_len, 1);
    for (int s = 0; s < n_slots; ++s) {
        rtx_csr* a = new rtx_csr();
        rtx_csr* t = new rtx_csr();
        c->in.push_back(a);
        c->tg.push_back(t);
        a->n_cols = c->n_items + c->n_cond;
        t->n_cols = c->n_items;
        // max_row_len is the SOURCE matrix's bound (+ 1 for the condition entry), not the batch's longest row.  Every reader takes
        // an upper bound: engine.hip sizes buffers with it (gather_batch: the scatter lists' capacity; sparse_in_ok: the chunk
        // stream's capacity), loss.hip only asks whether the longest target row fits k_dlogits_row's LDS list (a bound that is too
        // large picks the chunked kernel, which computes the same), prefetch_next only asks > 0.  avg_row_len (resolve_batch:
        // nnz / n_rows, a speed heuristic of sparse_in_ok) is exact when rtx_cond_build is told the batch's entry counts.
        a->max_row_len = (int32_t)std::min<int64_t>((int64_t)c->tr->max_row_len + 1, INT32_MAX);
        t->max_row_len = c->te->max_row_len;
        RTX_TRY(cond_alloc((void**)&a->indptr, sizeof(int64_t) * ((size_t)c->max_batch + 1)));
        RTX_TRY(cond_alloc((void**)&t->indptr, sizeof(int64_t) * ((size_t)c->max_batch + 1)));
        RTX_TRY(cond_alloc((void**)&a->indices, sizeof(int32_t) * (size_t)c->in_cap));
        RTX_TRY(cond_alloc((void**)&t->indices, sizeof(int32_t) * (size_t)c->tg_cap));
        if (c->tr->values) RTX_TRY(cond_alloc((void**)&a->values, sizeof(float) * (size_t)c->in_cap));
        if (c->te->values) RTX_TRY(cond_alloc((void**)&t->values, sizeof(float) * (size_t)c->tg_cap));
        // an empty matrix until the first build
        RTX_HIP(hipMemset(a->indptr, 0, sizeof(int64_t) * ((size_t)c->max_batch + 1)));
        RTX_HIP(hipMemset(t->indptr, 0, sizeof(int64_t) * ((size_t)c->max_batch + 1)));
    }
    if (c->n_ex > 0) {
        const int64_t blocks = (c->n_ex + 3) / 4;
        RTX_CHECK(blocks <= INT32_MAX, RTX_EINVAL, "cond_create: too many examples (%lld)", (long long)c->n_ex);
        hipLaunchKernelGGL(k_cond_count, dim3((unsigned)blocks), dim3(256), 0, nullptr, c->src, c->ilen, c->tlen);
        RTX_HIP(hipGetLastError());
    }
    RTX_HIP(hipStreamSynchronize(nullptr));   // creation is set-up time: the memsets and the counts are done when the call returns
    return RTX_OK;
}

extern "C" {

int rtx_cond_create(const rtx_csr* tr, const rtx_csr* te, int32_t n_cond, const uint32_t* bitmap_host, const uint32_t* any_host,
                    const int32_t* ex_row_host, const int32_t* ex_cond_host, int64_t n_ex, int32_t max_batch, int32_t n_slots,
                    rtx_cond** out)
{
    RTX_CHECK(tr && out, RTX_EINVAL, "cond_create: NULL argument");
    if (!te) te = tr;
    RTX_CHECK(n_cond >= 0 && max_batch >= 1 && n_ex >= 0, RTX_EINVAL, "cond_create: bad sizes (n_cond %d, max_batch %d, n_ex %lld)", n_cond,
              max_batch, (long long)n_ex);
    RTX_CHECK(n_slots >= RTX_COND_SLOTS_MIN && n_slots <= RTX_COND_SLOTS_MAX, RTX_EINVAL,
              "cond_create: %d slots; a trainer with one batch of look-ahead needs at least %d", n_slots, RTX_COND_SLOTS_MIN);
    RTX_CHECK(te->n_rows == tr->n_rows && te->n_cols == tr->n_cols, RTX_EINVAL, "cond_create: tr is %lld x %d, te %lld x %d", (long long)tr->n_rows,
              tr->n_cols, (long long)te->n_rows, te->n_cols);
    RTX_CHECK((int64_t)tr->n_cols + n_cond <= INT32_MAX, RTX_EINVAL, "cond_create: too many columns");
    RTX_CHECK(!bitmap_host == !any_host, RTX_EINVAL, "cond_create: the bitmap and its any-condition bits come together");
    RTX_CHECK(n_ex == 0 || (ex_row_host && ex_cond_host), RTX_EINVAL, "cond_create: the example table is NULL");
    // one round of the scan kernel (256 examples) sums in int32
    RTX_CHECK(256 * ((int64_t)std::max(tr->max_row_len, te->max_row_len) + 1) < INT32_MAX, RTX_EINVAL, "cond_create: rows too long");
    for (int64_t i = 0; i < n_ex; ++i) {
        RTX_CHECK(ex_row_host[i] >= 0 && ex_row_host[i] < tr->n_rows, RTX_EINVAL, "cond_create: example %lld names row %d of %lld", (long long)i,
                  ex_row_host[i], (long long)tr->n_rows);
        RTX_CHECK(ex_cond_host[i] >= -1 && ex_cond_host[i] < std::max(n_cond, 0), RTX_EINVAL, "cond_create: example %lld names condition %d of %d",
                  (long long)i, ex_cond_host[i], n_cond);
    }
    int ndev = 0;
    hipError_t h = hipGetDeviceCount(&ndev);
    RTX_CHECK(h == hipSuccess && ndev > 0, RTX_EHIP, "no HIP device available (%s): librectorch_hip has no CPU path", hipGetErrorString(h));
    rtx_cond* c = new rtx_cond();
    c->tr = tr; c->te = te; c->n_items = tr->n_cols; c->n_cond = n_cond; c->n_ex = n_ex; c->max_batch = max_batch;
    const int rc = cond_setup(c, bitmap_host, any_host, ex_row_host, ex_cond_host, n_slots);
    if (rc) { cond_free(c); return rc; }
    *out = c;
    return RTX_OK;
}

int rtx_cond_destroy(rtx_cond* c)
{
    cond_free(c);    // (hipFree waits for the device: no kernel still reads what is freed)
    return RTX_OK;
}

int rtx_cond_lengths(const rtx_cond* c, int32_t* in_len_host, int32_t* target_len_host)
{
    RTX_CHECK(c, RTX_EINVAL, "cond is NULL");
    if (in_len_host && c->n_ex) RTX_HIP(hipMemcpy(in_len_host, c->ilen, sizeof(int32_t) * (size_t)c->n_ex, hipMemcpyDeviceToHost));
    if (target_len_host && c->n_ex) RTX_HIP(hipMemcpy(target_len_host, c->tlen, sizeof(int32_t) * (size_t)c->n_ex, hipMemcpyDeviceToHost));
    return RTX_OK;
}

int rtx_cond_slot(const rtx_cond* c, int32_t slot, const rtx_csr** in, const rtx_csr** target)
{
    RTX_CHECK(c && slot >= 0 && slot < (int32_t)c->in.size(), RTX_EINVAL, "cond_slot: bad slot %d", slot);
    if (in) *in = c->in[slot];
    if (target) *target = c->tg[slot];
    return RTX_OK;
}

int rtx_cond_build(rtx_cond* c, int32_t slot, const int32_t* ex_ids, int32_t batch, int64_t nnz_in, int64_t nnz_target, void* stream)
{
    RTX_CHECK(c && slot >= 0 && slot < (int32_t)c->in.size(), RTX_EINVAL, "cond_build: bad slot %d", slot);
    RTX_CHECK(batch >= 0 && batch <= c->max_batch && (ex_ids || batch == 0), RTX_EINVAL, "cond_build: batch %d outside [0, max_batch = %d]", batch,
              c->max_batch);
    RTX_CHECK(nnz_in <= c->in_cap && nnz_target <= c->tg_cap, RTX_EINVAL, "cond_build: more entries announced than %d rows can hold", batch);
    rtx_csr* a = c->in[slot];
    rtx_csr* t = c->tg[slot];
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cond_scan, dim3(1), dim3(256), 0, st, ex_ids, batch, c->n_ex, c->ilen, c->tlen, a->indptr, t->indptr);
    RTX_HIP(hipGetLastError());
    if (batch > 0) {
        const CondDst d = {a->indptr, a->indices, a->values, c->in_cap, t->indptr, t->indices, t->values, c->tg_cap};
        hipLaunchKernelGGL(k_cond_fill, dim3((batch + 3) / 4), dim3(256), 0, st, c->src, ex_ids, batch, d);
        RTX_HIP(hipGetLastError());
    }
    // the host-side description of the slot's matrices: what the engine reads when it is handed them (n_rows bounds the row ids,
    // nnz / n_rows is resolve_batch's mean row length).  Unknown counts: the upper bound.
    a->n_rows = t->n_rows = batch;
    a->nnz = nnz_in >= 0 ? nnz_in : std::min<int64_t>((int64_t)batch * a->max_row_len, c->in_cap);
    t->nnz = nnz_target >= 0 ? nnz_target : std::min<int64_t>((int64_t)batch * t->max_row_len, c->tg_cap);
    return RTX_OK;
}

}  // extern "C"
