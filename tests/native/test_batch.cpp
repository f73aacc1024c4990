// Native (no Python) check of the batch-formation kernels -- what every training and scoring step starts with -- one launcher at a time,
// against a host mirror of batch_rows.h, bit for bit wherever the data make the arithmetic exact:
//   A  rtx_launch_gather, full-rewrite form (k_gather<float | bf16>): ALL Bp * ldx elements of the image and tsum.  Shapes (I, cond, ldx),
//      float32 | bf16 (LDS chunk 4 096 | 8 192 elements):
//        s0 (300, 0, 304) | same             one partial chunk, ldx a multiple of 8 and not of 128
//        s1 (4 000, 0, 4 096) | (8 000, 0, 8 192)      exactly one chunk
//        s2 (4 095, 0, 4 224) | (8 191, 0, 8 320)      ones column on the last element of chunk 0
//        s3 (4 096, 0, 4 224) | (8 192, 0, 8 320)      ones column on the first element of chunk 1
//        s4 (4 090, 16, 4 224) | (8 180, 16, 8 320)    condition columns straddle the boundary
//      Cases, each run with BOTH types (values: none = implicit feedback, half = ratings 0.5 .. 5 in steps of 0.5, real = 0.3 k and
//      48-bit random values; B / Bp; target: in = the input view, other = a second matrix with values and other row lengths):
//        a1  s0 none  raw 0 eval            no ids   5 / 8     in        a9   s3 half raw 0 train p 0.3 Philox ids  130 / 256 in  (kept AND dropped
//        a2  s0 half  raw 0 train p 0.5 Philox ids   5 / 8     other           in every row longer than 8, asserted)
//        a3  s0 real  raw 0 train p 0.3 Philox ids   8 / 8     in        a10  s3 real raw 0 train p 0.5 Philox no ids 8 / 8   other
//        a4  s1 half  raw 0 train p 1.0 Philox no ids 8 / 8    in        a11  s4 half raw 0 train p 0.5 MASK  ids    5 / 8    in
//        a5  s1 none  raw 1 eval            ids    130 / 256   in        a12  s4 real raw 0 train p 0.3 MASK  no ids 40 / 40  other
//        a6  s1 real  raw 1 train p 0.3 Philox ids   5 / 8     in        a13  s4 none raw 0 eval              ids    5 / 8    in  (implicit + cond:
//        a7  s2 none  raw 0 train p 0.5 Philox ids   5 / 8     in              the condition values are the implied ones)
//        a8  s2 real  raw 0 eval            no ids  40 / 40    in        a14  s4 half raw 1 train p 0.5 Philox ids  130 / 256 other
//                                                                        a15  s4 real raw 1 eval              no ids 8 / 8    in
//      Philox runs with seed and offset above 2^32; the mask is [B][I] bytes (0, 1, 2 or 255) with cond > 0, so indexing it by Iin shows.
//      With ids a row is named twice in every batch.
//   B  the scatter form (k_gather_scatter, `written` / `n_written`), both types: ONE image and one pair of lists, zeroed once, then five
//      launches without a reset: (1) long rows, B = Bp = 8; (2) other users, B = 5 of 8; (3) a user repeated in another slot; (4) training
//      with dropout; (5) launch 1 again.  After every launch the image and tsum equal, bit for bit, a fresh k_gather launch of the same
//      arguments (real ratings too: both run the same 256-thread reduction) and the mirror; n_written, the listed columns, what lies
//      behind the lists.  Two sequences per type: (I, cond, ldx) = (4 090 | 8 180, 16, 4 224 | 8 320) with real ratings, and
//      (4 096, 0, 4 224) with half steps (Iin on a chunk boundary of k_gather<float>; the scatter kernel has no chunks).
//   C  rtx_launch_in_chunks (k_in_chunks, 512 threads, chunk 8 192): shapes (8 191 | 8 192 | 8 180 + 16, ldx 8 320) and (300, 304), each
//      with X (image, tsum) and with X null: image and tsum against k_gather<bf16> of the same arguments (bit for bit in the exact regime,
//      under A's bound otherwise, counting the elements that differ from k_gather), the chunk stream decoded word by word, the stream
//      equal with and without X, the 16-way split against the rule in the kernel's comment, the capacity refusal (nothing written).
//        c1  (300)   none eval ids 5 / 8                      c4  (8 191) real eval no ids 40 / 40               c7  (8 180+16) half train p 0.5 MASK ids 5 / 8
//        c2  (300)   real train p 0.3 ids B = 1 of 8          c5  (8 192) none train p 0.5, long last user 5 / 8 c8  (8 180+16) real train p 0.3 MASK no ids 40 / 48
//        c3  (8 191) half train p 0.5 ids 130 / 256, other    c6  (8 192) real train p 0.3 ids 130 / 256         c9  (8 180+16) real eval, long last user 5 / 8
//   D  rtx_launch_csr_to_dense: I in {1, 7, 301, 4 095, 4 096, 4 097, 8 200} x values {no, yes} x row_ids {no, yes}; bit for bit.
//   E  dense -> CSR (k_dense_count, k_scan_counts, k_dense_fill): I in {1, 255, 256, 257, 600}, B = 9, rows all zero / all non-zero /
//      alternating / non-zero only in the last partial block of 256 / -0.0, a denormal, +-inf and NaN / random; the round trip through
//      k_csr_to_dense; the resulting view (max_row_len = 0) fed to k_gather on a conditioned shape against the gather of the CSR it came from.
//   R  the refusals of the launchers that return before the first HIP call (in --host mode too).
//   S  (--host) the judging of A, B and C fed a synthetic device result with one defect at a time; every defect must be rejected.
// Every output is poisoned (all bits set) before the launch and carries a poisoned guard behind its end; whatever a launch must leave alone
// is compared with the poison.  The CSR rows no batch row names hold junk values (|v| in [500, 1500)) at valid columns of the image.
//
// The matrix (one generator, 40 rows): row 0 empty, row 1 one entry, rows 2 / 3 / 4 of 255 / 256 / 257 entries (the workgroup stride and
// its neighbours), row 5 of 700, row 6 of 520 (more than the 512 threads of k_in_chunks), row 7 with every stored value 0.0 (norm 0, inv =
// 1e12, products 0), the rest 2 .. 120; lengths are cut to I.  Rows 2 .. 6 and every third row hold columns 0, I - 1, 4 095, 4 096, 8 191
// and 8 192 where they exist.  With cond > 0 two thirds of the rows carry one to three condition columns in [I, Iin), values not 1.
//
// The two regimes.  EXACT (no values, half steps, or raw = 1): the sum of squares (<= 700 x 25, in units of 0.25) and the target sum are
// exact in float32 in any order; sqrtf and the float32 division are correctly rounded on the device (hipcc's default; the Makefile's flags
// leave it on), so the host runs the same float32 expressions in the same order, without contraction, and every element is compared BIT
// FOR BIT (bf16: f32_to_bf16 of the mirror).  BOUNDED (real ratings, raw = 0): the device sums the squares in another order (per thread,
// 64-lane butterfly, 4 or 8 wave partials), so the image is judged against the same formula in float64.  With n item entries in the row
// every term meets at most n roundings on its way into the sum (its fma, then at most n - 1 additions of non-zero partners): n E24
// relative, halved by the square root: n / 2.  Then sqrt, the reciprocal, v * inv and the product with the scale (the scale itself is the
// same float32 number on both sides) add one E24 each, and second-order terms stay below one more: (n / 2 + 5) E24 relative.  bf16: the
// stored bits must lie between f32_to_bf16 of the interval's ends.  tsum: n - 1 additions, (n - 1) E24 sum|v|.  Zeros, the ones column,
// the condition columns, the padding and the dropped entries are exact in this regime too.
//
//   test_batch          the device run
//   test_batch --host   no HIP call: the generator's promises, the float32 mirror against the float64 formula under the bound, the
//                       refusals, and section S
#include "../../rectorch_amd/csrc/rtx_kernels.h"

#include "check.h"

#include <set>

#pragma clang fp contract(off)   // the host mirror: the float32 expressions of batch_rows.h as written, one rounding per operation

static const int N_ROWS = 40;
static const int FORCED[4] = {4095, 4096, 8191, 8192};
static const uint64_t SEED = 0x1234567800000000ull + 1234, OFFSET = (1ull << 33) + 5;
enum { V_NONE = 0, V_HALF = 1, V_REAL = 2 };

static double g_worst_bounded = 0;             // worst error / bound over the bounded float32 elements of the run
static long g_bounded_elems = 0;
static long g_c_differs = 0, g_c_compared = 0;   // section C, bounded regime: elements of k_in_chunks' image that differ from k_gather's

// ---- the matrix ----------------------------------------------------------------------------------------------------------------------
struct Csr {
    int I = 0, Iin = 0, longest = 0;
    bool has_val = false;
    std::vector<int64_t> indptr;
    std::vector<int32_t> idx;
    std::vector<float> val;
    float value(int64_t k) const { return has_val ? val[k] : 1.f; }
    int len(int64_t u) const { return (int)(indptr[u + 1] - indptr[u]); }
};

static int slot_of(int r, int variant) { return variant ? (r * 7 + 3) % N_ROWS : r; }   // variant 1: the same lengths on other rows
static int slot_len(int slot, Rng& r)
{
    static const int special[8] = {0, 1, 255, 256, 257, 700, 520, 20};
    const int drawn = r.i(2, 120);
    return slot < 8 ? special[slot] : drawn;
}
static bool slot_flagged(int slot) { return (slot >= 2 && slot <= 6) || slot % 3 == 2; }

static Csr gen_matrix(int I, int cond, int vk, uint32_t seed, int variant = 0)
{
    Rng r = {seed};
    Csr c;
    c.I = I; c.Iin = I + cond; c.has_val = vk != V_NONE;
    c.indptr.push_back(0);
    for (int row = 0; row < N_ROWS; ++row) {
        const int slot = slot_of(row, variant);
        const int want = std::min(slot_len(slot, r), I);
        const bool has_cond = cond > 0 && row % 3 != 0;
        std::vector<char> used(c.Iin, 0);
        std::vector<int32_t> items, conds;
        auto add_item = [&](int col) {
            if (col >= 0 && col < I && !used[col] && (int)items.size() < want) { used[col] = 1; items.push_back(col); }
        };
        if (slot_flagged(slot)) {
            add_item(0);
            add_item(I - 1);
            for (int f : FORCED) {
                if (f < I) add_item(f);
                else if (f < c.Iin && has_cond && !used[f]) { used[f] = 1; conds.push_back(f); }
            }
        }
        std::vector<int32_t> rest;
        for (int col = 0; col < I; ++col) if (!used[col]) rest.push_back(col);
        for (int k = 0; (int)items.size() < want; ++k) {   // distinct columns: a partial shuffle
            std::swap(rest[k], rest[k + r.below((int)rest.size() - k)]);
            items.push_back(rest[k]);
        }
        if (has_cond) {
            const int n = std::min(cond, std::max<int>(r.i(1, 3), (int)conds.size()));
            while ((int)conds.size() < n) {
                const int col = I + r.below(cond);
                if (!used[col]) { used[col] = 1; conds.push_back(col); }
            }
        }
        std::sort(items.begin(), items.end());
        std::sort(conds.begin(), conds.end());
        for (int32_t col : items) {
            c.idx.push_back(col);
            if (!c.has_val) continue;
            float v;
            if (vk == V_HALF) v = 0.5f * (1 + r.below(10));
            else {
                const float step = 0.3f * r.i(1, 16), any = (float)(r.f48() * 5.0);
                v = (r.u() & 1) ? step : any;
                if (v == 0.f) v = 0.3f;
            }
            c.val.push_back(slot == 7 ? 0.f : v);
        }
        for (int32_t col : conds) {
            c.idx.push_back(col);
            if (c.has_val) c.val.push_back(vk == V_HALF ? 1.5f + 0.5f * r.below(6) : 0.3f * r.i(2, 9));
        }
        c.indptr.push_back((int64_t)c.idx.size());
        c.longest = std::max(c.longest, (int)(items.size() + conds.size()));
    }
    return c;
}

// ---- a batch and its reference ---------------------------------------------------------------------------------------------------------
struct Batch {
    Csr in, tg;
    bool tg_is_in = true;
    int vk = 0, tvk = 0;
    std::vector<int32_t> ids;
    bool has_ids = false;
    int B = 0, Bp = 0, I = 0, Iin = 0, ldx = 0, raw = 0, training = 0;
    float p = 0.5f;
    std::vector<uint8_t> mask;
    bool has_mask = false;
    uint64_t seed = SEED, offset = OFFSET;
    const Csr& target() const { return tg_is_in ? in : tg; }
    int64_t row(int b) const { return has_ids ? ids[b] : b; }
    bool keep(int b, int i) const
    {
        const uint64_t e = (uint64_t)b * (uint64_t)I + (uint64_t)i;
        return has_mask ? mask[e] != 0 : rtx_dropout_keep(seed, offset, e, p);
    }
};

// ids_kind 0: rows 0 .. B - 1;  1: the special rows first (row 5 twice), then random rows;  2: short rows, then row 5 (700 entries) last
static std::vector<int32_t> make_ids(int B, int kind, Rng& r)
{
    static const int first[9] = {5, 0, 4, 5, 7, 1, 2, 3, 6};
    static const int long_last[5] = {1, 0, 8, 9, 5};
    std::vector<int32_t> ids(B);
    for (int b = 0; b < B; ++b) ids[b] = kind == 2 ? long_last[b % 5] : b < 9 ? first[b] : r.below(N_ROWS);
    return ids;
}

// the rows no batch row names: junk values (their columns are valid columns of the image already)
static void junk_unnamed(Batch& bt, Rng& r)
{
    std::vector<char> named(N_ROWS, 0);
    for (int b = 0; b < bt.B; ++b) named[bt.row(b)] = 1;
    for (Csr* c : {&bt.in, &bt.tg}) {
        if (!c->has_val) continue;
        for (int u = 0; u < N_ROWS; ++u)
            if (!named[u]) for (int64_t k = c->indptr[u]; k < c->indptr[u + 1]; ++k) c->val[k] = r.junk();
    }
}

static bool both_kept_and_dropped(const Batch& bt)
{
    for (int b = 0; b < bt.B; ++b) {
        const int64_t u = bt.row(b);
        int kept = 0, dropped = 0;
        for (int64_t k = bt.in.indptr[u]; k < bt.in.indptr[u + 1]; ++k)
            if (bt.in.idx[k] < bt.I) (bt.keep(b, bt.in.idx[k]) ? kept : dropped)++;
        if (kept + dropped > 8 && (!kept || !dropped)) return false;
    }
    return true;
}

static Batch make_batch(int I, int cond, int ldx, int vk, int raw, int training, float p, bool mask, int ids_kind, int B, int Bp,
                        bool other_target, uint32_t seed)
{
    Rng r = {seed * 2654435761u + 17};
    Batch bt;
    bt.in = gen_matrix(I, cond, vk, seed);
    bt.vk = bt.tvk = vk;
    if (other_target) {
        bt.tvk = vk == V_NONE ? V_HALF : vk;
        bt.tg = gen_matrix(I, cond, bt.tvk, seed + 1000, 1);
        bt.tg_is_in = false;
    }
    bt.has_ids = ids_kind != 0;
    if (bt.has_ids) bt.ids = make_ids(B, ids_kind, r);
    bt.B = B; bt.Bp = Bp; bt.I = I; bt.Iin = I + cond; bt.ldx = ldx; bt.raw = raw; bt.training = training; bt.p = p;
    if (mask) {
        bt.has_mask = true;
        bt.mask.resize((size_t)B * I);
        static const uint8_t kept[3] = {1, 2, 255};
        for (auto& m : bt.mask) m = r.below(10) < 4 ? 0 : kept[r.below(3)];
    }
    junk_unnamed(bt, r);
    return bt;
}

struct Ref {
    int B = 0, Bp = 0, I = 0, Iin = 0, ldx = 0;
    std::vector<float> m;        // the float32 mirror of batch_rows.h, [Bp][ldx]
    std::vector<double> x;       // the same formula in float64
    std::vector<double> rel;     // per row: the relative bound of its item columns; 0 = bit for bit against m
    std::vector<float> ts;       // tsum, mirror
    std::vector<double> ts64, ts_bnd;
    std::vector<int> nitem;
    long kept = 0, dropped = 0;
    double mirror_worst = 0;     // |m - x| / bound over the bounded elements (--host)
    double ts_mirror_worst = 0;
};

static Ref build_ref(const Batch& bt)
{
    Ref R;
    R.B = bt.B; R.Bp = bt.Bp; R.I = bt.I; R.Iin = bt.Iin; R.ldx = bt.ldx;
    const size_t n = (size_t)bt.Bp * bt.ldx;
    R.m.assign(n, 0.f); R.x.assign(n, 0.0);
    R.rel.assign(bt.Bp, 0.0); R.ts.assign(bt.Bp, 0.f); R.ts64.assign(bt.Bp, 0.0); R.ts_bnd.assign(bt.Bp, 0.0); R.nitem.assign(bt.Bp, 0);
    const bool cond = bt.Iin > bt.I;
    const bool drop = bt.training && bt.p > 0.f;
    const float scale = drop ? (bt.p < 1.f ? 1.f / (1.f - bt.p) : 0.f) : 1.f;
    for (int b = 0; b < bt.B; ++b) {
        const Csr& c = bt.in;
        const int64_t u = bt.row(b), beg = c.indptr[u], end = c.indptr[u + 1];
        float ss = 0.f;
        double ss64 = 0.0;
        int nitem = 0;
        for (int64_t k = beg; k < end; ++k) {
            if (c.idx[k] >= bt.I) continue;
            const float v = c.value(k);
            ss += v * v;
            ss64 += (double)v * (double)v;
            ++nitem;
        }
        if (!c.has_val && !cond) ss = (float)(end - beg);
        R.nitem[b] = nitem;
        const float inv = bt.raw ? 1.f : 1.f / fmaxf(sqrtf(ss), 1e-12f);
        const double inv64 = bt.raw ? 1.0 : 1.0 / std::max(sqrt(ss64), (double)1e-12f);
        if (bt.vk == V_REAL && !bt.raw) R.rel[b] = (0.5 * nitem + 5.0) * E24;
        for (int64_t k = beg; k < end; ++k) {
            const int i = c.idx[k];
            float v = c.value(k);
            double v64 = v;
            if (i < bt.I) { v *= inv; v64 *= inv64; }
            if (drop && i < bt.I) {
                const bool keep = bt.keep(b, i);
                v = keep ? v * scale : 0.f;
                v64 = keep ? v64 * (double)scale : 0.0;
                (keep ? R.kept : R.dropped)++;
            }
            const size_t at = (size_t)b * bt.ldx + i;
            R.m[at] = v; R.x[at] = v64;
            if (R.rel[b] > 0 && v64 != 0) R.mirror_worst = std::max(R.mirror_worst, fabs((double)v - v64) / (R.rel[b] * fabs(v64)));
        }
        R.m[(size_t)b * bt.ldx + bt.Iin] = 1.f; R.x[(size_t)b * bt.ldx + bt.Iin] = 1.0;
        // the target row's sum over the item columns
        const Csr& t = bt.target();
        const int64_t tb = t.indptr[u], te = t.indptr[u + 1];
        float ts = 0.f;
        double ts64 = 0.0, tabs = 0.0;
        int nt = 0;
        for (int64_t k = tb; k < te; ++k) {
            if (t.idx[k] >= bt.I) continue;
            ts += t.value(k); ts64 += (double)t.value(k); tabs += fabs((double)t.value(k)); ++nt;
        }
        if (!t.has_val && !cond) ts = (float)(te - tb);
        R.ts[b] = ts; R.ts64[b] = ts64;
        if (bt.tvk == V_REAL && nt > 1) {
            R.ts_bnd[b] = (nt - 1) * E24 * tabs;
            R.ts_mirror_worst = std::max(R.ts_mirror_worst, fabs((double)ts - ts64) / R.ts_bnd[b]);
        }
    }
    return R;
}

// ---- the judging (the device run and section S share it) -------------------------------------------------------------------------------
static uint32_t elem_bits(float v, bool bf) { return bf ? (uint32_t)f32_to_bf16(v) : f_bits(v); }

// every element of the image: bit for bit against the mirror in an exact row, at a zero and beyond the item columns; an item column of a
// bounded row against the float64 formula (float32), or between the roundings of the interval's ends (bf16)
static void judge_image(const Ref& R, const std::vector<uint32_t>& got, bool bf, Line& L, const char* what = "X")
{
    for (int b = 0; b < R.Bp; ++b)
        for (int i = 0; i < R.ldx; ++i) {
            const size_t at = (size_t)b * R.ldx + i;
            const double x = R.x[at], rel = R.rel[b];
            if (rel == 0 || x == 0 || i >= R.I) { judge_bits(got[at], elem_bits(R.m[at], bf), L, what, b, i); continue; }
            if (!bf) {
                const double ratio = judge((double)bits_f(got[at]), x, rel * fabs(x), L, what, b, i);
                g_worst_bounded = std::max(g_worst_bounded, ratio);
                ++g_bounded_elems;
                continue;
            }
            double lo = x - rel * fabs(x), hi = x + rel * fabs(x);
            float flo = (float)lo, fhi = (float)hi;
            if ((double)flo < lo) flo = nextafterf(flo, INFINITY);    // the float32 values inside the interval
            if ((double)fhi > hi) fhi = nextafterf(fhi, -INFINITY);
            const float g = bf16_to_f32((bf16_t)got[at]);
            if (!(g >= bf16_to_f32(f32_to_bf16(flo)) && g <= bf16_to_f32(f32_to_bf16(fhi)))) {
                if (L.bad < 4) printf("    %s holds bf16 %04x = %.9g, expected the rounding of [%.9g, %.9g]\n", where(what, b, i).c_str(), got[at], g, lo, hi);
                ++L.bad;
            }
        }
}
static void judge_tsum(const Ref& R, const std::vector<float>& got, Line& L)
{
    for (int b = 0; b < R.Bp; ++b) {
        if (R.ts_bnd[b] == 0) judge_bits(f_bits(got[b]), f_bits(R.ts[b]), L, "tsum", b);
        else judge(got[b], R.ts64[b], R.ts_bnd[b], L, "tsum", b);
    }
}
// the scatter form's lists: n_written = len + 1 (0 in a padding slot), the listed columns = the row's columns and Iin, and nothing
// changed behind them (`before` = the lists as they were before the launch)
static void judge_lists(const Batch& bt, int cap, const std::vector<int32_t>& n_written, const std::vector<int32_t>& written,
                        const std::vector<int32_t>& before, Line& L)
{
    for (int b = 0; b < bt.Bp; ++b) {
        std::vector<int32_t> want;
        if (b < bt.B) {
            const int64_t u = bt.row(b);
            want.assign(bt.in.idx.begin() + bt.in.indptr[u], bt.in.idx.begin() + bt.in.indptr[u + 1]);
            want.push_back(bt.Iin);
            std::sort(want.begin(), want.end());
        }
        const int n = n_written[b];
        if (n != (int)want.size()) { host_fail(L, "n_written[%.0f] = %.0f", b, n); continue; }
        std::vector<int32_t> have(written.begin() + (size_t)b * cap, written.begin() + (size_t)b * cap + n);
        std::sort(have.begin(), have.end());
        if (have != want) host_fail(L, "written[%.0f]: not the row's columns and Iin", b);
        for (int k = n; k < cap; ++k)
            if (written[(size_t)b * cap + k] != before[(size_t)b * cap + k]) { host_fail(L, "written[%.0f][%.0f] changed behind the list", b, k); break; }
    }
}
// chunks of every user of the batch
static std::vector<int> user_chunks(const Batch& bt)
{
    std::vector<int> n(bt.B);
    for (int b = 0; b < bt.B; ++b) n[b] = std::max(1, (bt.in.len(bt.row(b)) + 63) / 64);
    return n;
}
// the 16-way split: ends, monotone, every entry the first chunk of a user or the total, and the rule of the kernel's comment
static void judge_split(const std::vector<int>& nch, const int32_t* ws, Line& L)
{
    std::vector<long> first(nch.size() + 1, 0);
    for (size_t b = 0; b < nch.size(); ++b) first[b + 1] = first[b] + nch[b];
    const long total = first.back();
    std::set<long> starts(first.begin(), first.end());
    if (ws[0] != 0) host_fail(L, "wsplit[0] = %.0f", ws[0]);
    if (ws[RTX_SPMM_WAVES] != total) host_fail(L, "wsplit[16] = %.0f, expected %.0f", ws[RTX_SPMM_WAVES], (double)total);
    for (int w = 0; w <= RTX_SPMM_WAVES; ++w) {
        if (w && ws[w] < ws[w - 1]) host_fail(L, "wsplit[%.0f] = %.0f: not monotone", w, ws[w]);
        if (!starts.count(ws[w])) host_fail(L, "wsplit[%.0f] = %.0f: inside a user", w, ws[w]);
        long want = total;
        for (size_t b = 0; b < nch.size(); ++b)
            if (first[b] * RTX_SPMM_WAVES >= total * w) { want = first[b]; break; }
        if (ws[w] != want) host_fail(L, "wsplit[%.0f] = %.0f: not the first user at or past total * w / 16", w, ws[w]);
    }
}
// the chunk stream against the image of the same launch
static void judge_stream(const Batch& bt, const std::vector<uint32_t>& img, const std::vector<uint32_t>& ent, const std::vector<int32_t>& desc, Line& L)
{
    const std::vector<int> nch = user_chunks(bt);
    long c0 = 0;
    for (int b = 0; b < bt.B; ++b) {
        const int64_t u = bt.row(b), beg = bt.in.indptr[u];
        const int len = bt.in.len(u);
        for (int c = 0; c < nch[b]; ++c)
            if (desc[c0 + c] != b) host_fail(L, "desc[%.0f] = %.0f", (double)(c0 + c), desc[c0 + c]);
        for (int t = 0; t < nch[b] * 64; ++t) {
            uint32_t want = 0;
            if (t < len) { const uint32_t i = bt.in.idx[beg + t]; want = i | (img[(size_t)b * bt.ldx + i] << 16); }
            judge_bits(ent[(size_t)c0 * 64 + t], want, L, "ent", b, t);
        }
        c0 += nch[b];
    }
    if (desc[c0] != -1) host_fail(L, "desc[total] = %.0f", desc[c0]);
}

// ---- the device side -------------------------------------------------------------------------------------------------------------------
struct DevBatch {
    RtxCsrView in, tg;
    const uint8_t* mask;
};
static DevBatch upload(const Batch& bt)
{
    DevBatch d;
    const int32_t* ids = bt.has_ids ? to_dev(bt.ids) : nullptr;
    auto view = [&](const Csr& c) {
        RtxCsrView v = {};
        v.indptr = to_dev(c.indptr); v.indices = to_dev(c.idx); v.values = c.has_val ? to_dev(c.val) : nullptr;
        v.row_ids = ids; v.max_row_len = c.longest; v.avg_row_len = std::max<int>(1, (int)(c.idx.size() / N_ROWS));
        return v;
    };
    d.in = view(bt.in);
    d.tg = bt.tg_is_in ? d.in : view(bt.tg);
    d.mask = bt.has_mask ? to_dev(bt.mask) : nullptr;
    return d;
}
static RtxGatherArgs gather_args(const Batch& bt, const DevBatch& d, void* X, float* tsum)
{
    RtxGatherArgs a = {};
    a.in = d.in; a.target = d.tg; a.B = bt.B; a.Bp = bt.Bp; a.I = bt.I; a.ldx = bt.ldx; a.Iin = bt.Iin; a.raw = bt.raw; a.X = X; a.tsum = tsum;
    a.training = bt.training; a.dropout_p = bt.p; a.mask = d.mask; a.seed = bt.seed; a.offset = bt.offset;
    return a;
}
static std::vector<uint32_t> fetch_bits(const void* d, size_t n, bool bf, Line& L, const char* what)
{
    std::vector<uint32_t> o(n);
    if (bf) { const std::vector<bf16_t> h = fetch<bf16_t>(d, n, L, what); for (size_t i = 0; i < n; ++i) o[i] = h[i]; }
    else { const std::vector<float> h = fetch<float>(d, n, L, what); for (size_t i = 0; i < n; ++i) o[i] = f_bits(h[i]); }
    return o;
}
static void* image_out(size_t n, bool bf) { return bf ? (void*)dev_out<bf16_t>(n) : (void*)dev_out<float>(n); }
// a fresh full-rewrite k_gather launch of the batch: image bits and tsum
static void run_gather(const Batch& bt, const DevBatch& d, bool bf, Line& L, std::vector<uint32_t>& img, std::vector<float>& ts)
{
    const size_t n = (size_t)bt.Bp * bt.ldx;
    void* X = image_out(n, bf);
    float* tsum = dev_out<float>(bt.Bp);
    RT(rtx_launch_gather(gather_args(bt, d, X, tsum), bf, 0));
    CK(hipDeviceSynchronize());
    img = fetch_bits(X, n, bf, L, "X");
    ts = fetch<float>(tsum, bt.Bp, L, "tsum");
}
static void equal_bits(const std::vector<uint32_t>& got, const std::vector<uint32_t>& want, int ld, Line& L, const char* what)
{
    for (size_t k = 0; k < want.size(); ++k) judge_bits(got[k], want[k], L, what, (long)(k / ld), (long)(k % ld));
}
static std::vector<uint32_t> bits_of(const std::vector<float>& v)
{
    std::vector<uint32_t> o(v.size());
    for (size_t k = 0; k < v.size(); ++k) o[k] = f_bits(v[k]);
    return o;
}

// ---- the generator's promises (--host) --------------------------------------------------------------------------------------------------
static void check_matrix(const Csr& c, int vk, int cond, int variant, const std::vector<char>& named, Line& L)
{
    static const int special[7] = {0, 1, 255, 256, 257, 700, 520};
    std::set<int> seen;
    int with_cond = 0;
    for (int u = 0; u < N_ROWS; ++u) {
        const int slot = slot_of(u, variant);
        std::set<int> cols;
        int nc = 0, items = 0;
        float fwd = 0.f, bwd = 0.f, tf = 0.f, tb = 0.f;   // the sum of squares and the target sum, forwards and backwards
        double s64 = 0.0, t64 = 0.0;
        for (int64_t k = c.indptr[u]; k < c.indptr[u + 1]; ++k) {
            if (c.idx[k] < 0 || c.idx[k] >= c.Iin || !cols.insert(c.idx[k]).second) host_fail(L, "row %.0f: column %.0f out of range or twice", u, c.idx[k]);
            seen.insert(c.idx[k]);
            const float v = c.value(k);
            if (!named[u]) {   // a row no batch row names: junk at valid columns
                nc += c.idx[k] >= c.I; items += c.idx[k] < c.I;
                if (c.has_val && !is_junk(v)) host_fail(L, "row %.0f is not named and holds %.9g", u, v);
                continue;
            }
            if (c.idx[k] >= c.I) { ++nc; if (c.has_val && v == 1.f) host_fail(L, "row %.0f: a condition value of 1", u); continue; }
            ++items;
            fwd += v * v; s64 += (double)v * (double)v;
            tf += v; t64 += (double)v;
            if (slot == 7 && c.has_val && v != 0.f) host_fail(L, "the zero row %.0f holds %.9g", u, v);
            if (slot != 7 && v == 0.f) host_fail(L, "row %.0f holds a zero", u);
        }
        for (int64_t k = c.indptr[u + 1] - 1; k >= c.indptr[u]; --k)
            if (named[u] && c.idx[k] < c.I) { bwd += c.value(k) * c.value(k); tb += c.value(k); }
        if (vk != V_REAL && (fwd != bwd || (double)fwd != s64)) host_fail(L, "row %.0f: the sum of squares is not exact in float32", u);
        if (vk != V_REAL && (tf != tb || (double)tf != t64)) host_fail(L, "row %.0f: the sum of the values is not exact in float32", u);
        if (slot < 7 && items != std::min(special[slot], c.I)) host_fail(L, "row %.0f holds %.0f item entries", u, items);
        if (nc > 3) host_fail(L, "row %.0f: %.0f condition columns", u, nc);
        with_cond += nc > 0;
    }
    if (cond && with_cond != N_ROWS - (N_ROWS + 2) / 3) host_fail(L, "%.0f rows with condition columns", with_cond);
    if (!cond && with_cond) host_fail(L, "condition columns without cond");
    for (int f : {0, c.I - 1, FORCED[0], FORCED[1], FORCED[2], FORCED[3]})
        if (f < c.Iin && !seen.count(f)) host_fail(L, "no row holds column %.0f", f);
}

// ---- section A -------------------------------------------------------------------------------------------------------------------------
static const int SHAPE[2][5][3] = {{{300, 0, 304}, {4000, 0, 4096}, {4095, 0, 4224}, {4096, 0, 4224}, {4090, 16, 4224}},
                                   {{300, 0, 304}, {8000, 0, 8192}, {8191, 0, 8320}, {8192, 0, 8320}, {8180, 16, 8320}}};
struct ACase {
    const char* name;
    int shape, vk, raw, training;
    float p;
    int mask, ids, B, Bp, other, need_both;
};
static const ACase A_CASES[] = {
    {"a1 none eval", 0, V_NONE, 0, 0, 0.5f, 0, 0, 5, 8, 0, 0},
    {"a2 half train p=0.5 ids target=other", 0, V_HALF, 0, 1, 0.5f, 0, 1, 5, 8, 1, 0},
    {"a3 real train p=0.3 ids", 0, V_REAL, 0, 1, 0.3f, 0, 1, 8, 8, 0, 0},
    {"a4 half train p=1.0", 1, V_HALF, 0, 1, 1.0f, 0, 0, 8, 8, 0, 0},
    {"a5 none raw eval ids 130/256", 1, V_NONE, 1, 0, 0.5f, 0, 1, 130, 256, 0, 0},
    {"a6 real raw train p=0.3 ids", 1, V_REAL, 1, 1, 0.3f, 0, 1, 5, 8, 0, 0},
    {"a7 none train p=0.5 ids", 2, V_NONE, 0, 1, 0.5f, 0, 1, 5, 8, 0, 0},
    {"a8 real eval 40/40", 2, V_REAL, 0, 0, 0.5f, 0, 0, 40, 40, 0, 0},
    {"a9 half train p=0.3 ids 130/256 kept+dropped", 3, V_HALF, 0, 1, 0.3f, 0, 1, 130, 256, 0, 1},
    {"a10 real train p=0.5 target=other", 3, V_REAL, 0, 1, 0.5f, 0, 0, 8, 8, 1, 0},
    {"a11 half train p=0.5 mask ids", 4, V_HALF, 0, 1, 0.5f, 1, 1, 5, 8, 0, 0},
    {"a12 real train p=0.3 mask 40/40 target=other", 4, V_REAL, 0, 1, 0.3f, 1, 0, 40, 40, 1, 0},
    {"a13 none+cond eval ids", 4, V_NONE, 0, 0, 0.5f, 0, 1, 5, 8, 0, 0},
    {"a14 half raw train p=0.5 ids 130/256 target=other", 4, V_HALF, 1, 1, 0.5f, 0, 1, 130, 256, 1, 0},
    {"a15 real raw eval", 4, V_REAL, 1, 0, 0.5f, 0, 0, 8, 8, 0, 0},
};

static Batch a_batch(const ACase& c, int bf, uint32_t seed)
{
    const int* s = SHAPE[bf][c.shape];
    Batch bt = make_batch(s[0], s[1], s[2], c.vk, c.raw, c.training, c.p, c.mask, c.ids, c.B, c.Bp, c.other, seed);
    for (int t = 0; c.need_both && t < 200 && !both_kept_and_dropped(bt); ++t) ++bt.offset;   // an offset at which every longer row shows both
    return bt;
}
static const char* regime(const Ref& R)
{
    for (double r : R.rel) if (r > 0) return "  [bounded]";
    return "  [bit for bit]";
}
// --host: what the reference and the generator promise for this batch
static std::vector<char> named_rows(const Batch& bt)
{
    std::vector<char> named(N_ROWS, 0);
    for (int b = 0; b < bt.B; ++b) named[bt.row(b)] = 1;
    return named;
}
static void host_checks(const Batch& bt, const Ref& R, Line& L, bool need_both, bool expect_twice)
{
    check_matrix(bt.in, bt.vk, bt.Iin - bt.I, 0, named_rows(bt), L);
    if (!bt.tg_is_in) check_matrix(bt.tg, bt.tvk, bt.Iin - bt.I, 1, named_rows(bt), L);
    if (bt.training && bt.p > 0.f && bt.p < 1.f && (!R.kept || !R.dropped)) host_fail(L, "kept %.0f, dropped %.0f", (double)R.kept, (double)R.dropped);
    if (bt.training && bt.p >= 1.f && R.kept) host_fail(L, "p = 1 keeps %.0f entries", (double)R.kept);
    if (need_both && !both_kept_and_dropped(bt)) host_fail(L, "a row longer than 8 without a kept or without a dropped entry");
    if (expect_twice) {
        std::set<int32_t> s(bt.ids.begin(), bt.ids.end());
        if (s.size() == bt.ids.size()) host_fail(L, "no row is named twice");
    }
    L.worst = std::max(R.mirror_worst, R.ts_mirror_worst);   // the float32 mirror against the float64 formula, of the derived bound
    if (!(L.worst <= 1.0)) host_fail(L, "the float32 mirror leaves the bound: %.3f", L.worst);
}

static void section_a()
{
    printf("== A: rtx_launch_gather, full rewrite ==\n");
    for (int bf = 0; bf < 2; ++bf)
        for (size_t ci = 0; ci < sizeof A_CASES / sizeof A_CASES[0]; ++ci) {
            const ACase& c = A_CASES[ci];
            const Batch bt = a_batch(c, bf, 100 + (uint32_t)ci);
            const Ref R = build_ref(bt);
            char name[160];
            snprintf(name, sizeof name, "A %s %s I=%d+%d ldx=%d", bf ? "bf16" : "f32", c.name, bt.I, bt.Iin - bt.I, bt.ldx);
            g_tag = name;
            Line L;
            if (g_host) { host_checks(bt, R, L, c.need_both, c.ids == 1); report(name, L, regime(R)); continue; }
            const size_t mark = pool_size();
            const DevBatch d = upload(bt);
            std::vector<uint32_t> img;
            std::vector<float> ts;
            run_gather(bt, d, bf, L, img, ts);
            judge_image(R, img, bf, L);
            judge_tsum(R, ts, L);
            report(name, L, regime(R));
            free_from(mark);
        }
}

// ---- section B -------------------------------------------------------------------------------------------------------------------------
static void section_b()
{
    printf("== B: rtx_launch_gather, scatter form ==\n");
    static const int32_t IDS[5][8] = {{5, 4, 3, 2, 6, 8, 9, 10}, {11, 0, 1, 12, 7}, {12, 11, 5, 5, 0, 13, 2, 1}, {2, 3, 4, 13, 14, 0, 6, 1}, {5, 4, 3, 2, 6, 8, 9, 10}};
    static const int NB[5] = {8, 5, 8, 8, 8};
    static const char* WHAT[5] = {"1 long rows", "2 others, B=5 of 8", "3 a user in another slot", "4 training p=0.5", "5 launch 1 again"};
    for (int bf = 0; bf < 2; ++bf)
        for (int seq = 0; seq < 2; ++seq) {
            const int I = seq ? 4096 : SHAPE[bf][4][0], cond = seq ? 0 : 16, ldx = seq ? 4224 : SHAPE[bf][4][2], vk = seq ? V_HALF : V_REAL;
            const int Bp = 8;
            const size_t mark = pool_size();
            const Csr m = gen_matrix(I, cond, vk, 500 + seq);
            const int cap = m.longest + 2;
            void* X = nullptr;
            int32_t *written = nullptr, *n_written = nullptr;
            if (!g_host) {   // zeroed once, as gather_batch does; the guards stay poisoned
                X = image_out((size_t)Bp * ldx, bf);
                CK(hipMemset(X, 0, (size_t)Bp * ldx * (bf ? 2 : 4)));
                written = dev_out<int32_t>((size_t)Bp * cap);
                CK(hipMemset(written, 0, (size_t)Bp * cap * 4));
                n_written = dev_out<int32_t>(Bp);
                CK(hipMemset(n_written, 0, Bp * 4));
            }
            std::vector<int32_t> before((size_t)Bp * cap, 0);
            for (int l = 0; l < 5; ++l) {
                Batch bt;
                bt.in = m; bt.vk = bt.tvk = vk;
                bt.has_ids = true; bt.ids.assign(IDS[l], IDS[l] + NB[l]);
                bt.B = NB[l]; bt.Bp = Bp; bt.I = I; bt.Iin = I + cond; bt.ldx = ldx; bt.training = l == 3; bt.p = 0.5f;
                Rng r = {900u + l};
                junk_unnamed(bt, r);
                const Ref R = build_ref(bt);
                char name[160];
                snprintf(name, sizeof name, "B %s I=%d+%d ldx=%d launch %s", bf ? "bf16" : "f32", I, cond, ldx, WHAT[l]);
                g_tag = name;
                Line L;
                if (g_host) { host_checks(bt, R, L, false, l == 2); report(name, L, regime(R)); continue; }
                const size_t inner = pool_size();
                const DevBatch d = upload(bt);
                std::vector<uint32_t> fresh;
                std::vector<float> fresh_ts;
                run_gather(bt, d, bf, L, fresh, fresh_ts);
                float* tsum = dev_out<float>(Bp);
                RtxGatherArgs a = gather_args(bt, d, X, tsum);
                a.written = written; a.n_written = n_written; a.written_cap = cap;
                RT(rtx_launch_gather(a, bf, 0));
                CK(hipDeviceSynchronize());
                const std::vector<uint32_t> img = fetch_bits(X, (size_t)Bp * ldx, bf, L, "X");
                const std::vector<float> ts = fetch<float>(tsum, Bp, L, "tsum");
                const std::vector<int32_t> nw = fetch<int32_t>(n_written, Bp, L, "n_written");
                const std::vector<int32_t> wr = fetch<int32_t>(written, (size_t)Bp * cap, L, "written");
                equal_bits(img, fresh, ldx, L, "X (scatter against k_gather)");
                equal_bits(bits_of(ts), bits_of(fresh_ts), 1, L, "tsum (scatter against k_gather)");
                judge_image(R, img, bf, L);
                judge_tsum(R, ts, L);
                judge_lists(bt, cap, nw, wr, before, L);
                before = wr;
                report(name, L, regime(R));
                free_from(inner);
            }
            free_from(mark);
        }
}

// ---- section C -------------------------------------------------------------------------------------------------------------------------
static const int C_SHAPE[4][3] = {{300, 0, 304}, {8191, 0, 8320}, {8192, 0, 8320}, {8180, 16, 8320}};
struct CCase {
    const char* name;
    int shape, vk, training;
    float p;
    int mask, ids, B, Bp, other;
};
static const CCase C_CASES[] = {
    {"c1 none eval ids", 0, V_NONE, 0, 0.5f, 0, 1, 5, 8, 0},
    {"c2 real train p=0.3 ids B=1", 0, V_REAL, 1, 0.3f, 0, 1, 1, 8, 0},
    {"c3 half train p=0.5 ids 130/256 target=other", 1, V_HALF, 1, 0.5f, 0, 1, 130, 256, 1},
    {"c4 real eval 40/40", 1, V_REAL, 0, 0.5f, 0, 0, 40, 40, 0},
    {"c5 none train p=0.5 long last user", 2, V_NONE, 1, 0.5f, 0, 2, 5, 8, 0},
    {"c6 real train p=0.3 ids 130/256", 2, V_REAL, 1, 0.3f, 0, 1, 130, 256, 0},
    {"c7 half train p=0.5 mask ids", 3, V_HALF, 1, 0.5f, 1, 1, 5, 8, 0},
    {"c8 real train p=0.3 mask 40/48", 3, V_REAL, 1, 0.3f, 1, 0, 40, 48, 0},
    {"c9 real eval long last user", 3, V_REAL, 0, 0.5f, 0, 2, 5, 8, 0},
};
static RtxInChunksArgs chunk_args(const Batch& bt, const DevBatch& d, uint32_t* ent, int32_t* desc, int32_t* wsplit, int64_t cap, bf16_t* X, float* tsum)
{
    RtxInChunksArgs a = {};
    a.in = d.in; a.B = bt.B; a.I = bt.I; a.Iin = bt.Iin; a.training = bt.training; a.dropout_p = bt.p; a.mask = d.mask; a.seed = bt.seed;
    a.offset = bt.offset; a.ent = ent; a.desc = desc; a.wsplit = wsplit; a.cap_chunks = cap;
    if (X) { a.target = d.tg; a.tsum = tsum; a.X = X; a.ldx = bt.ldx; a.Bp = bt.Bp; }
    return a;
}
static void all_poison(const void* d, size_t bytes, Line& L, const char* what)
{
    const std::vector<unsigned char> h = to_host((const unsigned char*)d, bytes);
    size_t k = 0;
    if (!guard_intact(h.data(), bytes, &k)) { if (L.bad < 4) printf("    %s %s: byte %zu was written by a refused launch\n", g_tag.c_str(), what, k); ++L.bad; }
}

static void section_c()
{
    printf("== C: rtx_launch_in_chunks ==\n");
    for (size_t ci = 0; ci < sizeof C_CASES / sizeof C_CASES[0]; ++ci) {
        const CCase& c = C_CASES[ci];
        const int* s = C_SHAPE[c.shape];
        const Batch bt = make_batch(s[0], s[1], s[2], c.vk, 0, c.training, c.p, c.mask, c.ids, c.B, c.Bp, c.other, 300 + (uint32_t)ci);
        const Ref R = build_ref(bt);
        const std::vector<int> nch = user_chunks(bt);
        int total = 0;
        for (int n : nch) total += n;
        char name[160];
        snprintf(name, sizeof name, "C %s I=%d+%d ldx=%d chunks=%d", c.name, bt.I, bt.Iin - bt.I, bt.ldx, total);
        g_tag = name;
        Line L;
        if (g_host) {
            host_checks(bt, R, L, false, c.ids == 1 && c.B > 1);
            if (c.ids == 2 && !(nch.back() * RTX_SPMM_WAVES > total)) host_fail(L, "the last user is not longer than a part");
            report(name, L, regime(R));
            continue;
        }
        const size_t mark = pool_size();
        const DevBatch d = upload(bt);
        std::vector<uint32_t> gimg;
        std::vector<float> gts;
        run_gather(bt, d, true, L, gimg, gts);
        const size_t n = (size_t)bt.Bp * bt.ldx;
        // with X
        bf16_t* X = dev_out<bf16_t>(n);
        float* tsum = dev_out<float>(bt.Bp);
        uint32_t* ent = dev_out<uint32_t>((size_t)total * 64);
        int32_t* desc = dev_out<int32_t>(total + 1);
        int32_t* wsplit = dev_out<int32_t>(RTX_SPMM_WAVES + 1);
        RT(rtx_launch_in_chunks(chunk_args(bt, d, ent, desc, wsplit, total + 1, X, tsum), 0));
        CK(hipDeviceSynchronize());
        const std::vector<uint32_t> img = fetch_bits(X, n, true, L, "X");
        const std::vector<float> ts = fetch<float>(tsum, bt.Bp, L, "tsum");
        const std::vector<uint32_t> e1 = fetch<uint32_t>(ent, (size_t)total * 64, L, "ent");
        const std::vector<int32_t> d1 = fetch<int32_t>(desc, total + 1, L, "desc");
        const std::vector<int32_t> w1 = fetch<int32_t>(wsplit, RTX_SPMM_WAVES + 1, L, "wsplit");
        judge_image(R, img, true, L);
        judge_tsum(R, ts, L);
        char extra[96] = "";
        if (c.vk == V_REAL) {   // another reduction width than k_gather's: the same bound, and how often the two images differ
            long differs = 0;
            for (size_t k = 0; k < n; ++k) differs += img[k] != gimg[k];
            g_c_differs += differs; g_c_compared += (long)n;
            snprintf(extra, sizeof extra, "  [bounded; %ld elements differ from k_gather<bf16>]", differs);
        } else {
            equal_bits(img, gimg, bt.ldx, L, "X (k_in_chunks against k_gather)");
            equal_bits(bits_of(ts), bits_of(gts), 1, L, "tsum (k_in_chunks against k_gather)");
            snprintf(extra, sizeof extra, "  [bit for bit]");
        }
        judge_stream(bt, img, e1, d1, L);
        judge_split(nch, w1.data(), L);
        // without X: the same stream
        uint32_t* ent2 = dev_out<uint32_t>((size_t)total * 64);
        int32_t* desc2 = dev_out<int32_t>(total + 1);
        int32_t* wsplit2 = dev_out<int32_t>(RTX_SPMM_WAVES + 1);
        RT(rtx_launch_in_chunks(chunk_args(bt, d, ent2, desc2, wsplit2, total + 1, nullptr, nullptr), 0));
        CK(hipDeviceSynchronize());
        equal_bits(fetch<uint32_t>(ent2, (size_t)total * 64, L, "ent"), e1, 64, L, "ent (X null)");
        const std::vector<int32_t> d2 = fetch<int32_t>(desc2, total + 1, L, "desc"), w2 = fetch<int32_t>(wsplit2, RTX_SPMM_WAVES + 1, L, "wsplit");
        if (d2 != d1) host_fail(L, "desc differs without X");
        if (w2 != w1) host_fail(L, "wsplit differs without X");
        // one chunk too few: nothing of the stream, of the real rows of X or of their tsum is written
        repoison(X, n); repoison(tsum, bt.Bp); repoison(ent, (size_t)total * 64); repoison(desc, total + 1); repoison(wsplit, RTX_SPMM_WAVES + 1);
        RT(rtx_launch_in_chunks(chunk_args(bt, d, ent, desc, wsplit, total, X, tsum), 0));
        CK(hipDeviceSynchronize());
        all_poison(ent, ((size_t)total * 64 + GUARD) * 4, L, "ent");
        all_poison(desc, (size_t)(total + 1 + GUARD) * 4, L, "desc");
        all_poison(wsplit, (RTX_SPMM_WAVES + 1 + GUARD) * 4, L, "wsplit");
        all_poison(X, (size_t)bt.B * bt.ldx * 2, L, "X (real rows)");
        all_poison(tsum, (size_t)bt.B * 4, L, "tsum (real rows)");
        report(name, L, extra);
        free_from(mark);
    }
}

// ---- section D -------------------------------------------------------------------------------------------------------------------------
static void section_d()
{
    printf("== D: rtx_launch_csr_to_dense ==\n");
    static const int WIDTHS[7] = {1, 7, 301, 4095, 4096, 4097, 8200};
    for (int I : WIDTHS)
        for (int combo = 0; combo < 4; ++combo) {
            const bool values = combo & 1, ids = combo & 2;
            const int B = ids ? 9 : N_ROWS;
            Batch bt = make_batch(I, 0, I, values ? V_REAL : V_NONE, 1, 0, 0.5f, false, ids ? 1 : 0, B, B, false, 700 + I + combo);
            char name[160];
            snprintf(name, sizeof name, "D I=%d values=%d row_ids=%d B=%d", I, (int)values, (int)ids, B);
            g_tag = name;
            Line L;
            std::vector<float> want((size_t)B * I, 0.f);
            int empty = 0;
            for (int b = 0; b < B; ++b) {
                const int64_t u = bt.row(b);
                empty += bt.in.len(u) == 0;
                for (int64_t k = bt.in.indptr[u]; k < bt.in.indptr[u + 1]; ++k) want[(size_t)b * I + bt.in.idx[k]] = bt.in.value(k);
            }
            if (!empty) host_fail(L, "no empty row");
            if (g_host) { check_matrix(bt.in, bt.vk, 0, 0, named_rows(bt), L); report(name, L, "  [bit for bit]"); continue; }
            const size_t mark = pool_size();
            const DevBatch d = upload(bt);
            float* out = dev_out<float>((size_t)B * I);
            RT(rtx_launch_csr_to_dense(d.in, B, I, out, 0));
            CK(hipDeviceSynchronize());
            equal_bits(bits_of(fetch<float>(out, (size_t)B * I, L, "out")), bits_of(want), I, L, "out");
            report(name, L, "  [bit for bit]");
            free_from(mark);
        }
}

// ---- section E -------------------------------------------------------------------------------------------------------------------------
static std::vector<float> e_dense(int I, int B, Rng& r)
{
    const float specials[5] = {-0.0f, bits_f(0x00000001u), INFINITY, -INFINITY, NAN};   // -0.0 is not stored; the others are
    std::vector<float> x((size_t)B * I, 0.f);
    const int last_block = ((I - 1) / 256) * 256;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < I; ++i) {
            float v = 0.f;
            const float any = r.f() == 0.f ? 0.25f : r.f();
            switch (b) {
            case 0: break;
            case 1: v = any == 0.f ? 1.f : any; break;
            case 2: v = (i & 1) ? 0.f : 1.5f; break;
            case 3: v = i >= last_block ? 2.f + i : 0.f; break;
            case 4: v = specials[i % 5]; break;
            default: {
                const int q = r.below(8);
                v = q < 5 ? 0.f : q == 5 ? specials[r.below(5)] : any;
            }
            }
            x[(size_t)b * I + i] = v;
        }
    if (I == 1) for (int b = 4; b < B; ++b) x[b] = specials[b - 4];   // one column: one special per row
    return x;
}

static void section_e()
{
    printf("== E: dense -> CSR ==\n");
    static const int WIDTHS[5] = {1, 255, 256, 257, 600};
    const int B = 9;
    for (int I : WIDTHS) {
        Rng r = {4000u + I};
        const std::vector<float> x = e_dense(I, B, r);
        char name[160];
        snprintf(name, sizeof name, "E I=%d B=%d count / scan / fill / round trip", I, B);
        g_tag = name;
        Line L;
        std::vector<int32_t> counts(B, 0), idx;
        std::vector<int64_t> indptr(B + 1, 0);
        std::vector<float> val;
        int kinds[5] = {0, 0, 0, 0, 0};   // -0.0, denormal, inf, NaN, stored
        for (int b = 0; b < B; ++b) {
            for (int i = 0; i < I; ++i) {
                const float v = x[(size_t)b * I + i];
                kinds[0] += f_bits(v) == 0x80000000u; kinds[1] += f_bits(v) == 1u; kinds[2] += std::isinf(v); kinds[3] += std::isnan(v);
                if (v != 0.f) { ++counts[b]; idx.push_back(i); val.push_back(v); ++kinds[4]; }
            }
            indptr[b + 1] = indptr[b] + counts[b];
        }
        for (int k = 0; k < 4; ++k) if (!kinds[k]) host_fail(L, "special value %.0f is absent", k);
        if (counts[0] != 0 || counts[1] != I) host_fail(L, "the all-zero or the all-non-zero row is not");
        if (g_host) { report(name, L, "  [bit for bit]"); continue; }
        const size_t mark = pool_size();
        const float* dx = to_dev(x);
        int32_t* dcounts = dev_out<int32_t>(B);
        int64_t* dindptr = dev_out<int64_t>(B + 1);
        int32_t* dindices = dev_out<int32_t>((size_t)B * I);   // room for every element: a count that disagrees cannot make the fill write out of bounds
        float* dvalues = dev_out<float>((size_t)B * I);
        RT(rtx_launch_dense_count(dx, B, I, dcounts, 0));
        RT(rtx_launch_scan_counts(dcounts, B, dindptr, 0));
        CK(hipDeviceSynchronize());
        const std::vector<int32_t> gc = fetch<int32_t>(dcounts, B, L, "counts");
        const std::vector<int64_t> gp = fetch<int64_t>(dindptr, B + 1, L, "indptr");
        bool sane = gp[0] == 0;
        for (int b = 0; b < B; ++b) {
            if (gc[b] != counts[b]) host_fail(L, "counts[%.0f] = %.0f", b, gc[b]);
            if (gp[b + 1] != gp[b] + gc[b]) host_fail(L, "indptr[%.0f] is not the prefix sum of the device's counts", b + 1);
            sane = sane && gc[b] >= 0 && gc[b] <= I && gp[b + 1] == gp[b] + gc[b];
        }
        if (!sane) { host_fail(L, "counts out of range: the fill is not launched"); report(name, L); free_from(mark); continue; }
        RT(rtx_launch_dense_fill(dx, B, I, dindptr, dindices, dvalues, 0));
        CK(hipDeviceSynchronize());
        const std::vector<int32_t> gi = fetch<int32_t>(dindices, (size_t)B * I, L, "indices");
        const std::vector<float> gv = fetch<float>(dvalues, (size_t)B * I, L, "values");
        // count and fill against each other: every slot below the device's total is written, none behind it
        const size_t nnz = (size_t)gp[B];
        for (size_t k = 0; k < (size_t)B * I; ++k) {
            const bool written = (uint32_t)gi[k] != ~0u;
            if (written != (k < nnz)) { host_fail(L, "indices[%.0f]: count and fill disagree", (double)k); break; }
            if (k >= nnz && !is_poison(gv[k])) { host_fail(L, "values[%.0f] written behind the last row", (double)k); break; }
        }
        if (nnz == idx.size()) {
            for (size_t k = 0; k < nnz; ++k) { judge_bits((uint32_t)gi[k], (uint32_t)idx[k], L, "indices", (long)k); judge_bits(f_bits(gv[k]), f_bits(val[k]), L, "values", (long)k); }
        } else host_fail(L, "%.0f stored entries, the host predicate v != 0 gives %.0f", (double)nnz, (double)idx.size());
        // the round trip: the input's bits, -0.0 as +0.0
        RtxCsrView v = {};
        v.indptr = dindptr; v.indices = dindices; v.values = dvalues;
        float* back = dev_out<float>((size_t)B * I);
        RT(rtx_launch_csr_to_dense(v, B, I, back, 0));
        CK(hipDeviceSynchronize());
        std::vector<uint32_t> want = bits_of(x);
        for (auto& w : want) if (w == 0x80000000u) w = 0;
        equal_bits(bits_of(fetch<float>(back, (size_t)B * I, L, "round trip")), want, I, L, "round trip");
        report(name, L, "  [bit for bit]");
        free_from(mark);
    }
    // the path of dense_to_view: a conditioned batch as a dense tensor -> CSR on the device -> k_gather, against the gather of the CSR itself
    for (int bf = 0; bf < 2; ++bf) {
        const int I = 300, cond = 16, Iin = I + cond, ldx = 320, B = 9, Bp = 16;
        Batch bt = make_batch(I, cond, ldx, V_REAL, 0, 1, 0.3f, true, 0, B, Bp, false, 4500);
        char name[160];
        snprintf(name, sizeof name, "E %s dense -> CSR -> k_gather I=%d+%d against the gather of the CSR", bf ? "bf16" : "f32", I, cond);
        g_tag = name;
        Line L;
        const Ref R = build_ref(bt);
        if (g_host) { host_checks(bt, R, L, false, false); report(name, L, regime(R)); continue; }
        const size_t mark = pool_size();
        std::vector<float> x((size_t)B * Iin, 0.f);
        for (int b = 0; b < B; ++b)
            for (int64_t k = bt.in.indptr[b]; k < bt.in.indptr[b + 1]; ++k) x[(size_t)b * Iin + bt.in.idx[k]] = bt.in.value(k);
        const float* dx = to_dev(x);
        int32_t* dcounts = dev_out<int32_t>(B);
        int64_t* dindptr = dev_out<int64_t>(B + 1);
        int32_t* dindices = dev_out<int32_t>((size_t)B * Iin);
        float* dvalues = dev_out<float>((size_t)B * Iin);
        RT(rtx_launch_dense_count(dx, B, Iin, dcounts, 0));
        RT(rtx_launch_scan_counts(dcounts, B, dindptr, 0));
        CK(hipDeviceSynchronize());
        const std::vector<int64_t> gp = fetch<int64_t>(dindptr, B + 1, L, "indptr");
        int64_t stored = 0;
        for (int b = 0; b < B; ++b) for (int64_t k = bt.in.indptr[b]; k < bt.in.indptr[b + 1]; ++k) stored += bt.in.value(k) != 0.f;
        if (gp[0] != 0 || gp[B] != stored) { host_fail(L, "indptr[B] = %.0f, expected %.0f", (double)gp[B], (double)stored); report(name, L); free_from(mark); continue; }
        RT(rtx_launch_dense_fill(dx, B, Iin, dindptr, dindices, dvalues, 0));
        CK(hipDeviceSynchronize());
        DevBatch d = upload(bt);
        std::vector<uint32_t> from_csr, from_dense;
        std::vector<float> ts_csr, ts_dense;
        run_gather(bt, d, bf, L, from_csr, ts_csr);
        DevBatch dd = d;
        dd.in = RtxCsrView{};
        dd.in.indptr = dindptr; dd.in.indices = dindices; dd.in.values = dvalues;   // max_row_len = 0: a densified batch
        dd.tg = dd.in;
        run_gather(bt, dd, bf, L, from_dense, ts_dense);
        equal_bits(from_dense, from_csr, ldx, L, "X (from the dense tensor against from the CSR)");
        equal_bits(bits_of(ts_dense), bits_of(ts_csr), 1, L, "tsum (from the dense tensor against from the CSR)");
        judge_image(R, from_dense, bf, L);
        judge_tsum(R, ts_dense, L);
        report(name, L, regime(R));
        free_from(mark);
    }
}

// ---- section R: refusals that come before the first HIP call ---------------------------------------------------------------------------
static void section_r()
{
    printf("== R: refusals ==\n");
    static int32_t dummy_i[4];
    static bf16_t dummy_x[8];
    g_tag = "R";
    auto expect = [&](const char* name, int got, int want) {
        Line L;
        if (got != want) host_fail(L, "returned %.0f, expected %.0f", got, want);
        report(std::string("R ") + name, L);
    };
    RtxGatherArgs g = {};   // B = Bp = 0: even a launch that were not refused would start no workgroup
    g.I = 300; g.Iin = 300; g.ldx = 304; g.in.max_row_len = 10; g.written_cap = 12;
    { RtxGatherArgs a = g; a.ldx = 300; expect("gather: ldx % 8 != 0", rtx_launch_gather(a, 0, 0), RTX_EINVAL); }
    { RtxGatherArgs a = g; a.written = dummy_i; expect("gather, scatter form: n_written null", rtx_launch_gather(a, 1, 0), RTX_EINVAL); }
    { RtxGatherArgs a = g; a.written = a.n_written = dummy_i; a.in.max_row_len = 0; expect("gather, scatter form: max_row_len = 0", rtx_launch_gather(a, 0, 0), RTX_EINVAL); }
    { RtxGatherArgs a = g; a.written = a.n_written = dummy_i; a.in.max_row_len = 12; expect("gather, scatter form: max_row_len = written_cap", rtx_launch_gather(a, 1, 0), RTX_EINVAL); }
    { RtxGatherArgs a = g; a.written = a.n_written = dummy_i; a.Iin = 304; expect("gather, scatter form: Iin = ldx", rtx_launch_gather(a, 0, 0), RTX_EINVAL); }
    RtxInChunksArgs c = {};
    c.B = 1; c.I = 300; c.Iin = 300;
    { RtxInChunksArgs a = c; a.B = 0; expect("in_chunks: B = 0", rtx_launch_in_chunks(a, 0), RTX_EINVAL); }
    { RtxInChunksArgs a = c; a.Iin = 299; expect("in_chunks: Iin < I", rtx_launch_in_chunks(a, 0), RTX_EINVAL); }
    { RtxInChunksArgs a = c; a.I = a.Iin = 65537; expect("in_chunks: Iin = 65 537", rtx_launch_in_chunks(a, 0), RTX_EINVAL); }
    { RtxInChunksArgs a = c; a.X = dummy_x; a.ldx = 300; a.Bp = 8; expect("in_chunks: ldx % 8 != 0", rtx_launch_in_chunks(a, 0), RTX_EINVAL); }
    { RtxInChunksArgs a = c; a.X = dummy_x; a.ldx = 304; a.Bp = 0; expect("in_chunks: Bp < B", rtx_launch_in_chunks(a, 0), RTX_EINVAL); }
    RtxCsrView v = {};
    expect("csr_to_dense: B = 0 launches nothing", rtx_launch_csr_to_dense(v, 0, 7, nullptr, 0), RTX_OK);
    expect("dense_count: B = 0 launches nothing", rtx_launch_dense_count(nullptr, 0, 7, nullptr, 0), RTX_OK);
    expect("dense_fill: B = 0 launches nothing", rtx_launch_dense_fill(nullptr, 0, 7, nullptr, nullptr, nullptr, 0), RTX_OK);
}

// ---- section S (--host): the judging can fail ------------------------------------------------------------------------------------------
static void section_s()
{
    printf("== S: every defect is rejected by the judging of the device run ==\n");
    g_tag = "S";
    const ACase& c = A_CASES[10];   // a11: half steps, conditioned, dropout by mask, B = 5 of 8
    const Batch bt = a_batch(c, 0, 110);
    const Ref R = build_ref(bt);
    const size_t n = (size_t)bt.Bp * bt.ldx;
    std::vector<uint32_t> good(n);
    for (size_t k = 0; k < n; ++k) good[k] = f_bits(R.m[k]);
    // a kept item entry and a condition entry of batch row 0 (CSR row 5)
    const int64_t u = bt.row(0);
    int item = -1, condc = -1;
    float cond_raw = 0.f, ss = 0.f;
    for (int64_t k = bt.in.indptr[u]; k < bt.in.indptr[u + 1]; ++k) {
        const int i = bt.in.idx[k];
        if (i < bt.I) { ss += bt.in.value(k) * bt.in.value(k); if (item < 0 && R.m[i] != 0.f) item = i; }
        else { condc = i; cond_raw = bt.in.value(k); }
    }
    auto must_fail = [&](const char* name, long bad_of_defect, long bad_of_good) {
        Line L;
        if (bad_of_good != 0) host_fail(L, "the unchanged result is rejected (%.0f elements)", (double)bad_of_good);
        if (bad_of_defect == 0) host_fail(L, "the defect passes");
        printf("    (the lines above are the rejection this case asks for)\n");
        report(std::string("S ") + name, L);
    };
    auto image_bad = [&](const std::vector<uint32_t>& img) { Line L; judge_image(R, img, false, L); return L.bad; };
    const long good_bad = image_bad(good);
    if (item < 0 || condc < 0) { Line L; host_fail(L, "row 0 of the batch has no kept item entry or no condition column"); report("S setup", L); return; }
    { std::vector<uint32_t> x = good; x[bt.Iin] = 0; must_fail("ones column missing", image_bad(x), good_bad); }
    { std::vector<uint32_t> x = good; x[(size_t)6 * bt.ldx + 17] = f_bits(0.25f); must_fail("a stale non-zero in a padding row", image_bad(x), good_bad); }
    { std::vector<uint32_t> x = good; x[item] += 1; must_fail("one entry off by one float32 ulp", image_bad(x), good_bad); }
    { std::vector<uint32_t> x = good; x[condc] = f_bits(cond_raw * (1.f / fmaxf(sqrtf(ss), 1e-12f))); must_fail("a condition column normalised", image_bad(x), good_bad); }
    {   // the lists of the scatter form
        const int cap = bt.in.longest + 2;
        std::vector<int32_t> nw(bt.Bp, 0), wr((size_t)bt.Bp * cap, 0), before((size_t)bt.Bp * cap, 0);
        for (int b = 0; b < bt.B; ++b) {
            const int64_t r = bt.row(b);
            const int len = bt.in.len(r);
            for (int k = 0; k < len; ++k) wr[(size_t)b * cap + k] = bt.in.idx[bt.in.indptr[r] + k];
            wr[(size_t)b * cap + len] = bt.Iin;
            nw[b] = len + 1;
        }
        before = wr;   // (behind the lists nothing changes)
        Line Lg, Ld;
        judge_lists(bt, cap, nw, wr, before, Lg);
        std::vector<int32_t> nw2 = nw;
        --nw2[2];
        judge_lists(bt, cap, nw2, wr, before, Ld);
        must_fail("one written list short by one", Ld.bad, Lg.bad);
    }
    {   // the split
        const std::vector<int> nch = user_chunks(bt);   // rows 5, 0, 4, 5, 7: 11 or 12, 1, 5, 11 or 12, 1 chunks
        std::vector<long> first(nch.size() + 1, 0);
        for (size_t b = 0; b < nch.size(); ++b) first[b + 1] = first[b] + nch[b];
        int32_t ws[RTX_SPMM_WAVES + 1];
        for (int w = 0; w <= RTX_SPMM_WAVES; ++w) {
            ws[w] = (int32_t)first.back();
            for (size_t b = 0; b < nch.size(); ++b) if (first[b] * RTX_SPMM_WAVES >= first.back() * w) { ws[w] = (int32_t)first[b]; break; }
        }
        Line Lg, Ld;
        judge_split(nch, ws, Lg);
        int32_t ws2[RTX_SPMM_WAVES + 1];
        memcpy(ws2, ws, sizeof ws);
        ws2[1] = 5;   // inside user 0, and still monotone
        judge_split(nch, ws2, Ld);
        must_fail("one wsplit entry in the middle of a user", Ld.bad, Lg.bad);
    }
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    g_name_width = 96;
    section_a();
    section_b();
    section_c();
    section_d();
    section_e();
    section_r();
    if (g_host) section_s();
    else {
        printf("bounded regime, float32: %ld elements, worst error %.3f of the bound (n / 2 + 5) 2^-24\n", g_bounded_elems, g_worst_bounded);
        printf("section C, bounded regime: %ld of %ld elements of k_in_chunks' image differ from k_gather<bf16>'s\n", g_c_differs, g_c_compared);
        free_all();
    }
    return finish("BATCH");
}
