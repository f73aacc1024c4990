// Native (no Python) check of the four launchers of adam.hip, one at a time, against plain float64 host code:
//   A  rtx_launch_adam: k_adam on each of its five walks (flat whole tile, flat tail with nv < 4, 2-D float4 tiles, 2-D 4-byte tiles,
//      the transposed compute copy through the LDS tile), single tensors, row shards built as rtx_engine_apply_adam_rows builds them,
//      and multi-tensor launches of 1 .. 17 tiles and of RTX_MAX_TENSORS tensors (every launch bit-identical to its tensors one by one)
//   C  rtx_launch_cast_f32_bf16, bit for bit against a round-to-nearest-even written from the bit pattern by hand
//   D  rtx_launch_dw_slab_reduce, bit for bit against a host float32 loop in slab order from +0
//   S  rtx_launch_sumsq, six tensors in one call, twice into the same (poisoned) sums
// Every buffer a kernel writes is poisoned (all bits set: a NaN in f32 and in bf16) before each launch and carries a poisoned guard
// behind its end; p / m / v, updated in place, carry the guard too, and the rows of a sharded matrix outside the shard, the float32
// gradient where a bf16 image is given, and slab memory outside [M_real][N_real + 1] hold finite junk of magnitude ~1e3 that must come
// back unchanged / unused.  Each element is judged against ITS OWN scale and every line prints the worst error as a fraction of its bound.
//
// One Adam case is ONE update from a drawn state (p in +-1, m in +-0.1, v >= 0 with exact 0, 1e-30 and 10, g in +-1 with exact zeros,
// rounded to bf16 once where the bf16 image is used), so every bound is a one-update bound.  The reference reads the same float32 bits
// and the scalars as the float32 values passed; 1.f - beta is exact in float32 for 0.9f and 0.999f (Sterbenz; checked in --host).
// With d = 2^-24 (one float32 rounding, relative; sqrtf and the division are correctly rounded in hipcc's default mode), first order,
// a fused multiply-add only removing roundings from the sequence below:
//   g  = gv gs + reg pv + wd pv        a = gv gs, b = reg pv (reg = lam / sqrtf(sumsq): 2 roundings of its own), c = wd pv
//        e_g = d (3 |a| + 5 |b| + 2 |c|)                      (a product rounding per term, a rounding per partial sum)
//   m' = m + (g - m) (1 - b1)          e_m = (1 - b1) e_g + 2 d (1 - b1) |g - m| + d |m'|
//   v' = v b2 + (1 - b2) g g           e_v = d v b2 + 2 d (1 - b2) g^2 + (1 - b2) (2 |g| e_g + e_g^2) + d v'
//   D  = sqrtf(v') / bc2 + eps         e_D = (e_v / (sqrt(v') + sqrt(max(v' - e_v, 0))) + 2 d sqrt(v')) / bc2 + d D
//   p' = p - ss (m' / D)               e_p = ss [(e_m + |m'| / D e_D) / (D - e_D) + d |m' / D|] + d ss |m' / D| + d |p'|
// (v' has no cancellation: both terms are >= 0; D >= eps > 0).  Each of the three is a count of roundings times the quantity's own
// scale -- |p'| + ss |m' / D|, |m| + |g|, |v| + g^2 -- written term by term so that none is charged to a scale it does not act on.
// Measured on the MI355X, none of these bounds (nor the one of k_sumsq, derived at its case) stayed below 0.05 of itself, so by the rule
// of DESIGN.md section 6 all stay as derived: no tightening factor.
//   test_adam          the device run
//   test_adam --host   no HIP call: the float64 reference against a second formulation in long double (other operation order) and
//                      against orc_adam of oracle/mvae_oracle.c, the hand-written bf16 rounding against the host build of f32_to_bf16
//                      over all 65 536 high halves, the conditions the bounds assume, and the launchers' returns that come before the
//                      first HIP call
#include "../../rectorch_amd/csrc/rtx_kernels.h"
#include "../../oracle/mvae_oracle.h"

#include "check.h"

static const float BETA1 = 0.9f, BETA2 = 0.999f, EPS = 1e-8f;
static const double LR = 1e-3;

static int r128(int z) { return (z + 127) / 128 * 128; }

// round to nearest even, float32 bits -> bf16 bits, from the bit pattern by hand (no call of f32_to_bf16): a NaN keeps its sign and high
// payload and gets the quiet bit; anything else keeps its upper half, plus one when the lower half is above a half, or is exactly a half
// and the upper half is odd -- the carry may run into the exponent and up to infinity, which is the right result
static uint16_t rne_by_hand(uint32_t u)
{
    const uint32_t ex = (u >> 23) & 0xff, man = u & 0x7fffff;
    uint32_t hi = u >> 16;
    const uint32_t lo = u & 0xffff;
    if (ex == 0xff && man) return (uint16_t)(hi | 0x40);
    if (lo > 0x8000 || (lo == 0x8000 && (hi & 1))) ++hi;
    return (uint16_t)hi;
}

// ---- judging ------------------------------------------------------------------------------------------------------------------------
enum { FLAT, VEC2D, ELEM2D, NROUTE };
static const char* const ROUTE_NAME[NROUTE] = {"flat", "2-D float4", "2-D 4-byte"};
enum { Q_P, Q_M, Q_V, NQA };
static const char* const QA_NAME[NQA] = {"p", "m", "v"};
static double g_qworst[NROUTE][NQA], g_sumsq_worst;
static long g_qn[NROUTE][NQA];

// feeds a walk's table from judge()'s error / bound
static void tally(int route, int q, double ratio)
{
    if (ratio > g_qworst[route][q]) g_qworst[route][q] = ratio;
    ++g_qn[route][q];
}

// =====================================================================================================================================
// A: rtx_launch_adam
// =====================================================================================================================================
enum { DRAWN, STILL, REFRESH };      // STILL: g == 0 and m == 0 (with wd == lam == 0: p unchanged); REFRESH: update == 0, special values in p
struct Spec {
    int rows, cols;           // the tensor as launched
    int mat_rows, row_lo;     // rows [row_lo, row_lo + rows) of a [mat_rows][cols] matrix (mat_rows == rows, row_lo == 0: no shard)
    int sh, shT;
    int g16;                  // 0: float32 gradient, 1: bf16 image, 2: bf16 image under every variant
    int sumsq;                // 0: null, 1: given, 2: given, the tensor all zeros (*sumsq == 0)
    int route;                // the walk the case is meant to take
};
struct Scal { int mode, step; float wd, lam, gs; };
struct Tensor {
    Spec s;
    int ld_sh = 0, ld_shT = 0;
    size_t n_mat = 0, off = 0, n = 0;
    std::vector<float> p, g, m, v, g_dev;      // [n_mat]; g: what the kernel must read (decoded from g16 where given); g_dev: the f32 buffer
    std::vector<uint16_t> g16;
    float sumsq = 0;
    float *dp = nullptr, *dg = nullptr, *dm = nullptr, *dv = nullptr, *dss = nullptr;
    uint16_t* dg16 = nullptr;
    unsigned char *dsh = nullptr, *dshT = nullptr;
    int tiles() const { return s.route == FLAT ? (int)((n + 4095) / 4096) : ((s.rows + 63) / 64) * ((s.cols + 63) / 64); }
};
struct Snap { std::vector<float> p, m, v; std::vector<unsigned char> sh, shT; };

// values whose bf16 rounding separates two converters: both kinds of ties (to even down / up, both signs), a carry into the exponent,
// float32 subnormals (below, at and above half a bf16 subnormal step; the largest; a tie at an odd upper half)
static const uint32_t SPECIAL_P[] = {0x3f808000u, 0x3f818000u, 0xbf808000u, 0xbf818000u, 0x3fffffffu, 0x3f807fffu, 0x3f808001u,
                                     0x00000001u, 0x00008000u, 0x00008001u, 0x00018000u, 0x007fffffu, 0x807f8000u, 0x00400000u, 0x80000001u, 0x00028000u};
static const int N_SPECIAL_P = sizeof SPECIAL_P / sizeof SPECIAL_P[0];

static void gen_tensor(Tensor& t, const Spec& s, int mode, Rng& r)
{
    t.s = s;
    t.n_mat = (size_t)s.mat_rows * s.cols; t.off = (size_t)s.row_lo * s.cols; t.n = (size_t)s.rows * s.cols;
    t.ld_sh = r128(s.cols); t.ld_shT = r128(s.rows);      // the engine's layout
    t.p.resize(t.n_mat); t.g.resize(t.n_mat); t.m.resize(t.n_mat); t.v.resize(t.n_mat); t.g_dev.resize(t.n_mat);
    t.g16.assign(s.g16 ? t.n_mat : 0, 0);
    double ss = 0;
    for (size_t k = 0; k < t.n_mat; ++k) {
        if (k < t.off || k >= t.off + t.n) {      // outside the shard: must come back unchanged
            t.p[k] = r.junk(); t.m[k] = r.junk(); t.v[k] = r.junk(); t.g[k] = t.g_dev[k] = r.junk();
            if (s.g16) t.g16[k] = f32_to_bf16(r.junk());
            continue;
        }
        const size_t i = k - t.off;
        t.p[k] = s.sumsq == 2 ? 0.f : r.f();
        if (mode == REFRESH && i % 3 == 0 && s.sumsq != 2) t.p[k] = bits_f(SPECIAL_P[(i / 3) % N_SPECIAL_P]);
        t.m[k] = mode == STILL ? 0.f : 0.1f * r.f();
        const float u = r.u01();
        t.v[k] = i % 7 == 0 ? 0.f : i % 7 == 1 ? 1e-30f : i % 7 == 2 ? 10.f : u * u;
        float g = (i % 5 == 0 || mode == STILL) ? 0.f : r.f();
        if (s.g16) { t.g16[k] = f32_to_bf16(g); g = bf16_to_f32(t.g16[k]); }
        t.g[k] = g;
        t.g_dev[k] = s.g16 ? r.junk() : g;      // with a bf16 image the float32 gradient may be read but must not be used
        ss += (double)t.p[k] * t.p[k];
    }
    t.sumsq = (float)ss;
}

static void alloc_tensor(Tensor& t, int esz)
{
    t.dp = dev_out<float>(t.n_mat); t.dm = dev_out<float>(t.n_mat); t.dv = dev_out<float>(t.n_mat);
    t.dg = to_dev(t.g_dev);
    if (t.s.g16) t.dg16 = to_dev(t.g16);
    if (t.s.sumsq) t.dss = to_dev(std::vector<float>(1, t.sumsq));
    if (t.s.sh) t.dsh = (unsigned char*)dev_bytes(((size_t)t.s.mat_rows * t.ld_sh + GUARD) * esz, 0xff);
    if (t.s.shT) t.dshT = (unsigned char*)dev_bytes(((size_t)t.s.cols * t.ld_shT + GUARD) * esz, 0xff);
}
// the drawn state into p / m / v, poison into the compute copies
static void upload(Tensor& t, int esz)
{
    if (t.n_mat) {
        CK(hipMemcpy(t.dp, t.p.data(), t.n_mat * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(t.dm, t.m.data(), t.n_mat * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(t.dv, t.v.data(), t.n_mat * 4, hipMemcpyHostToDevice));
    }
    if (t.dsh) CK(hipMemset(t.dsh, 0xff, ((size_t)t.s.mat_rows * t.ld_sh + GUARD) * esz));
    if (t.dshT) CK(hipMemset(t.dshT, 0xff, ((size_t)t.s.cols * t.ld_shT + GUARD) * esz));
}

static void scalars(RtxAdamArgs& a, const Scal& s)
{
    a.update = s.mode != REFRESH;
    a.step_size = (float)(LR / (1.0 - pow((double)BETA1, s.step)));
    a.bc2_sqrt = (float)sqrt(1.0 - pow((double)BETA2, s.step));
    a.beta1 = BETA1; a.beta2 = BETA2; a.eps = EPS; a.weight_decay = s.wd; a.lam = s.lam; a.grad_scale = s.gs;
}
// a tensor of the launch, built the way rtx_engine_apply_adam_rows builds a shard: p / g / m / v (and the bf16 image) offset by
// row_lo * cols elements, the compute copy by row_lo * ld_sh
static RtxAdamTensor arg_of(const Tensor& t, int update, int esz)
{
    RtxAdamTensor w = {};
    w.p = t.dp + t.off;
    if (update) { w.g = t.dg + t.off; w.m = t.dm + t.off; w.v = t.dv + t.off; }
    if (t.dg16) w.g16 = t.dg16 + t.off;
    if (t.dsh) w.sh = t.dsh + (size_t)t.s.row_lo * t.ld_sh * esz;
    w.shT = t.dshT;
    w.sumsq = t.dss;
    w.rows = t.s.rows; w.cols = t.s.cols; w.ld_sh = t.ld_sh; w.ld_shT = t.ld_shT;
    return w;
}

struct Ref { double p, m, v, ep, em, ev; };
static Ref adam_ref(float pv, float gv, float mv, float vv, double reg, const RtxAdamArgs& A)
{
    const double a = (double)gv * A.grad_scale, b = reg * pv, c = (double)A.weight_decay * pv;
    const double g = a + b + c, eg = E24 * (3 * fabs(a) + 5 * fabs(b) + 2 * fabs(c));
    const double ob1 = (double)(1.f - A.beta1), ob2 = (double)(1.f - A.beta2);
    Ref r;
    r.m = mv + (g - mv) * ob1;
    r.em = ob1 * eg + 2 * E24 * ob1 * fabs(g - mv) + E24 * fabs(r.m);
    r.v = (double)vv * A.beta2 + ob2 * g * g;
    r.ev = E24 * (double)vv * A.beta2 + 2 * E24 * ob2 * g * g + ob2 * (2 * fabs(g) * eg + eg * eg) + E24 * r.v;
    const double sq = sqrt(r.v), D = sq / A.bc2_sqrt + A.eps;
    const double dsq = r.ev > 0 ? r.ev / (sq + sqrt(std::max(r.v - r.ev, 0.0))) : 0.0;
    const double eD = (dsq + 2 * E24 * sq) / A.bc2_sqrt + E24 * D;
    const double q = r.m / D, eq = (r.em + fabs(q) * eD) / (D - eD) + E24 * fabs(q);
    r.p = pv - (double)A.step_size * q;
    r.ep = A.step_size * eq + E24 * A.step_size * fabs(q) + E24 * fabs(r.p);
    return r;
}
static double reg_of(const Tensor& t, const RtxAdamArgs& A)
{
    if (A.lam == 0.f || !t.s.sumsq) return 0.0;
    return t.sumsq > 0.f ? (double)A.lam / sqrt((double)t.sumsq) : 0.0;
}

static uint32_t copy_bits(const std::vector<unsigned char>& b, size_t i, int esz)
{
    if (esz == 2) { uint16_t h; memcpy(&h, &b[i * 2], 2); return h; }
    uint32_t u; memcpy(&u, &b[i * 4], 4); return u;
}
static uint32_t copy_from(float x, int esz) { return esz == 2 ? (uint32_t)f32_to_bf16(x) : f_bits(x); }

// everything the launch left of one tensor: p / m / v against float64 (or bit for bit where nothing may change), the compute copies
// bit for bit against the DEVICE's own new p, their padding and every guard against the poison
static void check_tensor(const Tensor& t, const RtxAdamArgs& A, int mode, int esz, Line& L, Snap& sn)
{
    sn.p = fetch<float>(t.dp, t.n_mat, L, "p"); sn.m = fetch<float>(t.dm, t.n_mat, L, "m"); sn.v = fetch<float>(t.dv, t.n_mat, L, "v");
    const double reg = reg_of(t, A);
    const int rt = t.s.route;
    for (size_t k = 0; k < t.n_mat; ++k) {
        const bool in = k >= t.off && k < t.off + t.n;
        if (!in || mode == REFRESH) {
            judge_bits(f_bits(sn.p[k]), f_bits(t.p[k]), L, in ? "p (update == 0)" : "p outside the shard", (long)k);
            judge_bits(f_bits(sn.m[k]), f_bits(t.m[k]), L, in ? "m (update == 0)" : "m outside the shard", (long)k);
            judge_bits(f_bits(sn.v[k]), f_bits(t.v[k]), L, in ? "v (update == 0)" : "v outside the shard", (long)k);
            continue;
        }
        const Ref r = adam_ref(t.p[k], t.g[k], t.m[k], t.v[k], reg, A);
        tally(rt, Q_P, judge(sn.p[k], r.p, r.ep, L, "p", (long)k));
        tally(rt, Q_M, judge(sn.m[k], r.m, r.em, L, "m", (long)k));
        tally(rt, Q_V, judge(sn.v[k], r.v, r.ev, L, "v", (long)k));
        if (mode == STILL && A.weight_decay == 0.f && A.lam == 0.f) judge_bits(f_bits(sn.p[k]), f_bits(t.p[k]), L, "p (g == m == 0)", (long)k);
    }
    const uint32_t poison = esz == 2 ? 0xffffu : 0xffffffffu;
    sn.sh.clear(); sn.shT.clear();
    if (t.dsh) {
        sn.sh = fetch<unsigned char>(t.dsh, (size_t)t.s.mat_rows * t.ld_sh * esz, L, "sh");      // (guard: GUARD bytes of the GUARD elements)
        for (int r = 0; r < t.s.mat_rows; ++r)
            for (int c = 0; c < t.ld_sh; ++c) {
                const bool in = r >= t.s.row_lo && r < t.s.row_lo + t.s.rows && c < t.s.cols;
                const uint32_t got = copy_bits(sn.sh, (size_t)r * t.ld_sh + c, esz);
                if (in) judge_bits(got, copy_from(sn.p[(size_t)r * t.s.cols + c], esz), L, "sh vs Elem<T>::from(p)", r, c);
                else judge_bits(got, poison, L, "sh padding", r, c);
            }
    }
    if (t.dshT) {
        sn.shT = fetch<unsigned char>(t.dshT, (size_t)t.s.cols * t.ld_shT * esz, L, "shT");
        for (int c = 0; c < t.s.cols; ++c)
            for (int r = 0; r < t.ld_shT; ++r) {
                const uint32_t got = copy_bits(sn.shT, (size_t)c * t.ld_shT + r, esz);
                if (r < t.s.rows) {
                    judge_bits(got, copy_from(sn.p[(size_t)r * t.s.cols + c], esz), L, "shT vs Elem<T>::from(p)", c, r);
                    if (t.dsh) judge_bits(got, copy_bits(sn.sh, (size_t)r * t.ld_sh + c, esz), L, "shT vs sh", c, r);
                } else judge_bits(got, poison, L, "shT padding", c, r);
            }
    }
}
static bool same(const Snap& a, const Snap& b)
{
    return a.p.size() == b.p.size() && !memcmp(a.p.data(), b.p.data(), a.p.size() * 4) && !memcmp(a.m.data(), b.m.data(), a.m.size() * 4) &&
           !memcmp(a.v.data(), b.v.data(), a.v.size() * 4) && a.sh == b.sh && a.shT == b.shT;
}

// --host: the reference against a second formulation in long double with the operations in another order, the drawn state, the
// special values, the conditions the bounds assume
static void host_check_tensor(const Tensor& t, const RtxAdamArgs& A, int mode, Line& L)
{
    const long double reg = A.lam != 0.f && t.s.sumsq && t.sumsq > 0.f ? (long double)A.lam / sqrtl((long double)t.sumsq) : 0.0L;
    if (t.s.sumsq == 2 && t.sumsq != 0.f) host_fail(L, "the all-zero tensor has sumsq %g", t.sumsq);
    long v0 = 0, vtiny = 0, v10 = 0, g0 = 0, nbad = 0, ties = 0, subs = 0;
    for (size_t k = 0; k < t.n_mat; ++k) {
        if (k < t.off || k >= t.off + t.n) {
            nbad += !is_junk(t.p[k]) || !is_junk(t.m[k]) || !is_junk(t.v[k]) || !is_junk(t.g_dev[k]);
            continue;
        }
        if (t.s.g16 && !is_junk(t.g_dev[k])) ++nbad;
        if (t.s.g16 && bf16_to_f32(t.g16[k]) != t.g[k]) host_fail(L, "g[%g] is not the value of its bf16 image", (double)k);
        if (!(fabsf(t.p[k]) <= (mode == REFRESH ? 2.f : 1.f)) || !(fabsf(t.m[k]) <= 0.1f) || !(t.v[k] >= 0.f) || !(fabsf(t.g[k]) <= 1.f)) host_fail(L, "element %g outside the drawn ranges", (double)k);
        v0 += t.v[k] == 0.f; vtiny += t.v[k] == 1e-30f; v10 += t.v[k] == 10.f; g0 += t.g[k] == 0.f;
        const uint32_t u = f_bits(t.p[k]);
        ties += (u & 0xffff) == 0x8000 && (u & 0x7f800000u) != 0; subs += (u & 0x7f800000u) == 0 && (u & 0x7fffffu) != 0;
        if (mode == REFRESH) continue;
        const Ref r = adam_ref(t.p[k], t.g[k], t.m[k], t.v[k], (double)reg, A);
        const long double ob1 = 1.0L - (long double)A.beta1, ob2 = 1.0L - (long double)A.beta2;
        const long double g = (long double)t.p[k] * ((long double)A.weight_decay + reg) + (long double)A.grad_scale * t.g[k];
        const long double m = (long double)A.beta1 * t.m[k] + ob1 * g, v = ob2 * (g * g) + (long double)A.beta2 * t.v[k];
        const long double p = (long double)t.p[k] - (long double)A.step_size * m * A.bc2_sqrt / (sqrtl(v) + (long double)A.eps * A.bc2_sqrt);
        // agreement demanded: 1e-6 of each bound (float64 rounds at 2^-53 = 2e-9 of a float32 rounding, on the same scales)
        if (!(fabsl(m - r.m) <= 1e-6L * r.em)) host_fail(L, "m %.17g, long double %.17g", r.m, (double)m);
        if (!(fabsl(v - r.v) <= 1e-6L * r.ev)) host_fail(L, "v %.17g, long double %.17g", r.v, (double)v);
        if (!(fabsl(p - r.p) <= 1e-6L * r.ep)) host_fail(L, "p %.17g, long double %.17g", r.p, (double)p);
        // the bounds' relative-error model: no product of the sequence may underflow
        const double gg = (1.0 - (double)A.beta2) * (double)g * (double)g;
        if (gg != 0 && gg < 1e-30) host_fail(L, "(1 - beta2) g^2 = %g may underflow", gg);
        if (!(r.ep > 0 && r.em >= 0 && r.ev >= 0 && r.ep < 1e30)) host_fail(L, "bound of p %g at p' = %g", r.ep, r.p);
    }
    if (nbad) host_fail(L, "%g elements the kernel must not use hold no junk", (double)nbad);
    if (t.n >= 8 && !(v0 && vtiny && v10 && g0)) host_fail(L, "the state lacks v = 0 / 1e-30 / 10 or g = 0");
    if (mode == REFRESH && t.s.sumsq != 2 && t.n >= 3u * N_SPECIAL_P && !(ties >= 4 && subs >= 6)) host_fail(L, "p holds %g ties and %g subnormals", (double)ties, (double)subs);
}

// the shapes of the issue; none is the workload's
static const Spec FLAT_SHAPES[] = {      // no shT, aligned pointers
    {1, 5, 1, 0, 0, 0, 0, 0, FLAT},    {1, 4096, 1, 0, 0, 0, 0, 0, FLAT}, {1, 4097, 1, 0, 0, 0, 0, 0, FLAT}, {5, 6, 5, 0, 0, 0, 0, 0, FLAT},
    {3, 1367, 3, 0, 0, 0, 0, 0, FLAT}, {64, 128, 64, 0, 0, 0, 0, 0, FLAT}, {70, 100, 70, 0, 0, 0, 0, 0, FLAT}};
static const Spec T_SHAPES[] = {         // shT (and sh): the 2-D walk
    {64, 64, 64, 0, 1, 1, 0, 0, VEC2D},  {65, 68, 65, 0, 1, 1, 0, 0, VEC2D},   {130, 36, 130, 0, 1, 1, 0, 0, VEC2D}, {33, 67, 33, 0, 1, 1, 0, 0, ELEM2D},
    {100, 1, 100, 0, 1, 1, 0, 0, ELEM2D}, {1, 70, 1, 0, 1, 1, 0, 0, ELEM2D}, {17, 130, 17, 0, 1, 1, 0, 0, ELEM2D}};
static const Spec SHARD_A = {26, 17, 40, 3, 1, 0, 0, 0, ELEM2D};      // rows [3, 29) of 40 x 17: the offset is 51 floats
static const Spec SHARD_B = {39, 20, 40, 1, 1, 0, 2, 0, VEC2D};       // rows [1, 40) of 40 x 20 with a bf16 image: p aligned, g16 at 8 mod 16

// the variants: every one on every shape (both compute-copy types)
struct Variant { const char* name; Scal s; int g16, sumsq; };
static const Variant VARIANTS[] = {
    {"step 1", {DRAWN, 1, 0.f, 0.f, 1.f}, 0, 0},
    {"step 1000 g16 wd lam sumsq gs/8", {DRAWN, 1000, 0.01f, 0.5f, 0.125f}, 1, 1},
    {"step 1000 g16 lam, sumsq null", {DRAWN, 1000, 0.f, 0.5f, 1.f}, 1, 0},
    {"step 1 wd lam sumsq gs/8", {DRAWN, 1, 0.01f, 0.5f, 0.125f}, 0, 1},
    {"all zeros, *sumsq == 0, lam", {DRAWN, 1, 0.f, 0.5f, 1.f}, 0, 2},
    {"g == m == 0", {STILL, 1, 0.f, 0.f, 1.f}, 0, 0},
    {"g == m == 0, g16", {STILL, 1000, 0.f, 0.f, 0.125f}, 1, 0},
    {"update == 0", {REFRESH, 1, 0.f, 0.f, 1.f}, 0, 0},
};

static void check_route(const RtxAdamArgs& a, const std::vector<Tensor*>& ts, Line& L)
{
    int tiles = 0;
    for (size_t k = 0; k < ts.size(); ++k) {
        if (a.t[k].flat != (ts[k]->s.route == FLAT)) host_fail(L, "tensor %g: flat = %g, not the route the case is meant to take", (double)k, a.t[k].flat);
        if (a.t[k].tile_start != tiles) host_fail(L, "tensor %g: tile_start %g", (double)k, a.t[k].tile_start);
        tiles += ts[k]->tiles();
    }
    if (a.total_tiles != tiles) host_fail(L, "total_tiles = %g, expected %g", a.total_tiles, tiles);
}

static void single_case(Spec s, const Variant& v, int bf16, uint32_t seed)
{
    const int esz = bf16 ? 2 : 4;
    Rng r = {seed};
    if (s.g16 != 2) s.g16 = v.g16;      // (SHARD_B takes its route BY its bf16 image: always given)
    s.sumsq = v.sumsq;
    Tensor t;
    gen_tensor(t, s, v.s.mode, r);
    char name[200];
    snprintf(name, sizeof name, "A k_adam<%s> %s %dx%d%s%s%s: %s", bf16 ? "bf16" : "f32", ROUTE_NAME[s.route], s.rows, s.cols,
             s.mat_rows != s.rows ? " (shard)" : "", s.sh ? " sh" : "", s.shT ? " shT" : "", v.name);
    Line L;
    RtxAdamArgs a = {};
    scalars(a, v.s);
    if (g_host) { host_check_tensor(t, a, v.s.mode, L); report(name, L); return; }
    alloc_tensor(t, esz);
    upload(t, esz);
    a.n = 1; a.t[0] = arg_of(t, a.update, esz);
    RT(rtx_launch_adam(a, bf16, 0));
    CK(hipDeviceSynchronize());
    std::vector<Tensor*> ts(1, &t);
    check_route(a, ts, L);
    Snap sn;
    check_tensor(t, a, v.s.mode, esz, L, sn);
    report(name, L);
    free_all();
}

// several tensors in one launch: every element of every tensor updated exactly once (a tile visited twice moves p twice: in place),
// and the launch bit-identical to its tensors launched one by one
static void multi_case(const char* what, const std::vector<Spec>& specs, const Scal& sc, int want_tiles, int bf16, uint32_t seed)
{
    const int esz = bf16 ? 2 : 4;
    Rng r = {seed};
    std::vector<Tensor> T(specs.size());
    for (size_t k = 0; k < specs.size(); ++k) gen_tensor(T[k], specs[k], sc.mode, r);
    char name[200];
    snprintf(name, sizeof name, "A k_adam<%s> %s: %zu tensors, %d tiles, step %d wd %g lam %g gs %g%s", bf16 ? "bf16" : "f32", what, specs.size(), want_tiles,
             sc.step, sc.wd, sc.lam, sc.gs, sc.mode == REFRESH ? ", update == 0" : "");
    Line L;
    RtxAdamArgs a = {};
    scalars(a, sc);
    std::vector<Tensor*> ts;
    int tiles = 0;
    for (Tensor& t : T) { ts.push_back(&t); tiles += t.tiles(); }
    if (tiles != want_tiles) host_fail(L, "the case holds %g tiles, meant %g", tiles, want_tiles);
    if (g_host) { for (Tensor& t : T) host_check_tensor(t, a, sc.mode, L); report(name, L); return; }
    a.n = (int)T.size();
    for (size_t k = 0; k < T.size(); ++k) { alloc_tensor(T[k], esz); upload(T[k], esz); a.t[k] = arg_of(T[k], a.update, esz); }
    RT(rtx_launch_adam(a, bf16, 0));
    CK(hipDeviceSynchronize());
    check_route(a, ts, L);
    std::vector<Snap> together(T.size());
    for (size_t k = 0; k < T.size(); ++k) {
        char tag[32]; snprintf(tag, sizeof tag, "tensor %zu", k); g_tag = tag;
        check_tensor(T[k], a, sc.mode, esz, L, together[k]);
    }
    long differ = 0;
    for (size_t k = 0; k < T.size(); ++k) {
        if (!T[k].n) continue;
        upload(T[k], esz);
        RtxAdamArgs one = {};
        scalars(one, sc);
        one.n = 1; one.t[0] = arg_of(T[k], one.update, esz);
        RT(rtx_launch_adam(one, bf16, 0));
        CK(hipDeviceSynchronize());
        Line unused;
        Snap alone;
        g_tag = "(alone)";
        check_tensor(T[k], one, sc.mode, esz, unused, alone);
        if (!same(together[k], alone)) { if (L.bad < 4) printf("    tensor %zu differs from its own launch\n", k); ++L.bad; ++differ; }
    }
    g_tag.clear();
    report(name, L, differ ? "" : "  = one by one, bit for bit");
    free_all();
}

// one tensor on two routes: the same values at an aligned address (flat) and offset by one row (2-D).  Reported, not asserted:
// contraction may differ between the unrolled bodies.
static void route_compare(const Spec& shard, int bf16, uint32_t seed)
{
    if (g_host) return;
    const int esz = bf16 ? 2 : 4;
    Spec two[2] = {shard, shard};
    two[0].mat_rows = shard.rows; two[0].row_lo = 0; two[0].route = FLAT;
    two[1].mat_rows = shard.rows + 1; two[1].row_lo = 1;
    const Scal sc = {DRAWN, 1000, 0.01f, 0.5f, 0.125f};
    Snap sn[2];
    Line L;
    for (int w = 0; w < 2; ++w) {
        Rng r = {seed};
        Tensor t;
        two[w].sumsq = 1;
        gen_tensor(t, two[w], DRAWN, r);
        if (w) {      // the same state behind one row of junk (gen_tensor drew the junk first: redraw the shard from the same seed)
            Rng r0 = {seed};
            Tensor base;
            gen_tensor(base, two[0], DRAWN, r0);
            std::copy(base.p.begin(), base.p.end(), t.p.begin() + t.off); std::copy(base.m.begin(), base.m.end(), t.m.begin() + t.off);
            std::copy(base.v.begin(), base.v.end(), t.v.begin() + t.off); std::copy(base.g.begin(), base.g.end(), t.g.begin() + t.off);
            std::copy(base.g_dev.begin(), base.g_dev.end(), t.g_dev.begin() + t.off);
            if (shard.g16) std::copy(base.g16.begin(), base.g16.end(), t.g16.begin() + t.off);
            t.sumsq = base.sumsq;
        }
        alloc_tensor(t, esz);
        upload(t, esz);
        RtxAdamArgs a = {};
        scalars(a, sc);
        a.n = 1; a.t[0] = arg_of(t, 1, esz);
        RT(rtx_launch_adam(a, bf16, 0));
        CK(hipDeviceSynchronize());
        std::vector<Tensor*> ts(1, &t);
        check_route(a, ts, L);
        Snap all;
        check_tensor(t, a, DRAWN, esz, L, all);
        sn[w].p.assign(all.p.begin() + t.off, all.p.begin() + t.off + t.n); sn[w].m.assign(all.m.begin() + t.off, all.m.begin() + t.off + t.n);
        sn[w].v.assign(all.v.begin() + t.off, all.v.begin() + t.off + t.n);
        free_all();
    }
    long dp = 0, dm = 0, dv = 0;
    for (size_t k = 0; k < sn[0].p.size(); ++k) {
        dp += f_bits(sn[0].p[k]) != f_bits(sn[1].p[k]); dm += f_bits(sn[0].m[k]) != f_bits(sn[1].m[k]); dv += f_bits(sn[0].v[k]) != f_bits(sn[1].v[k]);
    }
    char name[200], extra[120];
    snprintf(name, sizeof name, "A k_adam<%s> %dx%d%s flat against %s", bf16 ? "bf16" : "f32", shard.rows, shard.cols, shard.g16 ? " g16" : "", ROUTE_NAME[shard.route]);
    snprintf(extra, sizeof extra, "  elements whose bits differ between the routes: p %ld, m %ld, v %ld of %zu (reported)", dp, dm, dv, sn[0].p.size());
    report(name, L, extra);
}

static Spec with(Spec s, int g16, int sumsq) { if (s.g16 != 2) s.g16 = g16; s.sumsq = sumsq; return s; }

static void adam_cases()
{
    uint32_t seed = 100;
    for (int bf16 = 0; bf16 < 2; ++bf16)
        for (const Variant& v : VARIANTS) {
            for (const Spec& s : FLAT_SHAPES)
                for (int sh = 0; sh < 2; ++sh) { Spec c = s; c.sh = sh; single_case(c, v, bf16, ++seed); }
            for (const Spec& s : T_SHAPES) single_case(s, v, bf16, ++seed);
            single_case(SHARD_A, v, bf16, ++seed);
            single_case(SHARD_B, v, bf16, ++seed);
        }
    const Spec *F = FLAT_SHAPES, *T = T_SHAPES;
    Spec zero_rows = {0, 10, 0, 0, 1, 0, 0, 1, FLAT}, f_sh[7];
    for (int k = 0; k < 7; ++k) { f_sh[k] = F[k]; f_sh[k].sh = k != 0 && k != 3; }
    const Scal S1 = {DRAWN, 1, 0.f, 0.f, 1.f}, S2 = {DRAWN, 1000, 0.01f, 0.5f, 0.125f}, S0 = {REFRESH, 1, 0.f, 0.f, 1.f};
    // (g16, sumsq) mixed within a launch: given for some tensors, null for others, one all-zero tensor with *sumsq == 0
    const std::vector<Spec> M1 = {with(zero_rows, 0, 1), with(f_sh[3], 1, 1)};
    const std::vector<Spec> M7 = {with(T[1], 0, 1), with(f_sh[4], 1, 0), with(SHARD_A, 0, 1)};
    const std::vector<Spec> M8 = {with(T[2], 1, 0), with(T[6], 0, 2), with(f_sh[6], 0, 1)};
    const std::vector<Spec> M9 = {with(T[3], 1, 1), with(T[1], 1, 0), with(f_sh[2], 0, 2), with(SHARD_B, 1, 1)};
    const std::vector<Spec> M17 = {with(T[1], 0, 0), with(T[2], 0, 1), with(T[6], 1, 1), with(f_sh[5], 1, 0), with(T[4], 0, 1), with(T[5], 1, 2), with(T[0], 0, 1)};
    std::vector<Spec> M32;      // RTX_MAX_TENSORS tensors, one of zero rows in the middle
    int t32 = 0;
    {
        std::vector<Spec> pool(f_sh, f_sh + 7);
        pool.insert(pool.end(), T, T + 7);
        pool.push_back(SHARD_A); pool.push_back(SHARD_B);
        for (int k = 0; k < RTX_MAX_TENSORS; ++k) {
            M32.push_back(k == 15 ? with(zero_rows, 0, 1) : with(pool[(k * 5) % pool.size()], k % 2, k % 3));
            Tensor probe; probe.s = M32.back(); probe.n = (size_t)probe.s.rows * probe.s.cols;
            t32 += probe.tiles();
        }
    }
    for (int bf16 = 0; bf16 < 2; ++bf16)
        for (const Scal& sc : {S1, S2, S0}) {
            multi_case("a tensor of zero rows first", M1, sc, 1, bf16, ++seed);
            multi_case("2-D + flat + shard", M7, sc, 7, bf16, ++seed);
            multi_case("2-D + 2-D + flat", M8, sc, 8, bf16, ++seed);
            multi_case("4-byte + float4 + flat + g16 shard", M9, sc, 9, bf16, ++seed);
            multi_case("seven tensors", M17, sc, 17, bf16, ++seed);
            multi_case("RTX_MAX_TENSORS", M32, sc, t32, bf16, ++seed);
        }
    for (int bf16 = 0; bf16 < 2; ++bf16) { route_compare(SHARD_A, bf16, ++seed); route_compare(SHARD_B, bf16, ++seed); }
}

// =====================================================================================================================================
// C: rtx_launch_cast_f32_bf16
// =====================================================================================================================================
static const uint32_t CAST_SPECIAL[] = {
    0x3f808000u, 0x3f818000u, 0xbf808000u, 0xbf818000u,      // ties: to even down, to even up, both signs
    0x3f7fffffu, 0x3fffc000u, 0x7f7fffffu, 0xff7fffffu,      // round up into the next exponent; the largest finite value -> infinity
    0x7f800000u, 0xff800000u, 0x00000000u, 0x80000000u,      // +-inf, +-0
    0x00000001u, 0x00008000u, 0x00018000u, 0x007fffffu, 0x807f8001u,      // subnormals
    0x7fc00000u, 0x7f800001u, 0xffa00000u, 0x7fc12345u, 0x7f80ffffu};     // NaNs with and without the quiet bit, payload in the low half only
static const int N_CAST_SPECIAL = sizeof CAST_SPECIAL / sizeof CAST_SPECIAL[0];

static void cast_case(long n, int idx, uint32_t seed)
{
    Rng r = {seed};
    std::vector<float> src((size_t)n + 8);      // (behind n: junk the kernel has no business with)
    for (long k = 0; k < n + 8; ++k)
        src[k] = k >= n ? r.junk() : (k < 2 * N_CAST_SPECIAL || k % 4 == 0) ? bits_f(CAST_SPECIAL[(k + 5 * idx) % N_CAST_SPECIAL]) : bits_f((r.u() << 8) ^ r.u());
    char name[120];
    snprintf(name, sizeof name, "C k_cast_f32_bf16 n=%ld", n);
    Line L;
    if (g_host) {
        for (long k = 0; k < n; ++k)
            if (rne_by_hand(f_bits(src[k])) != f32_to_bf16(src[k])) host_fail(L, "element %g: the two roundings differ on the host", (double)k);
        report(name, L);
        return;
    }
    float* d_src = to_dev(src);
    uint16_t* d_dst = dev_out<uint16_t>(n);
    RT(rtx_launch_cast_f32_bf16(d_src, d_dst, n, 0));
    CK(hipDeviceSynchronize());
    const std::vector<uint16_t> dst = fetch<uint16_t>(d_dst, n, L, "dst");
    for (long k = 0; k < n; ++k) judge_bits(dst[k], rne_by_hand(f_bits(src[k])), L, "dst", k);
    report(name, L);
    free_all();
}

// =====================================================================================================================================
// D: rtx_launch_dw_slab_reduce
// =====================================================================================================================================
static void slab_case(int splits, int M, int N, int with_bias, uint32_t seed)
{
    Rng r = {seed};
    const int M_pad = M + 3;
    const long ldc = N + 1 + 5, stride = (long)M_pad * ldc + 37;
    std::vector<float> C((size_t)splits * stride);
    for (int s = 0; s < splits; ++s)
        for (long k = 0; k < stride; ++k) {
            const long m = k / ldc, n = k % ldc;
            C[(size_t)s * stride + k] = (m < M && n <= N) ? r.f() : r.junk();
        }
    char name[160];
    snprintf(name, sizeof name, "D k_dw_slab_reduce splits=%d %dx%d ldc=%ld slab_stride=%ld gbias %s", splits, M, N, ldc, stride, with_bias ? "given" : "null");
    Line L;
    auto sum = [&](int m, int n, long double* exact, long double* abs_sum) {      // float32 additions in slab order from +0
        float v = 0.f;
        long double e = 0, a = 0;
        for (int s = 0; s < splits; ++s) { const float c = C[(size_t)s * stride + (size_t)m * ldc + n]; v += c; e += c; a += fabsl(c); }
        if (exact) { *exact = e; *abs_sum = a; }
        return v;
    };
    if (g_host) {
        long nbad = 0;
        for (int s = 0; s < splits; ++s)
            for (long k = 0; k < stride; ++k) if (!(k / ldc < M && k % ldc <= N)) nbad += !is_junk(C[(size_t)s * stride + k]);
        if (nbad) host_fail(L, "%g masked slab elements hold no junk", (double)nbad);
        if (!(ldc > N + 1 && stride > M_pad * ldc)) host_fail(L, "no gap");
        for (int m = 0; m < M; ++m)
            for (int n = 0; n <= N; ++n) {
                long double e, a;
                const float f = sum(m, n, &e, &a);
                if (!(fabsl(e - f) <= splits * E24 * a)) host_fail(L, "slab sum %.9g, long double %.9g", f, (double)e);
            }
        report(name, L);
        return;
    }
    const float* d_C = to_dev(C);
    float* gW = dev_out<float>((size_t)M * N);
    float* gb = dev_out<float>(M);
    RT(rtx_launch_dw_slab_reduce(d_C, splits, stride, ldc, M, N, gW, with_bias ? gb : nullptr, 0));
    CK(hipDeviceSynchronize());
    const std::vector<float> W = fetch<float>(gW, (size_t)M * N, L, "gW"), B = fetch<float>(gb, M, L, "gbias");
    for (int m = 0; m < M; ++m) {
        for (int n = 0; n < N; ++n) judge_bits(f_bits(W[(size_t)m * N + n]), f_bits(sum(m, n, nullptr, nullptr)), L, "gW", m, n);
        judge_bits(f_bits(B[m]), with_bias ? f_bits(sum(m, N, nullptr, nullptr)) : 0xffffffffu, L, with_bias ? "gbias" : "gbias (not passed)", m);
    }
    report(name, L);
    free_all();
}

// =====================================================================================================================================
// S: rtx_launch_sumsq
// =====================================================================================================================================
// Bound: a thread squares and adds its k = ceil(n / (256 grid)) elements (k + 1 roundings at most on its partial sum), the 64-lane
// butterfly adds 6 levels, the block 3 wave partials, and the grid's atomics arrive in any order: grid - 1 more additions, each rounding
// a partial sum <= the total.  All terms are >= 0, so every partial sum is <= sum p^2:  (k + 1 + 6 + 3 + grid - 1) 2^-24 sum p^2.
static void sumsq_case()
{
    const long sizes[6] = {1, 255, 256, 4097, 1024L * 4096 + 3, 1000};
    Rng r = {4242};
    std::vector<std::vector<float>> P(6);
    double want[6], bound[6];
    for (int t = 0; t < 6; ++t) {
        P[t].resize(sizes[t]);
        double s = 0;
        for (float& x : P[t]) { x = t == 5 ? 0.f : r.f(); s += (double)x * x; }
        const long grid = std::min<long>(1024, std::max<long>(1, (sizes[t] + 4095) / 4096)), k = (sizes[t] + 256 * grid - 1) / (256 * grid);
        want[t] = s;
        bound[t] = (double)(k + 1 + 6 + 3 + grid - 1) * E24 * s;
    }
    const char* name = "S k_sumsq 1, 255, 256, 4097, 1024 * 4096 + 3 elements and 1000 zeros, two calls";
    Line L;
    if (g_host) {
        for (int t = 0; t < 6; ++t) {      // the float64 sum against long double, summed backwards (n roundings of 2^-53 at most)
            long double s = 0;
            for (long k = sizes[t] - 1; k >= 0; --k) s += (long double)P[t][k] * P[t][k];
            if (!(fabsl(s - want[t]) <= sizes[t] * 1.2e-16L * s)) host_fail(L, "sum of squares %.17g, long double %.17g", want[t], (double)s);
        }
        if (want[5] != 0) host_fail(L, "the zero tensor is not zero");
        if ((sizes[4] + 4095) / 4096 <= 1024) host_fail(L, "the largest tensor does not reach the grid cap");
        report(name, L);
        return;
    }
    const float* ptrs[6];
    for (int t = 0; t < 6; ++t) ptrs[t] = to_dev(P[t]);
    float* d_out = dev_out<float>(6);      // poisoned: the launcher's memset has work to do in both calls
    for (int call = 0; call < 2; ++call) {
        RT(rtx_launch_sumsq(ptrs, sizes, 6, d_out, 0));
        CK(hipDeviceSynchronize());
        const std::vector<float> out = fetch<float>(d_out, 6, L, "sumsq");
        g_tag = call ? "(second call)" : "(first call)";
        for (int t = 0; t < 6; ++t) {
            if (want[t] == 0) judge_bits(f_bits(out[t]), 0, L, "sumsq of zeros", t);
            else g_sumsq_worst = std::max(g_sumsq_worst, judge(out[t], want[t], bound[t], L, "sumsq", t));
        }
    }
    g_tag.clear();
    report(name, L);
    free_all();
}

// =====================================================================================================================================
// --host only
// =====================================================================================================================================
static void host_only_cases()
{
    {   // 1.f - beta in float32 is exact for both betas (Sterbenz: 1 / 2 <= beta <= 2)
        Line L;
        for (float b : {BETA1, BETA2})
            if ((double)(1.f - b) != 1.0 - (double)b) host_fail(L, "1.f - %.9g is rounded", b);
        report("H 1.f - beta1 and 1.f - beta2 are exact in float32", L);
    }
    {   // the hand-written rounding against the host build of f32_to_bf16: every high half, six low halves each
        Line L;
        static const uint32_t LOW[6] = {0, 1, 0x7fff, 0x8000, 0x8001, 0xffff};
        for (uint32_t hi = 0; hi < 65536; ++hi)
            for (uint32_t lo : LOW) {
                const uint32_t u = (hi << 16) | lo;
                if (rne_by_hand(u) != f32_to_bf16(bits_f(u))) host_fail(L, "bits %g: by hand %g", u, rne_by_hand(u));
            }
        report("H round-to-nearest-even by hand == f32_to_bf16 (host build), 65 536 x 6 bit patterns", L);
    }
    for (int step : {1, 1000})      // the float64 reference against orc_adam (float32 results from float64 arithmetic, scalars in float64), lam = 0
        for (float wd : {0.f, 0.01f}) {
            Line L;
            Rng r = {777u + step};
            Tensor t;
            const Spec s = {70, 100, 70, 0, 0, 0, 0, 0, FLAT};
            gen_tensor(t, s, DRAWN, r);
            RtxAdamArgs a = {};
            const Scal sc = {DRAWN, step, wd, 0.f, 1.f};
            scalars(a, sc);
            std::vector<float> p = t.p, m = t.m, v = t.v;
            orc_adam((int64_t)t.n, p.data(), t.g.data(), m.data(), v.data(), step, (float)LR, BETA1, BETA2, EPS, wd);
            for (size_t k = 0; k < t.n; ++k) {
                const Ref ref = adam_ref(t.p[k], t.g[k], t.m[k], t.v[k], 0.0, a);
                // the oracle rounds p', m', v' to float32 once; its step size and bias correction are float64 where the launch passes
                // float32 (one rounding each, on the step ss m'/D), and its lr is the float32 1e-3f
                judge(p[k], ref.p, E24 * fabs(ref.p) + 4 * E24 * fabs(ref.p - t.p[k]), L, "p against orc_adam", (long)k);
                judge(m[k], ref.m, E24 * fabs(ref.m), L, "m against orc_adam", (long)k);
                judge(v[k], ref.v, E24 * fabs(ref.v), L, "v against orc_adam", (long)k);
            }
            char name[120];
            snprintf(name, sizeof name, "H float64 reference against orc_adam, step %d, weight_decay %g", step, wd);
            report(name, L);
        }
    // the launchers' returns that come before the first HIP call
    auto ret = [](const char* what, int rc, int want) {
        Line L;
        if (rc != want) host_fail(L, "returned %g, expected %g", rc, want);
        char name[160];
        snprintf(name, sizeof name, "R %s: %s", what, want == RTX_EINVAL ? "refused" : "RTX_OK, nothing launched");
        report(name, L, rc == RTX_EINVAL ? (std::string("  [") + rtx_last_error_str() + "]").c_str() : "");
    };
    static float dummy[16] __attribute__((aligned(16)));
    RtxAdamArgs a = {};
    a.n = 0;
    ret("adam, no tensor", rtx_launch_adam(a, 0, 0), RTX_EINVAL);
    a.n = RTX_MAX_TENSORS + 1;
    ret("adam, 33 tensors", rtx_launch_adam(a, 0, 0), RTX_EINVAL);
    a = {};
    a.n = 2; a.total_tiles = -7;
    a.t[0].p = dummy; a.t[0].rows = 0; a.t[0].cols = 10; a.t[1].p = dummy; a.t[1].rows = 5; a.t[1].cols = 0; a.t[1].shT = dummy;
    ret("adam, tensors without elements", rtx_launch_adam(a, 1, 0), RTX_OK);
    ret("cast, src 4 bytes off", rtx_launch_cast_f32_bf16(dummy + 1, (bf16_t*)dummy, 8, 0), RTX_EINVAL);
    ret("cast, dst 2 bytes off", rtx_launch_cast_f32_bf16(dummy, (bf16_t*)dummy + 1, 8, 0), RTX_EINVAL);
    ret("cast, n = 0", rtx_launch_cast_f32_bf16(dummy, (bf16_t*)dummy, 0, 0), RTX_OK);
    ret("cast, n = -5", rtx_launch_cast_f32_bf16(dummy + 1, (bf16_t*)dummy, -5, 0), RTX_OK);
    ret("slab reduce, M_real = 0", rtx_launch_dw_slab_reduce(dummy, 2, 64, 8, 0, 7, dummy, dummy, 0), RTX_OK);
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    g_name_width = 84;
    setvbuf(stdout, nullptr, _IOLBF, 0);
    adam_cases();
    int idx = 0;
    for (long n : {1L, 7L, 8L, 9L, 2047L, 2048L, 2049L, 4100L}) cast_case(n, idx++, 9000u + (uint32_t)n);
    static const int MN[3][2] = {{5, 7}, {3, 300}, {64, 1}};
    uint32_t seed = 9500;
    for (int splits : {1, 2, 17})
        for (const auto& mn : MN)
            for (int with_bias = 0; with_bias < 2; ++with_bias) slab_case(splits, mn[0], mn[1], with_bias, ++seed);
    sumsq_case();
    if (g_host) host_only_cases();
    else {
        printf("worst error / bound by quantity and walk (DESIGN.md section 6):\n");
        for (int rt = 0; rt < NROUTE; ++rt)
            for (int q = 0; q < NQA; ++q) printf("    k_adam %-12s %s   %.4f   (%ld elements)\n", ROUTE_NAME[rt], QA_NAME[q], g_qworst[rt][q], g_qn[rt][q]);
        printf("    k_sumsq                  %.4f\n", g_sumsq_worst);
    }
    return finish("ADAM");
}
