// Native (no Python) check of the update rules of adam.hip's multi-tensor walk, k_optim<T, Rule> behind rtx_launch_adam, against plain
// float64 host code: every rule (Adam, decoupled Adam / AdamW, SGD without and with momentum -- first update, later update, nesterov --,
// Adagrad, RMSprop without and with momentum) on every walk of the kernel (flat whole tile, flat tail with nv < 4, 2-D float4 tiles, 2-D
// 4-byte tiles, the transposed compute copy through the LDS tile), with the tensor shapes, the row shards and the poison / guard
// discipline of section A of test_adam.cpp (whose Adam cases run the same kernel, instantiated for Adam): p and the state slots the rule
// keeps carry a poisoned guard, the compute copies are poisoned before each launch, rows outside a shard and the float32 gradient under
// a bf16 image hold finite junk of magnitude ~1e3 -- and so does every state slot the rule does NOT keep, which must come back bit for
// bit (a rule with fewer state tensors neither loads nor stores the others).  Multi-tensor launches, and update == 0 under every rule.
// The scalars of a launch come from rtx_optim_scalars, as the engine's do.
//
// One case is ONE update from a drawn state (p in +-1, m in +-0.1, v >= 0 with exact 0, 1e-30 and 10, g in +-1 with exact zeros), so
// every bound is a one-update bound; the reference reads the same float32 bits and the float32 scalars of the launch.  With
// d = 2^-24 (one float32 rounding, relative; sqrtf and the division are correctly rounded), first order, a fused multiply-add only
// removing roundings.  The prepared gradient is test_adam.cpp's:
//   g  = gv gs + reg pv + wd pv         a = gv gs, b = reg pv, c = wd pv (c = 0 where the decay is decoupled)
//        e_g = d (3 |a| + 5 |b| + 2 |c|)
// Adam:     test_adam.cpp's bounds.  Decoupled: p1 = p decay first, e_p1 = d |p1|, carried into e_p.
// SGD:      buf = first ? g : m mom + damp1 g      e_b = first ? e_g : d (|m mom| + damp1 |g|) + damp1 e_g + d |buf|
//           D = nesterov ? g + mom buf : buf       e_D = nesterov ? e_g + mom e_b + d |mom buf| + d |D| : e_b      (no momentum: D = g)
//           p' = p - lr D                           e_p = lr e_D + d lr |D| + d |p'|
// Adagrad:  v' = v + g g                            e_v = 2 |g| e_g + e_g^2 + d g^2 + d v'
//           S = sqrtf(v') + eps                     e_S = e_v / (sqrt(v') + sqrt(max(v' - e_v, 0))) + d sqrt(v') + d S
//           q = g / S                               e_q = (e_g + |q| e_S) / (S - e_S) + d |q|
//           p' = p - clr q                          e_p = clr e_q + d clr |q| + d |p'|
// RMSprop:  v' = v al + al1 g g                     e_v = d v al + 2 d al1 g^2 + al1 (2 |g| e_g + e_g^2) + d v'     (as Adam's)
//           S, q as Adagrad's; without momentum p' = p - lr q as Adagrad's with lr;
//           buf = m mom + q                         e_b = d |m mom| + e_q + d |buf|
//           p' = p - lr buf                         e_p = lr e_b + d lr |buf| + d |p'|
// Each is a count of roundings times the quantity's own scale, term by term.  By the rule of DESIGN.md section 6 a bound stays as
// derived unless the measured worst error stays below 0.05 of it; the table this driver prints is what that rule reads.
//   test_optim          the device run
//   test_optim --host   no HIP call: the float64 references against a second formulation in long double (other operation order), SGD's
//                       first update and Adagrad's clr against torch's formulas restated in long double from the optimizer's own
//                       hyper-parameters, what rtx_optim_validate refuses
#include "../../rectorch_amd/csrc/rtx_kernels.h"

#include "check.h"

static const float BETA1 = 0.9f, BETA2 = 0.999f;
static int r128(int z) { return (z + 127) / 128 * 128; }

enum { FLAT, VEC2D, ELEM2D, NROUTE };
static const char* const ROUTE_NAME[NROUTE] = {"flat", "2-D float4", "2-D 4-byte"};

// ---- the rules under test -----------------------------------------------------------------------------------------------------------
struct RuleCase {
    const char* name;
    RtxOptim o;
    float lr, eps;
    bool use_m, use_v;
};
static RtxOptim mk(int kind, int flags, double mom, double damp, double alpha, double lr_decay)
{
    RtxOptim o;
    o.kind = kind; o.flags = flags; o.momentum = mom; o.dampening = damp; o.alpha = alpha; o.lr_decay = lr_decay;
    return o;
}
static const RuleCase RULES[] = {
    {"Adam", mk(RTX_OPT_ADAM, 0, 0, 0, 0, 0), 1e-3f, 1e-8f, true, true},
    {"AdamW", mk(RTX_OPT_ADAM, RTX_OPTF_DECOUPLED, 0, 0, 0, 0), 1e-3f, 1e-8f, true, true},
    {"SGD", mk(RTX_OPT_SGD, 0, 0, 0, 0, 0), 0.05f, 0.f, false, false},
    {"SGD momentum, first", mk(RTX_OPT_SGD, RTX_OPTF_FIRST, 0.9, 0.1, 0, 0), 0.05f, 0.f, true, false},
    {"SGD momentum", mk(RTX_OPT_SGD, 0, 0.9, 0.1, 0, 0), 0.05f, 0.f, true, false},
    {"SGD nesterov", mk(RTX_OPT_SGD, RTX_OPTF_NESTEROV, 0.9, 0, 0, 0), 0.05f, 0.f, true, false},
    {"SGD nesterov, first", mk(RTX_OPT_SGD, RTX_OPTF_NESTEROV | RTX_OPTF_FIRST, 0.9, 0, 0, 0), 0.05f, 0.f, true, false},
    {"Adagrad", mk(RTX_OPT_ADAGRAD, 0, 0, 0, 0, 0.1), 0.05f, 1e-10f, false, true},
    {"RMSprop", mk(RTX_OPT_RMSPROP, 0, 0, 0, 0.99, 0), 1e-3f, 1e-8f, false, true},
    {"RMSprop momentum", mk(RTX_OPT_RMSPROP, 0, 0.5, 0, 0.9, 0), 1e-3f, 1e-8f, true, true},
};
static const int N_RULES = sizeof RULES / sizeof RULES[0];
enum { Q_P, Q_M, Q_V, NQ };
static const char* const Q_NAME[NQ] = {"p", "m", "v"};
static double g_worst[N_RULES][NROUTE][NQ];
static long g_n[N_RULES][NROUTE][NQ];

// ---- one tensor ---------------------------------------------------------------------------------------------------------------------
enum { DRAWN, REFRESH };
struct Spec {
    int rows, cols, mat_rows, row_lo;      // rows [row_lo, row_lo + rows) of a [mat_rows][cols] matrix
    int sh, shT, g16, sumsq, route;
};
struct Scal { int mode, step; float wd, lam, gs; };
struct Tensor {
    Spec s;
    int ld_sh = 0, ld_shT = 0;
    size_t n_mat = 0, off = 0, n = 0;
    std::vector<float> p, g, m, v, g_dev;
    std::vector<uint16_t> g16;
    float sumsq = 0;
    float *dp = nullptr, *dg = nullptr, *dm = nullptr, *dv = nullptr, *dss = nullptr;
    uint16_t* dg16 = nullptr;
    unsigned char *dsh = nullptr, *dshT = nullptr;
    int tiles() const { return s.route == FLAT ? (int)((n + 4095) / 4096) : ((s.rows + 63) / 64) * ((s.cols + 63) / 64); }
};

static void gen_tensor(Tensor& t, const Spec& s, const RuleCase& rc, Rng& r)
{
    t.s = s;
    t.n_mat = (size_t)s.mat_rows * s.cols; t.off = (size_t)s.row_lo * s.cols; t.n = (size_t)s.rows * s.cols;
    t.ld_sh = r128(s.cols); t.ld_shT = r128(s.rows);
    t.p.resize(t.n_mat); t.g.resize(t.n_mat); t.m.resize(t.n_mat); t.v.resize(t.n_mat); t.g_dev.resize(t.n_mat);
    t.g16.assign(s.g16 ? t.n_mat : 0, 0);
    double ss = 0;
    for (size_t k = 0; k < t.n_mat; ++k) {
        const bool in = k >= t.off && k < t.off + t.n;
        const size_t i = k - t.off;
        t.p[k] = in ? r.f() : r.junk();
        const float md = 0.1f * r.f(), u = r.u01();
        // a slot the rule does not keep holds junk everywhere: it must come back untouched
        t.m[k] = in && rc.use_m ? md : r.junk();
        t.v[k] = !(in && rc.use_v) ? r.junk() : i % 7 == 0 ? 0.f : i % 7 == 1 ? 1e-30f : i % 7 == 2 ? 10.f : u * u;
        float g = in ? (i % 5 == 0 ? 0.f : r.f()) : r.junk();
        if (s.g16) { t.g16[k] = f32_to_bf16(g); g = bf16_to_f32(t.g16[k]); }
        t.g[k] = g;
        t.g_dev[k] = s.g16 ? r.junk() : g;
        if (in) ss += (double)t.p[k] * t.p[k];
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
// the scalars of the launch, as the engine fills them
static void scalars(RtxAdamArgs& a, const RuleCase& rc, const Scal& s, Line& L)
{
    if (rtx_optim_scalars(rc.o, rc.lr, BETA1, BETA2, rc.eps, s.wd, s.step, a) != RTX_OK) host_fail(L, "rtx_optim_scalars refused the rule");
    a.update = s.mode != REFRESH;
    a.lam = s.lam; a.grad_scale = s.gs;
}
static RtxAdamTensor arg_of(const Tensor& t, int esz)
{
    RtxAdamTensor w = {};
    w.p = t.dp + t.off; w.g = t.dg + t.off; w.m = t.dm + t.off; w.v = t.dv + t.off;      // (every slot bound, kept by the rule or not)
    if (t.dg16) w.g16 = t.dg16 + t.off;
    if (t.dsh) w.sh = t.dsh + (size_t)t.s.row_lo * t.ld_sh * esz;
    w.shT = t.dshT;
    w.sumsq = t.dss;
    w.rows = t.s.rows; w.cols = t.s.cols; w.ld_sh = t.ld_sh; w.ld_shT = t.ld_shT;
    return w;
}

// ---- the float64 references and their bounds (header) ---------------------------------------------------------------------------------
struct Ref { double p, m, v, ep, em, ev; };
static Ref rule_ref(float pv, float gv, float mv, float vv, double reg, const RtxAdamArgs& A)
{
    const bool decoupled = A.rule == RTX_RULE_ADAMW;
    const double a = (double)gv * A.grad_scale, b = reg * pv, c = decoupled ? 0.0 : (double)A.weight_decay * pv;
    const double g = a + b + c, eg = E24 * (3 * fabs(a) + 5 * fabs(b) + 2 * fabs(c));
    Ref r = {};
    r.m = mv; r.v = vv;
    auto sq_den = [&](double v, double ev, double eps, double* S, double* eS) {
        const double sq = sqrt(v);
        *S = sq + eps;
        *eS = (ev > 0 ? ev / (sq + sqrt(std::max(v - ev, 0.0))) : 0.0) + E24 * sq + E24 * *S;
    };
    switch (A.rule) {
    case RTX_RULE_ADAM: case RTX_RULE_ADAMW: {
        const double p1 = decoupled ? (double)pv * A.decay : (double)pv, ep1 = decoupled ? E24 * fabs(p1) : 0.0;
        const double ob1 = (double)(1.f - A.beta1), ob2 = (double)(1.f - A.beta2);
        r.m = mv + (g - mv) * ob1;
        r.em = ob1 * eg + 2 * E24 * ob1 * fabs(g - mv) + E24 * fabs(r.m);
        r.v = (double)vv * A.beta2 + ob2 * g * g;
        r.ev = E24 * (double)vv * A.beta2 + 2 * E24 * ob2 * g * g + ob2 * (2 * fabs(g) * eg + eg * eg) + E24 * r.v;
        const double sq = sqrt(r.v), D = sq / A.bc2_sqrt + A.eps;
        const double dsq = r.ev > 0 ? r.ev / (sq + sqrt(std::max(r.v - r.ev, 0.0))) : 0.0;
        const double eD = (dsq + 2 * E24 * sq) / A.bc2_sqrt + E24 * D;
        const double q = r.m / D, eq = (r.em + fabs(q) * eD) / (D - eD) + E24 * fabs(q);
        r.p = p1 - (double)A.step_size * q;
        r.ep = ep1 + A.step_size * eq + E24 * A.step_size * fabs(q) + E24 * fabs(r.p);
        break;
    }
    case RTX_RULE_SGD: case RTX_RULE_SGD_MOM: {
        double D = g, eD = eg;
        if (A.rule == RTX_RULE_SGD_MOM) {
            const double mm = (double)mv * A.momentum;
            const double buf = A.first ? g : mm + (double)A.damp1 * g;
            const double eb = A.first ? eg : E24 * (fabs(mm) + A.damp1 * fabs(g)) + A.damp1 * eg + E24 * fabs(buf);
            r.m = buf; r.em = eb;
            if (A.nesterov) {
                D = g + (double)A.momentum * buf;
                eD = eg + A.momentum * eb + E24 * fabs(A.momentum * buf) + E24 * fabs(D);
            } else { D = buf; eD = eb; }
        }
        r.p = pv - (double)A.lr * D;
        r.ep = A.lr * eD + E24 * A.lr * fabs(D) + E24 * fabs(r.p);
        break;
    }
    case RTX_RULE_ADAGRAD: case RTX_RULE_RMSPROP: case RTX_RULE_RMSPROP_MOM: {
        if (A.rule == RTX_RULE_ADAGRAD) {
            r.v = (double)vv + g * g;
            r.ev = 2 * fabs(g) * eg + eg * eg + E24 * g * g + E24 * r.v;
        } else {
            r.v = (double)vv * A.alpha + (double)A.alpha1 * g * g;
            r.ev = E24 * (double)vv * A.alpha + 2 * E24 * A.alpha1 * g * g + A.alpha1 * (2 * fabs(g) * eg + eg * eg) + E24 * r.v;
        }
        double S, eS;
        sq_den(r.v, r.ev, A.eps, &S, &eS);
        const double q = g / S, eq = (eg + fabs(q) * eS) / (S - eS) + E24 * fabs(q);
        double D = q, eD = eq;
        if (A.rule == RTX_RULE_RMSPROP_MOM) {
            const double mm = (double)mv * A.momentum;
            D = mm + q;
            eD = E24 * fabs(mm) + eq + E24 * fabs(D);
            r.m = D; r.em = eD;
        }
        r.p = pv - (double)A.lr * D;
        r.ep = A.lr * eD + E24 * A.lr * fabs(D) + E24 * fabs(r.p);
        break;
    }
    }
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

struct Snap { std::vector<float> p, m, v; std::vector<unsigned char> sh, shT; };
static void check_tensor(const Tensor& t, const RtxAdamArgs& A, int ri, int mode, int esz, Line& L, Snap& sn)
{
    const RuleCase& rc = RULES[ri];
    sn.p = fetch<float>(t.dp, t.n_mat, L, "p"); sn.m = fetch<float>(t.dm, t.n_mat, L, "m"); sn.v = fetch<float>(t.dv, t.n_mat, L, "v");
    const double reg = reg_of(t, A);
    const int rt = t.s.route;
    for (size_t k = 0; k < t.n_mat; ++k) {
        const bool in = k >= t.off && k < t.off + t.n;
        const bool upd = in && mode != REFRESH;
        if (!upd) judge_bits(f_bits(sn.p[k]), f_bits(t.p[k]), L, in ? "p (update == 0)" : "p outside the shard", (long)k);
        if (!upd || !rc.use_m) judge_bits(f_bits(sn.m[k]), f_bits(t.m[k]), L, upd ? "m, a slot the rule does not keep" : "m (no update)", (long)k);
        if (!upd || !rc.use_v) judge_bits(f_bits(sn.v[k]), f_bits(t.v[k]), L, upd ? "v, a slot the rule does not keep" : "v (no update)", (long)k);
        if (!upd) continue;
        const Ref r = rule_ref(t.p[k], t.g[k], rc.use_m ? t.m[k] : 0.f, rc.use_v ? t.v[k] : 0.f, reg, A);
        auto tally = [&](int q, double ratio) { if (ratio > g_worst[ri][rt][q]) g_worst[ri][rt][q] = ratio; ++g_n[ri][rt][q]; };
        tally(Q_P, judge(sn.p[k], r.p, r.ep, L, "p", (long)k));
        if (rc.use_m) tally(Q_M, judge(sn.m[k], r.m, r.em, L, "m", (long)k));
        if (rc.use_v) tally(Q_V, judge(sn.v[k], r.v, r.ev, L, "v", (long)k));
    }
    const uint32_t poison = esz == 2 ? 0xffffu : 0xffffffffu;
    sn.sh.clear(); sn.shT.clear();
    if (t.dsh) {
        sn.sh = fetch<unsigned char>(t.dsh, (size_t)t.s.mat_rows * t.ld_sh * esz, L, "sh");
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
                if (r < t.s.rows) judge_bits(got, copy_from(sn.p[(size_t)r * t.s.cols + c], esz), L, "shT vs Elem<T>::from(p)", c, r);
                else judge_bits(got, poison, L, "shT padding", c, r);
            }
    }
}

// --host: each reference against a second formulation in long double with the operations in another order, from the optimizer's own
// hyper-parameters where torch's formula has an order of its own (SGD's first update, Adagrad's clr)
static void host_check_tensor(const Tensor& t, const RtxAdamArgs& A, const RuleCase& rc, const Scal& sc, Line& L)
{
    typedef long double LD;
    const LD reg = A.lam != 0.f && t.s.sumsq && t.sumsq > 0.f ? (LD)A.lam / sqrtl((LD)t.sumsq) : 0.0L;
    long nbad = 0;
    for (size_t k = 0; k < t.n_mat; ++k) {
        const bool in = k >= t.off && k < t.off + t.n;
        nbad += !in && !(is_junk(t.p[k]) && is_junk(t.g_dev[k]));
        nbad += !(in && rc.use_m) && !is_junk(t.m[k]);
        nbad += !(in && rc.use_v) && !is_junk(t.v[k]);
        if (!in || sc.mode == REFRESH) continue;
        const float mv = rc.use_m ? t.m[k] : 0.f, vv = rc.use_v ? t.v[k] : 0.f;
        const Ref r = rule_ref(t.p[k], t.g[k], mv, vv, (double)reg, A);
        const LD wd = A.weight_decay, p0 = t.p[k];
        LD p = 0, m = mv, v = vv;
        const bool decoupled = (rc.o.flags & RTX_OPTF_DECOUPLED) != 0;
        const LD g = p0 * ((decoupled ? 0.0L : wd) + reg) + (LD)A.grad_scale * t.g[k];
        if (rc.o.kind == RTX_OPT_ADAM) {
            const LD b1 = A.beta1, b2 = A.beta2;
            m = b1 * m + (1.0L - b1) * g; v = (1.0L - b2) * (g * g) + b2 * v;
            const LD bc1 = 1.0L - powl((LD)BETA1, sc.step), bc2 = 1.0L - powl((LD)BETA2, sc.step);
            // torch: p (1 - lr wd) first (decoupled); step_size = lr / bc1; denom = sqrt(v) / sqrt(bc2) + eps
            const LD p1 = decoupled ? p0 - p0 * (LD)rc.lr * wd : p0;
            p = p1 - ((LD)rc.lr * m / bc1) * sqrtl(bc2) / (sqrtl(v) + (LD)A.eps * sqrtl(bc2));
        } else if (rc.o.kind == RTX_OPT_SGD) {
            LD d = g;
            if (rc.o.momentum != 0) {
                // torch: momentum_buffer absent -> buf = clone(g), no dampening; else buf = mom buf + (1 - dampening) g
                m = (rc.o.flags & RTX_OPTF_FIRST) ? g : (LD)rc.o.momentum * m + g - (LD)rc.o.dampening * g;
                d = (rc.o.flags & RTX_OPTF_NESTEROV) ? (LD)rc.o.momentum * m + g : m;
            }
            p = p0 - (LD)rc.lr * d;
        } else if (rc.o.kind == RTX_OPT_ADAGRAD) {
            // torch: clr = lr / (1 + (step - 1) lr_decay), then addcdiv(grad, sqrt(sum) + eps, value = -clr)
            const LD clr = (LD)rc.lr / (1.0L + (LD)(sc.step - 1) * (LD)rc.o.lr_decay);
            v = g * g + v;
            p = p0 - (clr * g) / (sqrtl(v) + (LD)A.eps);
        } else {
            v = (LD)rc.o.alpha * v + (g * g) * (1.0L - (LD)rc.o.alpha);
            const LD q = g / (sqrtl(v) + (LD)A.eps);
            if (rc.o.momentum != 0) { m = q + (LD)rc.o.momentum * m; p = p0 - (LD)rc.lr * m; }
            else p = p0 - (LD)rc.lr * q;
        }
        // agreement demanded: the bound's 2^-24 roundings leave room for the float32 scalars the launch carries (damp1, alpha1, decay,
        // clr, step_size, bc2_sqrt: one rounding each of a factor of the step) -- half of each bound -- and nothing else
        if (!(fabsl(p - r.p) <= 0.5L * r.ep)) host_fail(L, "p %.17g, long double %.17g", r.p, (double)p);
        if (rc.use_m && !(fabsl(m - r.m) <= 0.5L * r.em + 1e-300L)) host_fail(L, "m %.17g, long double %.17g", r.m, (double)m);
        if (rc.use_v && !(fabsl(v - r.v) <= 0.5L * r.ev + 1e-300L)) host_fail(L, "v %.17g, long double %.17g", r.v, (double)v);
        if (!(r.ep > 0 && r.em >= 0 && r.ev >= 0 && r.ep < 1e30)) host_fail(L, "bound of p %g at p' = %g", r.ep, r.p);
    }
    if (nbad) host_fail(L, "%g elements the kernel must not use hold no junk", (double)nbad);
}

// the shapes of section A of test_adam.cpp
static const Spec FLAT_SHAPES[] = {
    {1, 5, 1, 0, 0, 0, 0, 0, FLAT},    {1, 4096, 1, 0, 0, 0, 0, 0, FLAT}, {1, 4097, 1, 0, 0, 0, 0, 0, FLAT}, {5, 6, 5, 0, 0, 0, 0, 0, FLAT},
    {3, 1367, 3, 0, 0, 0, 0, 0, FLAT}, {64, 128, 64, 0, 0, 0, 0, 0, FLAT}, {70, 100, 70, 0, 0, 0, 0, 0, FLAT}};
static const Spec T_SHAPES[] = {
    {64, 64, 64, 0, 1, 1, 0, 0, VEC2D},  {65, 68, 65, 0, 1, 1, 0, 0, VEC2D},   {130, 36, 130, 0, 1, 1, 0, 0, VEC2D}, {33, 67, 33, 0, 1, 1, 0, 0, ELEM2D},
    {100, 1, 100, 0, 1, 1, 0, 0, ELEM2D}, {1, 70, 1, 0, 1, 1, 0, 0, ELEM2D}, {17, 130, 17, 0, 1, 1, 0, 0, ELEM2D}};
static const Spec SHARD_A = {26, 17, 40, 3, 1, 0, 0, 0, ELEM2D};
static const Spec SHARD_B = {39, 20, 40, 1, 1, 0, 2, 0, VEC2D};

struct Variant { const char* name; Scal s; int g16, sumsq; };
static const Variant VARIANTS[] = {
    {"step 1", {DRAWN, 1, 0.f, 0.f, 1.f}, 0, 0},
    {"step 7 g16 wd lam sumsq gs/8", {DRAWN, 7, 0.01f, 0.5f, 0.125f}, 1, 1},
    {"update == 0", {REFRESH, 1, 0.f, 0.f, 1.f}, 0, 0},
};

static void check_route(const RtxAdamArgs& a, const std::vector<Tensor*>& ts, Line& L)
{
    int tiles = 0;
    for (size_t k = 0; k < ts.size(); ++k) {
        if (a.t[k].flat != (ts[k]->s.route == FLAT)) host_fail(L, "tensor %g: flat = %g, not the route the case is meant to take", (double)k, a.t[k].flat);
        tiles += ts[k]->tiles();
    }
    if (a.total_tiles != tiles) host_fail(L, "total_tiles = %g, expected %g", a.total_tiles, tiles);
}

static void run_case(const char* what, int ri, const std::vector<Spec>& specs, const Variant& v, int bf16, uint32_t seed)
{
    const RuleCase& rc = RULES[ri];
    const int esz = bf16 ? 2 : 4;
    Rng r = {seed};
    std::vector<Tensor> T(specs.size());
    for (size_t k = 0; k < specs.size(); ++k) {
        Spec s = specs[k];
        if (s.g16 != 2) s.g16 = v.g16;
        s.sumsq = v.sumsq;
        gen_tensor(T[k], s, rc, r);
    }
    char name[200];
    snprintf(name, sizeof name, "k_optim<%s, %s> %s: %s", bf16 ? "bf16" : "f32", rc.name, what, v.name);
    Line L;
    RtxAdamArgs a = {};
    scalars(a, rc, v.s, L);
    if (g_host) { for (Tensor& t : T) host_check_tensor(t, a, rc, v.s, L); report(name, L); return; }
    a.n = (int)T.size();
    std::vector<Tensor*> ts;
    for (size_t k = 0; k < T.size(); ++k) { alloc_tensor(T[k], esz); upload(T[k], esz); a.t[k] = arg_of(T[k], esz); ts.push_back(&T[k]); }
    RT(rtx_launch_adam(a, bf16, 0));
    CK(hipDeviceSynchronize());
    check_route(a, ts, L);
    for (size_t k = 0; k < T.size(); ++k) {
        char tag[32]; snprintf(tag, sizeof tag, "tensor %zu", k);
        if (T.size() > 1) g_tag = tag;
        Snap sn;
        check_tensor(T[k], a, ri, v.s.mode, esz, L, sn);
    }
    g_tag.clear();
    report(name, L);
    free_all();
}

// Adam through the rule template: a launch whose scalars come from rtx_optim_scalars (the default optimizer) against a launch whose
// arguments are filled the way every caller filled k_adam's before the rules existed -- the rule fields left zero, step_size and
// bc2_sqrt by the formulas of test_adam.cpp -- bit for bit: p, m, v and both compute copies.  (k_adam itself is now the Adam
// instantiation of k_optim; test_adam.cpp runs it unchanged.)  A third launch judges decoupled Adam with weight_decay == 0 (decay
// exactly 1) against float64; its bits need not be coupled Adam's: p decay - ss q and p - ss q contract into different fused
// multiply-adds.
static void adam_launches_agree(int bf16, uint32_t seed)
{
    if (g_host) return;
    const int esz = bf16 ? 2 : 4;
    Snap sn[3];
    Line L;
    for (int w = 0; w < 3; ++w) {
        Rng r = {seed};
        Tensor t;
        Spec s = T_SHAPES[1];
        s.sumsq = 1;
        gen_tensor(t, s, RULES[0], r);
        alloc_tensor(t, esz);
        upload(t, esz);
        RtxAdamArgs a = {};
        const Scal sc = {DRAWN, 7, w == 2 ? 0.f : 0.01f, 0.5f, 0.125f};
        if (w == 1) {
            a.update = 1;
            a.step_size = (float)((double)RULES[0].lr / (1.0 - pow((double)BETA1, sc.step)));
            a.bc2_sqrt = (float)sqrt(1.0 - pow((double)BETA2, sc.step));
            a.beta1 = BETA1; a.beta2 = BETA2; a.eps = RULES[0].eps; a.weight_decay = sc.wd; a.lam = sc.lam; a.grad_scale = sc.gs;
        } else scalars(a, RULES[w == 2 ? 1 : 0], sc, L);
        a.n = 1; a.t[0] = arg_of(t, esz);
        RT(rtx_launch_adam(a, bf16, 0));
        CK(hipDeviceSynchronize());
        Line unused;
        check_tensor(t, a, w == 2 ? 1 : 0, DRAWN, esz, w == 2 ? L : unused, sn[w]);
        free_all();
    }
    if (sn[0].p.size() != sn[1].p.size() || memcmp(sn[0].p.data(), sn[1].p.data(), sn[0].p.size() * 4) || memcmp(sn[0].m.data(), sn[1].m.data(), sn[0].m.size() * 4) ||
        memcmp(sn[0].v.data(), sn[1].v.data(), sn[0].v.size() * 4) || sn[0].sh != sn[1].sh || sn[0].shT != sn[1].shT)
        host_fail(L, "Adam through rtx_optim_scalars differs from Adam with the rule fields zero");
    char name[160];
    snprintf(name, sizeof name, "k_optim<%s, Adam>: scalars of rtx_optim_scalars == the rule fields left zero, bit for bit", bf16 ? "bf16" : "f32");
    report(name, L);
}

static void host_only_cases()
{
    {   // the scalars that carry torch's operation order: Adagrad's clr, SGD's flags, AdamW's decay
        Line L;
        RtxAdamArgs a = {};
        rtx_optim_scalars(RULES[7].o, 0.05f, 0, 0, 1e-10f, 0.f, 7, a);
        const long double clr = (long double)0.05f / (1.0L + 6.0L * (long double)0.1);
        if (a.rule != RTX_RULE_ADAGRAD || !(fabsl(a.lr - clr) <= E24 * clr)) host_fail(L, "Adagrad: clr %.9g, expected %.9g", a.lr, (double)clr);
        rtx_optim_scalars(RULES[7].o, 0.05f, 0, 0, 1e-10f, 0.f, 1, a);
        if (a.lr != 0.05f) host_fail(L, "Adagrad: clr %.9g at step 1, expected lr", a.lr);
        a = {};
        rtx_optim_scalars(RULES[3].o, 0.05f, 0, 0, 0, 0.f, 1, a);
        if (a.rule != RTX_RULE_SGD_MOM || !a.first || a.nesterov || a.damp1 != (float)(1.0 - 0.1)) host_fail(L, "SGD momentum, first: rule %g first %g", a.rule, a.first);
        a = {};
        rtx_optim_scalars(RULES[5].o, 0.05f, 0, 0, 0, 0.f, 2, a);
        if (a.rule != RTX_RULE_SGD_MOM || a.first || !a.nesterov) host_fail(L, "SGD nesterov: rule %g first %g", a.rule, a.first);
        a = {};
        rtx_optim_scalars(RULES[2].o, 0.05f, 0, 0, 0, 0.f, 2, a);
        if (a.rule != RTX_RULE_SGD) host_fail(L, "SGD without momentum: rule %g", a.rule);
        a = {};
        rtx_optim_scalars(RULES[1].o, 1e-3f, BETA1, BETA2, 1e-8f, 0.01f, 3, a);
        if (a.rule != RTX_RULE_ADAMW || a.decay != (float)(1.0 - (double)1e-3f * (double)0.01f)) host_fail(L, "AdamW: decay %.9g", a.decay);
        RtxAdamArgs z = {}, b = {};
        rtx_optim_scalars(RtxOptim(), 1e-3f, BETA1, BETA2, 1e-8f, 0.01f, 3, b);
        if (z.rule != RTX_RULE_ADAM || b.rule != RTX_RULE_ADAM) host_fail(L, "zeroed arguments / the default optimizer are not Adam");
        report("H rtx_optim_scalars: clr, first / nesterov, decay, the default rule", L);
    }
    auto ret = [](const char* what, int rc, int want) {
        Line L;
        if (rc != want) host_fail(L, "returned %g, expected %g", rc, want);
        char name[160];
        snprintf(name, sizeof name, "R %s: %s", what, want == RTX_EINVAL ? "refused" : "accepted");
        report(name, L, rc == RTX_EINVAL ? (std::string("  [") + rtx_last_error_str() + "]").c_str() : "");
    };
    for (int k = 0; k < N_RULES; ++k) ret(RULES[k].name, rtx_optim_validate(RULES[k].o), RTX_OK);
    ret("kind 4", rtx_optim_validate(mk(4, 0, 0, 0, 0, 0)), RTX_EINVAL);
    ret("kind -1", rtx_optim_validate(mk(-1, 0, 0, 0, 0, 0)), RTX_EINVAL);
    ret("flag bit 8", rtx_optim_validate(mk(RTX_OPT_ADAM, 8, 0, 0, 0, 0)), RTX_EINVAL);
    ret("decoupled SGD", rtx_optim_validate(mk(RTX_OPT_SGD, RTX_OPTF_DECOUPLED, 0, 0, 0, 0)), RTX_EINVAL);
    ret("nesterov without momentum", rtx_optim_validate(mk(RTX_OPT_SGD, RTX_OPTF_NESTEROV, 0, 0, 0, 0)), RTX_EINVAL);
    ret("nesterov with dampening", rtx_optim_validate(mk(RTX_OPT_SGD, RTX_OPTF_NESTEROV, 0.9, 0.1, 0, 0)), RTX_EINVAL);
    ret("first without momentum", rtx_optim_validate(mk(RTX_OPT_SGD, RTX_OPTF_FIRST, 0, 0, 0, 0)), RTX_EINVAL);
    ret("first on RMSprop", rtx_optim_validate(mk(RTX_OPT_RMSPROP, RTX_OPTF_FIRST, 0.5, 0, 0.9, 0)), RTX_EINVAL);
    RtxAdamArgs a = {};
    static float dummy[16] __attribute__((aligned(16)));
    a.n = 1; a.rule = RTX_RULE_COUNT; a.t[0].p = dummy; a.t[0].rows = 1; a.t[0].cols = 4;
    ret("launch, rule out of range", rtx_launch_adam(a, 0, 0), RTX_EINVAL);
    a.rule = -1;
    ret("launch, rule -1", rtx_launch_adam(a, 0, 0), RTX_EINVAL);
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    g_name_width = 100;
    setvbuf(stdout, nullptr, _IOLBF, 0);
    uint32_t seed = 300;
    const Spec *F = FLAT_SHAPES, *T = T_SHAPES;
    Spec f_sh[7];
    for (int k = 0; k < 7; ++k) { f_sh[k] = F[k]; f_sh[k].sh = k != 0 && k != 3; }
    const Spec zero_rows = {0, 10, 0, 0, 1, 0, 0, 1, FLAT};
    const std::vector<Spec> M9 = {T[3], T[1], f_sh[2], SHARD_B};
    const std::vector<Spec> M17 = {T[1], T[2], T[6], f_sh[5], zero_rows, T[4], T[5], T[0]};
    for (int ri = 0; ri < N_RULES; ++ri)
        for (int bf16 = 0; bf16 < 2; ++bf16)
            for (const Variant& v : VARIANTS) {
                char what[96];
                for (const Spec& s : FLAT_SHAPES)
                    for (int sh = 0; sh < 2; ++sh) {
                        Spec c = s; c.sh = sh;
                        snprintf(what, sizeof what, "%s %dx%d%s", ROUTE_NAME[c.route], c.rows, c.cols, sh ? " sh" : "");
                        run_case(what, ri, {c}, v, bf16, ++seed);
                    }
                for (const Spec& s : T_SHAPES) {
                    snprintf(what, sizeof what, "%s %dx%d sh shT", ROUTE_NAME[s.route], s.rows, s.cols);
                    run_case(what, ri, {s}, v, bf16, ++seed);
                }
                run_case("2-D 4-byte 26x17 (shard) sh", ri, {SHARD_A}, v, bf16, ++seed);
                run_case("2-D float4 39x20 (shard) sh g16", ri, {SHARD_B}, v, bf16, ++seed);
                run_case("4 tensors, 9 tiles", ri, M9, v, bf16, ++seed);
                run_case("8 tensors (one of zero rows), 17 tiles", ri, M17, v, bf16, ++seed);
            }
    for (int bf16 = 0; bf16 < 2; ++bf16) adam_launches_agree(bf16, ++seed);
    if (g_host) host_only_cases();
    else {
        printf("worst error / bound by rule, walk and quantity (DESIGN.md section 6):\n");
        for (int ri = 0; ri < N_RULES; ++ri)
            for (int rt = 0; rt < NROUTE; ++rt) {
                printf("    %-24s %-12s", RULES[ri].name, ROUTE_NAME[rt]);
                for (int q = 0; q < NQ; ++q)
                    if (g_n[ri][rt][q]) printf("  %s %.4f (%ld)", Q_NAME[q], g_worst[ri][rt][q], g_n[ri][rt][q]);
                printf("\n");
            }
    }
    return finish("OPTIM");
}
