// Native (no Python) check of gradient clipping in adam.hip against plain float64 host code: the norm kernels (k_grad_norm_part /
// k_grad_norm_finish behind rtx_launch_grad_norm) on tensor sets chosen to break the flat walk, and the clipping instantiations of the
// optimizer walk (k_optim<T, Rule, Clip> behind rtx_launch_clipped_adam) for every rule of test_optim.cpp x {coefficient, value} x every
// walk (flat whole tile, flat tail, 2-D float4 tiles and 2-D 4-byte tiles with a transposed copy, a one-row bias) x {float, bf16 compute
// copy}.  The rules, their float64 references with their one-update bounds (rule_ref), the case generator and the tensor plumbing are
// test_optim.cpp's own: that file is included below with its main() renamed, so nothing of it is copied and nothing of it changes.
//
// N  the norm.  Reference: G = gv gs + reg pv in double per element (reg = lam / sqrt(sumsq) from the float32 sumsq the kernel reads),
//    the sum of squares in double.  Bound of the 2-norm: 4 x 2^-24 relative -- the kernel accumulates in double and rounds once behind
//    the double square root (1/2 rounding); what remains is the float32 G it squares: gv gs (1 rounding) and the fused multiply-add
//    (1 rounding), plus 2 roundings of reg on the regulariser's share.  The max-norm is judged bit for bit against max |G| with G formed
//    on the host by the kernel's own float32 expression (fmaf(reg, p, gv gs); sqrtf and the division are correctly rounded on both
//    sides).  The coefficient is judged bit for bit against min(1, max_norm / (total + 1e-6f)) evaluated in float32 on the DEVICE's
//    total.  Two launches on the same data: the same bits, partial sums included.
// C  the clipped update.  Reference: Gc = clip(G) in double with the float64 norm's coefficient, then rule_ref from the prepared gradient
//    Gc (+ the decay, which the rule adds after the clip).  Bound: rule_ref's one-update bound, widened by what the clip adds in front of
//    the rule: the error of the device's Gc, dG = c E24 (3 |a| + 5 |b|) + 6 E24 |Gc|.  The first term is test_optim.cpp's own count for
//    forming G = a + b, a = gv gs, b = reg pv (the two may cancel, so it is NOT relative to G), scaled by the coefficient c (1 for
//    value clipping, whose clamp is exact); the second counts the roundings the coefficient adds, relative to Gc: the norm to float32,
//    + 1e-6, max_norm as float32, the division (4), the product G coef (1), and the reference's own hand-over of Gc to rule_ref as a
//    float32 (1).  The widening is the change of rule_ref's result when Gc moves by dG either way.
// I  one inf gradient element: the coefficient is 0, that element's G is inf x 0 = NaN and so are its parameter and states; every other
//    element moves by the rule at Gc = 0 (the decay alone) -- all from the float64 formula.
// B  Clip = none through rtx_launch_clipped_adam against rtx_launch_adam, all rules: bit for bit.
//   test_clip          the device run
//   test_clip --host   no HIP call: the norm reference against a long double sum in the opposite order, the coefficient and the clamp
//                      against second formulations, the clipped update's reference through test_optim's long double rules, and what
//                      rtx_clip_validate refuses
#define main optim_driver_main
#include "test_optim.cpp"
#undef main

static double c_worst[2][2];      // [mode: coefficient, value][quantity: p, state]
static const double ETA = 6 * E24;      // roundings the coefficient, the product and the hand-over add, relative to Gc

// ---- the float64 clip -----------------------------------------------------------------------------------------------------------------
static double G_of(const Tensor& t, size_t k, const RtxAdamArgs& A) { return (double)t.g[k] * A.grad_scale + reg_of(t, A) * t.p[k]; }
static double coef_of(double total, double max_norm)
{
    const double c = max_norm / (total + 1e-6);
    return c > 1.0 ? 1.0 : c;       // a NaN stays
}
static double clamp_of(double G, double v) { return G < -v ? -v : (G > v ? v : G); }
static double norm_of(const std::vector<Tensor>& T, const RtxAdamArgs& A, bool inf)
{
    double acc = 0;
    for (const Tensor& t : T)
        for (size_t k = 0; k < t.n; ++k) {
            const double G = G_of(t, t.off + k, A);
            if (inf) acc = (acc != acc || !(fabs(G) <= acc)) ? (acc != acc ? acc : fabs(G)) : acc;
            else acc += G * G;
        }
    return inf ? acc : sqrt(acc);
}

// the update of one element from the prepared, clipped gradient Gc: rule_ref with grad_scale 1 and no regulariser; its bound widened by
// the move of its result under Gc +- dG (header); c: the coefficient (1 for value clipping)
static Ref clipped_ref(const Tensor& t, size_t k, double Gc, double c, float mv, float vv, const RtxAdamArgs& A)
{
    RtxAdamArgs B = A;
    B.grad_scale = 1.f; B.lam = 0.f;
    const float pv = t.p[k], gf = (float)Gc;
    Ref r = rule_ref(pv, gf, mv, vv, 0.0, B);
    if (gf != gf) return r;        // (a NaN is judged as a NaN)
    const double a = (double)t.g[k] * A.grad_scale, b = reg_of(t, A) * pv;
    const double dG = c == c ? c * E24 * (3 * fabs(a) + 5 * fabs(b)) + ETA * fabs(Gc) : 0.0;
    if (!(dG > 0) || !(dG < INFINITY)) return r;
    double dp = 0, dm = 0, dv = 0;
    for (int s = -1; s <= 1; s += 2) {
        const Ref q = rule_ref(pv, (float)((double)gf + s * dG), mv, vv, 0.0, B);
        dp = std::max(dp, fabs(q.p - r.p)); dm = std::max(dm, fabs(q.m - r.m)); dv = std::max(dv, fabs(q.v - r.v));
    }
    r.ep += dp; r.em += dm; r.ev += dv;
    return r;
}

static void judge_nan_or(float got, double want, double bound, Line& L, const char* what, long k, double* worst)
{
    if (want != want) {
        if (got == got) {
            if (L.bad < 4) printf("    %s: expected a NaN, the device holds %g\n", where(what, k, -1).c_str(), got);
            ++L.bad;
        }
        return;
    }
    const double ratio = judge(got, want, bound, L, what, k);
    if (ratio > *worst) *worst = ratio;
}

// ---- C / I: the clipped update --------------------------------------------------------------------------------------------------------
static const Spec CLIP_SHAPES[] = {
    {1, 4097, 1, 0, 1, 0, 0, 1, FLAT},      // a whole 4096-element tile and a one-element tail, compute copy
    {3, 1367, 3, 0, 0, 0, 0, 0, FLAT},      // a tail with nv < 4, no regulariser term
    {65, 68, 65, 0, 1, 1, 0, 1, VEC2D},     // 2-D float4 tiles, both compute copies
    {33, 67, 33, 0, 1, 1, 0, 0, ELEM2D},    // 2-D 4-byte tiles, both compute copies, no regulariser term
    {1, 5, 1, 0, 0, 0, 0, 1, FLAT},         // a one-row bias
};
enum { BY_COEF, BY_VALUE };

static void run_clip_case(int ri, int mode, int bf16, bool with_inf, uint32_t seed)
{
    const RuleCase& rc = RULES[ri];
    const int esz = bf16 ? 2 : 4;
    Rng r = {seed};
    std::vector<Tensor> T(5);
    for (int k = 0; k < 5; ++k) gen_tensor(T[k], CLIP_SHAPES[k], rc, r);
    if (with_inf) T[2].g[T[2].off + 1234] = T[2].g_dev[T[2].off + 1234] = INFINITY;
    char name[200];
    snprintf(name, sizeof name, "k_optim<%s, %s, %s>%s: 5 tensors, every walk", bf16 ? "bf16" : "f32", rc.name, mode == BY_COEF ? "coefficient" : "value",
             with_inf ? ", one inf gradient" : "");
    Line L;
    RtxAdamArgs a = {};
    const Scal sc = {DRAWN, 7, 0.01f, 0.5f, 0.125f};
    scalars(a, rc, sc, L);
    const double max_norm = 0.75, value = 0.03125;      // (both exact in float32; |G| is up to 0.125 + 0.5 |p| / ||p||: the value bites often)
    const double total = norm_of(T, a, false), coef = coef_of(total, max_norm);
    if (!with_inf && mode == BY_COEF && !(total >= 2 * max_norm)) host_fail(L, "the case does not bite: total norm %g", total);
    if (g_host) {
        // the clipped gradient through test_optim's long double rules: a tensor whose gradient IS Gc, grad_scale 1, no regulariser
        for (Tensor& t : T) {
            Tensor u = t;
            RtxAdamArgs b = a;
            b.grad_scale = 1.f; b.lam = 0.f;
            for (size_t k = 0; k < t.n; ++k) {
                const double G = G_of(t, t.off + k, a);
                u.g[t.off + k] = (float)(mode == BY_COEF ? G * coef : clamp_of(G, value));
            }
            u.s.sumsq = 0;
            if (!with_inf) host_check_tensor(u, b, rc, sc, L);
        }
        report(name, L);
        return;
    }
    a.n = 5;
    for (int k = 0; k < 5; ++k) { alloc_tensor(T[k], esz); upload(T[k], esz); a.t[k] = arg_of(T[k], esz); }
    RtxClipState cs;
    cs.mode = mode == BY_COEF ? RTX_CLIPM_NORM2 : RTX_CLIPM_VALUE;
    cs.bound = mode == BY_COEF ? max_norm : value;
    RT(rtx_launch_clipped_adam(a, bf16, cs, 7, 0));
    CK(hipDeviceSynchronize());
    if (mode == BY_COEF) {
        float host2[2] = {0, 0};
        uint32_t tag = 0;
        RT(rtx_clip_wait_norm(cs, "test_clip", host2, 5.0, &tag));
        const std::vector<float> pair = to_host(cs.pair, 2);
        if (f_bits(pair[0]) != f_bits(host2[0]) || f_bits(pair[1]) != f_bits(host2[1]) || tag != 7) host_fail(L, "the mailbox holds %g, the device pair %g", host2[0], pair[0]);
        if (with_inf) { if (!(pair[0] == INFINITY && pair[1] == 0.f)) host_fail(L, "total %g coefficient %g, expected inf and 0", pair[0], pair[1]); }
        else judge(pair[0], total, 4 * E24 * total, L, "total norm", 0);
    }
    for (int k = 0; k < 5; ++k) {
        const Tensor& t = T[k];
        char tag[32]; snprintf(tag, sizeof tag, "tensor %d", k);
        g_tag = tag;
        const std::vector<float> p = fetch<float>(t.dp, t.n_mat, L, "p"), m = fetch<float>(t.dm, t.n_mat, L, "m"), v = fetch<float>(t.dv, t.n_mat, L, "v");
        for (size_t e = 0; e < t.n_mat; ++e) {
            const double G = G_of(t, e, a);
            const double Gc = mode == BY_COEF ? G * coef : clamp_of(G, value);
            const Ref ref = clipped_ref(t, e, Gc, mode == BY_COEF ? coef : 1.0, rc.use_m ? t.m[e] : 0.f, rc.use_v ? t.v[e] : 0.f, a);
            judge_nan_or(p[e], ref.p, ref.ep, L, "p", (long)e, &c_worst[mode][0]);
            if (rc.use_m) judge_nan_or(m[e], ref.m, ref.em, L, "m", (long)e, &c_worst[mode][1]);
            else judge_bits(f_bits(m[e]), f_bits(t.m[e]), L, "m, a slot the rule does not keep", (long)e);
            if (rc.use_v) judge_nan_or(v[e], ref.v, ref.ev, L, "v", (long)e, &c_worst[mode][1]);
            else judge_bits(f_bits(v[e]), f_bits(t.v[e]), L, "v, a slot the rule does not keep", (long)e);
        }
        // the compute copies are the new parameters, element for element
        if (t.dsh) {
            const std::vector<unsigned char> sh = fetch<unsigned char>(t.dsh, (size_t)t.s.mat_rows * t.ld_sh * esz, L, "sh");
            for (int rr = 0; rr < t.s.rows; ++rr)
                for (int c = 0; c < t.s.cols; ++c)
                    judge_bits(copy_bits(sh, (size_t)rr * t.ld_sh + c, esz), copy_from(p[(size_t)rr * t.s.cols + c], esz), L, "sh vs Elem<T>::from(p)", rr, c);
        }
        if (t.dshT) {
            const std::vector<unsigned char> shT = fetch<unsigned char>(t.dshT, (size_t)t.s.cols * t.ld_shT * esz, L, "shT");
            for (int c = 0; c < t.s.cols; ++c)
                for (int rr = 0; rr < t.s.rows; ++rr)
                    judge_bits(copy_bits(shT, (size_t)c * t.ld_shT + rr, esz), copy_from(p[(size_t)rr * t.s.cols + c], esz), L, "shT vs Elem<T>::from(p)", c, rr);
        }
    }
    g_tag.clear();
    report(name, L);
    rtx_clip_release(cs);
    free_all();
}

// ---- B: Clip = none -------------------------------------------------------------------------------------------------------------------
static void none_is_the_plain_launch(int ri, int bf16, uint32_t seed)
{
    if (g_host) return;
    const int esz = bf16 ? 2 : 4;
    std::vector<float> keep[2][3];
    std::vector<unsigned char> keep_sh[2];
    Line L;
    for (int w = 0; w < 2; ++w) {
        Rng r = {seed};
        Tensor t;
        gen_tensor(t, CLIP_SHAPES[2], RULES[ri], r);
        alloc_tensor(t, esz);
        upload(t, esz);
        RtxAdamArgs a = {};
        const Scal sc = {DRAWN, 7, 0.01f, 0.5f, 0.125f};
        scalars(a, RULES[ri], sc, L);
        a.n = 1; a.t[0] = arg_of(t, esz);
        RtxClipState cs;
        if (w == 0) RT(rtx_launch_adam(a, bf16, 0));
        else RT(rtx_launch_clipped_adam(a, bf16, cs, 7, 0));
        CK(hipDeviceSynchronize());
        if (w == 1 && (cs.last_has_norm || cs.part || cs.pair || cs.mailbox)) host_fail(L, "no clip mode, yet the launch prepared a norm");
        keep[w][0] = fetch<float>(t.dp, t.n_mat, L, "p"); keep[w][1] = fetch<float>(t.dm, t.n_mat, L, "m"); keep[w][2] = fetch<float>(t.dv, t.n_mat, L, "v");
        keep_sh[w] = fetch<unsigned char>(t.dsh, (size_t)t.s.mat_rows * t.ld_sh * esz, L, "sh");
        free_all();
    }
    for (int q = 0; q < 3; ++q)
        if (memcmp(keep[0][q].data(), keep[1][q].data(), keep[0][q].size() * 4)) host_fail(L, "quantity %g differs between the two launches", q);
    if (keep_sh[0] != keep_sh[1]) host_fail(L, "the compute copies differ between the two launches");
    char name[200];
    snprintf(name, sizeof name, "B k_optim<%s, %s>: no clip mode == rtx_launch_adam, bit for bit", bf16 ? "bf16" : "f32", RULES[ri].name);
    report(name, L);
}

// ---- N: the norm kernels --------------------------------------------------------------------------------------------------------------
struct NormSet { const char* name; std::vector<long> sizes; int offset; bool zero; int reg_every; float gs, lam; };

static void run_norm_case(const NormSet& ns, uint32_t seed)
{
    Rng r = {seed};
    const int n = (int)ns.sizes.size();
    std::vector<std::vector<float>> g(n), p(n);
    std::vector<float> sumsq(n, 0.f);
    for (int k = 0; k < n; ++k) {
        g[k].resize(ns.sizes[k]); p[k].resize(ns.sizes[k]);
        double ss = 0;
        for (long i = 0; i < ns.sizes[k]; ++i) {
            g[k][i] = ns.zero ? 0.f : (i % 5 == 0 ? 0.f : r.f());
            p[k][i] = r.f();
            ss += (double)p[k][i] * p[k][i];
        }
        sumsq[k] = (float)ss;
    }
    auto live = [&](int k) { return ns.reg_every && k % ns.reg_every == 0 && ns.lam != 0.f; };
    // the references: double (forward order) for the 2-norm, the kernel's own float32 expression for the max-norm
    double acc = 0;
    float mx = 0.f;
    long double acc_ld = 0;
    for (int k = 0; k < n; ++k) {
        const bool lv = live(k) && sumsq[k] > 0.f;
        const double regd = lv ? (double)ns.lam / sqrt((double)sumsq[k]) : 0.0;
        const float regf = lv ? ns.lam / sqrtf(sumsq[k]) : 0.f;
        for (long i = 0; i < ns.sizes[k]; ++i) {
            const double G = (double)g[k][i] * ns.gs + regd * p[k][i];
            acc += G * G;
            const float Gf = lv ? fmaf(regf, p[k][i], g[k][i] * ns.gs) : g[k][i] * ns.gs;
            mx = fmaxf(mx, fabsf(Gf));
        }
    }
    for (int k = n - 1; k >= 0; --k) {
        const long double regd = live(k) && sumsq[k] > 0.f ? (long double)ns.lam / sqrtl((long double)sumsq[k]) : 0.0L;
        for (long i = ns.sizes[k] - 1; i >= 0; --i) {
            const long double G = regd * p[k][i] + (long double)ns.gs * g[k][i];
            acc_ld += G * G;
        }
    }
    const double total = sqrt(acc);
    Line L;
    char name[200];
    if (g_host) {
        // (a plain double sum of n non-negative terms: at most n roundings relative on the sum, half of that on its root)
        long n_el = 0;
        for (long sz : ns.sizes) n_el += sz;
        if (!(fabsl(sqrtl(acc_ld) - total) <= (0.5 * n_el + 8) * U53 * total)) host_fail(L, "double sum %.17g, long double in the opposite order %.17g", total, (double)sqrtl(acc_ld));
        if (ns.zero && (total != 0 || coef_of(total, 1.0) != 1.0)) host_fail(L, "all-zero gradients: total %g coefficient %g", total, coef_of(total, 1.0));
        snprintf(name, sizeof name, "N %s: the float64 norm against a long double sum in the opposite order", ns.name);
        report(name, L);
        return;
    }
    RtxAdamArgs a = {};
    a.n = n; a.grad_scale = ns.gs; a.lam = ns.lam;
    for (int k = 0; k < n; ++k) {
        std::vector<float> gb(ns.offset, 0.f), pb(ns.offset, 0.f);
        gb.insert(gb.end(), g[k].begin(), g[k].end()); pb.insert(pb.end(), p[k].begin(), p[k].end());
        gb.insert(gb.end(), 8, 1e30f); pb.insert(pb.end(), 8, 1e30f);      // behind the end: huge, a read out of bounds shows in the norm
        a.t[k].g = to_dev(gb) + ns.offset;
        a.t[k].p = to_dev(pb) + ns.offset;
        a.t[k].rows = 1; a.t[k].cols = (int)ns.sizes[k];
        if (ns.sizes[k] == 77 * 21) { a.t[k].rows = 77; a.t[k].cols = 21; }
        if (live(k)) a.t[k].sumsq = to_dev(std::vector<float>(1, sumsq[k]));
    }
    const long parts = rtx_grad_norm_parts(a);
    const float max_norm = 0.5f;
    uint32_t bits[2][2][2];
    std::vector<double> part_keep[2];
    for (int inf = 0; inf < 2; ++inf)
        for (int rep = 0; rep < 2; ++rep) {
            double* part = dev_out<double>((size_t)parts);
            float* pair = dev_out<float>(2);
            RT(rtx_launch_grad_norm(a, inf, max_norm, part, pair, nullptr, 0, 0, 0));
            CK(hipDeviceSynchronize());
            const std::vector<float> got = fetch<float>(pair, 2, L, "pair");
            const std::vector<double> pk = fetch<double>(part, (size_t)parts, L, "partial sums");
            bits[inf][rep][0] = f_bits(got[0]); bits[inf][rep][1] = f_bits(got[1]);
            if (!inf) part_keep[rep] = pk;
            if (inf) judge_bits(f_bits(got[0]), f_bits(mx), L, "max-norm", 0);
            else judge(got[0], total, 4 * E24 * total, L, "2-norm", 0);
            float coef = max_norm / (got[0] + 1e-6f);
            coef = coef > 1.f ? 1.f : coef;
            judge_bits(f_bits(got[1]), f_bits(coef), L, "coefficient", inf);
            if (ns.zero && !(got[0] == 0.f && got[1] == 1.f)) host_fail(L, "all-zero gradients: total %g coefficient %g", got[0], got[1]);
        }
    for (int inf = 0; inf < 2; ++inf)
        if (bits[inf][0][0] != bits[inf][1][0] || bits[inf][0][1] != bits[inf][1][1]) host_fail(L, "two launches on the same data differ (norm type %g)", inf);
    if (part_keep[0].size() != part_keep[1].size() || memcmp(part_keep[0].data(), part_keep[1].data(), part_keep[0].size() * 8)) host_fail(L, "the partial sums of two launches differ");
    snprintf(name, sizeof name, "N %s: %d tensors, %ld partial sums", ns.name, n, parts);
    report(name, L);
    free_all();
}

static void host_only_clip_cases()
{
    Line L;
    if (coef_of(13.0, 6.5) != 6.5 / (13.0 + 1e-6) || coef_of(0.0, 1.0) != 1.0 || coef_of(INFINITY, 1.0) != 0.0 || coef_of(NAN, 1.0) == coef_of(NAN, 1.0) ||
        coef_of(3.0, INFINITY) != 1.0)
        host_fail(L, "the coefficient's reference");
    for (double G : {-2.0, -0.5, 0.0, 0.25, 0.5, 7.0})
        if (clamp_of(G, 0.5) != fmin(fmax(G, -0.5), 0.5)) host_fail(L, "the clamp's reference at %g", G);
    if (clamp_of(NAN, 0.5) == clamp_of(NAN, 0.5)) host_fail(L, "the clamp's reference lost a NaN");
    report("H the coefficient and the clamp against second formulations", L);
    auto ret = [](const char* what, int rc, int want) {
        Line L2;
        if (rc != want) host_fail(L2, "returned %g, expected %g", rc, want);
        char name[160];
        snprintf(name, sizeof name, "R %s: %s", what, want == RTX_EINVAL ? "refused" : "accepted");
        report(name, L2, rc == RTX_EINVAL ? (std::string("  [") + rtx_last_error_str() + "]").c_str() : "");
    };
    ret("mode none", rtx_clip_validate(RTX_CLIPM_NONE, 0, "t"), RTX_OK);
    ret("2-norm, bound 1", rtx_clip_validate(RTX_CLIPM_NORM2, 1.0, "t"), RTX_OK);
    ret("max-norm, bound inf", rtx_clip_validate(RTX_CLIPM_NORMINF, INFINITY, "t"), RTX_OK);
    ret("value, bound 0", rtx_clip_validate(RTX_CLIPM_VALUE, 0.0, "t"), RTX_OK);
    ret("mode 4", rtx_clip_validate(4, 1.0, "t"), RTX_EINVAL);
    ret("mode -1", rtx_clip_validate(-1, 1.0, "t"), RTX_EINVAL);
    ret("negative bound", rtx_clip_validate(RTX_CLIPM_NORM2, -1.0, "t"), RTX_EINVAL);
    ret("NaN bound", rtx_clip_validate(RTX_CLIPM_VALUE, NAN, "t"), RTX_EINVAL);
    RtxAdamArgs a = {};
    static float dummy[16] __attribute__((aligned(16)));
    a.n = 1; a.update = 1; a.t[0].p = dummy; a.t[0].g = dummy; a.t[0].rows = 1; a.t[0].cols = 4;
    a.clip = 3;
    ret("launch, clip mode out of range", rtx_launch_adam(a, 0, 0), RTX_EINVAL);
    a.clip = RTX_CLIPK_COEF;
    ret("launch, coefficient without its device pair", rtx_launch_adam(a, 0, 0), RTX_EINVAL);
    a.clip = RTX_CLIPK_VALUE; a.update = 0;
    ret("launch, a clip mode on a refresh", rtx_launch_adam(a, 0, 0), RTX_EINVAL);
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    g_name_width = 100;
    setvbuf(stdout, nullptr, _IOLBF, 0);
    uint32_t seed = 900;
    std::vector<long> many(RTX_MAX_TENSORS);
    for (int k = 0; k < RTX_MAX_TENSORS; ++k) many[k] = 1 + (k * 977) % 5000;
    const NormSet SETS[] = {
        {"sizes 1, 3, 4095, 4096, 4097, 77 x 21, 3 x 4096 + 5", {1, 3, 4095, 4096, 4097, 77 * 21, 3 * 4096 + 5}, 0, false, 0, 1.f, 0.f},
        {"the same, regulariser on every other tensor, gs = 0.125", {1, 3, 4095, 4096, 4097, 77 * 21, 3 * 4096 + 5}, 0, false, 2, 0.125f, 0.5f},
        {"one tensor of 300 007 elements", {300007}, 0, false, 0, 1.f, 0.f},
        {"one tensor of 300 007 elements, regulariser, gs = 3", {300007}, 0, false, 1, 3.f, 0.2f},
        {"32 tensors", many, 0, false, 3, 0.5f, 0.5f},
        {"buffers offset by 4 bytes", {4097, 5, 8192}, 1, false, 2, 1.f, 0.5f},
        {"all-zero gradients", {4097, 3}, 0, true, 0, 1.f, 0.f},
    };
    for (const NormSet& ns : SETS) run_norm_case(ns, ++seed);
    for (int ri = 0; ri < N_RULES; ++ri)
        for (int mode = 0; mode < 2; ++mode)
            for (int bf16 = 0; bf16 < 2; ++bf16) run_clip_case(ri, mode, bf16, false, ++seed);
    run_clip_case(0, BY_COEF, 0, true, ++seed);
    run_clip_case(4, BY_COEF, 1, true, ++seed);
    for (int ri = 0; ri < N_RULES; ++ri)
        for (int bf16 = 0; bf16 < 2; ++bf16) none_is_the_plain_launch(ri, bf16, ++seed);
    if (g_host) host_only_clip_cases();
    else printf("worst error / bound: coefficient p %.4f states %.4f, value p %.4f states %.4f\n", c_worst[0][0], c_worst[0][1], c_worst[1][0], c_worst[1][1]);
    return finish("CLIP");
}
