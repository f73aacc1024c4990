// Native (no Python) check of the seven kernels every layer between the first and the last product of a step runs through, one
// launcher at a time, against plain float64 host code:
//   S  small_layers.hip: k_fwd_hidden, k_fwd_head, k_bwd_hidden, k_bwd_head at all eight K widths (128 .. 1024) and under every
//      launch shape (waves per workgroup, waves that share K) -- 96 instantiations
//   P  post_layers.hip: k_post (forward / backward, float32 / bf16, both BURST forms), k_vae_fwd and k_vae_bwd
// Every output buffer is poisoned (all bits set: a NaN in f32 and in bf16) before each launch and carries a poisoned guard behind
// its end; everything a kernel may load but must mask (padded batch rows, weight rows past the real ones, slab gaps, C columns past
// Np) holds finite junk of magnitude ~1e3; output padding and the ones column are compared bit for bit.  Each element is judged
// against ITS OWN scale (the bounds and where they come from: DESIGN.md section 6), and every line prints the worst error as a
// fraction of its bound.
//   test_layers          the device run
//   test_layers --host   no HIP call: the case generator and the float64 references, checked against a second formulation in long
//                        double (other loop order, tanhl / expl, an operand image decoded from the bf16 bits by hand), the two
//                        backward references against central differences of the forward ones, the conditions the bounds assume,
//                        and the refusals of the launchers (every RTX_CHECK returns before the first HIP call)
#include "../../rectorch_amd/csrc/rtx_kernels.h"

#include "check.h"

static const float BETA = 0.3f;
// Device tanhf / expf: the ROCm documentation is not at hand, so the OpenCL full-profile limits the device library is built to are
// ASSUMED: tanh <= 5 ulp, exp <= 3 ulp (one ulp = 2^-23 relative at worst = 2 x 2^-24).
static const double TANH_ULPS = 5, EXP_ULPS = 3;
// Tightening: a derived bound whose worst / bound stayed below 0.05 on the MI355X is multiplied by a factor so
// that it sits 4 .. 10 x above the measured worst.  Only one did: the MFMA pre-activation bound (K_real + 2) 2^-24 (sum |a w| + |bias|)
// -- the worst case of ANY order of float32 additions -- as it enters O32 of k_fwd_hidden: worst / derived 0.0071 without tanh (0.017
// with it), so T_PRE_HID = 0.05 = 7 x the measured worst.  The same bound stays as derived (factor 1) where it enters mu32 / lv32 of
// k_fwd_head (0.095: at in = 28 a logvar of 20 is rounded a few times against a bound of 30 roundings) and the bf16 outputs of the
// backward kernels (whose bf16 rounding fills the bound).  tanhf at 5 ulp (0.23) and expf at 3 ulp (0.20 .. 0.89) stay as assumed.
static const double T_PRE_HID = 0.05;
// the noise: TOL / TOL_EXACT of tests/test_philox_draws.py (8 x the host build's worst over 131 072 draws; TOL_EXACT where
// (x >> 8) < 2^23, so that u1 is exact in float32), |got - ref| <= tol max(1, |ref|) -- cited, not re-measured
static const double PHILOX_TOL = 8 * 5.76e-6, PHILOX_TOL_EXACT = 8 * 1.52e-7;
static const uint64_t SEED = 0x9E3779B97F4A7C15ull, OFFSET = (1ull << 33) + 5;     // bits above 32 set

static double bd(uint16_t h) { return (double)bf16_to_f32(h); }
static float rb(float f) { return bf16_to_f32(f32_to_bf16(f)); }     // rounded to bf16 once
// --host: the bf16 bits decoded by hand (sign, exponent, 7 mantissa bits), independent of bf16_to_f32
static long double bf_ld(uint16_t h)
{
    const int e = (h >> 7) & 0xff, m = h & 0x7f;
    const long double v = e ? ldexpl((long double)(128 + m), e - 134) : ldexpl((long double)m, -133);
    return (h >> 15) ? -v : v;
}
static int r16(int z) { return (z + 15) & ~15; }

// ---- judging ------------------------------------------------------------------------------------------------------------------------
enum {
    Q_HF_LIN, Q_HF_TANH, Q_HF_R, Q_HD_MULV, Q_HD_Z, Q_HD_EPS, Q_HB_D, Q_DB_DMU, Q_DB_DL,
    Q_PF_TANH32, Q_PF_TANH16, Q_PB_TANH32, Q_PB_TANH16, Q_VF_Z32, Q_VF_Z16, Q_VF_EPS, Q_VB_DMU32, Q_VB_DMU16, Q_VB_DL32, Q_VB_DL16, NQ
};
static const char* const Q_NAME[NQ] = {
    "k_fwd_hidden O32, no tanh", "k_fwd_hidden O32, tanh", "k_fwd_hidden R (bf16)", "k_fwd_head mu32 / lv32", "k_fwd_head z (bf16)",
    "k_fwd_head eps32 (Philox)", "k_bwd_hidden Dout (bf16)", "k_bwd_head dmu (bf16)", "k_bwd_head dlogvar (bf16)",
    "k_post fwd tanh, f32", "k_post fwd tanh, bf16", "k_post bwd tanh, f32", "k_post bwd tanh, bf16", "k_vae_fwd z, f32", "k_vae_fwd z, bf16",
    "k_vae_fwd eps32 (Philox)", "k_vae_bwd dmu, f32", "k_vae_bwd dmu, bf16", "k_vae_bwd dlogvar, f32", "k_vae_bwd dlogvar, bf16"};
static double g_qworst[NQ];
static long g_qn[NQ];

// feeds a quantity's table from judge()'s error / bound
static void tally(int q, double ratio)
{
    if (ratio > g_qworst[q]) g_qworst[q] = ratio;
    ++g_qn[q];
}

// the launch shapes of small_layers.hip: (waves per workgroup, waves that share K); (4, 2) is capped to 2 waves by the launcher
struct Shape { int w, kw; };
static const Shape SHAPES[] = {{1, 1}, {2, 1}, {4, 1}, {1, 2}, {2, 2}, {4, 2}, {1, 4}, {2, 4}};
static const Shape PHILOX_SHAPES[] = {{1, 1}, {1, 4}};
// runs `once` under every shape; results of equal kw must be bit-identical (the same MFMA chains)
template <typename F>
static void over_shapes(const Shape* shapes, int n, Line& L, F once)
{
    std::vector<unsigned char> first[5];
    for (int k = 0; k < n; ++k) {
        char tag[32];
        snprintf(tag, sizeof tag, "(w%d,kw%d)", shapes[k].w, shapes[k].kw);
        g_tag = tag;
        rtx_small_set_waves(shapes[k].w);
        rtx_small_set_kw(shapes[k].kw);
        const long before = L.bad;
        std::vector<unsigned char> raw;
        once(raw);
        std::vector<unsigned char>& f = first[shapes[k].kw];
        if (f.empty()) f = raw;
        else if (f != raw) {
            size_t d = 0;
            for (size_t i = 0; i < raw.size(); ++i) d += raw[i] != f[i];
            if (L.bad < 4) printf("    %s: %zu bytes differ from the first launch with kw = %d\n", tag, d, shapes[k].kw);
            ++L.bad;
        }
        if (L.bad != before) L.failed += std::string(" ") + tag;
    }
    g_tag.clear();
}

// =====================================================================================================================================
// S: small_layers.hip
// =====================================================================================================================================
static const int SBp = 128;      // two workgroup rows at 4 waves per workgroup

// a product operand pair: X [Bp][K] (rows >= B: junk; columns [0, in) real, column `in` = ones_at_in, beyond it 0) and
// Y [y_rows][K] (rows [0, real) real with columns >= in zero, the rest junk); P[b][n] = sum_k X[b][k] Y[n][k] in float64 with S = sum |.|
struct Product {
    int K, in, B, real, y_rows;
    std::vector<uint16_t> X, Y;
    std::vector<double> P, S;
};
static void gen_product(Product& p, int K, int in, int B, int real, int y_rows, bool ones, float yscale, Rng& r)
{
    p.K = K; p.in = in; p.B = B; p.real = real; p.y_rows = y_rows;
    p.X.assign((size_t)SBp * K, 0);
    p.Y.assign((size_t)y_rows * K, 0);
    for (int b = 0; b < SBp; ++b)
        for (int k = 0; k < K; ++k)
            p.X[(size_t)b * K + k] = b >= B ? f32_to_bf16(r.junk()) : k < in ? f32_to_bf16(r.f()) : (k == in && ones) ? f32_to_bf16(1.f) : 0;
    for (int n = 0; n < y_rows; ++n)
        for (int k = 0; k < K; ++k)
            p.Y[(size_t)n * K + k] = n >= real ? f32_to_bf16(r.junk()) : k < in ? f32_to_bf16(yscale * r.f()) : 0;
}
static void ref_product(Product& p)
{
    p.P.assign((size_t)p.B * p.real, 0);
    p.S.assign((size_t)p.B * p.real, 0);
    for (int b = 0; b < p.B; ++b)
        for (int n = 0; n < p.real; ++n) {
            double s = 0, a = 0;
            const uint16_t *x = &p.X[(size_t)b * p.K], *y = &p.Y[(size_t)n * p.K];
            for (int k = 0; k < p.K; ++k) { const double t = bd(x[k]) * bd(y[k]); s += t; a += fabs(t); }
            p.P[(size_t)b * p.real + n] = s;
            p.S[(size_t)b * p.real + n] = a;
        }
}
// the worst case of any order of float32 accumulation of exact bf16 x bf16 products (and of the kw recombination), bias included
static double pre_bound(int in, double S, double bias) { return (in + 2) * E24 * (S + fabs(bias)); }

// --host: the product against long double over a hand-decoded dense image, k descending, on a sample of rows; and the generator
static void host_check_product(const Product& p, bool ones, bool full_width, Line& L)
{
    const int K = p.K;
    std::vector<long double> Yd((size_t)p.real * K);
    for (int n = 0; n < p.real; ++n) for (int k = 0; k < K; ++k) Yd[(size_t)n * K + k] = bf_ld(p.Y[(size_t)n * K + k]);
    for (int b = 0; b < p.B; b += (b + 8 < p.B ? 7 : 1)) {
        std::vector<long double> xd(K);
        for (int k = 0; k < K; ++k) xd[k] = bf_ld(p.X[(size_t)b * K + k]);
        for (int n = 0; n < p.real; ++n) {
            long double s = 0;
            for (int k = K - 1; k >= 0; --k) s += xd[k] * Yd[(size_t)n * K + k];
            const double want = p.P[(size_t)b * p.real + n], scale = p.S[(size_t)b * p.real + n];
            if (!(fabsl(s - (long double)want) <= 1e-12L * scale + 1e-300L)) host_fail(L, "product: float64 %.17g, long double %.17g", want, (double)s);
        }
    }
    // junk in every masked region, the engine's operand contract, real data in the last lane group of the last fragment
    long nj = 0, nbad = 0, last = 0;
    for (int b = p.B; b < SBp; ++b) for (int k = 0; k < K; ++k) { ++nj; nbad += !is_junk(bd(p.X[(size_t)b * K + k])); }
    for (int n = p.real; n < p.y_rows; ++n) for (int k = 0; k < K; ++k) { ++nj; nbad += !is_junk(bd(p.Y[(size_t)n * K + k])); }
    if (nbad) host_fail(L, "%g masked operand elements hold no junk", (double)nbad);
    if (p.B < SBp && p.real < p.y_rows && !nj) host_fail(L, "no masked region");
    for (int b = 0; b < p.B; ++b) {
        if (bd(p.X[(size_t)b * K + p.in]) != (ones ? 1.0 : 0.0)) host_fail(L, "row %g: column `in` of the left operand", b);
        for (int k = p.in + 1; k < K; ++k) if (p.X[(size_t)b * K + k]) host_fail(L, "row %g: non-zero beyond `in`", b);
    }
    for (int n = 0; n < p.real; ++n) for (int k = p.in; k < K; ++k) if (p.Y[(size_t)n * K + k]) host_fail(L, "weight row %g: non-zero at / beyond `in`", n);
    for (int k = K - 8; k < p.in; ++k) last += p.X[(size_t)(p.B - 1) * K + k] != 0 && p.Y[(size_t)(p.real - 1) * K + k] != 0;
    if (full_width && !last) host_fail(L, "no real value in the last 8-wide lane group of the last fragment");
    if (!full_width && p.in > K - 96) host_fail(L, "no trailing fragment of padding");
}

// ---- the latent variables of the two head backward kernels: row B - 1 holds logvar = +20, -20, ~0 by j % 3, row 0 (B >= 2) |logvar| < 1e-3
static void gen_latent(int B, int Z, Rng& r, std::vector<float>& mu, std::vector<float>& lv, std::vector<float>& eps)
{
    mu.resize((size_t)B * Z); lv.resize((size_t)B * Z); eps.resize((size_t)B * Z);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < Z; ++j) {
            const size_t at = (size_t)b * Z + j;
            mu[at] = 2.f * r.f();
            eps[at] = 2.5f * r.f();
            lv[at] = 2.f * r.f();
            if (b == B - 1) lv[at] = (j % 3 == 0 ? 20.f : j % 3 == 1 ? -20.f : 0.f) + 0.25f * r.f();
            else if (b == 0) lv[at] = r.f() * (1.f / 2048.f);
        }
}
static void host_check_latent(int B, int Z, const std::vector<float>& lv, Line& L)
{
    float hi = -1e9f, lo = 1e9f, tiny = 1e9f;
    for (float x : lv) { hi = std::max(hi, x); lo = std::min(lo, x); tiny = std::min(tiny, fabsf(x)); }
    if (!(hi >= 19.f && hi <= 21.f)) host_fail(L, "no logvar near +20 (largest %g)", hi);
    if (Z >= 2 && !(lo <= -19.f && lo >= -21.f)) host_fail(L, "no logvar near -20 (smallest %g)", lo);
    if (B >= 2 && !(tiny < 1e-3f)) host_fail(L, "no |logvar| < 1e-3 (smallest %g)", tiny);
}

// z = mu + eps exp(logvar / 2) from the DEVICE's mu32 / lv32 / eps32: isolates the reparameterisation and the store.
// Bound: expf to EXP_ULPS ulps, the product and the sum one rounding each (2 (EXP_ULPS + 1) 2^-24 |eps s| + 2^-24 |z|); eval: z = mu exactly
static double z_ref(float mu, float lv, float eps, int training, bool bf16, double* bound)
{
    const double s = exp(0.5 * (double)lv), z = training ? (double)mu + (double)eps * s : (double)mu;
    *bound = (training ? 2 * (EXP_ULPS + 1) * E24 * fabs((double)eps * s) + E24 * fabs(z) : 0.0) + (bf16 ? fabs(z) / 256.0 : 0.0);
    return z;
}
// the head's gradients from dz (float64, known to e_dz): dmu = dz + beta mu / B, dlogvar = beta (e^lv - 1) / (2B) + dz eps e^(lv/2) / 2.
// dlogvar is judged against the scale of its TERMS (e^lv + 1: the cancellation at lv ~ 0): expf to EXP_ULPS ulps and three roundings each
static void head_grads(double dz, double e_dz, float mu, float lv, float eps, int training, float beta, float inv_batch, bool bf16,
                       double* dmu, double* bmu, double* dl, double* bl)
{
    const double bi = (double)beta * (double)inv_batch, s = exp(0.5 * (double)lv), e = exp((double)lv);
    *dmu = dz + bi * mu;
    *bmu = e_dz + 3 * E24 * fabs(bi * mu) + E24 * fabs(*dmu) + (bf16 ? fabs(*dmu) / 256.0 : 0.0);
    *dl = 0.5 * bi * (e - 1.0) + (training ? dz * eps * 0.5 * s : 0.0);
    const double scale = 0.5 * bi * (e + 1.0) + (training ? fabs(dz * eps) * 0.5 * s : 0.0);
    *bl = (2 * EXP_ULPS + 6) * E24 * scale + (training ? e_dz * fabs((double)eps) * 0.5 * s : 0.0) + (bf16 ? fabs(*dl) / 256.0 : 0.0);
}
// --host: both gradients against central differences (long double, h = 1e-4: truncation h^2 / 6 |f'''| <= 2e-9 of the scale, rounding
// 1e-19 |f| / h far below) of  f(mu, lv) = dz z + beta KL / B,  KL = -(1 + lv - mu^2 - e^lv) / 2;  agreement demanded: 1e-7 of the scale
static void host_check_head_grads(double dz, float mu, float lv, float eps, int training, float beta, float inv_batch, Line& L)
{
    double dmu, bmu, dl, bl;
    head_grads(dz, 0, mu, lv, eps, training, beta, inv_batch, false, &dmu, &bmu, &dl, &bl);
    const long double bi = (long double)beta * (long double)inv_batch, h = 1e-4L;
    auto f = [&](long double m, long double l) {
        const long double z = training ? m + (long double)eps * expl(0.5L * l) : m;
        return (long double)dz * z + bi * -0.5L * (1.0L + l - m * m - expl(l));
    };
    const long double gm = (f(mu + h, lv) - f(mu - h, lv)) / (2 * h), gl = (f(mu, lv + h) - f(mu, lv - h)) / (2 * h);
    const long double scale = 0.5L * bi * (expl(lv) + 1.0L) + fabsl((long double)dz * eps) * 0.5L * expl(0.5L * lv) + fabsl((long double)dz) + bi * fabsl(mu);
    if (!(fabsl(gm - dmu) <= 1e-7L * scale + 1e-12L)) host_fail(L, "dmu %.12g, central difference %.12g", dmu, (double)gm);
    if (!(fabsl(gl - dl) <= 1e-7L * scale + 1e-12L)) host_fail(L, "dlogvar %.12g, central difference %.12g", dl, (double)gl);
}

// ---- hidden layer, forward ---------------------------------------------------------------------------------------------------------
struct HidVar { int Np, N_real, tanh_act, o32, B, in_off; };
static const HidVar HID[] = {{96, 95, 1, 1, 70, 2},  {96, 80, 0, 1, 128, 2}, {96, 64, 1, 0, 1, 2},
                             {96, 33, 0, 0, 70, 100}, {32, 31, 1, 1, 70, 2},  {128, 100, 1, 1, 128, 2}};

static void fwd_hidden_case(int K, const HidVar& v, uint32_t seed)
{
    Rng r = {seed};
    const int in = K - v.in_off, B = v.B, N = v.N_real, Np = v.Np;
    Product p;
    gen_product(p, K, in, B, N, Np, true, 2.f / sqrtf((float)in), r);     // (std of a pre-activation: 2 / 3)
    std::vector<float> bias(N);
    for (auto& x : bias) x = 0.5f * r.f();
    ref_product(p);
    char name[128];
    snprintf(name, sizeof name, "S k_fwd_hidden K=%d in=%d B=%d N=%d/%d tanh=%d O32=%d", K, in, B, N, Np, v.tanh_act, v.o32);
    Line L;
    if (g_host) {
        host_check_product(p, true, v.in_off == 2, L);
        for (int b = 0; b < B; ++b)
            for (int n = 0; n < N; ++n) {
                const double x = p.P[(size_t)b * N + n] + bias[n];
                if (!(fabs(x) <= 4.0)) host_fail(L, "pre-activation %g outside +-4", x);
                if (v.tanh_act && !(fabsl(tanhl((long double)x) - (long double)tanh(x)) <= 1e-15L)) host_fail(L, "tanh(%g)", x);
            }
        report(name, L);
        return;
    }
    RtxSmallFwdArgs a = {};
    a.A = to_dev(p.X); a.W = to_dev(p.Y); a.lda = K; a.ldw = K; a.w_rows = Np;
    a.B = B; a.Bp = SBp; a.N_real = N; a.Np = Np; a.tanh_act = v.tanh_act;
    a.bias = to_dev(bias);
    const size_t n_out = (size_t)SBp * Np;
    a.O32 = v.o32 ? dev_out<float>(n_out) : nullptr;
    a.R = dev_out<uint16_t>(n_out);
    over_shapes(SHAPES, 8, L, [&](std::vector<unsigned char>& raw) {
        repoison(a.O32, n_out); repoison(a.R, n_out);
        RT(rtx_launch_small_fwd(a, 0));
        CK(hipDeviceSynchronize());
        std::vector<float> o;
        if (v.o32) o = fetch<float>(a.O32, n_out, L, "O32", &raw);
        const std::vector<uint16_t> R = fetch<uint16_t>(a.R, n_out, L, "R", &raw);
        for (int b = 0; b < SBp; ++b)
            for (int n = 0; n < Np; ++n) {
                const size_t at = (size_t)b * Np + n;
                if (b >= B || n >= N) {      // padding: +0; the ones column: 1 for b < B
                    if (v.o32) judge_bits(f_bits(o[at]), 0, L, "pad O32", b, n);
                    judge_bits(R[at], (b < B && n == N) ? 0x3f80 : 0, L, n == N ? "ones column R" : "pad R", b, n);
                    continue;
                }
                const double x = p.P[(size_t)b * N + n] + bias[n], e = T_PRE_HID * pre_bound(in, p.S[(size_t)b * N + n], bias[n]);
                const double t = tanh(x), want = v.tanh_act ? t : x;
                // through tanh: the pre-activation error times the derivative (second order: |tanh''| < 0.77) + tanhf's own error
                const double bound = v.tanh_act ? e * (1 - t * t) + e * e + 2 * TANH_ULPS * E24 * fabs(t) : e;
                if (v.o32) {
                    tally(v.tanh_act ? Q_HF_TANH : Q_HF_LIN, judge(o[at], want, bound, L, "O32", b, n));
                    judge_bits(R[at], f32_to_bf16(o[at]), L, "R vs f32_to_bf16(O32)", b, n);
                }
                tally(Q_HF_R, judge(bd(R[at]), want, bound + fabs(want) / 256.0, L, "R", b, n));
            }
    });
    report(name, L);
    free_all();
}

// ---- hidden layer, backward: Dout = (D W) (1 - o^2) ---------------------------------------------------------------------------------
static void bwd_hidden_case(int K, const HidVar& v, uint32_t seed)
{
    Rng r = {seed};
    const int in = K - v.in_off, B = v.B, N = v.N_real, Np = v.Np;
    Product p;
    gen_product(p, K, in, B, N, Np, false, 2.f / sqrtf((float)in), r);
    std::vector<float> o32((size_t)SBp * Np);
    for (int b = 0; b < SBp; ++b)
        for (int n = 0; n < Np; ++n) o32[(size_t)b * Np + n] = (b < B && n < N) ? ((b + n) % 11 == 0 ? 0.9999f : 0.999f * r.f()) : r.junk();
    ref_product(p);
    char name[128];
    snprintf(name, sizeof name, "S k_bwd_hidden K=%d in=%d B=%d N=%d/%d tanh=%d", K, in, B, N, Np, v.tanh_act);
    Line L;
    if (g_host) {
        host_check_product(p, false, v.in_off == 2, L);
        // dA = (D W) (1 - o^2) against the central difference of  F(q) = sum_n G_n tanh(q_n)  at q = atanh(o), which is separable:
        // (G tanh(q + h) - G tanh(q - h)) / 2h in long double, h = 1e-4 (truncation h^2 / 6 |tanh'''| <= 4e-9); agreement 1e-7 |G|
        for (int b = 0; b < B; ++b)
            for (int n = 0; n < N; ++n) {
                const double G = p.P[(size_t)b * N + n], o = o32[(size_t)b * Np + n];
                if (!(fabs(o) < 1.0)) host_fail(L, "activation %g outside (-1, 1)", o);
                const long double q = atanhl((long double)o), h = 1e-4L;
                const long double fd = (long double)G * (tanhl(q + h) - tanhl(q - h)) / (2 * h);
                if (!(fabsl(fd - (long double)(G * (1 - o * o))) <= 1e-7L * fabsl(G) + 1e-300L)) host_fail(L, "dA %.12g, central difference %.12g", G * (1 - o * o), (double)fd);
            }
        long nbad = 0;
        for (int b = 0; b < SBp; ++b) for (int n = 0; n < Np; ++n) if (b >= B || n >= N) nbad += !is_junk(o32[(size_t)b * Np + n]);
        if (nbad) host_fail(L, "%g masked activations hold no junk", (double)nbad);
        report(name, L);
        return;
    }
    RtxSmallBwdArgs a = {};
    a.D = to_dev(p.X); a.WT = to_dev(p.Y); a.ld = K; a.wt_rows = Np;
    a.B = B; a.Bp = SBp; a.N_real = N; a.Np = Np; a.tanh_act = v.tanh_act;
    a.O32 = v.tanh_act ? to_dev(o32) : nullptr;
    const size_t n_out = (size_t)SBp * Np;
    a.Dout = dev_out<uint16_t>(n_out);
    over_shapes(SHAPES, 8, L, [&](std::vector<unsigned char>& raw) {
        repoison(a.Dout, n_out);
        RT(rtx_launch_small_bwd(a, 0));
        CK(hipDeviceSynchronize());
        const std::vector<uint16_t> D = fetch<uint16_t>(a.Dout, n_out, L, "Dout", &raw);
        for (int b = 0; b < SBp; ++b)
            for (int n = 0; n < Np; ++n) {
                const size_t at = (size_t)b * Np + n;
                if (b >= B || n >= N) { judge_bits(D[at], 0, L, "pad Dout", b, n); continue; }
                const double G = p.P[(size_t)b * N + n], e = pre_bound(in, p.S[(size_t)b * N + n], 0), o = v.tanh_act ? (double)o32[at] : 0.0;
                const double want = G * (1 - o * o);
                // 1 - o o in float32: two roundings, absolute <= 2 x 2^-24; the product one more
                const double bound = e * (1 - o * o) + (v.tanh_act ? 2 * E24 * fabs(G) + E24 * fabs(want) : 0.0) + fabs(want) / 256.0;
                tally(Q_HB_D, judge(bd(D[at]), want, bound, L, "Dout", b, n));
            }
    });
    report(name, L);
    free_all();
}

// ---- VAE head, forward ---------------------------------------------------------------------------------------------------------------
struct HeadVar { int Z, Np_fwd, Np_bwd; };
static const HeadVar HEAD[] = {{1, 128, 128}, {20, 128, 128}, {32, 64, 64}, {40, 64, 96}};
static const int ROT_B[4] = {70, 128, 1, 70};

// noise 0: eval (an injected array is passed and must be ignored), 1: injected, 2: Philox
static void fwd_head_case(int K, const HeadVar& hv, int B, int in_off, int noise, bool outs, uint32_t seed)
{
    Rng r = {seed};
    const int in = K - in_off, Z = hv.Z, Np = hv.Np_fwd, w_rows = Z + r16(Z), training = noise != 0;
    Product p;
    gen_product(p, K, in, B, 2 * Z, w_rows, true, 2.f / sqrtf((float)in), r);
    std::vector<float> bias(2 * Z), eps_in((size_t)B * Z);
    for (int j = 0; j < Z; ++j) { bias[j] = 0.5f * r.f(); bias[Z + j] = r.f() * (1.f / 4096.f); }
    for (auto& x : eps_in) x = 2.5f * r.f();
    // input column 0 carries the logvar extremes: A[B - 1][0] = 4 against W_logvar[j][0] = +5, -5, 0 by j % 3 (row B - 1 otherwise
    // small); row 0 (B >= 2) is ~2^-13, so that with the small logvar bias |logvar| < 1e-3 there
    for (int b = 0; b < B; ++b) p.X[(size_t)b * K] = f32_to_bf16(b == B - 1 ? 4.f : 0.f);
    for (int k = 1; k < in; ++k) p.X[(size_t)(B - 1) * K + k] = f32_to_bf16(bf16_to_f32(p.X[(size_t)(B - 1) * K + k]) * 0.0625f);
    if (B >= 2) for (int k = 1; k < in; ++k) p.X[k] = f32_to_bf16(bf16_to_f32(p.X[k]) * (1.f / 8192.f));
    for (int j = 0; j < Z; ++j) p.Y[(size_t)(Z + j) * K] = f32_to_bf16(j % 3 == 0 ? 5.f : j % 3 == 1 ? -5.f : 0.f);
    ref_product(p);
    char name[160];
    snprintf(name, sizeof name, "S k_fwd_head K=%d in=%d B=%d Z=%d Np=%d w_rows=%d %s%s", K, in, B, Z, Np, w_rows,
             noise == 0 ? "eval" : noise == 1 ? "injected" : "Philox", outs ? " mu_out" : "");
    Line L;
    if (g_host) {
        host_check_product(p, true, in_off == 2, L);
        std::vector<float> lv((size_t)B * Z);
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < Z; ++j) {
                const double m = p.P[(size_t)b * 2 * Z + j] + bias[j], l = p.P[(size_t)b * 2 * Z + Z + j] + bias[Z + j];
                lv[(size_t)b * Z + j] = (float)l;
                if (!(fabs(m) <= 4.5) || !(fabs(l) <= (b == B - 1 ? 21.5 : 4.5))) host_fail(L, "mu %g / logvar %g out of range", m, l);
                double bz;      // the reparameterisation in long double
                const double z = z_ref((float)m, (float)l, eps_in[(size_t)b * Z + j], training, false, &bz);
                const long double zl = training ? (long double)(float)m + (long double)eps_in[(size_t)b * Z + j] * sqrtl(expl((long double)(float)l)) : (long double)(float)m;
                if (!(fabsl(zl - z) <= 1e-13L * (fabsl(zl) + 1))) host_fail(L, "z %.17g, long double %.17g", z, (double)zl);
            }
        host_check_latent(B, Z, lv, L);
        report(name, L);
        return;
    }
    RtxSmallFwdArgs a = {};
    a.A = to_dev(p.X); a.W = to_dev(p.Y); a.lda = K; a.ldw = K; a.w_rows = w_rows;
    a.B = B; a.Bp = SBp; a.N_real = Z; a.Np = Np; a.bias = to_dev(bias);
    a.Z = Z; a.training = training;
    a.eps_in = noise == 2 ? nullptr : to_dev(eps_in);
    a.seed = SEED; a.offset = OFFSET;
    const size_t n_r = (size_t)SBp * Np, n_l = (size_t)B * Z;
    a.R = dev_out<uint16_t>(n_r);
    a.mu32 = dev_out<float>(n_l); a.lv32 = dev_out<float>(n_l); a.eps32 = dev_out<float>(n_l);
    a.mu_out = outs ? dev_out<float>(n_l) : nullptr; a.lv_out = outs ? dev_out<float>(n_l) : nullptr;
    over_shapes(noise == 2 ? PHILOX_SHAPES : SHAPES, noise == 2 ? 2 : 8, L, [&](std::vector<unsigned char>& raw) {
        repoison(a.R, n_r); repoison(a.mu32, n_l); repoison(a.lv32, n_l); repoison(a.eps32, n_l); repoison(a.mu_out, n_l); repoison(a.lv_out, n_l);
        RT(rtx_launch_small_fwd(a, 0));
        CK(hipDeviceSynchronize());
        const std::vector<uint16_t> R = fetch<uint16_t>(a.R, n_r, L, "R", &raw);
        const std::vector<float> mu = fetch<float>(a.mu32, n_l, L, "mu32", &raw), lv = fetch<float>(a.lv32, n_l, L, "lv32", &raw), ep = fetch<float>(a.eps32, n_l, L, "eps32", &raw);
        if (outs) {
            const std::vector<float> mo = fetch<float>(a.mu_out, n_l, L, "mu_out", &raw), lo = fetch<float>(a.lv_out, n_l, L, "lv_out", &raw);
            for (size_t k = 0; k < n_l; ++k) {
                judge_bits(f_bits(mo[k]), f_bits(mu[k]), L, "mu_out vs mu32", (int)(k / Z), (int)(k % Z));
                judge_bits(f_bits(lo[k]), f_bits(lv[k]), L, "lv_out vs lv32", (int)(k / Z), (int)(k % Z));
            }
        }
        for (int b = 0; b < SBp; ++b)
            for (int j = 0; j < Np; ++j) {
                const size_t at = (size_t)b * Np + j;
                if (b >= B || j >= Z) { judge_bits(R[at], (b < B && j == Z) ? 0x3f80 : 0, L, j == Z ? "ones column R" : "pad R", b, j); continue; }
                const size_t o = (size_t)b * Z + j;
                const double m = p.P[(size_t)b * 2 * Z + j] + bias[j], l = p.P[(size_t)b * 2 * Z + Z + j] + bias[Z + j];
                tally(Q_HD_MULV, judge(mu[o], m, pre_bound(in, p.S[(size_t)b * 2 * Z + j], bias[j]), L, "mu32", b, j));
                tally(Q_HD_MULV, judge(lv[o], l, pre_bound(in, p.S[(size_t)b * 2 * Z + Z + j], bias[Z + j]), L, "lv32", b, j));
                if (noise == 0) judge_bits(f_bits(ep[o]), 0, L, "eps32 (eval)", b, j);
                else if (noise == 1) judge_bits(f_bits(ep[o]), f_bits(eps_in[o]), L, "eps32 (injected)", b, j);
                else {
                    const double ref = rtx_normal(SEED, OFFSET, (uint64_t)b * Z + j);
                    const bool exact = (philox4x32_10(SEED, OFFSET ^ 0x5851F42D4C957F2DULL, (uint64_t)b * Z + j).x >> 8) < (1u << 23);
                    tally(Q_HD_EPS, judge(ep[o], ref, (exact ? PHILOX_TOL_EXACT : PHILOX_TOL) * std::max(1.0, fabs(ref)), L, "eps32 (Philox)", b, j));
                }
                double bz;
                const double z = z_ref(mu[o], lv[o], ep[o], training, true, &bz);
                tally(Q_HD_Z, judge(bd(R[at]), z, bz, L, "z", b, j));
            }
    });
    report(name, L);
    free_all();
}

// ---- VAE head, backward --------------------------------------------------------------------------------------------------------------
static void bwd_head_case(int K, const HeadVar& hv, int B, int in_off, int training, float beta, uint32_t seed)
{
    Rng r = {seed};
    const int in = K - in_off, Z = hv.Z, Np = hv.Np_bwd, wt_rows = r16(Z);
    const float inv_batch = 1.f / B;
    Product p;
    gen_product(p, K, in, B, Z, wt_rows, false, 2.f / sqrtf((float)in), r);
    std::vector<float> mu, lv, eps;
    gen_latent(B, Z, r, mu, lv, eps);
    ref_product(p);
    char name[160];
    snprintf(name, sizeof name, "S k_bwd_head K=%d in=%d B=%d Z=%d Np=%d wt_rows=%d training=%d beta=%.1f", K, in, B, Z, Np, wt_rows, training, beta);
    Line L;
    if (g_host) {
        host_check_product(p, false, in_off == 2, L);
        host_check_latent(B, Z, lv, L);
        for (size_t k = 0; k < (size_t)B * Z; ++k) host_check_head_grads(p.P[k], mu[k], lv[k], eps[k], training, beta, inv_batch, L);
        report(name, L);
        return;
    }
    RtxSmallBwdArgs a = {};
    a.D = to_dev(p.X); a.WT = to_dev(p.Y); a.ld = K; a.wt_rows = wt_rows;
    a.B = B; a.Bp = SBp; a.Np = Np; a.Z = Z; a.training = training;
    a.mu32 = to_dev(mu); a.lv32 = to_dev(lv); a.eps32 = to_dev(eps);
    a.beta = beta; a.inv_batch = inv_batch;
    const size_t n_out = (size_t)SBp * Np;
    a.Dout = dev_out<uint16_t>(n_out);
    over_shapes(SHAPES, 8, L, [&](std::vector<unsigned char>& raw) {
        repoison(a.Dout, n_out);
        RT(rtx_launch_small_bwd(a, 0));
        CK(hipDeviceSynchronize());
        const std::vector<uint16_t> D = fetch<uint16_t>(a.Dout, n_out, L, "Dout", &raw);
        for (int b = 0; b < SBp; ++b)
            for (int n = 0; n < Np; ++n) {
                const size_t at = (size_t)b * Np + n;
                if (b >= B || n >= 2 * Z) { judge_bits(D[at], 0, L, "pad Dout", b, n); continue; }
                const int j = n < Z ? n : n - Z;
                const size_t o = (size_t)b * Z + j;
                double dmu, bmu, dl, bl;
                head_grads(p.P[o], pre_bound(in, p.S[o], 0), mu[o], lv[o], eps[o], training, beta, inv_batch, true, &dmu, &bmu, &dl, &bl);
                if (n < Z) tally(Q_DB_DMU, judge(bd(D[at]), dmu, bmu, L, "dmu", b, j));
                else tally(Q_DB_DL, judge(bd(D[at]), dl, bl, L, "dlogvar", b, j));
            }
    });
    report(name, L);
    free_all();
}

static void small_cases()
{
    uint32_t seed = 1000;
    for (int ki = 0; ki < 8; ++ki) {
        const int K = 128 * (ki + 1);
        for (const HidVar& v : HID) fwd_hidden_case(K, v, ++seed);
        for (const HidVar& v : HID) bwd_hidden_case(K, v, ++seed);
        for (int zi = 0; zi < 4; ++zi) {     // B, the noise, the outputs and `in` rotate: every Z sees every value over the eight K
            const int rot = (zi + ki) % 4;
            fwd_head_case(K, HEAD[zi], ROT_B[rot], rot == 2 ? 100 : 2, rot == 1 ? 0 : 1, rot % 2 == 0, ++seed);
            fwd_head_case(K, HEAD[zi], 70, 2, 2, true, ++seed);
            bwd_head_case(K, HEAD[zi], ROT_B[rot], rot == 2 ? 100 : 2, rot != 1, (rot + ki / 4) % 2 ? 0.f : BETA, ++seed);
        }
    }
    rtx_small_set_waves(1);
    rtx_small_set_kw(1);
}

// =====================================================================================================================================
// P: post_layers.hip
// =====================================================================================================================================
static const int PBp = 32;

// slabs [splits][slab_stride] of [Bp][ldc]: real values where b < B and col < real_cols, junk everywhere else (padded rows, the columns
// behind the real ones and behind Np, the gap between Bp ldc and slab_stride)
static std::vector<float> gen_slabs(int splits, long stride, int ldc, int B, int real_cols, float scale, Rng& r)
{
    std::vector<float> C((size_t)splits * stride);
    for (int s = 0; s < splits; ++s)
        for (long k = 0; k < stride; ++k) {
            const long b = k / ldc, c = k % ldc;
            C[(size_t)s * stride + k] = (b < B && c < real_cols) ? scale * r.f() : r.junk();
        }
    return C;
}
// the slab sum as the kernels form it: float32 additions in slab order starting from +0
static float slab_sum(const std::vector<float>& C, int splits, long stride, size_t at, long double* exact = nullptr, long double* abs_sum = nullptr)
{
    float c = 0.f;
    long double e = 0, a = 0;
    for (int s = 0; s < splits; ++s) { const float t = C[(size_t)s * stride + at]; c += t; e += t; a += fabsl(t); }
    if (exact) { *exact = e; *abs_sum = a; }
    return c;
}
static void host_check_slabs(const std::vector<float>& C, int splits, long stride, int ldc, int B, int real_cols, Line& L)
{
    long nbad = 0;
    for (int s = 0; s < splits; ++s)
        for (long k = 0; k < stride; ++k) {
            const long b = k / ldc, c = k % ldc;
            if (b < B && c < real_cols) {
                if (s) continue;
                long double e, a;      // the float32 sum against long double: splits roundings of the partial sums
                const float f = slab_sum(C, splits, stride, (size_t)k, &e, &a);
                if (!(fabsl(e - f) <= splits * E24 * a)) host_fail(L, "slab sum %.9g, long double %.9g", f, (double)e);
            } else nbad += !is_junk(C[(size_t)s * stride + k]);
        }
    if (nbad) host_fail(L, "%g masked slab elements hold no junk", (double)nbad);
}

template <typename T> static double elem(T v);
template <> double elem<float>(float v) { return v; }
template <> double elem<uint16_t>(uint16_t v) { return bd(v); }
template <typename T> static uint32_t bits_of(T v);
template <> uint32_t bits_of<float>(float v) { return f_bits(v); }
template <> uint32_t bits_of<uint16_t>(uint16_t v) { return v; }
template <typename T> static uint32_t bits_from(float x);
template <> uint32_t bits_from<float>(float x) { return f_bits(x); }
template <> uint32_t bits_from<uint16_t>(float x) { return f32_to_bf16(x); }

struct PostCase { int splits, Np, N_real, mode, B, tanh_act, ones, o32_null, r_null; };

template <typename T>
static void post_case(const PostCase& c, uint32_t seed)
{
    const bool bf16 = sizeof(T) == 2, fwd = c.mode == RTX_POST_FWD;
    Rng r = {seed};
    const int Np = c.Np, N = c.N_real, B = c.B, ldc = Np + 4;
    const long stride = (long)PBp * ldc + 64;
    const std::vector<float> C = gen_slabs(c.splits, stride, ldc, B, N, 1.5f / c.splits, r);
    std::vector<float> bias(N), o32((size_t)PBp * Np);
    for (auto& x : bias) x = r.f();
    for (int b = 0; b < PBp; ++b) for (int n = 0; n < Np; ++n) o32[(size_t)b * Np + n] = (b < B && n < N) ? 0.999f * r.f() : r.junk();
    char name[160];
    snprintf(name, sizeof name, "P k_post<%s, %s, %d> splits=%d B=%d N=%d/%d tanh=%d ones=%d%s%s", bf16 ? "bf16" : "f32", fwd ? "FWD" : "BWD",
             c.splits <= 16 ? 16 : 32, c.splits, B, N, Np, c.tanh_act, c.ones, fwd && c.o32_null ? " O32=null" : "", c.r_null ? " R=null" : "");
    Line L;
    if (g_host) {
        host_check_slabs(C, c.splits, stride, ldc, B, N, L);
        for (int b = 0; b < B && c.tanh_act; ++b)      // the activation and its derivative in long double
            for (int n = 0; n < N; ++n) {
                const float s = slab_sum(C, c.splits, stride, (size_t)b * ldc + n), x = fwd ? s + bias[n] : s;
                const long double o = o32[(size_t)b * Np + n];
                const double want = fwd ? tanh((double)x) : (double)s * (1 - (double)o * (double)o);
                const long double second = fwd ? tanhl((long double)x) : (long double)s - (long double)s * o * o;
                if (!(fabs(x) <= 4.0) || !(fabsl(o) < 1.0L)) host_fail(L, "pre-activation %g / activation %g out of range", x, (double)o);
                if (!(fabsl(second - want) <= 1e-15L * (fabsl(second) + fabs((double)s)))) host_fail(L, "reference %.17g, long double %.17g", want, (double)second);
            }
        report(name, L);
        return;
    }
    RtxPostArgs a = {};
    a.C = to_dev(C); a.splits = c.splits; a.slab_stride = stride; a.ldc = ldc;
    a.B = B; a.Bp = PBp; a.N_real = N; a.Np = Np; a.tanh_act = c.tanh_act; a.ones_col = c.ones;
    const size_t n_out = (size_t)PBp * Np;
    const bool have_o32 = fwd && !c.o32_null, have_r = !c.r_null;
    if (fwd) { a.bias = to_dev(bias); a.O32 = have_o32 ? dev_out<float>(n_out) : nullptr; }
    else a.O32 = c.tanh_act ? to_dev(o32) : nullptr;
    a.R = have_r ? dev_out<T>(n_out) : nullptr;
    RT(rtx_launch_post(a, c.mode, bf16, 0));
    CK(hipDeviceSynchronize());
    std::vector<float> O;
    std::vector<T> R;
    if (have_o32) O = fetch<float>(a.O32, n_out, L, "O32");
    if (have_r) R = fetch<T>(a.R, n_out, L, "R");
    const int q = fwd ? (bf16 ? Q_PF_TANH16 : Q_PF_TANH32) : (bf16 ? Q_PB_TANH16 : Q_PB_TANH32);
    for (int b = 0; b < PBp; ++b)
        for (int n = 0; n < Np; ++n) {
            const size_t at = (size_t)b * Np + n;
            if (b >= B || n >= N) {
                if (have_o32) judge_bits(f_bits(O[at]), 0, L, "pad O32", b, n);
                const bool one = fwd && c.ones && b < B && n == N;
                if (have_r) judge_bits(bits_of<T>(R[at]), one ? bits_from<T>(1.f) : 0, L, n == N ? "ones column R" : "pad R", b, n);
                continue;
            }
            const float s = slab_sum(C, c.splits, stride, (size_t)b * ldc + n), x = fwd ? s + bias[n] : s;
            if (!c.tanh_act) {       // a fixed sequence of float32 additions: bit for bit
                if (have_o32) judge_bits(f_bits(O[at]), f_bits(x), L, "O32", b, n);
                if (have_r) judge_bits(bits_of<T>(R[at]), bits_from<T>(x), L, "R", b, n);
                continue;
            }
            double want, bound;
            if (fwd) { want = tanh((double)x); bound = 2 * TANH_ULPS * E24 * fabs(want); }
            else {                   // s (1 - o o): 1 - o o to 2 x 2^-24 absolute, the product one rounding
                const double o = o32[at];
                want = (double)s * (1 - o * o); bound = 2 * E24 * fabs((double)s) + E24 * fabs(want);
            }
            if (have_o32) tally(Q_PF_TANH32, judge(O[at], want, bound, L, "O32", b, n));
            if (have_r) tally(q, judge(elem<T>(R[at]), want, bound + (bf16 ? fabs(want) / 256.0 : 0.0), L, "R", b, n));
            if (have_o32 && have_r && bf16) judge_bits(bits_of<T>(R[at]), f32_to_bf16(O[at]), L, "R vs f32_to_bf16(O32)", b, n);
            if (have_o32 && have_r && !bf16) judge_bits(bits_of<T>(R[at]), f_bits(O[at]), L, "R vs O32", b, n);
        }
    report(name, L);
    free_all();
}

static void post_cases()
{
    static const int SPLITS[] = {1, 2, 16, 17, 32, 33}, BS[] = {32, 21, 1};
    uint32_t seed = 5000;
    int k = 0;
    for (int splits : SPLITS)
        for (int Np : {64, 128})
            for (int nr = 0; nr < 6; ++nr) {
                const int N = nr < 4 ? Np - 1 - nr : nr == 4 ? 64 : Np;
                if (nr == 4 && Np == 64) continue;
                for (int mode : {RTX_POST_FWD, RTX_POST_BWD})
                    for (int bf16 = 0; bf16 < 2; ++bf16, ++k) {      // B, tanh, the ones column and the null outputs rotate with coprime periods
                        PostCase c = {splits, Np, N, mode, BS[k % 3], (k / 3) % 2, mode == RTX_POST_FWD ? (k / 6) % 2 : 0, 0, 0};
                        if (mode == RTX_POST_FWD) { c.o32_null = k % 5 == 1; c.r_null = !c.o32_null && k % 7 == 2; }
                        if (bf16) post_case<uint16_t>(c, ++seed); else post_case<float>(c, ++seed);
                    }
            }
}

// ---- k_vae_fwd -------------------------------------------------------------------------------------------------------------------------
struct VaeShape { int Z, Zp, Np_bwd; };
static const VaeShape VAE[] = {{1, 64, 64}, {40, 64, 128}, {63, 64, 128}, {64, 128, 192}, {100, 128, 256}};

template <typename T>
static void vae_fwd_case(int splits, const VaeShape& vs, int B, int noise, bool outs, uint32_t seed)
{
    const bool bf16 = sizeof(T) == 2;
    Rng r = {seed};
    const int Z = vs.Z, Zp = vs.Zp, ldc = 2 * Z + 3, training = noise != 0;
    const long stride = (long)PBp * ldc + 64;
    std::vector<float> C = gen_slabs(splits, stride, ldc, B, 2 * Z, 1.5f / splits, r);
    std::vector<float> bias(2 * Z), eps_in((size_t)B * Z);
    for (int j = 0; j < Z; ++j) { bias[j] = 0.5f * r.f(); bias[Z + j] = r.f() * (1.f / 8192.f); }
    for (auto& x : eps_in) x = 2.5f * r.f();
    for (int s = 0; s < splits; ++s)      // logvar: row B - 1 = +20, -20, ~0 by j % 3 (slab 0; small parts in the others), row 0 (B >= 2) tiny
        for (int j = 0; j < Z; ++j) {
            C[(size_t)s * stride + (size_t)(B - 1) * ldc + Z + j] = s ? 0.01f * r.f() : (j % 3 == 0 ? 20.f : j % 3 == 1 ? -20.f : 0.f) + 0.25f * r.f();
            if (B >= 2) C[(size_t)s * stride + Z + j] = r.f() * (1.f / 16384.f);
        }
    char name[160];
    snprintf(name, sizeof name, "P k_vae_fwd<%s> splits=%d B=%d Z=%d/%d %s%s", bf16 ? "bf16" : "f32", splits, B, Z, Zp,
             noise == 0 ? "eval" : noise == 1 ? "injected" : "Philox", outs ? " mu_out" : "");
    Line L;
    if (g_host) {
        host_check_slabs(C, splits, stride, ldc, B, 2 * Z, L);
        std::vector<float> lv((size_t)B * Z);
        for (int b = 0; b < B; ++b) for (int j = 0; j < Z; ++j) lv[(size_t)b * Z + j] = slab_sum(C, splits, stride, (size_t)b * ldc + Z + j) + bias[Z + j];
        host_check_latent(B, Z, lv, L);
        report(name, L);
        return;
    }
    RtxVaeFwdArgs a = {};
    a.C = to_dev(C); a.splits = splits; a.slab_stride = stride; a.ldc = ldc;
    a.B = B; a.Bp = PBp; a.Z = Z; a.Zp = Zp; a.bias = to_dev(bias);
    const size_t n_r = (size_t)PBp * Zp, n_l = (size_t)B * Z;
    a.mu32 = dev_out<float>(n_l); a.lv32 = dev_out<float>(n_l); a.eps32 = dev_out<float>(n_l);
    a.mu_out = outs ? dev_out<float>(n_l) : nullptr; a.lv_out = outs ? dev_out<float>(n_l) : nullptr;
    a.Zr = dev_out<T>(n_r);
    a.training = training; a.eps_in = noise == 2 ? nullptr : to_dev(eps_in); a.seed = SEED; a.offset = OFFSET;
    RT(rtx_launch_vae_fwd(a, bf16, 0));
    CK(hipDeviceSynchronize());
    const std::vector<T> R = fetch<T>(a.Zr, n_r, L, "Zr");
    const std::vector<float> mu = fetch<float>(a.mu32, n_l, L, "mu32"), lv = fetch<float>(a.lv32, n_l, L, "lv32"), ep = fetch<float>(a.eps32, n_l, L, "eps32");
    if (outs) {
        const std::vector<float> mo = fetch<float>(a.mu_out, n_l, L, "mu_out"), lo = fetch<float>(a.lv_out, n_l, L, "lv_out");
        for (size_t k = 0; k < n_l; ++k) {
            judge_bits(f_bits(mo[k]), f_bits(mu[k]), L, "mu_out vs mu32", (int)(k / Z), (int)(k % Z));
            judge_bits(f_bits(lo[k]), f_bits(lv[k]), L, "lv_out vs lv32", (int)(k / Z), (int)(k % Z));
        }
    }
    for (int b = 0; b < PBp; ++b)
        for (int j = 0; j < Zp; ++j) {
            const size_t at = (size_t)b * Zp + j;
            if (b >= B || j >= Z) { judge_bits(bits_of<T>(R[at]), (b < B && j == Z) ? bits_from<T>(1.f) : 0, L, j == Z ? "ones column Zr" : "pad Zr", b, j); continue; }
            const size_t o = (size_t)b * Z + j;
            // one more float32 addition behind the slab sum: bit for bit
            judge_bits(f_bits(mu[o]), f_bits(slab_sum(C, splits, stride, (size_t)b * ldc + j) + bias[j]), L, "mu32", b, j);
            judge_bits(f_bits(lv[o]), f_bits(slab_sum(C, splits, stride, (size_t)b * ldc + Z + j) + bias[Z + j]), L, "lv32", b, j);
            if (noise == 0) judge_bits(f_bits(ep[o]), 0, L, "eps32 (eval)", b, j);
            else if (noise == 1) judge_bits(f_bits(ep[o]), f_bits(eps_in[o]), L, "eps32 (injected)", b, j);
            else {
                const double ref = rtx_normal(SEED, OFFSET, (uint64_t)b * Z + j);
                const bool exact = (philox4x32_10(SEED, OFFSET ^ 0x5851F42D4C957F2DULL, (uint64_t)b * Z + j).x >> 8) < (1u << 23);
                tally(Q_VF_EPS, judge(ep[o], ref, (exact ? PHILOX_TOL_EXACT : PHILOX_TOL) * std::max(1.0, fabs(ref)), L, "eps32 (Philox)", b, j));
            }
            double bz;
            const double z = z_ref(mu[o], lv[o], ep[o], training, bf16, &bz);
            if (bz > 0) tally(bf16 ? Q_VF_Z16 : Q_VF_Z32, judge(elem<T>(R[at]), z, bz, L, "z", b, j));
            else judge_bits(bits_of<T>(R[at]), bits_from<T>(mu[o]), L, "z (eval)", b, j);
        }
    report(name, L);
    free_all();
}

template <typename T>
static void vae_bwd_case(int splits, const VaeShape& vs, int B, int training, float beta, uint32_t seed)
{
    const bool bf16 = sizeof(T) == 2;
    Rng r = {seed};
    const int Z = vs.Z, Np = vs.Np_bwd, ldc = Z + 3;
    const long stride = (long)PBp * ldc + 64;
    const float inv_batch = 1.f / B;
    const std::vector<float> C = gen_slabs(splits, stride, ldc, B, Z, 1.5f / splits, r);
    std::vector<float> mu, lv, eps;
    gen_latent(B, Z, r, mu, lv, eps);
    char name[160];
    snprintf(name, sizeof name, "P k_vae_bwd<%s> splits=%d B=%d Z=%d Np=%d training=%d beta=%.1f", bf16 ? "bf16" : "f32", splits, B, Z, Np, training, beta);
    Line L;
    if (g_host) {
        host_check_slabs(C, splits, stride, ldc, B, Z, L);
        host_check_latent(B, Z, lv, L);
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < Z; ++j)
                host_check_head_grads(slab_sum(C, splits, stride, (size_t)b * ldc + j), mu[(size_t)b * Z + j], lv[(size_t)b * Z + j], eps[(size_t)b * Z + j],
                                      training, beta, inv_batch, L);
        report(name, L);
        return;
    }
    RtxVaeBwdArgs a = {};
    a.C = to_dev(C); a.splits = splits; a.slab_stride = stride; a.ldc = ldc;
    a.B = B; a.Bp = PBp; a.Z = Z; a.Np = Np;
    a.mu32 = to_dev(mu); a.lv32 = to_dev(lv); a.eps32 = to_dev(eps);
    a.training = training; a.beta = beta; a.inv_batch = inv_batch;
    const size_t n_out = (size_t)PBp * Np;
    a.D = dev_out<T>(n_out);
    RT(rtx_launch_vae_bwd(a, bf16, 0));
    CK(hipDeviceSynchronize());
    const std::vector<T> D = fetch<T>(a.D, n_out, L, "D");
    for (int b = 0; b < PBp; ++b)
        for (int n = 0; n < Np; ++n) {
            const size_t at = (size_t)b * Np + n;
            if (b >= B || n >= 2 * Z) { judge_bits(bits_of<T>(D[at]), 0, L, "pad D", b, n); continue; }
            const int j = n < Z ? n : n - Z;
            const size_t o = (size_t)b * Z + j;
            double dmu, bmu, dl, bl;      // dz: the float32 slab sum, exact to the bit
            head_grads(slab_sum(C, splits, stride, (size_t)b * ldc + j), 0, mu[o], lv[o], eps[o], training, beta, inv_batch, bf16, &dmu, &bmu, &dl, &bl);
            if (n < Z) tally(bf16 ? Q_VB_DMU16 : Q_VB_DMU32, judge(elem<T>(D[at]), dmu, bmu, L, "dmu", b, j));
            else tally(bf16 ? Q_VB_DL16 : Q_VB_DL32, judge(elem<T>(D[at]), dl, bl, L, "dlogvar", b, j));
        }
    report(name, L);
    free_all();
}

static void vae_cases()
{
    static const int BS[] = {32, 21, 1};
    uint32_t seed = 7000;
    int k = 0;
    for (int splits : {1, 2, 3, 5})
        for (const VaeShape& vs : VAE)
            for (int bf16 = 0; bf16 < 2; ++bf16, ++k) {      // B, the noise, the outputs, training and beta rotate with coprime periods
                const int B = BS[k % 3], noise = (k / 3 + k) % 3;
                const bool outs = (k / 2) % 2 == 0;
                const int training = k % 5 != 3;
                const float beta = (k / 5 + k) % 2 ? BETA : 0.f;
                if (bf16) { vae_fwd_case<uint16_t>(splits, vs, B, noise, outs, ++seed); vae_bwd_case<uint16_t>(splits, vs, B, training, beta, ++seed); }
                else { vae_fwd_case<float>(splits, vs, B, noise, outs, ++seed); vae_bwd_case<float>(splits, vs, B, training, beta, ++seed); }
            }
}

// =====================================================================================================================================
// --host: the launchers refuse what their kernels cannot take (every RTX_CHECK returns before the first HIP call)
// =====================================================================================================================================
static void refusal(const char* what, int rc)
{
    Line L;
    if (rc != RTX_EINVAL) host_fail(L, "accepted (return code %g)", rc);
    char name[160];
    snprintf(name, sizeof name, "R refused: %s", what);
    report(name, L, rc == RTX_EINVAL ? (std::string("  [") + rtx_last_error_str() + "]").c_str() : "");
}
static void refusal_cases()
{
    static uint16_t dummy[4];      // a non-null pointer no refused launch reads
    bf16_t* const out = (bf16_t*)dummy;
    auto fwd = [&](int K, int ldw, int w_rows, int B, int Bp, int N, int Np, int Z) {
        RtxSmallFwdArgs a = {};
        a.lda = K; a.ldw = ldw; a.w_rows = w_rows; a.B = B; a.Bp = Bp; a.N_real = N; a.Np = Np; a.Z = Z; a.R = out;
        return rtx_launch_small_fwd(a, 0);
    };
    auto bwd = [&](int K, int wt_rows, int B, int Bp, int N, int Np, int Z) {
        RtxSmallBwdArgs a = {};
        a.ld = K; a.wt_rows = wt_rows; a.B = B; a.Bp = Bp; a.N_real = N; a.Np = Np; a.Z = Z; a.Dout = out;
        return rtx_launch_small_bwd(a, 0);
    };
    refusal("small_fwd K = 64", fwd(64, 64, 96, 70, 128, 95, 96, 0));
    refusal("small_fwd K = 1088", fwd(1088, 1088, 96, 70, 128, 95, 96, 0));
    refusal("small_fwd K = 192", fwd(192, 192, 96, 70, 128, 95, 96, 0));
    refusal("small_fwd ldw != lda", fwd(128, 256, 96, 70, 128, 95, 96, 0));
    refusal("small_fwd Bp % 64 != 0", fwd(128, 128, 96, 70, 96, 95, 96, 0));
    refusal("small_fwd Np % 32 != 0", fwd(128, 128, 96, 70, 128, 47, 48, 0));
    refusal("small_fwd hidden w_rows one short", fwd(128, 128, 95, 70, 128, 95, 96, 0));
    refusal("small_fwd head w_rows one short", fwd(128, 128, 20 + 32 - 1, 70, 128, 20, 128, 20));
    refusal("small_fwd B = 0", fwd(128, 128, 96, 0, 128, 95, 96, 0));
    refusal("small_fwd head Np == Z", fwd(128, 128, 64, 70, 128, 32, 32, 32));
    refusal("small_bwd K = 64", bwd(64, 96, 70, 128, 95, 96, 0));
    refusal("small_bwd K = 1088", bwd(1088, 96, 70, 128, 95, 96, 0));
    refusal("small_bwd K = 192", bwd(192, 96, 70, 128, 95, 96, 0));
    refusal("small_bwd Bp % 64 != 0", bwd(128, 96, 70, 96, 95, 96, 0));
    refusal("small_bwd Np % 32 != 0", bwd(128, 96, 70, 128, 47, 48, 0));
    refusal("small_bwd hidden wt_rows one short", bwd(128, 95, 70, 128, 95, 96, 0));
    refusal("small_bwd head wt_rows one short", bwd(128, 31, 70, 128, 0, 128, 20));
    refusal("small_bwd head Np < 2 Z", bwd(128, 48, 70, 128, 0, 64, 40));
    auto post = [&](int Np, int ldc) {
        RtxPostArgs a = {};
        a.splits = 1; a.ldc = ldc; a.slab_stride = 32L * ldc; a.B = 21; a.Bp = 32; a.N_real = Np - 1; a.Np = Np; a.R = dummy;
        return rtx_launch_post(a, RTX_POST_FWD, 1, 0);
    };
    refusal("post Np % 64 != 0", post(96, 100));
    refusal("post ldc % 4 != 0", post(128, 130));
    auto vf = [&](int Z, int Zp, int B, int Bp, int ldc) {
        RtxVaeFwdArgs a = {};
        a.splits = 1; a.ldc = ldc; a.slab_stride = (long)Bp * ldc; a.B = B; a.Bp = Bp; a.Z = Z; a.Zp = Zp; a.Zr = dummy;
        return rtx_launch_vae_fwd(a, 1, 0);
    };
    refusal("vae_fwd Z = 0", vf(0, 64, 21, 32, 128));
    refusal("vae_fwd B = 0", vf(40, 64, 0, 32, 128));
    refusal("vae_fwd Zp % 64 != 0", vf(40, 96, 21, 32, 128));
    refusal("vae_fwd Zp == Z", vf(64, 64, 21, 32, 128));
    refusal("vae_fwd Bp % 16 != 0", vf(40, 64, 21, 24, 128));
    refusal("vae_fwd ldc < 2 Z", vf(40, 64, 21, 32, 79));
    auto vb = [&](int Z, int Np, int B, int Bp, int ldc) {
        RtxVaeBwdArgs a = {};
        a.splits = 1; a.ldc = ldc; a.slab_stride = (long)Bp * ldc; a.B = B; a.Bp = Bp; a.Z = Z; a.Np = Np; a.D = dummy;
        return rtx_launch_vae_bwd(a, 1, 0);
    };
    refusal("vae_bwd Z = 0", vb(0, 128, 21, 32, 64));
    refusal("vae_bwd B = 0", vb(40, 128, 0, 32, 64));
    refusal("vae_bwd Np % 64 != 0", vb(40, 96, 21, 32, 64));
    refusal("vae_bwd Np < 2 Z", vb(40, 64, 21, 32, 64));
    refusal("vae_bwd Bp % 16 != 0", vb(40, 128, 21, 24, 64));
    refusal("vae_bwd ldc < Z", vb(40, 128, 21, 32, 39));
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    setvbuf(stdout, nullptr, _IOLBF, 0);
    small_cases();
    post_cases();
    vae_cases();
    if (g_host) refusal_cases();
    else {
        printf("worst error / bound by quantity (DESIGN.md section 6):\n");
        for (int q = 0; q < NQ; ++q) printf("    %-32s %.4f   (%ld elements)\n", Q_NAME[q], g_qworst[q], g_qn[q]);
    }
    return finish("LAYER");
}
