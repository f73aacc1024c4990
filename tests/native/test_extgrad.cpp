// test_extgrad -- the kernels behind rtx_engine_backward (a loss computed outside the engine) against float64, element by element:
//   A  loss.hip: rtx_launch_import_dout, both output types, the identity and the sigmoid form, aligned / unaligned / strided sources
//   B  post_layers.hip k_vae_bwd and small_layers.hip k_bwd_head with the external d loss / d mu, d loss / d logvar set, and with them
//      null (the built-in KL terms: the numbers test_layers checks)
// Every output is poisoned before the launch and carries a poisoned guard; padding rows and columns are checked bit for bit.
//   test_extgrad          the kernels on the device
//   test_extgrad --host   no HIP call: the case generators and the float64 references against a second formulation
// Bounds.  float32 outputs that are one rounding of exact inputs (D = g; dmu = dz + g_mu from the float32 slab sum) are compared bit for
// bit.  bf16 outputs: half a bf16 unit of the float64 value, plus what the float32 arithmetic in front of the rounding may have moved.
// The sigmoid form as test_loss bounds its own sigmoid: p to 3 float32 ulps (expf, an addition, a division), then (g (1 - p)) p in
// three roundings: |g| (3 p^2 + 6 p (1 - p)) 2^-24 <= 8 |g| p 2^-24; where the float32 p is exactly 1 or 0 (y >= 18, y <= -89) the
// result must be a zero.  At y = -40 p (1 - p) = 4.2e-18 is an ordinary float32 (and bf16) number: the float64 value is demanded there,
// and that it is finite; at y = +40 the exact zero.
#include "../../rectorch_amd/csrc/rtx_kernels.h"

#include "check.h"

static const double EXP_ULPS = 3;      // device expf, as tests/native/test_layers.cpp assumes it
static double bd(uint16_t h) { return (double)bf16_to_f32(h); }
static int r16(int z) { return (z + 15) & ~15; }
// half a unit in the last place of the bf16 grid at x: |x| in [2^k, 2^(k + 1)) has 8 significant bits, a unit of 2^(k - 7)
static double half_ulp_bf16(double x)
{
    if (x == 0) return 0;
    int e;
    frexp(fabs(x), &e);     // |x| = m 2^e, m in [0.5, 1): k = e - 1
    return ldexp(1.0, e - 9);
}

// =====================================================================================================================================
// A: rtx_launch_import_dout
// =====================================================================================================================================
static const int ABp = 48;
static bool exact_zero(float y) { return y >= 18.f || y <= -89.f; }

template <typename T>
static void import_case(int B, int I, int ld, bool sigmoid, uint32_t seed)
{
    const bool bf16 = sizeof(T) == 2;
    Rng r = {seed};
    const int ldd = (I + 7) / 8 * 8 + 8, ldy = (I + 3) / 4 * 4 + 4;
    std::vector<float> G((size_t)B * ld), Y((size_t)ABp * ldy);
    static const float ext[6] = {40.f, -40.f, 20.f, 90.f, -90.f, 17.5f};
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < ld; ++i) G[(size_t)b * ld + i] = i < I ? 2.f * r.f() : r.junk();     // a strided source: junk between the rows
    for (int b = 0; b < ABp; ++b)
        for (int i = 0; i < ldy; ++i) Y[(size_t)b * ldy + i] = (b < B && i < I) ? 10.f * r.f() : r.junk();
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 6 && k < I; ++k) { Y[(size_t)b * ldy + (k + b) % I] = ext[k]; Y[(size_t)b * ldy + I - 1 - (k + 2 * b) % I] = ext[(k + b) % 6]; }
    char name[160];
    snprintf(name, sizeof name, "A import_dout<%s, %s> B=%d I=%d ld=%d ldd=%d ldy=%d", bf16 ? "bf16" : "f32", sigmoid ? "sigmoid" : "identity", B, I, ld, ldd, ldy);
    Line L;
    // float64 reference and bound
    std::vector<double> D((size_t)B * I), bound((size_t)B * I);
    long n40 = 0, nm40 = 0;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < I; ++i) {
            const double g = G[(size_t)b * ld + i], y = Y[(size_t)b * ldy + i];
            double d = g, db = 0;
            if (sigmoid) {
                // 1 - p as sigmoid(-y): in float64 too, 1.0 - p would cancel (at y = 40 to nothing)
                const double p = 1.0 / (1.0 + exp(-y)), q = 1.0 / (1.0 + exp(y));
                d = g * p * q;
                db = 8 * E24 * fabs(g) * p;
                n40 += y == 40.0; nm40 += y == -40.0;
                if (g_host) {      // second formulation: d sigmoid / dy = 1 / (2 + e^y + e^-y), in long double
                    const long double alt = (long double)g / (2.0L + expl((long double)y) + expl(-(long double)y));
                    if (!(fabsl(alt - (long double)d) <= 1e-12L * fabsl(alt) + 1e-300L)) host_fail(L, "sigmoid': %.17g, second formulation %.17g", d, (double)alt);
                    if (!(fabs(y) <= 10.0 || y == 40 || y == -40 || y == 20 || y == 90 || y == -90 || y == 17.5)) host_fail(L, "logit %g outside the generator's set", y);
                    if (!std::isfinite(d)) host_fail(L, "the reference is not finite at y = %g", y);
                }
            }
            if (bf16) db += half_ulp_bf16(d) + E24 * fabs(d);
            if (g_host && !(fabs(g) <= 2.0)) host_fail(L, "gradient %g outside [-2, 2]", g);
            D[(size_t)b * I + i] = d; bound[(size_t)b * I + i] = db;
        }
    if (g_host) {
        if (sigmoid && !(n40 >= B && nm40 >= B)) host_fail(L, "logits of +40 / -40: %g / %g, fewer than one per row", (double)n40, (double)nm40);
        for (int b = 0; b < B; ++b) for (int i = I; i < ld; ++i) if (!is_junk(G[(size_t)b * ld + i])) host_fail(L, "no junk between the source rows (row %g)", b);
        if (half_ulp_bf16(1.0) != 1.0 / 256 || half_ulp_bf16(-1.99) != 1.0 / 256 || half_ulp_bf16(2.0) != 1.0 / 128) host_fail(L, "half_ulp_bf16");
        report(name, L);
        return;
    }
    RtxDlogitsArgs a = {};
    a.loss.B = B; a.loss.I = I;
    if (sigmoid) { a.loss.Y = to_dev(Y); a.loss.ldy = ldy; }
    a.Bp = ABp; a.ldd = ldd;
    const size_t n_out = (size_t)ABp * ldd;
    a.D = dev_out<T>(n_out);
    const float* dG = to_dev(G);
    RT(rtx_launch_import_dout(a, dG, ld, sigmoid, bf16, 0));
    CK(hipDeviceSynchronize());
    const std::vector<T> got = fetch<T>(a.D, n_out, L, "D");
    for (int b = 0; b < ABp; ++b)
        for (int i = 0; i < ldd; ++i) {
            const size_t at = (size_t)b * ldd + i;
            uint32_t bits; double v;
            if (bf16) { bits = ((const uint16_t*)got.data())[at]; v = bd((uint16_t)bits); }
            else { const float f = ((const float*)got.data())[at]; bits = f_bits(f); v = f; }
            if (b >= B || i >= I) { judge_bits(bits, 0, L, "pad D", b, i); continue; }
            const size_t o = (size_t)b * I + i;
            if (sigmoid && exact_zero(Y[(size_t)b * ldy + i])) {
                if (!(v == 0.0)) { if (L.bad < 4) printf("    D[%d][%d] = %.9g at logit %g, expected a zero\n", b, i, v, Y[(size_t)b * ldy + i]); ++L.bad; }
            } else if (!sigmoid && !bf16) {
                judge_bits(bits, f_bits(G[(size_t)b * ld + i]), L, "D", b, i);
            } else {
                judge(v, D[o], bound[o], L, "D", b, i);
            }
        }
    report(name, L);
    free_all();
}

static void import_cases()
{
    static const int SH[3][3] = {{1, 9, 9}, {17, 4097, 4097}, {33, 8200, 8208}};
    uint32_t seed = 100;
    for (int sig = 0; sig < 2; ++sig)
        for (const auto& s : SH) {
            import_case<float>(s[0], s[1], s[2], sig != 0, ++seed);
            import_case<uint16_t>(s[0], s[1], s[2], sig != 0, ++seed);
        }
}

// =====================================================================================================================================
// B: the VAE head's backward with external d loss / d mu, d loss / d logvar
// =====================================================================================================================================
static const float BETA = 0.3f;
struct Latent { std::vector<float> mu, lv, eps, gmu, glv; };
// row B - 1 holds logvar = +20, -20, ~0 by j % 3 (the generator of test_layers)
static void gen_latent(int B, int Z, Rng& r, Latent& t)
{
    const size_t n = (size_t)B * Z;
    t.mu.resize(n); t.lv.resize(n); t.eps.resize(n); t.gmu.resize(n); t.glv.resize(n);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < Z; ++j) {
            const size_t at = (size_t)b * Z + j;
            t.mu[at] = 2.f * r.f(); t.eps[at] = 2.5f * r.f(); t.lv[at] = 2.f * r.f();
            if (b == B - 1) t.lv[at] = (j % 3 == 0 ? 20.f : j % 3 == 1 ? -20.f : 0.f) + 0.25f * r.f();
            t.gmu[at] = 3.f * r.f(); t.glv[at] = 3.f * r.f();
        }
}
// the head's gradients from dz (float64, known to e_dz) with their bounds.  ext: dmu = dz + g_mu (one rounding), dlogvar = dz eps
// e^(lv/2) / 2 + g_lv (expf to EXP_ULPS ulps, three products and a sum).  Built in: dmu = dz + beta mu / B, dlogvar = beta (e^lv - 1) /
// (2B) + dz eps e^(lv/2) / 2, judged as test_layers judges them (against the scale of the terms).
static void head_ref(bool ext, double dz, double e_dz, const Latent& t, size_t o, float beta, float inv_batch, bool bf16,
                     double* dmu, double* bmu, double* dl, double* bl)
{
    const double s = exp(0.5 * (double)t.lv[o]), e = exp((double)t.lv[o]), chain = dz * t.eps[o] * 0.5 * s;
    if (ext) {
        *dmu = dz + t.gmu[o];
        *bmu = e_dz + E24 * fabs(*dmu);
        *dl = chain + t.glv[o];
        *bl = (2 * EXP_ULPS + 6) * E24 * (fabs(chain) + fabs((double)t.glv[o])) + e_dz * fabs((double)t.eps[o]) * 0.5 * s;
    } else {
        const double bi = (double)beta * (double)inv_batch;
        *dmu = dz + bi * t.mu[o];
        *bmu = e_dz + 3 * E24 * fabs(bi * t.mu[o]) + E24 * fabs(*dmu);
        *dl = 0.5 * bi * (e - 1.0) + chain;
        *bl = (2 * EXP_ULPS + 6) * E24 * (0.5 * bi * (e + 1.0) + fabs(chain)) + e_dz * fabs((double)t.eps[o]) * 0.5 * s;
    }
    if (bf16) { *bmu += half_ulp_bf16(*dmu); *bl += half_ulp_bf16(*dl); }
}
// --host: the external form against central differences (long double, h = 1e-4) of f(mu, lv) = dz (mu + eps e^(lv/2)) + g_mu mu + g_lv lv
static void host_check_ext(double dz, const Latent& t, size_t o, Line& L)
{
    double dmu, bmu, dl, bl;
    head_ref(true, dz, 0, t, o, 0.f, 0.f, false, &dmu, &bmu, &dl, &bl);
    const long double h = 1e-4L, eps = t.eps[o], m0 = t.mu[o], l0 = t.lv[o];
    auto f = [&](long double m, long double l) { return (long double)dz * (m + eps * expl(0.5L * l)) + (long double)t.gmu[o] * m + (long double)t.glv[o] * l; };
    const long double gm = (f(m0 + h, l0) - f(m0 - h, l0)) / (2 * h), gl = (f(m0, l0 + h) - f(m0, l0 - h)) / (2 * h);
    const long double scale = fabsl((long double)dz) * (1.0L + fabsl(eps) * expl(0.5L * l0)) + fabsl((long double)t.gmu[o]) + fabsl((long double)t.glv[o]);
    if (!(fabsl(gm - dmu) <= 1e-7L * scale + 1e-12L)) host_fail(L, "dmu %.12g, central difference %.12g", dmu, (double)gm);
    if (!(fabsl(gl - dl) <= 1e-7L * scale + 1e-12L)) host_fail(L, "dlogvar %.12g, central difference %.12g", dl, (double)gl);
}

// ---- k_vae_bwd: dz = the float32 sum of `splits` slabs, in slab order (exact to the bit on the host) -----------------------------
static const int PBp = 32;
static float slab_sum(const std::vector<float>& C, int splits, long stride, size_t at)
{
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += C[(size_t)k * stride + at];
    return s;
}

template <typename T> static double elem_of(const std::vector<T>& v, size_t at);
template <> double elem_of<float>(const std::vector<float>& v, size_t at) { return v[at]; }
template <> double elem_of<uint16_t>(const std::vector<uint16_t>& v, size_t at) { return bd(v[at]); }
template <typename T> static uint32_t bits_at(const std::vector<T>& v, size_t at);
template <> uint32_t bits_at<float>(const std::vector<float>& v, size_t at) { return f_bits(v[at]); }
template <> uint32_t bits_at<uint16_t>(const std::vector<uint16_t>& v, size_t at) { return v[at]; }

template <typename T>
static void vae_bwd_case(int splits, int Z, int B, uint32_t seed)
{
    const bool bf16 = sizeof(T) == 2;
    Rng r = {seed};
    const int Np = (2 * Z + 63) / 64 * 64, ldc = Z + 3;
    const long stride = (long)PBp * ldc + 64;
    const float inv_batch = 1.f / B;
    std::vector<float> C((size_t)splits * stride);
    for (int s = 0; s < splits; ++s)
        for (long k = 0; k < stride; ++k) {
            const int b = (int)(k / ldc), j = (int)(k % ldc);
            C[(size_t)s * stride + k] = (b < B && j < Z) ? (1.5f / splits) * r.f() : r.junk();
        }
    Latent t;
    gen_latent(B, Z, r, t);
    char name[160];
    snprintf(name, sizeof name, "B k_vae_bwd<%s> splits=%d B=%d Z=%d Np=%d", bf16 ? "bf16" : "f32", splits, B, Z, Np);
    Line L;
    if (g_host) {
        for (int b = 0; b < B; ++b) for (int j = 0; j < Z; ++j) host_check_ext(slab_sum(C, splits, stride, (size_t)b * ldc + j), t, (size_t)b * Z + j, L);
        for (int b = 0; b < PBp; ++b) for (int j = 0; j < ldc; ++j) if ((b >= B || j >= Z) && !is_junk(C[(size_t)b * ldc + j])) host_fail(L, "no junk in the masked part of dz (row %g)", b);
        report(name, L);
        return;
    }
    RtxVaeBwdArgs a = {};
    a.C = to_dev(C); a.splits = splits; a.slab_stride = stride; a.ldc = ldc;
    a.B = B; a.Bp = PBp; a.Z = Z; a.Np = Np;
    a.mu32 = to_dev(t.mu); a.lv32 = to_dev(t.lv); a.eps32 = to_dev(t.eps);
    a.training = 1; a.beta = BETA; a.inv_batch = inv_batch;
    const size_t n_out = (size_t)PBp * Np;
    a.D = dev_out<T>(n_out);
    const float *dgm = to_dev(t.gmu), *dgl = to_dev(t.glv);
    const std::vector<float> zeros((size_t)B * Z, 0.f);
    const float* dzero = to_dev(zeros);
    std::vector<T> null_beta0, zero_ext;
    // four launches: null pointers (the built-in terms, beta = BETA), the external gradients, and the pair that ties the two paths
    // together: null pointers at beta = 0 against all-zero external gradients -- the same values (-0 == +0)
    for (int mode = 0; mode < 4; ++mode) {
        g_tag = mode == 0 ? "(null)" : mode == 1 ? "(ext)" : mode == 2 ? "(null, beta 0)" : "(ext zeros)";
        const bool ext = mode == 1 || mode == 3;
        a.g_mu = mode == 1 ? dgm : mode == 3 ? dzero : nullptr;
        a.g_lv = mode == 1 ? dgl : mode == 3 ? dzero : nullptr;
        a.beta = mode == 2 ? 0.f : BETA;
        repoison((T*)a.D, n_out);
        RT(rtx_launch_vae_bwd(a, bf16, 0));
        CK(hipDeviceSynchronize());
        const std::vector<T> D = fetch<T>(a.D, n_out, L, "D");
        if (mode == 2) null_beta0 = D;
        if (mode == 3) zero_ext = D;
        for (int b = 0; b < PBp; ++b)
            for (int n = 0; n < Np; ++n) {
                const size_t at = (size_t)b * Np + n;
                if (b >= B || n >= 2 * Z) { judge_bits(bits_at<T>(D, at), 0, L, "pad D", b, n); continue; }
                if (mode >= 2) continue;
                const int j = n < Z ? n : n - Z;
                const size_t o = (size_t)b * Z + j;
                const float dzf = slab_sum(C, splits, stride, (size_t)b * ldc + j);
                double dmu, bmu, dl, bl;
                head_ref(ext, dzf, 0, t, o, BETA, inv_batch, bf16, &dmu, &bmu, &dl, &bl);
                if (n < Z && ext && !bf16) judge_bits(bits_at<T>(D, at), f_bits(dzf + t.gmu[o]), L, "dmu", b, j);     // one rounding of exact inputs
                else if (n < Z) judge(elem_of<T>(D, at), dmu, bmu, L, "dmu", b, j);
                else judge(elem_of<T>(D, at), dl, bl, L, "dlogvar", b, j);
            }
    }
    g_tag = "(null, beta 0) vs (ext zeros)";
    for (size_t at = 0; at < n_out; ++at)
        if (!(elem_of<T>(null_beta0, at) == elem_of<T>(zero_ext, at))) {
            if (L.bad < 4) printf("    %s D[%zu]: %.9g against %.9g\n", g_tag.c_str(), at, elem_of<T>(null_beta0, at), elem_of<T>(zero_ext, at));
            ++L.bad;
        }
    g_tag.clear();
    report(name, L);
    free_all();
}

// ---- k_bwd_head: dz = D x W^T on MFMA from bf16 operands, float64 on the host with the bound of any order of float32 additions ------
static const int SBp = 64;
static void bwd_head_case(int K, int kw, int Z, int B, uint32_t seed)
{
    Rng r = {seed};
    const int in = K - 2, Np = (2 * Z + 31) / 32 * 32, wt_rows = r16(Z);
    const float inv_batch = 1.f / B;
    std::vector<uint16_t> X((size_t)SBp * K), W((size_t)wt_rows * K);
    for (int b = 0; b < SBp; ++b)
        for (int k = 0; k < K; ++k) X[(size_t)b * K + k] = b >= B ? f32_to_bf16(r.junk()) : k < in ? f32_to_bf16(r.f()) : 0;
    for (int n = 0; n < wt_rows; ++n)
        for (int k = 0; k < K; ++k) W[(size_t)n * K + k] = n >= Z ? f32_to_bf16(r.junk()) : k < in ? f32_to_bf16(2.f / sqrtf((float)in) * r.f()) : 0;
    std::vector<double> P((size_t)B * Z), S((size_t)B * Z);
    for (int b = 0; b < B; ++b)
        for (int n = 0; n < Z; ++n) {
            double s = 0, ab = 0;
            for (int k = 0; k < K; ++k) { const double q = bd(X[(size_t)b * K + k]) * bd(W[(size_t)n * K + k]); s += q; ab += fabs(q); }
            P[(size_t)b * Z + n] = s; S[(size_t)b * Z + n] = ab;
        }
    Latent t;
    gen_latent(B, Z, r, t);
    char name[160];
    snprintf(name, sizeof name, "B k_bwd_head K=%d kw=%d B=%d Z=%d Np=%d wt_rows=%d", K, kw, B, Z, Np, wt_rows);
    Line L;
    if (g_host) {
        for (size_t o = 0; o < (size_t)B * Z; ++o) host_check_ext(P[o], t, o, L);
        for (int b = 0; b < B; b += 5)       // the product against long double, k descending
            for (int n = 0; n < Z; ++n) {
                long double s = 0;
                for (int k = K - 1; k >= 0; --k) s += (long double)bd(X[(size_t)b * K + k]) * (long double)bd(W[(size_t)n * K + k]);
                if (!(fabsl(s - (long double)P[(size_t)b * Z + n]) <= 1e-12L * S[(size_t)b * Z + n] + 1e-300L)) host_fail(L, "product: float64 %.17g, long double %.17g", P[(size_t)b * Z + n], (double)s);
            }
        report(name, L);
        return;
    }
    rtx_small_set_waves(1);
    rtx_small_set_kw(kw);
    RtxSmallBwdArgs a = {};
    a.D = to_dev(X); a.WT = to_dev(W); a.ld = K; a.wt_rows = wt_rows;
    a.B = B; a.Bp = SBp; a.Np = Np; a.Z = Z; a.training = 1;
    a.mu32 = to_dev(t.mu); a.lv32 = to_dev(t.lv); a.eps32 = to_dev(t.eps);
    a.inv_batch = inv_batch;
    const size_t n_out = (size_t)SBp * Np;
    a.Dout = dev_out<uint16_t>(n_out);
    const float *dgm = to_dev(t.gmu), *dgl = to_dev(t.glv);
    const std::vector<float> zeros((size_t)B * Z, 0.f);
    const float* dzero = to_dev(zeros);
    std::vector<uint16_t> null_beta0, zero_ext;
    for (int mode = 0; mode < 4; ++mode) {
        g_tag = mode == 0 ? "(null)" : mode == 1 ? "(ext)" : mode == 2 ? "(null, beta 0)" : "(ext zeros)";
        const bool ext = mode == 1 || mode == 3;
        a.g_mu = mode == 1 ? dgm : mode == 3 ? dzero : nullptr;
        a.g_lv = mode == 1 ? dgl : mode == 3 ? dzero : nullptr;
        a.beta = mode == 2 ? 0.f : BETA;
        repoison(a.Dout, n_out);
        RT(rtx_launch_small_bwd(a, 0));
        CK(hipDeviceSynchronize());
        const std::vector<uint16_t> D = fetch<uint16_t>(a.Dout, n_out, L, "Dout");
        if (mode == 2) null_beta0 = D;
        if (mode == 3) zero_ext = D;
        for (int b = 0; b < SBp; ++b)
            for (int n = 0; n < Np; ++n) {
                const size_t at = (size_t)b * Np + n;
                if (b >= B || n >= 2 * Z) { judge_bits(D[at], 0, L, "pad Dout", b, n); continue; }
                if (mode >= 2) continue;
                const int j = n < Z ? n : n - Z;
                const size_t o = (size_t)b * Z + j;
                double dmu, bmu, dl, bl;
                head_ref(ext, P[o], (in + 2) * E24 * S[o], t, o, BETA, inv_batch, true, &dmu, &bmu, &dl, &bl);
                if (n < Z) judge(bd(D[at]), dmu, bmu, L, "dmu", b, j);
                else judge(bd(D[at]), dl, bl, L, "dlogvar", b, j);
            }
    }
    g_tag = "(null, beta 0) vs (ext zeros)";
    for (size_t at = 0; at < n_out; ++at)
        if (!(bd(null_beta0[at]) == bd(zero_ext[at]))) {
            if (L.bad < 4) printf("    %s Dout[%zu]: %.9g against %.9g\n", g_tag.c_str(), at, bd(null_beta0[at]), bd(zero_ext[at]));
            ++L.bad;
        }
    g_tag.clear();
    rtx_small_set_kw(1);
    report(name, L);
    free_all();
}

static void head_cases()
{
    uint32_t seed = 500;
    for (int Z : {1, 16, 200})
        for (int B : {1, 17}) {
            for (int splits : {1, 3}) {
                vae_bwd_case<float>(splits, Z, B, ++seed);
                vae_bwd_case<uint16_t>(splits, Z, B, ++seed);
            }
            for (int K : {128, 1024})
                for (int kw : {1, 2, 4}) bwd_head_case(K, kw, Z, B, ++seed);
        }
}

// --host: the launcher refuses what the kernel cannot take, before the first HIP call
static void refusal_cases()
{
    Line L;
    float x = 0.f;
    RtxDlogitsArgs a = {};
    a.loss.B = 4; a.loss.I = 9; a.Bp = 16; a.ldd = 16; a.D = (void*)16;
    auto refuse = [&](const char* what, int rc) { if (rc != RTX_EINVAL) host_fail(L, what); };
    refuse("import_dout: a row stride below n_items", rtx_launch_import_dout(a, &x, 8, 0, 0, 0));
    refuse("import_dout: a NULL gradient", rtx_launch_import_dout(a, nullptr, 9, 0, 0, 0));
    refuse("import_dout: the sigmoid form without logits", rtx_launch_import_dout(a, &x, 9, 1, 0, 0));
    a.ldd = 12;
    refuse("import_dout: ldd % 8 != 0", rtx_launch_import_dout(a, &x, 9, 0, 0, 0));
    RtxVaeBwdArgs v = {};
    v.Z = 4; v.B = 4; v.Np = 64; v.Bp = 16; v.ldc = 4; v.g_mu = &x;
    refuse("vae_bwd: d_mu without d_logvar", rtx_launch_vae_bwd(v, 0, 0));
    RtxSmallBwdArgs s = {};
    s.ld = 128; s.Bp = 64; s.Np = 32; s.Dout = (bf16_t*)16; s.B = 4; s.Z = 4; s.wt_rows = 16; s.g_lv = &x;
    refuse("small_bwd: d_logvar without d_mu", rtx_launch_small_bwd(s, 0));
    report("launchers refuse bad arguments before the first HIP call", L);
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    import_cases();
    head_cases();
    if (g_host) refusal_cases();
    return finish("EXTGRAD");
}
