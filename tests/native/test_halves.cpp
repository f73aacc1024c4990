// test_halves -- the kernels of the cut between the encoder and the decoder half (rtx_engine_encode_train / encode_backward /
// decode_train / decode_backward, rtx_reparam) against float64, element by element:
//   A  post_layers.hip rtx_launch_export_dz: d z = the sum of 1 and 3 split-K slabs, in slab order, into an unpadded tensor
//   B  post_layers.hip rtx_launch_import_dh: D = d h (1 - h^2) from an unpadded tensor, both output types, with and without tanh
//   C  post_layers.hip rtx_launch_reparam / rtx_launch_reparam_grad: injected and Philox draws
//   D  post_layers.hip k_vae_bwd with external gradients and NO slab (the head backward of rtx_engine_encode_backward): [g_mu | g_lv]
// Every output is poisoned before the launch and carries a poisoned guard; padding rows and columns are checked bit for bit.  The
// unpadded sources are followed by junk (|x| >= 500): a read at a clamped row or column would show as a wrong or non-zero element.
//   test_halves          the kernels on the device
//   test_halves --host   no HIP call: the case generators and the float64 references against a second formulation
// Bounds.  A: the float32 sum of the slabs in slab order is reproduced on the host: bit for bit; against float64: (splits - 1) roundings
// of the partial sums.  B: without tanh one rounding of exact inputs (f32: bit for bit); with it o o, 1 - o o and the product, three
// roundings of |d h| (1 + o^2) at most -- 4 x 2^-24 |d h|.  bf16 outputs add half a bf16 unit.  C: z as tests/native/test_layers.cpp
// bounds the head's (expf to 3 ulps, a product, a sum); d mu = d z bit for bit; d logvar: expf and three products.  Philox draws: the
// tolerance of tests/test_philox_draws.py against the host build of rtx_normal.  D: 0 + g in float32, bit for bit (bf16: its rounding).
#include "../../rectorch_amd/csrc/rtx_kernels.h"

#include "check.h"

static const double EXP_ULPS = 3;      // device expf, as tests/native/test_layers.cpp assumes it
static const double PHILOX_TOL = 8 * 5.76e-6, PHILOX_TOL_EXACT = 8 * 1.52e-7;     // tests/test_philox_draws.py, cited
static const uint64_t SEED = 0x9E3779B97F4A7C15ull, OFFSET = (1ull << 33) + 5;     // bits above 32 set
static double bd(uint16_t h) { return (double)bf16_to_f32(h); }
static double half_ulp_bf16(double x)
{
    if (x == 0) return 0;
    int e;
    frexp(fabs(x), &e);
    return ldexp(1.0, e - 9);
}
template <typename T> static double elem_of(const std::vector<T>& v, size_t at);
template <> double elem_of<float>(const std::vector<float>& v, size_t at) { return v[at]; }
template <> double elem_of<uint16_t>(const std::vector<uint16_t>& v, size_t at) { return bd(v[at]); }
template <typename T> static uint32_t bits_at(const std::vector<T>& v, size_t at);
template <> uint32_t bits_at<float>(const std::vector<float>& v, size_t at) { return f_bits(v[at]); }
template <> uint32_t bits_at<uint16_t>(const std::vector<uint16_t>& v, size_t at) { return v[at]; }
template <typename T> static uint32_t bits_of(float f);
template <> uint32_t bits_of<float>(float f) { return f_bits(f); }
template <> uint32_t bits_of<uint16_t>(float f) { return f32_to_bf16(f); }

// =====================================================================================================================================
// A: the d z export
// =====================================================================================================================================
static void export_case(int splits, int n, int Z, int Bp, int ldc, uint32_t seed)
{
    Rng r = {seed};
    const long stride = (long)Bp * ldc + 32;
    std::vector<float> C((size_t)splits * stride);
    for (int s = 0; s < splits; ++s)
        for (long k = 0; k < stride; ++k) {
            const long b = k / ldc, j = k % ldc;
            C[(size_t)s * stride + k] = (b < n && j < Z) ? 1.5f * r.f() : r.junk();
        }
    char name[160];
    snprintf(name, sizeof name, "A export_dz splits=%d n=%d Z=%d Bp=%d ldc=%d", splits, n, Z, Bp, ldc);
    Line L;
    std::vector<float> want((size_t)n * Z);
    std::vector<double> want64((size_t)n * Z), mag((size_t)n * Z);
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < Z; ++j) {
            float s32 = 0.f;
            double s64 = 0, ab = 0;
            for (int s = 0; s < splits; ++s) { const float c = C[(size_t)s * stride + (size_t)b * ldc + j]; s32 += c; s64 += c; ab += fabs((double)c); }
            want[(size_t)b * Z + j] = s32; want64[(size_t)b * Z + j] = s64; mag[(size_t)b * Z + j] = ab;
        }
    if (g_host) {
        for (int b = 0; b < n; ++b)
            for (int j = 0; j < Z; ++j) {       // second formulation: long double, slabs descending
                long double s = 0;
                for (int k = splits - 1; k >= 0; --k) s += (long double)C[(size_t)k * stride + (size_t)b * ldc + j];
                const size_t o = (size_t)b * Z + j;
                if (!(fabsl(s - (long double)want64[o]) <= 1e-15L * mag[o])) host_fail(L, "slab sum: float64 %.17g, long double %.17g", want64[o], (double)s);
                if (!(fabs((double)want[o] - want64[o]) <= (splits - 1) * E24 * mag[o])) host_fail(L, "float32 slab sum %.9g away from float64 %.17g", want[o], want64[o]);
            }
        for (long k = 0; k < (long)Bp * ldc; ++k)
            if ((k / ldc >= n || k % ldc >= Z) && !is_junk(C[k])) host_fail(L, "no junk in the masked part of the slabs (row %g)", (double)(k / ldc));
        report(name, L);
        return;
    }
    const size_t n_out = (size_t)n * Z;
    float* dz = dev_out<float>(n_out);
    RT(rtx_launch_export_dz(to_dev(C), splits, stride, ldc, n, Z, dz, 0));
    CK(hipDeviceSynchronize());
    const std::vector<float> got = fetch<float>(dz, n_out, L, "d_z");
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < Z; ++j) {
            const size_t o = (size_t)b * Z + j;
            judge_bits(f_bits(got[o]), f_bits(want[o]), L, "d_z (slab order)", b, j);
            judge(got[o], want64[o], (splits - 1) * E24 * mag[o], L, "d_z", b, j);
        }
    report(name, L);
    free_all();
}

// =====================================================================================================================================
// B: the d h import
// =====================================================================================================================================
template <typename T>
static void import_case(int B, int N, int Bp, int Np, int tanh_act, uint32_t seed)
{
    const bool bf16 = sizeof(T) == 2;
    Rng r = {seed};
    const size_t n_src = (size_t)B * N;
    std::vector<float> dh(n_src + 4096), O((size_t)Bp * Np);
    for (size_t k = 0; k < dh.size(); ++k) dh[k] = k < n_src ? 2.f * r.f() : r.junk();     // junk behind the unpadded tensor
    for (int b = 0; b < Bp; ++b)
        for (int n = 0; n < Np; ++n) O[(size_t)b * Np + n] = (b < B && n < N) ? 0.999f * r.f() : r.junk();
    char name[160];
    snprintf(name, sizeof name, "B import_dh<%s> tanh=%d B=%d N=%d Bp=%d Np=%d", bf16 ? "bf16" : "f32", tanh_act, B, N, Bp, Np);
    Line L;
    if (g_host) {
        for (int b = 0; b < B; ++b)
            for (int n = 0; n < N; ++n) {
                // second formulation: central difference of f(a) = d h tanh(a) at a = atanh(o), in long double
                const long double o = O[(size_t)b * Np + n], g = dh[(size_t)b * N + n], a = atanhl(o), h = 1e-5L;
                const long double fd = g * (tanhl(a + h) - tanhl(a - h)) / (2 * h), d = g * (1.0L - o * o);
                if (tanh_act && !(fabsl(fd - d) <= 1e-8L * fabsl(g) + 1e-12L)) host_fail(L, "d h (1 - o^2) = %.12g, central difference %.12g", (double)d, (double)fd);
                if (!(fabsl(o) < 1.0L && fabsl(g) <= 2.0L)) host_fail(L, "operand outside the generator's range (o %g, d h %g)", (double)o, (double)g);
            }
        for (size_t k = n_src; k < dh.size(); ++k) if (!is_junk(dh[k])) host_fail(L, "no junk behind the unpadded source (element %g)", (double)k);
        report(name, L);
        return;
    }
    const size_t n_out = (size_t)Bp * Np;
    T* D = dev_out<T>(n_out);
    RT(rtx_launch_import_dh(to_dev(dh), B, N, Bp, Np, tanh_act, to_dev(O), D, bf16, 0));
    CK(hipDeviceSynchronize());
    const std::vector<T> got = fetch<T>(D, n_out, L, "D");
    for (int b = 0; b < Bp; ++b)
        for (int n = 0; n < Np; ++n) {
            const size_t at = (size_t)b * Np + n;
            if (b >= B || n >= N) { judge_bits(bits_at<T>(got, at), 0, L, "pad D", b, n); continue; }
            const double g = dh[(size_t)b * N + n], o = O[at];
            if (!tanh_act) { judge_bits(bits_at<T>(got, at), bits_of<T>(dh[(size_t)b * N + n]), L, "D", b, n); continue; }
            const double d = g * (1.0 - o * o);
            judge(elem_of<T>(got, at), d, 4 * E24 * fabs(g) + (bf16 ? half_ulp_bf16(d) + E24 * fabs(d) : 0.0), L, "D", b, n);
        }
    report(name, L);
    free_all();
}

// =====================================================================================================================================
// C: the sampling step and its derivative
// =====================================================================================================================================
struct Latent { std::vector<float> mu, lv, eps, dz; };
// row n - 1 holds logvar = +20, -20, ~0 by j % 3 (the generator of test_layers)
static void gen_latent(int n, int Z, Rng& r, Latent& t)
{
    const size_t c = (size_t)n * Z;
    t.mu.resize(c); t.lv.resize(c); t.eps.resize(c); t.dz.resize(c);
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < Z; ++j) {
            const size_t at = (size_t)b * Z + j;
            t.mu[at] = 2.f * r.f(); t.eps[at] = 2.5f * r.f(); t.lv[at] = 2.f * r.f();
            if (b == n - 1) t.lv[at] = (j % 3 == 0 ? 20.f : j % 3 == 1 ? -20.f : 0.f) + 0.25f * r.f();
            t.dz[at] = 3.f * r.f();
        }
}

static void reparam_case(int n, int Z, bool philox, uint32_t seed)
{
    Rng r = {seed};
    Latent t;
    gen_latent(n, Z, r, t);
    const size_t c = (size_t)n * Z;
    char name[160];
    snprintf(name, sizeof name, "C reparam + reparam_grad n=%d Z=%d %s", n, Z, philox ? "Philox" : "injected");
    Line L;
    if (g_host) {
        for (size_t o = 0; o < c; ++o) {
            // second formulation: central differences (long double) of f(mu, lv) = d z (mu + eps e^(lv / 2))
            const long double h = 1e-4L, e = t.eps[o], m0 = t.mu[o], l0 = t.lv[o], dz = t.dz[o];
            auto f = [&](long double m, long double l) { return dz * (m + e * expl(0.5L * l)); };
            const long double gm = (f(m0 + h, l0) - f(m0 - h, l0)) / (2 * h), gl = (f(m0, l0 + h) - f(m0, l0 - h)) / (2 * h);
            const double dl = (double)t.dz[o] * t.eps[o] * 0.5 * exp(0.5 * (double)t.lv[o]);
            const long double scale = fabsl(dz) * (1.0L + fabsl(e) * expl(0.5L * l0));
            if (!(fabsl(gm - dz) <= 1e-7L * scale + 1e-12L)) host_fail(L, "d mu %.12g, central difference %.12g", (double)dz, (double)gm);
            if (!(fabsl(gl - dl) <= 1e-7L * scale + 1e-12L)) host_fail(L, "d logvar %.12g, central difference %.12g", dl, (double)gl);
        }
        report(name, L);
        return;
    }
    float *z = dev_out<float>(c), *eo = dev_out<float>(c), *dmu = dev_out<float>(c), *dlv = dev_out<float>(c);
    const float *dm = to_dev(t.mu), *dl = to_dev(t.lv);
    RT(rtx_launch_reparam(dm, dl, n, Z, philox ? nullptr : to_dev(t.eps), SEED, OFFSET, z, eo, 0));
    RT(rtx_launch_reparam_grad(to_dev(t.dz), dl, eo, n, Z, dmu, dlv, 0));
    CK(hipDeviceSynchronize());
    const std::vector<float> Zs = fetch<float>(z, c, L, "z"), E = fetch<float>(eo, c, L, "eps_out"), GM = fetch<float>(dmu, c, L, "d_mu"),
                             GL = fetch<float>(dlv, c, L, "d_logvar");
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < Z; ++j) {
            const size_t o = (size_t)b * Z + j;
            if (!philox) judge_bits(f_bits(E[o]), f_bits(t.eps[o]), L, "eps_out (injected)", b, j);
            else {
                const double ref = rtx_normal(SEED, OFFSET, (uint64_t)b * Z + j);
                const bool exact = (philox4x32_10(SEED, OFFSET ^ 0x5851F42D4C957F2DULL, (uint64_t)b * Z + j).x >> 8) < (1u << 23);
                judge(E[o], ref, (exact ? PHILOX_TOL_EXACT : PHILOX_TOL) * std::max(1.0, fabs(ref)), L, "eps_out (Philox)", b, j);
            }
            // from the DEVICE's draw: isolates the arithmetic
            const double s = exp(0.5 * (double)t.lv[o]), es = (double)E[o] * s, zz = (double)t.mu[o] + es;
            judge(Zs[o], zz, 2 * (EXP_ULPS + 1) * E24 * fabs(es) + E24 * fabs(zz), L, "z", b, j);
            judge_bits(f_bits(GM[o]), f_bits(t.dz[o]), L, "d_mu", b, j);
            const double g = (double)t.dz[o] * E[o] * 0.5 * s;
            judge(GL[o], g, (2 * EXP_ULPS + 6) * E24 * fabs(g), L, "d_logvar", b, j);
        }
    report(name, L);
    free_all();
}

// =====================================================================================================================================
// D: k_vae_bwd with external gradients and no slab
// =====================================================================================================================================
template <typename T>
static void head_noslab_case(int B, int Z, int Bp, uint32_t seed)
{
    const bool bf16 = sizeof(T) == 2;
    Rng r = {seed};
    Latent t;
    gen_latent(B, Z, r, t);
    const int Np = (2 * Z + 63) / 64 * 64, ldc = Np;
    std::vector<float> gmu((size_t)B * Z + 1024), glv((size_t)B * Z + 1024), junk((size_t)Bp * ldc);
    for (size_t k = 0; k < gmu.size(); ++k) { gmu[k] = k < (size_t)B * Z ? 3.f * r.f() : r.junk(); glv[k] = k < (size_t)B * Z ? 3.f * r.f() : r.junk(); }
    for (float& x : junk) x = r.junk();      // the scratch a slab would be in: nothing of it may be read
    if (B * Z >= 2) gmu[1] = -0.f;
    char name[160];
    snprintf(name, sizeof name, "D k_vae_bwd<%s> no slab, external gradients B=%d Z=%d Bp=%d Np=%d", bf16 ? "bf16" : "f32", B, Z, Bp, Np);
    Line L;
    if (g_host) {
        for (size_t k = (size_t)B * Z; k < gmu.size(); ++k) if (!is_junk(gmu[k]) || !is_junk(glv[k])) host_fail(L, "no junk behind the unpadded gradients (element %g)", (double)k);
        for (size_t k = 0; k < (size_t)B * Z; ++k) if (!(fabs(gmu[k]) <= 3.0 && fabs(glv[k]) <= 3.0)) host_fail(L, "gradient outside [-3, 3] (element %g)", (double)k);
        report(name, L);
        return;
    }
    RtxVaeBwdArgs a = {};
    a.C = to_dev(junk); a.splits = 0; a.slab_stride = 0; a.ldc = ldc;
    a.B = B; a.Bp = Bp; a.Z = Z; a.Np = Np;
    a.mu32 = to_dev(t.mu); a.lv32 = to_dev(t.lv); a.eps32 = to_dev(t.eps);
    a.training = 0; a.beta = 0.7f; a.inv_batch = 1.f / B;      // (beta and inv_batch are not read with external gradients)
    a.g_mu = to_dev(gmu); a.g_lv = to_dev(glv);
    const size_t n_out = (size_t)Bp * Np;
    a.D = dev_out<T>(n_out);
    RT(rtx_launch_vae_bwd(a, bf16, 0));
    CK(hipDeviceSynchronize());
    const std::vector<T> D = fetch<T>(a.D, n_out, L, "D");
    for (int b = 0; b < Bp; ++b)
        for (int n = 0; n < Np; ++n) {
            const size_t at = (size_t)b * Np + n;
            if (b >= B || n >= 2 * Z) { judge_bits(bits_at<T>(D, at), 0, L, "pad D", b, n); continue; }
            const size_t o = (size_t)b * Z + (n < Z ? n : n - Z);
            if (n < Z) judge_bits(bits_at<T>(D, at), bits_of<T>(0.f + gmu[o]), L, "d mu", b, n);      // an empty slab sum is +0
            else judge_bits(bits_at<T>(D, at), bits_of<T>(glv[o]), L, "d logvar", b, n - Z);
        }
    report(name, L);
    free_all();
}

// --host: the launchers refuse what the kernels cannot take, before the first HIP call
static void refusal_cases()
{
    Line L;
    float x = 0.f;
    auto refuse = [&](const char* what, int rc) { if (rc != RTX_EINVAL) host_fail(L, what); };
    refuse("export_dz: ldc below Z", rtx_launch_export_dz(&x, 1, 0, 4, 2, 5, &x, 0));
    refuse("export_dz: overlapping slabs", rtx_launch_export_dz(&x, 2, 8, 8, 2, 5, &x, 0));
    refuse("export_dz: no slab", rtx_launch_export_dz(&x, 0, 64, 8, 2, 5, &x, 0));
    refuse("import_dh: B above Bp", rtx_launch_import_dh(&x, 17, 5, 16, 64, 0, nullptr, &x, 0, 0));
    refuse("import_dh: N above Np", rtx_launch_import_dh(&x, 4, 65, 16, 64, 0, nullptr, &x, 0, 0));
    refuse("import_dh: tanh without the activation", rtx_launch_import_dh(&x, 4, 5, 16, 64, 1, nullptr, &x, 0, 0));
    refuse("reparam: a NULL output", rtx_launch_reparam(&x, &x, 1, 1, nullptr, 0, 0, nullptr, nullptr, 0));
    refuse("reparam_grad: d_logvar without eps", rtx_launch_reparam_grad(&x, &x, nullptr, 1, 1, &x, &x, 0));
    report("launchers refuse bad arguments before the first HIP call", L);
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    uint32_t seed = 900;
    // (n, Z, Bp, ldc): B = 1, G2c's ragged shapes, the wide shape (latent 64 -> Zp = 128), 3 B rows, more than one block
    static const int EX[5][4] = {{1, 1, 128, 128}, {7, 5, 128, 128}, {37, 64, 128, 128}, {111, 64, 128, 128}, {21, 200, 128, 256}};
    for (int splits : {1, 3})
        for (const auto& s : EX) export_case(splits, s[0], s[1], s[2], s[3], ++seed);
    // (B, N, Bp, Np)
    static const int IM[4][4] = {{1, 5, 128, 128}, {7, 5, 128, 128}, {37, 64, 128, 128}, {130, 200, 256, 256}};
    for (int tanh_act = 0; tanh_act < 2; ++tanh_act)
        for (const auto& s : IM) {
            import_case<float>(s[0], s[1], s[2], s[3], tanh_act, ++seed);
            import_case<uint16_t>(s[0], s[1], s[2], s[3], tanh_act, ++seed);
        }
    for (int philox = 0; philox < 2; ++philox)
        for (const auto& s : EX) reparam_case(s[0], s[1], philox != 0, ++seed);
    for (const auto& s : IM) {
        head_noslab_case<float>(s[0], s[1], s[2], ++seed);
        head_noslab_case<uint16_t>(s[0], s[1], s[2], ++seed);
    }
    if (g_host) refusal_cases();
    return finish("HALVES");
}
