// test_loss_grad -- the dense loss-and-gradient launchers of loss.hip (the kernels behind rtx_*_loss_grad) against float64, element by
// element:
//   M  rtx_launch_dense_loss_grad     multinomial likelihood (+ beta KL): row loss, d / d logits, d / d mu, d / d logvar
//   P  rtx_launch_dense_bce_kl_grad   binary cross-entropy on probabilities + KL
//   S  rtx_launch_dense_mse_grad      mean squared error
//   N  rtx_launch_sumsq_ordered + rtx_launch_norm_grad   d sum_t ||W_t||_2 / d W_t
// Every output is poisoned before the launch and carries a poisoned guard behind its end (and in front of its start where the base is
// offset).  Every row loss is also compared BIT FOR BIT with the launcher of the same loss without gradients (the value of a
// differentiable call is the value of the plain one), and a second launch on the same data must reproduce every output bit for bit.
//   test_loss_grad          the kernels on the device
//   test_loss_grad --host   no HIP call: the case generator's conditions, and the float64 gradients against a second formulation --
//                           central differences (long double) of the float64 loss
// Shapes: I in {1, 7, 255, 256, 257, 1000, 4099} x B in {1, 3, 64} x base aligned / offset by one float (the 16-byte route runs where
// the base is aligned and I % 4 == 0: 256 and 1000; everywhere else the 4-byte one) x Z in {none, 1, 5, 200} x beta in {0, 0.3}.
// Bounds: those tests/native/test_loss.cpp holds the d-logits kernels of the same losses to -- a row loss to SUM_TOL of the sum of
// the absolute values of its terms; the multinomial gradient to 2e-5 (s p + t) / B, plus s 2^-126 / B: test_loss's logits spread over
// 60, these over 160, where a softmax share (exp(-160) = 3e-70) lies under float32's smallest normal number and no float32 result can
// be within 2e-5 of it; the BCE gradient to 8 (p + x) 2^-24 of its
// scale 1 / (max(p (1 - p), 1e-12) N) (p and x are exact inputs here: 1 - p, the product, p - x, the division and the product with 1 / N
// are five roundings); MSE, KL and norm gradients to 4 float32 ulps.
#include "../../rectorch_amd/csrc/rtx_kernels.h"

#include "check.h"

static const double SUM_TOL = 1e-6;    // tests/native/test_loss.cpp's
static double ulp32(double x) { return x == 0 ? 0 : ldexp(1.0, ilogb(x) - 23); }
static const float CLAMP = 1e-12f;
static const double FLT_NORMAL_MIN = 1.1754943508222875e-38;     // 2^-126

enum { MULTINOMIAL = 0, BCE = 1, MSE = 2 };
static const char* KIND[3] = {"M dense_loss_grad", "P dense_bce_kl_grad", "S dense_mse_grad"};

struct Case {
    int kind, B, I, off, Z;
    float beta;
    uint32_t seed;
};
struct Data {
    std::vector<float> A, X, mu, lv;   // A: logits / probabilities / predictions [B][I]; X: targets
    int zero_row, ext_row;             // (multinomial) the row without a target, the row with logits of +-80; -1: none
};
// what the generator promises (checked in --host mode)
struct Seen { long zero_rows = 0, p80 = 0, m80 = 0, ratings = 0, clamp[2][3] = {{0, 0, 0}, {0, 0, 0}}; };

static float target_value(Rng& r)
{
    const int q = r.below(8);
    return q == 0 ? 1.f : q == 1 ? 3.5f : q == 2 ? 0.5f : 0.f;
}

static Data generate(const Case& c)
{
    Rng r = {c.seed};
    Data d;
    const int B = c.B, I = c.I;
    d.A.resize((size_t)B * I); d.X.resize((size_t)B * I);
    d.zero_row = B > 1 ? B - 1 : (I % 2 == 0 ? 0 : -1);
    d.ext_row = B > 1 ? 1 % B : (I % 2 == 1 ? 0 : -1);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < I; ++i) {
            const size_t at = (size_t)b * I + i;
            d.X[at] = target_value(r);
            if (c.kind == BCE) {      // probabilities, the ends of the interval included
                const int q = r.below(16);
                d.A[at] = q == 0 ? 0.f : q == 1 ? 1.f : 1e-4f + (1.f - 2e-4f) * r.u01();
                const int t = r.below(4);
                d.X[at] = t == 0 ? 1.f : t == 1 ? 3.5f : 0.f;
            } else {
                d.A[at] = 3.f * r.f();
            }
        }
    if (c.kind == MULTINOMIAL) {
        if (d.zero_row >= 0) for (int i = 0; i < I; ++i) d.X[(size_t)d.zero_row * I + i] = 0.f;
        if (d.ext_row >= 0) {
            float* y = &d.A[(size_t)d.ext_row * I];
            y[0] = 80.f;
            if (I > 1) y[I - 1] = -80.f;
            if (I > 4) { y[I / 2] = 80.f; y[I / 2 + 1] = -80.f; }
            d.X[(size_t)d.ext_row * I] = 3.5f;                       // a rated item at +80 ...
            if (I > 1) d.X[(size_t)d.ext_row * I + I - 1] = 1.f;     // ... and one at -80
        }
    }
    if (c.kind == BCE && I >= 6) {     // row 0: p exactly 0 and 1 against x = 0, 1 and 3.5 -- both clamps, every pairing
        static const float ps[2] = {0.f, 1.f}, xs[3] = {0.f, 1.f, 3.5f};
        for (int k = 0; k < 6; ++k) { d.A[k] = ps[k / 3]; d.X[k] = xs[k % 3]; }
    }
    if (c.Z) {
        d.mu.resize((size_t)B * c.Z); d.lv.resize((size_t)B * c.Z);
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < c.Z; ++j) {
                const size_t at = (size_t)b * c.Z + j;
                d.mu[at] = 2.f * r.f();
                d.lv[at] = 2.f * r.f();
                if (b == B - 1) d.lv[at] = j % 4 == 0 ? 0.f : (j % 4 == 1 ? 20.f : j % 4 == 2 ? -20.f : 0.f) + 0.25f * r.f();
            }
    }
    return d;
}

// ---- float64 references ---------------------------------------------------------------------------------------------------------------
struct Ref {
    std::vector<double> row, row_abs;        // [B] the row loss and the sum of the absolute values of its terms
    std::vector<double> dA, dA_bound;        // [B][I]
    std::vector<double> dmu, dlv;            // [B][Z]
};
static double kl_row(const Data& d, int b, int Z, double* abs_sum)
{
    double s = 0, a = 0;
    for (int j = 0; j < Z; ++j) {
        const double m = d.mu[(size_t)b * Z + j], l = d.lv[(size_t)b * Z + j];
        s += 1.0 + l - m * m - exp(l);
        a += 1.0 + fabs(l) + m * m + exp(l);
    }
    *abs_sum = 0.5 * a;
    return -0.5 * s;
}
// loss of row b in long double as a function of one perturbed operand (--host: the second formulation)
static long double row_loss_ld(const Case& c, const Data& d, int b, int at_i, long double delta, double inv_batch, double inv_elems)
{
    const int I = c.I;
    const float* a = &d.A[(size_t)b * I];
    const float* x = &d.X[(size_t)b * I];
    auto A = [&](int i) { return (long double)a[i] + (i == at_i ? delta : 0.0L); };
    if (c.kind == MULTINOMIAL) {
        long double M = -INFINITY, S = 0, sx = 0, dot = 0;
        for (int i = 0; i < I; ++i) M = std::max(M, A(i));
        for (int i = 0; i < I; ++i) { S += expl(A(i) - M); sx += x[i]; dot += (long double)x[i] * A(i); }
        return (sx * (M + logl(S)) - dot) * inv_batch;
    }
    long double s = 0;
    for (int i = 0; i < I; ++i) {
        if (c.kind == BCE) {
            const long double p = A(i);
            s += ((long double)x[i] - 1.0L) * std::max(log1pl(-p), -100.0L) - (x[i] == 0.f ? 0.0L : (long double)x[i] * std::max(logl(p), -100.0L));
        } else {
            const long double e = (long double)x[i] - A(i);
            s += e * e;
        }
    }
    return s * inv_elems;
}

static Ref reference(const Case& c, const Data& d, float inv_batch_f, float inv_elems_f, Line& L, Seen& seen)
{
    const int B = c.B, I = c.I, Z = c.Z;
    const double inv_batch = inv_batch_f, inv_elems = inv_elems_f, beta = c.kind == MULTINOMIAL ? (double)c.beta : 1.0;
    Ref R;
    R.row.assign(B, 0); R.row_abs.assign(B, 0);
    R.dA.resize((size_t)B * I); R.dA_bound.resize((size_t)B * I);
    for (int b = 0; b < B; ++b) {
        const float* a = &d.A[(size_t)b * I];
        const float* x = &d.X[(size_t)b * I];
        double* dA = &R.dA[(size_t)b * I];
        double* db = &R.dA_bound[(size_t)b * I];
        if (c.kind == MULTINOMIAL) {
            double M = -INFINITY, S = 0, sx = 0, dot = 0, dabs = 0;
            for (int i = 0; i < I; ++i) M = std::max(M, (double)a[i]);
            for (int i = 0; i < I; ++i) { S += exp(a[i] - M); sx += x[i]; dot += (double)x[i] * a[i]; dabs += fabs((double)x[i] * a[i]); }
            const double lse = M + log(S);
            R.row[b] = (sx * lse - dot) * inv_batch;
            R.row_abs[b] = (fabs(sx * lse) + dabs) * inv_batch;
            for (int i = 0; i < I; ++i) {
                const double p = exp(a[i] - lse);
                dA[i] = (sx * p - x[i]) * inv_batch;
                // (FLT_NORMAL_MIN: a softmax share under 2^-126 -- at a spread of 160 it is 1e-70 -- is no normal float32, and __expf may
                // return a zero for it: the format's resolution there, not the kernel's, is the floor of the bound)
                db[i] = 2e-5 * (sx * p + x[i]) * inv_batch + FLT_NORMAL_MIN * sx * inv_batch;
                seen.p80 += a[i] == 80.f; seen.m80 += a[i] == -80.f; seen.ratings += x[i] == 3.5f;
            }
            seen.zero_rows += sx == 0;
        } else if (c.kind == BCE) {
            for (int i = 0; i < I; ++i) {
                const double p = a[i], xv = x[i];
                const double t1 = (xv - 1.0) * std::max(log1p(-p), -100.0), t2 = xv == 0 ? 0.0 : -xv * std::max(log(p), -100.0);
                R.row[b] += (t1 + t2) * inv_elems;
                R.row_abs[b] += (fabs(t1) + fabs(t2)) * inv_elems;
                const double s = std::max(p * (1.0 - p), (double)CLAMP);
                dA[i] = (p - xv) / s * inv_elems;
                db[i] = 8 * E24 * (p + xv) / s * inv_elems;
                if (p == 0 || p == 1) ++seen.clamp[p == 1][xv == 0 ? 0 : xv == 1 ? 1 : 2];
                seen.ratings += xv == 3.5;
            }
        } else {
            for (int i = 0; i < I; ++i) {
                const double e = (double)x[i] - (double)a[i];
                R.row[b] += e * e * inv_elems;
                dA[i] = 2.0 * inv_elems * ((double)a[i] - (double)x[i]);
                db[i] = 4 * ulp32(dA[i]);
                seen.ratings += x[i] == 3.5f;
            }
            R.row_abs[b] = R.row[b];
        }
        if (Z) {
            double kl_abs;
            R.row[b] += beta * kl_row(d, b, Z, &kl_abs) * inv_batch;
            R.row_abs[b] += beta * kl_abs * inv_batch;
        }
        if (g_host && (b < 2 || b == B - 1)) {     // (rows 0 and 1 and the last one: the special rows are among them)
            // central differences of the long-double loss: every column of a short row, 16 spread columns of a long one
            const int step = std::max(1, I / 16);
            for (int i = 0; i < I; i += step) {
                if (!std::isfinite(dA[i])) host_fail(L, "the reference gradient is not finite (row %g, column %g)", b, i);
                long double h = 1e-4L;
                double tol = 1e-6;
                if (c.kind == BCE) {
                    const double p = a[i];
                    if (p == 0 || p == 1) {     // on the clamps the gradient is autograd's formula, not a derivative: (p - x) / 1e-12 / N
                        const double want = (p - x[i]) / (double)CLAMP * inv_elems;
                        if (!(fabs(dA[i] - want) <= 1e-12 * fabs(want))) host_fail(L, "clamped BCE gradient %.12g, expected %.12g", dA[i], want);
                        continue;
                    }
                    h = 1e-4L * std::min(p, 1.0 - p);
                }
                const long double up = row_loss_ld(c, d, b, i, h, inv_batch, inv_elems), dn = row_loss_ld(c, d, b, i, -h, inv_batch, inv_elems);
                const double cd = (double)((up - dn) / (2 * h));
                const double scale = c.kind == MULTINOMIAL ? (fabs(dA[i]) + db[i] / 2e-5) : c.kind == BCE ? db[i] / (8 * E24) : fabs(dA[i]) + inv_elems;
                if (!(fabs(cd - dA[i]) <= tol * scale + 1e-15)) host_fail(L, "gradient %.12g, central difference %.12g", dA[i], cd);
            }
        }
    }
    if (Z) {
        R.dmu.resize((size_t)B * Z); R.dlv.resize((size_t)B * Z);
        const double w = beta * inv_batch;
        for (size_t k = 0; k < (size_t)B * Z; ++k) {
            const double m = d.mu[k], l = d.lv[k];
            R.dmu[k] = w * m;
            R.dlv[k] = 0.5 * w * expm1(l);
            if (g_host) {     // central differences of w (-0.5) (1 + l - m^2 - e^l)
                const long double h = 1e-4L;
                auto f = [&](long double mm, long double ll) { return (long double)w * -0.5L * (1.0L + ll - mm * mm - expl(ll)); };
                const double gm = (double)((f(m + h, l) - f(m - h, l)) / (2 * h)), gl = (double)((f(m, l + h) - f(m, l - h)) / (2 * h));
                // (the e^l both evaluations carry, up to 4.9e8 w, cancels only to the long double's rounding: 1e-14 w e^l over 2 h)
                if (!(fabs(gm - R.dmu[k]) <= 1e-7 * w * (1 + fabs(m)) + 1e-14 * w * exp(l) + 1e-15)) host_fail(L, "d_mu %.12g, central difference %.12g", R.dmu[k], gm);
                if (!(fabs(gl - R.dlv[k]) <= 1e-7 * w * (1 + exp(l)) + 1e-15)) host_fail(L, "d_logvar %.12g, central difference %.12g", R.dlv[k], gl);
            }
        }
    }
    return R;
}

// ---- one case ---------------------------------------------------------------------------------------------------------------------------
// an input behind `off` floats of junk; an output of n floats behind `off` poisoned floats, poisoned and guarded
static const float* in_dev(const std::vector<float>& h, int off)
{
    if (h.empty()) return nullptr;
    std::vector<float> v(off, 777.f);
    v.insert(v.end(), h.begin(), h.end());
    return to_dev(v) + off;
}
static std::vector<float> out_host(const float* base, size_t n, int off, Line& L, const char* what)
{
    std::vector<float> h = fetch<float>(base, n + off, L, what);
    for (int k = 0; k < off; ++k)
        if (!is_poison(h[k])) { if (L.bad < 4) printf("    %s %s: written in front of its start\n", g_tag.c_str(), what); ++L.bad; }
    return std::vector<float>(h.begin() + off, h.end());
}

struct Ratios { double value = 0, grad = 0, kl = 0; };

static void run_case(const Case& c, Line& L, Ratios& w, Seen& seen)
{
    const int B = c.B, I = c.I, Z = c.Z, off = c.off;
    const float inv_batch = 1.f / (float)B, inv_elems = (float)(1.0 / ((double)B * (double)I));
    char tag[128];
    snprintf(tag, sizeof tag, "(B=%d Z=%d beta=%g)", B, Z, c.beta);
    g_tag = tag;
    const Data d = generate(c);
    const Ref R = reference(c, d, inv_batch, inv_elems, L, seen);
    if (g_host) return;
    const size_t mark = pool_size();
    const size_t n = (size_t)B * I, nz = (size_t)B * Z;
    const float *dA = in_dev(d.A, off), *dX = in_dev(d.X, off), *dmu = in_dev(d.mu, off), *dlv = in_dev(d.lv, off);
    float* rl = dev_out<float>(B);
    float* rl_plain = dev_out<float>(B);
    float* gA = dev_out<float>(n + off);
    float* gmu = Z ? dev_out<float>(nz + off) : nullptr;
    float* glv = Z ? dev_out<float>(nz + off) : nullptr;
    std::vector<float> first[4];
    for (int pass = 0; pass < 2; ++pass) {
        if (pass) { repoison(rl, B); repoison(gA, n + off); if (Z) { repoison(gmu, nz + off); repoison(glv, nz + off); } }
        if (c.kind == MULTINOMIAL)
            RT(rtx_launch_dense_loss_grad(dA, dX, B, I, dmu, dlv, Z, c.beta, inv_batch, rl, gA + off, Z ? gmu + off : nullptr, Z ? glv + off : nullptr, 0));
        else if (c.kind == BCE)
            RT(rtx_launch_dense_bce_kl_grad(dA, dX, B, I, dmu, dlv, Z, inv_elems, inv_batch, rl, gA + off, Z ? gmu + off : nullptr, Z ? glv + off : nullptr, 0));
        else
            RT(rtx_launch_dense_mse_grad(dA, dX, B, I, inv_elems, rl, gA + off, 0));
        CK(hipDeviceSynchronize());
        std::vector<float> got[4] = {fetch<float>(rl, B, L, "row_loss"), out_host(gA, n, off, L, "d_recon"),
                                     Z ? out_host(gmu, nz, off, L, "d_mu") : std::vector<float>(), Z ? out_host(glv, nz, off, L, "d_logvar") : std::vector<float>()};
        if (pass) {     // the second launch: every output to the bit
            static const char* names[4] = {"row_loss (2nd launch)", "d_recon (2nd launch)", "d_mu (2nd launch)", "d_logvar (2nd launch)"};
            for (int q = 0; q < 4; ++q)
                for (size_t k = 0; k < got[q].size(); ++k) judge_bits(f_bits(got[q][k]), f_bits(first[q][k]), L, names[q], (long)k);
            continue;
        }
        for (int q = 0; q < 4; ++q) first[q] = got[q];
        for (int b = 0; b < B; ++b) w.value = std::max(w.value, judge(got[0][b], R.row[b], SUM_TOL * R.row_abs[b], L, "row loss", b));
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < I; ++i) {
                const size_t at = (size_t)b * I + i;
                w.grad = std::max(w.grad, judge(got[1][at], R.dA[at], R.dA_bound[at], L, "d_recon", b, i));
            }
        if (c.kind == MULTINOMIAL && d.zero_row >= 0)     // a row without a target: zeros, not merely small numbers
            for (int i = 0; i < I; ++i) if (!(got[1][(size_t)d.zero_row * I + i] == 0.f)) { host_fail(L, "d_recon of the row without a target: %g", got[1][(size_t)d.zero_row * I + i]); break; }
        for (size_t k = 0; k < nz; ++k) {
            w.kl = std::max(w.kl, judge(got[2][k], R.dmu[k], 4 * ulp32(R.dmu[k]), L, "d_mu", (long)(k / Z), (long)(k % Z)));
            w.kl = std::max(w.kl, judge(got[3][k], R.dlv[k], 4 * ulp32(R.dlv[k]), L, "d_logvar", (long)(k / Z), (long)(k % Z)));
        }
    }
    // the launcher without gradients: the same row losses to the bit
    if (c.kind == MULTINOMIAL) RT(rtx_launch_dense_loss(dA, dX, B, I, dmu, dlv, Z, c.beta, inv_batch, rl_plain, 0));
    else if (c.kind == BCE) RT(rtx_launch_dense_bce_kl(dA, dX, B, I, dmu, dlv, Z, inv_elems, inv_batch, rl_plain, 0));
    else RT(rtx_launch_dense_mse(dA, dX, B, I, inv_elems, rl_plain, 0));
    CK(hipDeviceSynchronize());
    const std::vector<float> plain = fetch<float>(rl_plain, B, L, "row_loss (plain launcher)");
    for (int b = 0; b < B; ++b) judge_bits(f_bits(first[0][b]), f_bits(plain[b]), L, "row loss against the launcher without gradients", b);
    free_from(mark);
}

static void loss_cases()
{
    static const int Is[] = {1, 7, 255, 256, 257, 1000, 4099}, Bs[] = {1, 3, 64}, Zs[] = {0, 1, 5, 200};
    static const float betas[] = {0.f, 0.3f};
    uint32_t seed = 1000;
    for (int kind = 0; kind < 3; ++kind)
        for (int I : Is)
            for (int off = 0; off < 2; ++off) {
                Line L;
                Ratios w;
                Seen seen;
                for (int B : Bs)
                    for (int Z : Zs)
                        for (float beta : betas) {
                            if (kind == MSE && (Z || beta != 0.f)) continue;        // no KL term
                            if (kind == BCE && beta != 0.f) continue;               // no beta: the KL term at weight one
                            run_case({kind, B, I, off, Z, beta, ++seed}, L, w, seen);
                        }
                g_tag.clear();
                if (g_host) {
                    if (kind == MULTINOMIAL && !(seen.zero_rows > 0 && seen.p80 > 0 && (I == 1 || seen.m80 > 0))) host_fail(L, "no row without a target, or no logit of +-80");
                    if (I >= 255 && !(seen.ratings > 0)) host_fail(L, "no rating target (3.5)");
                    if (kind == BCE && I >= 6)
                        for (int p = 0; p < 2; ++p) for (int x = 0; x < 3; ++x) if (!seen.clamp[p][x]) host_fail(L, "p = %g against target kind %g never occurs", p, x);
                }
                char name[128], extra[96];
                snprintf(name, sizeof name, "%s I=%d %s (%s)", KIND[kind], I, off ? "base + 4 bytes" : "base aligned", !off && I % 4 == 0 ? "16-byte route" : "4-byte route");
                snprintf(extra, sizeof extra, "  [value %.3f  grad %.3f  kl %.3f]", w.value, w.grad, w.kl);
                report(name, L, extra);
            }
}

// ---- N: the norms ---------------------------------------------------------------------------------------------------------------------
static void norm_cases()
{
    static const long sizes[] = {1, 255, (1L << 20) + 3, 300};     // the last one all zeros
    const int n = 4;
    for (int off = 0; off < 2; ++off) {
        Line L;
        Rng r = {77u + off};
        std::vector<std::vector<float>> W(n);
        std::vector<double> nrm(n);
        for (int t = 0; t < n; ++t) {
            W[t].resize(sizes[t]);
            double s = 0;
            for (float& v : W[t]) { v = t == 3 ? 0.f : 0.5f * r.f(); s += (double)v * v; }
            if (t == 0) W[t][0] = -0.37f, s = 0.37f * (double)0.37f;
            nrm[t] = sqrt(s);
        }
        char name[96];
        snprintf(name, sizeof name, "N sumsq_ordered + norm_grad sizes 1, 255, 2^20 + 3, 300 (zeros) %s", off ? "base + 4 bytes" : "base aligned");
        if (g_host) {
            for (int t = 0; t < 3; ++t)       // central differences of sqrt(sum w^2) in a few elements
                for (long i = 0; i < sizes[t]; i += std::max<long>(1, sizes[t] / 8)) {
                    const long double h = 1e-4L, w0 = W[t][i], s0 = (long double)nrm[t] * nrm[t] - w0 * w0;
                    const double cd = (double)((sqrtl(s0 + (w0 + h) * (w0 + h)) - sqrtl(s0 + (w0 - h) * (w0 - h))) / (2 * h));
                    if (!(fabs(cd - W[t][i] / nrm[t]) <= 1e-6)) host_fail(L, "norm gradient %.12g, central difference %.12g", W[t][i] / nrm[t], cd);
                }
            if (nrm[3] != 0) host_fail(L, "the zero tensor is not zero");
            report(name, L);
            continue;
        }
        std::vector<const float*> ws(n);
        std::vector<float*> gs(n), gbase(n);
        for (int t = 0; t < n; ++t) { ws[t] = in_dev(W[t], off); gbase[t] = dev_out<float>(sizes[t] + off); gs[t] = gbase[t] + off; }
        float* sumsq = dev_out<float>(n);
        float* atomic_sumsq = dev_out<float>(n);
        float* part = dev_out<float>(rtx_sumsq_ordered_scratch(n));
        std::vector<long> sz(sizes, sizes + n);
        std::vector<std::vector<float>> first(n);
        std::vector<float> ss;
        double worst_n = 0;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass) { repoison(sumsq, n); for (int t = 0; t < n; ++t) repoison(gbase[t], sizes[t] + off); }
            RT(rtx_launch_sumsq_ordered(ws.data(), sz.data(), n, sumsq, part, 0));
            RT(rtx_launch_norm_grad(ws.data(), gs.data(), sz.data(), n, sumsq, 0));
            CK(hipDeviceSynchronize());
            const std::vector<float> s2 = fetch<float>(sumsq, n, L, "sumsq");
            if (pass) for (int t = 0; t < n; ++t) judge_bits(f_bits(s2[t]), f_bits(ss[t]), L, "sumsq (2nd launch)", t);
            else ss = s2;
            for (int t = 0; t < n; ++t) {
                char tag[32];
                snprintf(tag, sizeof tag, "(tensor %d)", t);
                g_tag = tag;
                const std::vector<float> g = out_host(gbase[t], sizes[t], off, L, "grad");
                if (pass) {     // the second launch: to the bit
                    for (long i = 0; i < sizes[t]; ++i) judge_bits(f_bits(g[i]), f_bits(first[t][i]), L, "grad (2nd launch)", i);
                    continue;
                }
                first[t] = g;
                worst_n = std::max(worst_n, judge(sqrt((double)ss[t]), nrm[t], SUM_TOL * nrm[t], L, "norm", t));
                for (long i = 0; i < sizes[t]; ++i) {
                    if (t == 3) { judge_bits(f_bits(g[i]), 0, L, "grad of the zero tensor", i); continue; }
                    const double want = W[t][i] / nrm[t];
                    judge(g[i], want, 4 * ulp32(want), L, "grad", i);
                }
            }
        }
        // a tensor of one block: the squared norm of rtx_launch_sumsq (the plain operator's) to the bit
        g_tag = "(against rtx_launch_sumsq)";
        RT(rtx_launch_sumsq(ws.data(), sz.data(), n, atomic_sumsq, 0));
        CK(hipDeviceSynchronize());
        const std::vector<float> as = fetch<float>(atomic_sumsq, n, L, "sumsq");
        for (int t = 0; t < n; ++t) if (sizes[t] <= 4096) judge_bits(f_bits(ss[t]), f_bits(as[t]), L, "sumsq", t);
        g_tag.clear();
        char extra[64];
        snprintf(extra, sizeof extra, "  [norm %.3f]", worst_n);
        report(name, L, extra);
        free_all();
    }
}

// --host: the launchers refuse what the kernels cannot take, before the first HIP call
static void refusal_cases()
{
    Line L;
    float x = 0.f;
    float* p = &x;
    auto refuse = [&](const char* what, int rc) { if (rc != RTX_EINVAL) host_fail(L, what); };
    refuse("dense_loss_grad: a NULL gradient", rtx_launch_dense_loss_grad(p, p, 2, 4, nullptr, nullptr, 0, 0.f, 0.5f, p, nullptr, nullptr, nullptr, 0));
    refuse("dense_loss_grad: mu without d_mu", rtx_launch_dense_loss_grad(p, p, 2, 4, p, p, 3, 0.f, 0.5f, p, p, nullptr, p, 0));
    refuse("dense_bce_kl_grad: mu without logvar", rtx_launch_dense_bce_kl_grad(p, p, 2, 4, p, nullptr, 3, 0.1f, 0.5f, p, p, p, p, 0));
    refuse("dense_mse_grad: a NULL target", rtx_launch_dense_mse_grad(p, nullptr, 2, 4, 0.1f, p, p, 0));
    const float* ws[1] = {p};
    float* gs[1] = {nullptr};
    long sz[1] = {4};
    refuse("norm_grad: a NULL gradient tensor", rtx_launch_norm_grad(ws, gs, sz, 1, p, 0));
    refuse("norm_grad: 33 tensors", rtx_launch_norm_grad(ws, gs, sz, 33, p, 0));
    report("launchers refuse bad arguments before the first HIP call", L);
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    loss_cases();
    norm_cases();
    if (g_host) refusal_cases();
    return finish("LOSSGRAD");
}
