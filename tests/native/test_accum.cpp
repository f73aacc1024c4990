// test_accum: the accumulating epilogues of the weight-gradient kernels alone (gradient accumulation, rtx_engine_set_grad_accum):
//   bf16   rtx_dw_launch / rtx_dw_launch_group with RTX_DW_GRAD_FIRST / RTX_DW_GRAD_ADD (dw_adam.hip), every tile configuration;
//   f32    rtx_gemm_f32_km_launch with RTX_EPI_GRAD_FIRST / _ADD (gemm_f32.hip) and the split-slab path's
//          rtx_launch_dw_slab_reduce_acc (adam.hip).
// For every case: the plain-store launch gives g; FIRST into a NaN-filled buffer must give scale * g BIT FOR BIT, leave no NaN inside
// [M_real][N_real] and write nothing in front of or behind the tensor (poisoned guard bands); ADD twice must give
// fmaf(scale, g, fmaf(scale, g, scale * g)) bit for bit against the host's fmaf; a plain-store launch into the same buffers afterwards
// gives g again (the mode is a template argument: it cannot leak).  `--host` checks the references themselves and makes no HIP call.
#include "../../rectorch_amd/csrc/rtx_gemm.h"
#include "../../rectorch_amd/csrc/rtx_kernels.h"
#include "check.h"

// ---- host references ----------------------------------------------------------------------------------------------------------------
static float ref_first(float s, float g) { volatile float r = s * g; return r; }     // (volatile: one rounded product, never contracted)
static float ref_add(float s, float g, float acc) { return fmaf(s, g, acc); }

static void host_checks()
{
    Line L;
    Rng r{7u};
    for (int i = 0; i < 100000; ++i) {
        const float g = r.f() * 8.f;
        if (ref_first(1.f, g) != g) host_fail(L, "scale 1 changes g");
        if (ref_add(0.5f, g, ref_first(0.5f, g)) != g) host_fail(L, "0.5 g + 0.5 g is not g");
        const float s = 1.f / 3.f;
        const float a3 = ref_add(s, g, ref_add(s, g, ref_first(s, g)));
        const double want = 3.0 * (double)s * (double)g;
        judge(a3, want, 3 * E24 * fabs(want), L, "three thirds", i);
    }
    report("host: scale * g and fmaf(scale, g, acc), 100000 draws", L);
}

// ---- operands -----------------------------------------------------------------------------------------------------------------------
static int pad_to(int v, int m) { return (v + m - 1) / m * m; }

struct Operands {
    int M, N, Kp, Mp, Np;
    std::vector<float> D, A;     // [Kp][Mp], [Kp][Np]: values k / 8, exact in bf16; column N of A holds ones (rows < K)
};
static Operands make_operands(int M, int N, int K, uint32_t seed)
{
    Operands o{M, N, pad_to(K, 128), pad_to(M, 128), pad_to(N + 1, 128)};     // (the engine's padding: rtx_pad)
    o.D.assign((size_t)o.Kp * o.Mp, 0.f);
    o.A.assign((size_t)o.Kp * o.Np, 0.f);
    Rng r{seed};
    for (int k = 0; k < K; ++k) {
        for (int m = 0; m < M; ++m) o.D[(size_t)k * o.Mp + m] = (float)r.i(-8, 8) / 8.f;
        for (int n = 0; n < N; ++n) o.A[(size_t)k * o.Np + n] = (float)r.i(-8, 8) / 8.f;
        o.A[(size_t)k * o.Np + N] = 1.f;
    }
    return o;
}
static std::vector<bf16_t> as_bf16(const std::vector<float>& v)
{
    std::vector<bf16_t> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) h[i] = f32_to_bf16(v[i]);
    return h;
}

// a float32 output with a poisoned guard band in FRONT of it as well as behind it
struct Guarded {
    float* base;
    size_t n;
    float* p() const { return base + GUARD; }
};
static Guarded guarded(size_t n) { return Guarded{dev_poison<float>(n + 2 * GUARD), n}; }
static void poison(const Guarded& b) { CK(hipMemset(b.base, 0xff, (b.n + 2 * GUARD) * sizeof(float))); }
static std::vector<float> take(const Guarded& b, Line& L, const char* what)
{
    std::vector<float> h = to_host(b.base, b.n + 2 * GUARD);
    size_t k = 0;
    if (!guard_intact((const unsigned char*)h.data(), GUARD * sizeof(float), &k) ||
        !guard_intact((const unsigned char*)(h.data() + GUARD + b.n), GUARD * sizeof(float), &k)) {
        if (L.bad < 4) printf("    %s %s: written outside the tensor\n", g_tag.c_str(), what);
        ++L.bad;
    }
    return std::vector<float>(h.begin() + GUARD, h.begin() + GUARD + b.n);
}

// what every case does with its three launch forms: plain(W, b), first(W, b, s), add(W, b, s)
template <typename Plain, typename Acc>
static void run_case(const std::string& name, const std::vector<std::pair<int, int>>& shapes, std::vector<Guarded>& W, std::vector<Guarded>& B,
                     const float* scales, int n_scales, Plain plain, Acc acc)
{
    for (int q = 0; q < n_scales; ++q) {
        const float s = scales[q];
        Line L;
        char nm[256];
        snprintf(nm, sizeof nm, "%s scale %.9g", name.c_str(), s);
        g_tag = nm;
        for (size_t k = 0; k < W.size(); ++k) { poison(W[k]); poison(B[k]); }
        plain();
        CK(hipDeviceSynchronize());
        std::vector<std::vector<float>> g(W.size()), gb(W.size());
        for (size_t k = 0; k < W.size(); ++k) {
            g[k] = take(W[k], L, "plain gW"); gb[k] = take(B[k], L, "plain gbias");
            for (float v : g[k]) if (v != v) { host_fail(L, "plain store left a NaN"); break; }
            double any = 0;
            for (float v : g[k]) any += fabs(v);
            if (!(any > 0)) host_fail(L, "the plain gradient is all zero");
        }
        for (size_t k = 0; k < W.size(); ++k) { poison(W[k]); poison(B[k]); }
        acc(false, s);      // FIRST into NaNs
        CK(hipDeviceSynchronize());
        std::vector<std::vector<float>> a1(W.size()), b1(W.size());
        for (size_t k = 0; k < W.size(); ++k) {
            a1[k] = take(W[k], L, "FIRST gW"); b1[k] = take(B[k], L, "FIRST gbias");
            for (size_t i = 0; i < a1[k].size(); ++i) judge_bits(f_bits(a1[k][i]), f_bits(ref_first(s, g[k][i])), L, "FIRST gW", (long)(i / shapes[k].second), (long)(i % shapes[k].second));
            for (size_t i = 0; i < b1[k].size(); ++i) judge_bits(f_bits(b1[k][i]), f_bits(ref_first(s, gb[k][i])), L, "FIRST gbias", (long)i);
        }
        acc(true, s);
        acc(true, s);       // ADD twice
        CK(hipDeviceSynchronize());
        for (size_t k = 0; k < W.size(); ++k) {
            const std::vector<float> a3 = take(W[k], L, "ADD gW"), b3 = take(B[k], L, "ADD gbias");
            for (size_t i = 0; i < a3.size(); ++i)
                judge_bits(f_bits(a3[i]), f_bits(ref_add(s, g[k][i], ref_add(s, g[k][i], a1[k][i]))), L, "ADD gW", (long)(i / shapes[k].second), (long)(i % shapes[k].second));
            for (size_t i = 0; i < b3.size(); ++i) judge_bits(f_bits(b3[i]), f_bits(ref_add(s, gb[k][i], ref_add(s, gb[k][i], b1[k][i]))), L, "ADD gbias", (long)i);
        }
        plain();            // the mode does not leak: a plain store overwrites what was accumulated
        CK(hipDeviceSynchronize());
        for (size_t k = 0; k < W.size(); ++k) {
            const std::vector<float> a = take(W[k], L, "plain again gW"), b = take(B[k], L, "plain again gbias");
            for (size_t i = 0; i < a.size(); ++i) judge_bits(f_bits(a[i]), f_bits(g[k][i]), L, "plain again gW", (long)i);
            for (size_t i = 0; i < b.size(); ++i) judge_bits(f_bits(b[i]), f_bits(gb[k][i]), L, "plain again gbias", (long)i);
        }
        report(nm, L);
    }
    g_tag.clear();
}

static const float SCALES[3] = {1.f, 0.5f, 1.f / 3.f};

// ---- bf16: dw_adam.hip --------------------------------------------------------------------------------------------------------------
static RtxDw dw_problem(const Operands& o, const bf16_t* dD, const bf16_t* dA, int cfg, float* gW, float* gb)
{
    RtxDw d = {};
    d.A = dD; d.lda = o.Mp; d.B = dA; d.ldb = o.Np;
    d.m_tiles = o.Mp / rtx_dw_tile_rows(cfg);
    d.n_tiles = (o.Np + rtx_dw_tile_cols(cfg) - 1) / rtx_dw_tile_cols(cfg);
    d.k_slices = o.Kp / 64;
    d.M_real = o.M; d.N_real = o.N;
    d.gW = gW; d.gbias = gb;
    return d;
}

static void dw_cases()
{
    const int shapes[4][2] = {{64, 128}, {70, 37}, {33, 130}, {200, 600}};
    for (int cfg = 0; cfg < RTX_DW_CFG_COUNT; ++cfg)
        for (const auto& sh : shapes) {
            const size_t mark = pool_size();
            const Operands o = make_operands(sh[0], sh[1], 128, 100u + cfg + 17u * sh[0]);
            const bf16_t* dD = to_dev(as_bf16(o.D));
            const bf16_t* dA = to_dev(as_bf16(o.A));
            std::vector<Guarded> W{guarded((size_t)o.M * o.N)}, B{guarded((size_t)o.M)};
            RtxDw d = dw_problem(o, dD, dA, cfg, W[0].p(), B[0].p());
            char nm[128];
            snprintf(nm, sizeof nm, "bf16 dw cfg %d (%d x %d tile) out %d in %d", cfg, rtx_dw_tile_rows(cfg), rtx_dw_tile_cols(cfg), o.M, o.N);
            run_case(nm, {{o.M, o.N}}, W, B, SCALES, 3, [&] { RT(rtx_dw_launch(d, RTX_DW_GRAD, cfg, 0)); },
                     [&](bool add, float s) { RtxDw a = d; a.acc_scale = s; RT(rtx_dw_launch(a, add ? RTX_DW_GRAD_ADD : RTX_DW_GRAD_FIRST, cfg, 0)); });
            free_from(mark);
        }
    // a grouped launch of three of them (the default tile and the 128 x 128 one), each with its own scale field
    for (int cfg : {(int)RTX_DW_64x128, (int)RTX_DW_128x128}) {
        const size_t mark = pool_size();
        const int gs[3][2] = {{70, 37}, {33, 130}, {200, 600}};
        std::vector<Operands> os;
        std::vector<Guarded> W, B;
        std::vector<RtxDw> ds;
        std::vector<std::pair<int, int>> dims;
        for (int k = 0; k < 3; ++k) {
            os.push_back(make_operands(gs[k][0], gs[k][1], 128, 900u + k));
            W.push_back(guarded((size_t)gs[k][0] * gs[k][1]));
            B.push_back(guarded((size_t)gs[k][0]));
            ds.push_back(dw_problem(os[k], to_dev(as_bf16(os[k].D)), to_dev(as_bf16(os[k].A)), cfg, W[k].p(), B[k].p()));
            dims.push_back({gs[k][0], gs[k][1]});
        }
        char nm[128];
        snprintf(nm, sizeof nm, "bf16 dw GROUP of three, cfg %d", cfg);
        run_case(nm, dims, W, B, SCALES, 3, [&] { RT(rtx_dw_launch_group(ds.data(), 3, RTX_DW_GRAD, cfg, 0)); },
                 [&](bool add, float s) {
                     std::vector<RtxDw> a = ds;
                     for (auto& x : a) x.acc_scale = s;
                     RT(rtx_dw_launch_group(a.data(), 3, add ? RTX_DW_GRAD_ADD : RTX_DW_GRAD_FIRST, cfg, 0));
                 });
        free_from(mark);
    }
}

// ---- float32: gemm_f32.hip and the split-slab reduce ----------------------------------------------------------------------------------
static void f32_cases()
{
    const int shapes[2][2] = {{128, 128}, {130, 70}};
    for (const auto& sh : shapes) {
        const size_t mark = pool_size();
        const Operands p = make_operands(sh[0], sh[1], 128, 500u + sh[0]);
        const float* dD = to_dev(p.D);
        const float* dA = to_dev(p.A);
        std::vector<Guarded> W{guarded((size_t)p.M * p.N)}, B{guarded((size_t)p.M)};
        RtxGemm g = {};
        g.form = RTX_FORM_TN;
        g.A = dD; g.lda = p.Mp; g.B = dA; g.ldb = p.Np;
        g.k_slices = p.Kp / 32; g.tile_shape = RTX_TILE_128x128; g.m_tiles = p.Mp / 128; g.n_tiles = p.Np / 128;
        g.splits = 1; g.C = W[0].p(); g.gbias = B[0].p(); g.M_real = p.M; g.N_real = p.N;
        char nm[128];
        snprintf(nm, sizeof nm, "f32 RTX_EPI_GRAD out %d in %d", p.M, p.N);
        run_case(nm, {{p.M, p.N}}, W, B, SCALES, 3, [&] { RT(rtx_gemm_f32_km_launch(g, RTX_EPI_GRAD, 0)); },
                 [&](bool add, float s) { RtxGemm a = g; a.acc_scale = s; RT(rtx_gemm_f32_km_launch(a, add ? RTX_EPI_GRAD_ADD : RTX_EPI_GRAD_FIRST, 0)); });
        // the split-slab path: 2 x 1 tiles (<= 64), 4 K slices in 2 splits; the slabs stay as the product left them
        if (sh[0] == 130) {
            const int sp = 2;
            float* slabs = dev_out<float>((size_t)sp * p.Mp * p.Np);
            RtxGemm q = g;
            q.splits = sp; q.C = slabs; q.ldc = p.Np; q.slab_stride = (long)p.Mp * p.Np; q.gbias = nullptr;
            RT(rtx_gemm_f32_km_launch(q, RTX_EPI_STORE, 0));
            CK(hipDeviceSynchronize());
            const std::vector<float> slabs0 = to_host(slabs, (size_t)sp * p.Mp * p.Np);
            run_case("f32 split-slab reduce, 2 splits, out 130 in 70", {{p.M, p.N}}, W, B, SCALES, 3,
                     [&] { RT(rtx_launch_dw_slab_reduce(slabs, sp, q.slab_stride, q.ldc, p.M, p.N, W[0].p(), B[0].p(), 0)); },
                     [&](bool add, float s) { RT(rtx_launch_dw_slab_reduce_acc(slabs, sp, q.slab_stride, q.ldc, p.M, p.N, W[0].p(), B[0].p(), add, s, 0)); });
            Line L;
            const std::vector<float> slabs1 = fetch<float>(slabs, (size_t)sp * p.Mp * p.Np, L, "slabs");
            if (memcmp(slabs0.data(), slabs1.data(), slabs0.size() * sizeof(float)) != 0) host_fail(L, "the reduce changed the slabs");
            report("f32 split-slab: the slabs are left as they were", L);
        }
        free_from(mark);
    }
}

int main(int argc, char** argv)
{
    take_host_flag(argc, argv);
    host_checks();
    if (!g_host) {
        dw_cases();
        f32_cases();
        free_all();
    }
    return finish("ACCUM");
}
