// The two relayouts of the tile-major optimizer state (dw_adam.hip: rtx_dw_state_relayout), bit for bit, on the harness of check.h:
//   tensors -> images: every element of the M x N exp_avg / exp_avg_sq sits where the fused kernel addresses it -- chunk number = the
//     tile's place in the kernel's short-dimension-fastest order (written out here a second time, not taken from rtx_dw_tile_of), element
//     (tile_row, tile_col) at tile_row * 128 + tile_col -- and every pad slot of the images holds zero;
//   images -> tensors: with junk in every pad slot of the images, the tensors get their own bits back and nothing else: the poisoned guard
//     behind them is intact, which is the only place a pad slot of the last tile row could go.
// Shapes: one whole tile; a partial last tile both ways with rows of a multiple of four floats; rows of an odd number of floats (the
// element-wise side).  Each with more column tiles than row tiles and with more row tiles than needed (the engine's m_tiles counts the
// padded rows: whole tiles of pad), so that both branches of the tile order run.
//   make -C tests/native -f state_tiles.mk   -> ../../build/native/test_state_tiles
#include "../../rectorch_amd/csrc/rtx_gemm.h"
#include "check.h"

static const int TM = 64, TNC = 128;

static size_t image_index(int r, int c, int m_tiles, int n_tiles)
{
    const int tm = r / TM, tn = c / TNC;
    const size_t tile = n_tiles <= m_tiles ? (size_t)tm * n_tiles + tn : (size_t)tn * m_tiles + tm;   // the short dimension runs fastest
    return tile * TM * TNC + (size_t)(r % TM) * TNC + c % TNC;
}

static void run_case(int M, int N, int m_tiles, int n_tiles)
{
    char name[128];
    snprintf(name, sizeof name, "relayout %3d x %3d as %d x %d tiles (%s)", M, N, m_tiles, n_tiles, n_tiles <= m_tiles ? "row tiles slowest" : "column tiles slowest");
    g_tag = name;
    Line L;
    const size_t mark = pool_size(), P = (size_t)M * N, E = rtx_dw_state_image_elems(m_tiles, n_tiles, RTX_DW_64x128);
    if (E != (size_t)m_tiles * n_tiles * TM * TNC) host_fail(L, "image of %g floats, expected %g", (double)E, (double)m_tiles * n_tiles * TM * TNC);
    Rng rng{(uint32_t)(M * 131 + N * 7 + m_tiles)};
    std::vector<float> hm(P), hv(P);
    for (size_t i = 0; i < P; ++i) { hm[i] = rng.f(); hv[i] = rng.u01() + 1.f; }
    float *m = to_dev(hm), *v = to_dev(hv);
    float *mi = dev_out<float>(E), *vi = dev_out<float>(E);
    RT(rtx_dw_state_relayout(m, v, mi, vi, M, N, m_tiles, n_tiles, RTX_DW_64x128, 1, 0));
    CK(hipDeviceSynchronize());
    std::vector<float> im = fetch<float>(mi, E, L, "exp_avg image"), iv = fetch<float>(vi, E, L, "exp_avg_sq image");
    std::vector<char> used(E, 0);
    for (int r = 0; r < M; ++r)
        for (int c = 0; c < N; ++c) {
            const size_t k = image_index(r, c, m_tiles, n_tiles);
            used[k] = 1;
            judge_bits(f_bits(im[k]), f_bits(hm[(size_t)r * N + c]), L, "exp_avg image of", r, c);
            judge_bits(f_bits(iv[k]), f_bits(hv[(size_t)r * N + c]), L, "exp_avg_sq image of", r, c);
        }
    for (size_t k = 0; k < E; ++k)
        if (!used[k]) {
            judge_bits(f_bits(im[k]), 0u, L, "exp_avg image pad", (long)k);
            judge_bits(f_bits(iv[k]), 0u, L, "exp_avg_sq image pad", (long)k);
            im[k] = rng.junk(); iv[k] = rng.junk();
        }
    // back: junk in every pad slot, poisoned tensors with a guard
    CK(hipMemcpy(mi, im.data(), E * sizeof(float), hipMemcpyHostToDevice));
    CK(hipMemcpy(vi, iv.data(), E * sizeof(float), hipMemcpyHostToDevice));
    float *m2 = dev_out<float>(P), *v2 = dev_out<float>(P);
    RT(rtx_dw_state_relayout(m2, v2, mi, vi, M, N, m_tiles, n_tiles, RTX_DW_64x128, 0, 0));
    CK(hipDeviceSynchronize());
    const std::vector<float> bm = fetch<float>(m2, P, L, "exp_avg"), bv = fetch<float>(v2, P, L, "exp_avg_sq");
    for (size_t i = 0; i < P; ++i) {
        judge_bits(f_bits(bm[i]), f_bits(hm[i]), L, "exp_avg", (long)(i / N), (long)(i % N));
        judge_bits(f_bits(bv[i]), f_bits(hv[i]), L, "exp_avg_sq", (long)(i / N), (long)(i % N));
    }
    report(name, L);
    free_from(mark);
}

int main()
{
    run_case(64, 128, 1, 1);
    run_case(64, 128, 1, 2);    // (a whole tile of pad columns)
    run_case(70, 260, 2, 3);
    run_case(70, 260, 4, 3);    // (whole tiles of pad rows, as the engine's padded row count gives)
    run_case(70, 263, 2, 3);
    run_case(70, 263, 4, 3);
    run_case(263, 70, 5, 1);    // (one column tile: the other order with real data in every row tile)
    // what the launcher refuses: tiles that do not cover the tensor, a missing buffer
    {
        g_tag = "refusals";
        Line L;
        float* a = dev_out<float>(TM * TNC);
        if (rtx_dw_state_relayout(a, a, a, a, 65, 128, 1, 1, RTX_DW_64x128, 1, 0) == RTX_OK) host_fail(L, "65 rows in one 64-row tile were accepted");
        if (rtx_dw_state_relayout(a, a, a, a, 64, 129, 1, 1, RTX_DW_64x128, 1, 0) == RTX_OK) host_fail(L, "129 columns in one 128-column tile were accepted");
        if (rtx_dw_state_relayout(a, a, nullptr, a, 64, 128, 1, 1, RTX_DW_64x128, 1, 0) == RTX_OK) host_fail(L, "a NULL image was accepted");
        CK(hipDeviceSynchronize());
        fetch<float>(a, TM * TNC, L, "untouched buffer");
        report("relayout refusals", L);
    }
    free_all();
    return finish("STATE TILES");
}
