// What the fused weight-gradient + Adam kernel's optimizer traffic costs when exp_avg and exp_avg_sq live TILE-MAJOR -- one contiguous
// 32-KB chunk per 64 x 128 tile and array -- while p and the bf16 compute copy stay row-major.  The access pattern alone, as
// test_gemm.cpp's "streams" kernel measures it (no K walk, no MFMA): 512 threads per workgroup, one float4 per thread and 16-row pass,
// every load of a thread issued before its first store, non-temporal, tiles ordered with the short dimension fastest and one contiguous
// run per XCD.  Three walks of the same bytes, on both ml-20m matrices, cold (rotating sets larger than the 256-MB cache), interleaved
// and repeated so that the three figures of a line group come from the same minutes of the same box:
//   flat   p, m, v as 32-KB contiguous chunks            (what a plain multi-tensor Adam does: the floor)
//   tile   p, m, v as 64 x 128 tiles of the row-major tensor (512-byte row pieces: what dw_adam.hip does today)
//   mixed  p and the copy as tile row pieces, m and v at tile_index * 8192 + tile_row * 128 + col4 of a padded image
//   make -C tests/native -f state_tiles.mk   -> ../../build/native/bench_state_tiles
#include "../../rectorch_amd/csrc/rtx_common.h"
#include "check.h"

enum { WALK_FLAT = 0, WALK_TILE = 1, WALK_MIXED = 2 };
static const int TM = 64, TN = 128, TILE = TM * TN;   // 8192 floats = 32 KB per tile and array

template <int WALK>
__global__ __launch_bounds__(512, 2) void k_state_walk(float* a0, float* a1, float* a2, bf16_t* sh, int M, int N, int ld_sh, int m_tiles, int n_tiles)
{
    typedef __attribute__((ext_vector_type(4))) float f4;
    typedef f4 f4u __attribute__((aligned(4)));
    float* arr[3] = {a0, a1, a2};
    const int tid = threadIdx.x;
    f4 v[3][4];
    size_t off[4], img[4];
    bool on[4];
    if (WALK == WALK_FLAT) {
        const size_t total = (size_t)M * N, base = (size_t)blockIdx.x * TILE;
#pragma unroll
        for (int q = 0; q < 4; ++q) { off[q] = img[q] = base + (size_t)(q * 512 + tid) * 4; on[q] = off[q] + 4 <= total; }
    } else {
        const int total = m_tiles * n_tiles, per_xcd = (total + 7) / 8;
        const int id = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
        if (id >= total) return;
        int tm, tn;
        if (n_tiles <= m_tiles) { tm = id / n_tiles; tn = id % n_tiles; } else { tn = id / m_tiles; tm = id % m_tiles; }
        const int rowl = tid / 32, col = tn * TN + (tid % 32) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = tm * TM + q * 16 + rowl;
            on[q] = row < M && col + 4 <= N;
            off[q] = (size_t)min(row, M - 1) * N + min(col, N - 4);
            img[q] = WALK == WALK_MIXED ? (size_t)id * TILE + (size_t)(q * 16 + rowl) * TN + (tid % 32) * 4 : off[q];   // the image is padded to whole tiles
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k][q] = __builtin_nontemporal_load((const f4u*)(arr[k] + (k ? img[q] : off[q])));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!on[q]) continue;
        f4 acc = v[0][q];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const f4 w = v[k][q] * 1.0001f + 1e-9f;
            acc += w;
            __builtin_nontemporal_store(w, (f4u*)(arr[k] + (k ? img[q] : off[q])));
        }
        const size_t r = off[q] / N, c = off[q] % N;
        store4<bf16_t>(sh + r * ld_sh + (c & ~(size_t)3), acc[0], acc[1], acc[2], acc[3]);
    }
}

template <int WALK> static void launch(float** arr, bf16_t* sh, int M, int N, size_t set_off)
{
    const int m_tiles = (M + TM - 1) / TM, n_tiles = (N + TN - 1) / TN;
    const unsigned grid = WALK == WALK_FLAT ? (unsigned)(((size_t)M * N + TILE - 1) / TILE) : (unsigned)(8 * ((m_tiles * n_tiles + 7) / 8));
    hipLaunchKernelGGL((k_state_walk<WALK>), dim3(grid), dim3(512), 0, 0, arr[0] + set_off, arr[1] + set_off, arr[2] + set_off, sh, M, N, rtx_pad(N), m_tiles, n_tiles);
}

template <int WALK> static double time_walk(float** arr, bf16_t* sh, int M, int N, size_t stride, int sets)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < sets; ++i) launch<WALK>(arr, sh, M, N, i * stride);
    CK(hipDeviceSynchronize());
    const int it = 12;
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < it; ++i) launch<WALK>(arr, sh, M, N, (i % sets) * stride);   // rotating sets: cold in the 256-MB cache
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return ms * 1000.0 / it;
}

int main()
{
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    printf("device:   CUs=%d  gcnArch=%s\n", prop.multiProcessorCount, prop.gcnArchName);
    const int shapes[2][2] = {{20108, 600}, {600, 20108}};
    // a set holds the larger of the two padded images (10 x 158 tiles): every walk of either shape stays inside it
    const size_t stride = (size_t)1580 * TILE;
    const int sets = 3, reps = 4;
    float* arr[3];
    for (int k = 0; k < 3; ++k) arr[k] = (float*)dev_bytes(stride * sets * 4, 0);
    bf16_t* sh = (bf16_t*)dev_bytes((size_t)rtx_pad(20108) * rtx_pad(600) * 2, 0);
    for (auto& shp : shapes) {
        const int M = shp[0], N = shp[1];
        if ((size_t)((M + TM - 1) / TM) * ((N + TN - 1) / TN) * TILE > stride) { printf("shape %d x %d does not fit its set\n", M, N); return 2; }
        const double bytes = (double)M * N * 26.0;
        double best[3] = {1e30, 1e30, 1e30};
        for (int rep = 0; rep < reps; ++rep) {
            const double us[3] = {time_walk<WALK_FLAT>(arr, sh, M, N, stride, sets), time_walk<WALK_TILE>(arr, sh, M, N, stride, sets),
                                  time_walk<WALK_MIXED>(arr, sh, M, N, stride, sets)};
            for (int w = 0; w < 3; ++w) best[w] = std::min(best[w], us[w]);
            printf("[state-tiles] %5dx%-5d rep %d  flat %6.1f us %5.2f TB/s | 64x128 tiles %6.1f us %5.2f TB/s | p + copy tiles, m + v tile-major image %6.1f us %5.2f TB/s\n", M, N, rep,
                   us[0], bytes / us[0] * 1e-6, us[1], bytes / us[1] * 1e-6, us[2], bytes / us[2] * 1e-6);
        }
        printf("[state-tiles] %5dx%-5d best   flat %6.1f us | tiles %6.1f us | mixed %6.1f us   (mixed closes %.0f %% of the tile - flat gap; 16/26 = 62 %% if m and v became flat)\n", M, N,
               best[0], best[1], best[2], 100.0 * (best[1] - best[2]) / (best[1] - best[0]));
    }
    free_all();
    return 0;
}
