// The harness the native float64 drivers share (test_loss, test_layers, test_adam, test_solver; test_spmm takes CK, RT and to_dev):
// the error macros, the case generators' random numbers, bit helpers and the poison, the pool of device buffers, the judging of one
// element against its bound, the poisoned guard behind every output, and the --host switch with the closing line.  Everything is
// static / inline: a driver includes this header and links nothing more.  A new driver includes it too and copies none of it;
// check_selftest.cpp checks that the checks in here can fail.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

const char* rtx_last_error_str();

#define CK(x)                                                                            \
    do {                                                                                 \
        hipError_t e = (x);                                                              \
        if (e != hipSuccess) {                                                           \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
            exit(2);                                                                     \
        }                                                                                \
    } while (0)
#define RT(x)                                                                                 \
    do {                                                                                      \
        if ((x) != RTX_OK) {                                                                  \
            printf("launch failed at %s:%d: %s\n", __FILE__, __LINE__, rtx_last_error_str()); \
            exit(2);                                                                          \
        }                                                                                     \
    } while (0)

static const double E24 = 5.9604644775390625e-08;   // 2^-24: one float32 rounding, relative
static const double U53 = 1.1102230246251565e-16;   // 2^-53: one float64 rounding, relative

static inline uint32_t f_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float bits_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint64_t d_bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static inline bool is_junk(double v) { return fabs(v) >= 400.0 && fabs(v) <= 1600.0; }   // what Rng::junk() draws, with room for one bf16 rounding
// the poison: all bits set, a NaN in float64, in float32 and in bf16 (either half of a float32); memset(0xff) writes it
static inline float poison_f32() { return bits_f(~0u); }
static inline double poison_f64() { const uint64_t u = ~0ull; double v; memcpy(&v, &u, 8); return v; }
static inline bool is_poison(float v) { return f_bits(v) == ~0u; }
static inline bool is_poison(double v) { return d_bits(v) == ~0ull; }

struct Rng {
    uint32_t s;
    uint32_t u() { s = s * 1664525u + 1013904223u; return s >> 8; }   // 24 bits
    float u01() { return u() * (1.0f / 16777216.0f); }                // [0, 1), exact in float32 (and so in float64)
    float f() { return u01() * 2.f - 1.f; }                           // [-1, 1), one draw
    double f48() { const double hi = u(), lo = u(); return (hi + lo * (1.0 / 16777216.0)) * (1.0 / 8388608.0) - 1.0; }   // [-1, 1), two draws: 48 random bits
    float junk() { const float m = 500.f + 1000.f * u01(); return (u() & 1) ? m : -m; }   // finite, |x| in [500, 1500), two draws
    int below(int n) { return (int)(u() % (uint32_t)n); }
    int i(int lo, int hi) { return lo + (int)(u() % (uint32_t)(hi - lo + 1)); }   // [lo, hi]
};

// ---- device buffers (never touched in --host mode) -------------------------------------------------------------------------------
// outputs carry a guard of GUARD poisoned elements behind their end: a write out of bounds shows (fetch)
static const int GUARD = 64;
static std::vector<void*> g_allocs;
static inline void* dev_bytes(size_t bytes, int fill)
{
    void* d = nullptr;
    CK(hipMalloc(&d, std::max<size_t>(bytes, 16)));
    CK(hipMemset(d, fill, std::max<size_t>(bytes, 16)));
    g_allocs.push_back(d);
    return d;
}
template <typename T>
static T* to_dev(const std::vector<T>& h)
{
    T* d = (T*)dev_bytes(h.size() * sizeof(T), 0);
    if (!h.empty()) CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <typename T> static T* dev_poison(size_t n) { return (T*)dev_bytes(n * sizeof(T), 0xff); }
template <typename T> static T* dev_out(size_t n) { return dev_poison<T>(n + GUARD); }
template <typename T> static void repoison(T* d, size_t n) { if (d) CK(hipMemset(d, 0xff, (n + GUARD) * sizeof(T))); }
template <typename T>
static std::vector<T> to_host(const T* d, size_t n)
{
    std::vector<T> h(n);
    if (n) CK(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}
// frees the buffers allocated since `mark` = pool_size() at an earlier moment, the latest first; free_all(): every buffer
static inline size_t pool_size() { return g_allocs.size(); }
static inline void free_from(size_t mark)
{
    for (; g_allocs.size() > mark; g_allocs.pop_back()) CK(hipFree(g_allocs.back()));
}
static inline void free_all() { free_from(0); }

// ---- judging ------------------------------------------------------------------------------------------------------------------------
struct Line {
    double worst = 0;        // worst error / bound
    long bad = 0;
    std::string failed;      // the launch shapes that failed (test_layers)
};
static std::string g_tag;    // what is being judged: a launch shape, a tensor, a call (printed with a failing element)
static int g_failed = 0, g_cases = 0;
static int g_name_width = 78;   // of the name column of report(); test_adam, whose names are longer, sets 84
static bool g_host = false;

static inline std::string where(const char* what, long i, long j)
{
    char idx[64];
    if (j < 0) snprintf(idx, sizeof idx, "[%ld]", i);
    else snprintf(idx, sizeof idx, "[%ld][%ld]", i, j);
    return (g_tag.empty() ? "" : g_tag + " ") + what + idx;
}
// one element against its bound; returns error / bound (0 where the bound is 0) for the drivers' tables.  !(err <= bound): a NaN fails.
static inline double judge(double got, double want, double bound, Line& L, const char* what, long i, long j = -1)
{
    const double err = fabs(got - want);
    if (!(err <= bound)) {
        if (L.bad < 4) printf("    %s = %.9g, expected %.9g (error %.3g, bound %.3g)\n", where(what, i, j).c_str(), got, want, err, bound);
        ++L.bad;
    }
    const double ratio = bound > 0 ? err / bound : 0.0;
    if (ratio > L.worst) L.worst = ratio;
    return ratio;
}
static inline void judge_bits(uint32_t got, uint32_t want, Line& L, const char* what, long i, long j = -1)
{
    if (got != want) {
        if (L.bad < 4) printf("    %s holds the bits %08x, expected %08x\n", where(what, i, j).c_str(), got, want);
        ++L.bad;
    }
}
static inline void host_fail(Line& L, const char* fmt, double a = 0, double b = 0)
{
    if (L.bad < 4) { printf("    "); printf(fmt, a, b); printf("\n"); }
    ++L.bad;
}
static inline void report(const std::string& name, const Line& L, const char* extra = "")
{
    printf("%-*s worst %.3f of bound  bad=%ld%s  %s%s\n", g_name_width, name.c_str(), L.worst, L.bad, extra, L.bad ? "FAIL" : "ok",
           L.failed.empty() ? "" : (" at" + L.failed).c_str());
    ++g_cases;
    if (L.bad) ++g_failed;
}

// ---- the guard ----------------------------------------------------------------------------------------------------------------------
// true when all `bytes` bytes of a guard still hold the poison; otherwise *first_bad is the offset of the first byte that does not
static inline bool guard_intact(const unsigned char* tail, size_t bytes, size_t* first_bad)
{
    for (size_t k = 0; k < bytes; ++k)
        if (tail[k] != 0xff) { *first_bad = k; return false; }
    return true;
}
// n elements of an output made by dev_out, its guard checked; `raw` collects the bytes of the n elements
template <typename T>
static std::vector<T> fetch(const void* d, size_t n, Line& L, const char* what, std::vector<unsigned char>* raw = nullptr)
{
    std::vector<T> h = to_host((const T*)d, n + GUARD);
    size_t k = 0;
    if (!guard_intact((const unsigned char*)(h.data() + n), GUARD * sizeof(T), &k)) {
        if (L.bad < 4) printf("    %s%s%s: written %zu bytes past its end\n", g_tag.c_str(), g_tag.empty() ? "" : " ", what, k);
        ++L.bad;
    }
    h.resize(n);
    if (raw) raw->insert(raw->end(), (const unsigned char*)h.data(), (const unsigned char*)(h.data() + n));
    return h;
}

// ---- entry and exit -----------------------------------------------------------------------------------------------------------------
// takes --host out of the arguments (the driver reads the rest) and sets g_host
static inline bool take_host_flag(int& argc, char** argv)
{
    int kept = 1;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--host")) g_host = true;
        else argv[kept++] = argv[i];
    }
    argc = kept;
    return g_host;
}
// the closing line and the exit status
static inline int finish(const char* family)
{
    if (g_failed) printf("%s TESTS FAILED (%d failing cases)\n", family, g_failed);
    else if (!g_cases) printf("%s TESTS PASSED (0 failing cases)\n", family);   // test_solver's own report line counts failures only
    else printf("%s TESTS PASSED (%d cases%s)\n", family, g_cases, g_host ? ", host reference only" : "");
    return g_failed ? 1 : 0;
}
