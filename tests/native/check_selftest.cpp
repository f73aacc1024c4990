// Host-only check of check.h: that the checks the native drivers rely on can fail.  No HIP call; exits 0 only if every line holds.
#include "check.h"

static int g_wrong = 0;
static void expect(bool ok, const char* what)
{
    printf("%-86s %s\n", what, ok ? "ok" : "WRONG");
    if (!ok) ++g_wrong;
}

int main()
{
    printf("(the indented lines below are the failures this program feeds to the harness on purpose)\n");
    const double bound = 1e-6;
    {   // judge: the comparison is !(err <= bound)
        Line L;
        const double r = judge(nextafter(bound, 1.0), 0.0, bound, L, "just above", 0, 0);
        expect(L.bad == 1 && r > 1.0 && L.worst == r, "judge: an error just above the bound is bad");
        judge(NAN, 1.0, bound, L, "nan", 1);
        expect(L.bad == 2, "judge: a NaN is bad");
        judge(1.0, 1.0, NAN, L, "nan bound", 2);
        expect(L.bad == 3, "judge: a NaN bound is bad");
    }
    {
        Line L;
        const double r = judge(3.0, 2.0, 1.0, L, "at the bound", 0);
        expect(L.bad == 0 && r == 1.0 && L.worst == 1.0, "judge: an error equal to the bound is good, ratio 1");
        const double z = judge(2.5, 2.5, 0.0, L, "exact", 0);
        expect(L.bad == 0 && z == 0.0 && L.worst == 1.0, "judge: an exact match at bound 0 is good and returns 0");
        judge(2.5, 2.5000001, 0.0, L, "inexact at bound 0", 0);
        expect(L.bad == 1, "judge: any error at bound 0 is bad");
    }
    {
        Line L;
        judge_bits(f_bits(0.f), f_bits(-0.f), L, "zero", 0, 0);
        expect(L.bad == 1, "judge_bits: +0 against -0 is bad");
        judge_bits(f_bits(-0.f), f_bits(-0.f), L, "zero", 0, 0);
        expect(L.bad == 1, "judge_bits: equal bits are good");
    }
    {   // the guard scan
        const size_t n = GUARD * sizeof(double);
        std::vector<unsigned char> tail(n, 0xff);
        size_t at = 12345;
        expect(guard_intact(tail.data(), n, &at) && at == 12345, "guard_intact: an all-0xff tail is intact");
        tail[0] = 0xfe;
        expect(!guard_intact(tail.data(), n, &at) && at == 0, "guard_intact: the first byte cleared is seen at offset 0");
        tail[0] = 0xff; tail[n - 1] = 0x7f;
        expect(!guard_intact(tail.data(), n, &at) && at == n - 1, "guard_intact: the last byte cleared is seen at the last offset");
    }
    {   // the poison: what memset(0xff) leaves
        unsigned char raw[8];
        memset(raw, 0xff, 8);
        float f; double d;
        memcpy(&f, raw, 4); memcpy(&d, raw, 8);
        const float hi16 = bits_f(0xffffu << 16);      // a bf16 of all bits set is the upper half of this float32
        expect(f != f && d != d && hi16 != hi16, "poison: all bits set is a NaN in float32, in float64 and in bf16");
        expect(is_poison(f) && is_poison(d) && is_poison(poison_f32()) && is_poison(poison_f64()), "poison: memset(0xff) is poison_f32() / poison_f64()");
        expect(!is_poison(NAN) && !is_poison((double)NAN) && !is_poison(0.f), "is_poison: another NaN and a zero are not the poison");
    }
    {   // report and the closing line
        Line good, bad;
        bad.bad = 1;
        const int before = g_failed;
        report("a line without a bad element", good);
        expect(g_failed == before && g_cases == 1, "report: a Line with bad == 0 leaves g_failed");
        expect(finish("SELFTEST (passing case)") == 0, "finish: 0 while g_failed == 0");
        report("a line with a bad element", bad);
        expect(g_failed == before + 1 && g_cases == 2, "report: a Line with bad > 0 raises g_failed");
        expect(finish("SELFTEST (failing case, on purpose)") != 0, "finish: non-zero when g_failed > 0");
    }
    {   // --host is taken out of the arguments, the rest stays in order
        char a0[] = "x", a1[] = "--mutate", a2[] = "--host", a3[] = "2";
        char* argv[] = {a0, a1, a2, a3, nullptr};
        int argc = 4;
        expect(take_host_flag(argc, argv) && g_host && argc == 3 && !strcmp(argv[1], "--mutate") && !strcmp(argv[2], "2"), "take_host_flag: --host found and removed");
    }
    printf(g_wrong ? "CHECK SELFTEST WRONG (%d lines)\n" : "CHECK SELFTEST HOLDS\n", g_wrong);
    return g_wrong ? 1 : 0;
}
