// span_start_check.cpp -- the division-free decode of the span cache's use kernel (hg_span_start.h) against frame_group (hg_dev.h), whose arithmetic
// is transcribed below with its divisions: every block id of every grid of the tables, for fixed bands, rotating bands and sub-bands, and the
// multiply-shift pairs on their own at the edges of their range.  Stand-alone, host code only: tests/test_span_start_cpu.py builds it under
// AddressSanitizer + UndefinedBehaviorSanitizer and runs it.
#include "hg_span_start.h"

#include <cstdio>
#include <cstdlib>
#include <cstdint>

using namespace hg;

static long g_checks = 0, g_bad = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_bad++; if (g_bad < 40) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// frame_group (hg_dev.h), as the row kernels other than the use kernel run it
static bool frame_group_ref(int xcc_log2, int xcc_rotate, int sub_groups, int n_frames, int xcd, int bi, int groups_per_xcd, int &f, int &g)
{
    if (sub_groups > 0) {
        const int per_sub = sub_groups * n_frames, sb = bi / per_sub, rem = bi - sb * per_sub;
        f = rem / sub_groups;
        g = ((sb << xcc_log2) + xcd) * sub_groups + (rem - f * sub_groups);
        return g < (groups_per_xcd << xcc_log2);
    }
    f = bi / groups_per_xcd;
    g = ((xcd + (xcc_rotate ? f : 0)) & ((1 << xcc_log2) - 1)) * groups_per_xcd + (bi - f * groups_per_xcd);
    return true;
}
// the launcher's grid (launch_pw_rows, sub_groups_of / padded_groups in hg_dev.h)
static int sub_groups_of(int sub_bands, int groups_per_xcd) { return sub_bands > 1 ? (groups_per_xcd + sub_bands - 1) / sub_bands : 0; }
static int padded_groups(int groups_per_xcd, int sub_groups) { return sub_groups > 0 ? ((groups_per_xcd + sub_groups - 1) / sub_groups) * sub_groups : groups_per_xcd; }

static void check_grid(int xcc_log2, int rotate, int sub_bands, int n_frames, int max_h, int rg)
{
    const int nx = 1 << xcc_log2;
    const int rpx = ((max_h + rg - 1) / rg + nx - 1) / nx;
    const int sub = sub_groups_of(sub_bands, rpx);
    const long grid = (long)padded_groups(rpx, sub) * nx * n_frames;
    const SpanStartDecode d = span_start_decode_make(xcc_log2, rotate, sub, n_frames, rpx);
    long valid = 0;
    for (long bid = 0; bid < grid; bid++) {
        int f0 = -1, g0 = -1, f1 = -2, g1 = -2;
        const bool ok0 = frame_group_ref(xcc_log2, rotate, sub, n_frames, (int)bid & (nx - 1), (int)bid >> xcc_log2, rpx, f0, g0);
        const bool ok1 = span_start_decode(d, (int)bid, f1, g1);
        CHECK(ok0 == ok1);
        CHECK(f0 == f1 && g0 == g1);
        CHECK(f1 >= 0 && f1 < n_frames);
        valid += ok1;
    }
    CHECK(valid == (long)rpx * nx * n_frames);          // every group slot of every frame exactly once, the padding besides
}

int main()
{
    // the pairs on their own: divisors around powers of two and the largest, dividends at the multiples' edges and at the top of the range
    const uint32_t ds[] = { 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 139, 140, 557, 1000, 4095, 4096, 4097, 65535, 65536, 65537, 1u << 20, (1u << 30) - 1, 1u << 30,
                            (1u << 30) + 1, 0x7ffffffeu, 0x7fffffffu };
    for (uint32_t d : ds) {
        const SpanDiv v = span_div_make(d);
        CHECK(v.shift >= 31 && v.shift <= 62);
        for (uint64_t q = 0; q * d < (1ull << 31) && q < 70; q++)
            for (int e = -1; e <= 1; e++) {
                const int64_t n = (int64_t)(q * d) + e;
                if (n < 0 || n >= (1ll << 31)) continue;
                CHECK(span_div((uint32_t)n, v) == (uint32_t)n / d);
            }
        const uint64_t top = ((1ull << 31) - 1) / d;
        for (uint64_t q = top > 3 ? top - 3 : 0; q <= top; q++)
            for (int e = -1; e <= 1; e++) {
                const int64_t n = (int64_t)(q * d) + e;
                if (n < 0 || n >= (1ll << 31)) continue;
                CHECK(span_div((uint32_t)n, v) == (uint32_t)n / d);
            }
        CHECK(span_div(0x7fffffffu, v) == 0x7fffffffu / d);
    }
    uint32_t lcg = 12345u;
    for (int i = 0; i < 200000; i++) {
        lcg = lcg * 1664525u + 1013904223u; const uint32_t bits = lcg >> 27;               // divisors of every size, 1 .. 2^31 - 1
        lcg = lcg * 1664525u + 1013904223u; const uint32_t d = ((lcg >> 1) >> bits) | 1u;
        lcg = lcg * 1664525u + 1013904223u; const uint32_t n = lcg >> 1;
        CHECK(span_div(n, span_div_make(d)) == n / d);
    }

    // the grids: XCC counts 1, 2, 4, 8; fixed bands, rotating bands, sub-bands 2, 3, 8; frame counts 1, 3, 64, 513; heights whose group count does
    // and does not divide by the XCC count and by the sub-bands (4-row groups and one-row groups)
    const int heights[] = { 1, 3, 4, 9, 22, 31, 32, 33, 127, 128, 129, 257, 2160, 2170 };
    const int frames[] = { 1, 3, 64, 513 };
    for (int xl = 0; xl <= 3; xl++)
        for (int nf : frames)
            for (int h : heights)
                for (int rg : { 4, 1 }) {
                    if ((long)nf * h > 300000) continue;            // (the walk is per block id: the largest sets once, below)
                    check_grid(xl, 0, 0, nf, h, rg);
                    check_grid(xl, 1, 0, nf, h, rg);
                    for (int sb : { 2, 3, 8 }) check_grid(xl, 0, sb, nf, h, rg);
                }
    check_grid(3, 0, 0, 513, 2170, 4); check_grid(3, 1, 0, 513, 2170, 4); check_grid(3, 0, 2, 513, 2170, 4); check_grid(3, 0, 3, 513, 2160, 4);
    check_grid(3, 0, 8, 513, 2170, 4); check_grid(3, 0, 3, 64, 2170, 4);       // (the last: the headline's shape)

    std::printf("span_start_check: checks %ld failures %ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
