// span_lean_check -- span_cells_lean (hg_math.h; what the self-span prologues of k_pw_rows / k_pw_patch / k_pw_tile run) against span_cells,
// the restatement of the reference's predictXLimits + fill() that k_map_fill and the CPU tests trust.  Host only: no HIP call, no device.
//   for every row of every generated triangle, both EDGES_TOGETHER forms:
//     (k < fin) agrees with span_cells, and where the span is not empty k and fin are span_cells' (the kernels never use an empty span's ends);
//     the first output row span_first_row gives is the row cell k lies in.
// Built and run by tests/test_span_lean_cpu.py (with -fsanitize=undefined).  usage: span_lean_check [triangles] [seed]
#include "hg_math.h"
#include <cstdio>
#include <cstdlib>

using namespace hg;

static uint64_t g_state;
static uint64_t next_u64()                          // splitmix64
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static int next_int(int lo, int hi) { return lo + (int)(next_u64() % (uint64_t)(hi - lo + 1)); }      // inclusive
static double next_unit() { return (double)(next_u64() >> 11) * 0x1p-53; }

// one vertex coordinate around the window [lo, hi): arbitrary doubles, f32 values (what the kernels are given), integers, .5 ties, specials
static double coord(double lo, double hi)
{
    static const double special[] = { 0.0, -0.0, 0.5, -0.5, 1.5, 2.5, 0.49999999999999994, NAN, INFINITY, -INFINITY, 16777216.0, -16777216.0 };
    const double span = hi - lo, v = lo - 0.5 * span + 2.0 * span * next_unit();
    switch (next_int(0, 15)) {
    case 0: return special[next_int(0, (int)(sizeof special / sizeof *special) - 1)];
    case 1: case 2: case 3: return floor(v);
    case 4: case 5: case 6: return floor(v) + 0.5;
    case 7: case 8: case 9: case 10: return v;
    default: return (double)(float)v;
    }
}

int main(int argc, char **argv)
{
    const long n_tris = argc > 1 ? atol(argv[1]) : 11000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 778;
    long rows = 0, nonempty = 0, bad = 0;
    for (long it = 0; it < n_tris; it++) {
        const int W = next_int(1, 300), H = next_int(1, 300), y_off = next_int(-20, 20);
        double p[6];
        for (int v = 0; v < 3; v++) { p[2 * v] = coord(0.0, (double)W); p[2 * v + 1] = coord((double)y_off, (double)(y_off + H)); }
        Seg seg[3];
        define_seg(p[0], p[1], p[2], p[3], seg[0]);
        define_seg(p[0], p[1], p[4], p[5], seg[1]);
        define_seg(p[2], p[3], p[4], p[5], seg[2]);
        const int64_t len = (int64_t)W * H;
        for (int y = y_off - H - 3; y <= y_off + 2 * H + 3; y++) {         // both fill "images" and rows that wrap
            int64_t k, fin;
            span_cells(seg, (double)y, (double)y_off, (double)W, len, k, fin);
            rows++;
            if (k < fin) nonempty++;
            for (int form = 0; form < 2; form++) {
                int lk, lfin;
                const bool any = form ? span_cells_lean<true>(seg, (double)y, (double)y_off, (double)W, (double)len, lk, lfin)
                                      : span_cells_lean<false>(seg, (double)y, (double)y_off, (double)W, (double)len, lk, lfin);
                bool ok = any == (k < fin) && any == (lk < lfin);
                if (ok && any) ok = lk == k && lfin == fin && span_first_row(y, y_off, H, W, lk) == lk / W;
                if (!ok && bad++ < 10)
                    fprintf(stderr, "MISMATCH form %d W %d H %d y_off %d y %d pts %a %a %a %a %a %a: span_cells [%lld, %lld) lean %d [%d, %d)\n", form, W, H, y_off,
                            y, p[0], p[1], p[2], p[3], p[4], p[5], (long long)k, (long long)fin, (int)any, lk, lfin);
            }
        }
    }
    printf("triangles %ld rows %ld nonempty %ld (%.1f %%) mismatches %ld\n", n_tris, rows, nonempty, 100.0 * (double)nonempty / (double)rows, bad);
    if (bad) return 1;
    if (nonempty * 10 < rows) { fprintf(stderr, "vacuous: fewer than 10 %% of the rows have a span\n"); return 2; }
    return 0;
}
