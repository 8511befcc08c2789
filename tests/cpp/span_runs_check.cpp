// span_runs_check.cpp -- the run form of a cached row (hg_span_runs.h): the resolve the build kernel runs, driven lane by lane as the kernel drives
// it, and the window lookup, against a brute-force largest-id scan; tables plus seeded random rows.  Stand-alone: tests/test_span_runs_cpu.py
// builds it under AddressSanitizer + UndefinedBehaviorSanitizer and runs it.  `--over-limit N` answers whether the row of the GPU test
// (one wide span under N separated blocks) exceeds the run limit; `--row W lo hi id ...` checks one row given by position (the capacity rows of
// tests/test_gpu_span_runs_wide.py, as the oracle draws them).
#include "hg_span_runs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace hg;

static long g_checks = 0, g_bad = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_bad++; if (g_bad < 40) std::printf("FAIL %s:%d: %s (row %ld)\n", __FILE__, __LINE__, #cond, g_row); } } while (0)
static long g_row = 0;

constexpr int KS = 14;                                  // the kernel's key: id << KS | slot * 48 | unsafe
struct Span { int lo, hi, id, unsafe; };

struct Resolved { int n = 0; std::vector<uint32_t> runs; };

// The resolve as a wave runs it: phase 1 in every lane, then phase 2 in every lane.  The arrays have exactly the sizes the kernel's have.
static Resolved resolve(const std::vector<Span> &sp, int W)
{
    const int cnt = (int)sp.size();
    std::vector<int> lo(cnt), hi(cnt), key(cnt);
    for (int i = 0; i < cnt; i++) { lo[i] = sp[i].lo; hi[i] = sp[i].hi; key[i] = (sp[i].id << KS) | (i * 48) | sp[i].unsafe; }
    std::vector<uint32_t> cand(kRunCands, 0xdeadbeefu);
    Resolved r;
    r.runs.assign(kRunCap, 0xffffffffu);
    for (int lane = 0; lane < 64; lane++) run_candidates(lo.data(), hi.data(), key.data(), cnt, W, KS, lane, cand.data());
    for (int lane = 0; lane < 64; lane++) {
        const int n = run_place(cand.data(), cnt, lane, r.runs.data());
        if (lane == 0) r.n = n;
        CHECK(n == r.n);                                // the same count in every lane
    }
    return r;
}

static int brute_winner(const std::vector<Span> &sp, int x)      // largest id over the spans that hold x, -1 none
{
    int id = -1;
    for (const Span &s : sp) if (s.lo <= x && x < s.hi && s.id > id) id = s.id;
    return id;
}

// Returns the row's number of runs by brute force; checks everything the resolve and the lookup promise.
static int check_row(const std::vector<Span> &sp, int W)
{
    g_row++;
    const int cnt = (int)sp.size();
    std::vector<int> want(W);
    int brute_runs = 0;
    for (int x = 0; x < W; x++) { want[x] = brute_winner(sp, x); brute_runs += x == 0 || want[x] != want[x - 1]; }
    const Resolved r = resolve(sp, W);
    CHECK(r.n == brute_runs);
    if (r.n > kRunCap) {                                // over the limit: reported, nothing written
        for (uint32_t e : r.runs) CHECK(e == 0xffffffffu);
        return brute_runs;
    }
    const int n = r.n;
    bool dup_ids = false;
    for (int i = 0; i < cnt; i++) for (int j = 0; j < i; j++) dup_ids = dup_ids || sp[i].id == sp[j].id;
    // sorted, disjoint, covering [0, W); adjacent runs differ in winner
    CHECK(n >= 1 && run_ent_start(r.runs[0]) == 0);
    std::vector<int> start(n), rid(n);
    uint64_t unsafe_mask = 0, gap_mask = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t e = r.runs[i];
        CHECK(e != 0xffffffffu && (e & ~kRunEntMask) == 0);
        start[i] = run_ent_start(e);
        CHECK(start[i] < W);
        if (i) CHECK(start[i] > start[i - 1]);
        const int slot = run_ent_slot(e), gap = run_ent_gap(e);
        CHECK(gap || slot < cnt);
        rid[i] = gap ? -1 : sp[slot < cnt ? slot : 0].id;
        if (i) CHECK(rid[i] != rid[i - 1]);
        // unsafe: gaps always; else the OR over the row's slots of the winner's id (sound where two slots of one triangle take turns)
        int u = gap;
        for (const Span &s : sp) if (!gap && s.id == rid[i]) u |= s.unsafe;
        CHECK(run_ent_unsafe(e) == u);
        if (!gap && !dup_ids) CHECK(sp[slot].lo <= start[i] && start[i] < sp[slot].hi);
        unsafe_mask |= (uint64_t)run_ent_unsafe(e) << i;
        gap_mask |= (uint64_t)gap << i;
    }
    for (int i = n; i < kRunCap; i++) CHECK(r.runs[i] == 0xffffffffu);
    // the winner of every pixel
    std::vector<int> run_of(W);
    for (int x = 0, i = 0; x < W; x++) {
        while (i + 1 < n && start[i + 1] <= x) i++;
        run_of[x] = i;
        CHECK(rid[i] == want[x]);
    }
    // the lookup: every window, every lane, every pixel of a lane
    for (int c0 = 0; c0 < W; c0 += 256) {
        int first;
        uint64_t interior;
        run_window(start.data(), n, c0, &first, &interior);
        CHECK(first == run_of[c0]);
        bool px_safe = true, px_empty = true;
        for (int lane = 0; lane < 64; lane++)
            for (int k = 0; k < 4; k++) {
                const int x = c0 + lane + 64 * k, idx = run_index(start.data(), first, interior, x);
                CHECK(idx >= 0 && idx < n);              // (also past the row end: the slot read stays inside the row's block)
                if (x >= W) continue;
                CHECK(idx == run_of[x]);
                px_safe = px_safe && !((unsafe_mask >> run_of[x]) & 1);
                px_empty = px_empty && ((gap_mask >> run_of[x]) & 1);
            }
        CHECK(run_window_safe(unsafe_mask, run_range(first, interior)) == px_safe);
        CHECK(run_window_empty(gap_mask, first, interior) == px_empty);
    }
    return brute_runs;
}

// the GPU test's over-limit row: one wide span of id 0 under `blocks` separated four-pixel blocks of higher ids
static std::vector<Span> blocks_row(int blocks, int W)
{
    std::vector<Span> sp{ {0, W, 0, 0} };
    for (int b = 0; b < blocks; b++) sp.push_back({ 4 + 8 * b, 8 + 8 * b, 1 + b, 0 });
    return sp;
}

static uint32_t g_lcg = 12345u;
static int rnd(int n) { g_lcg = g_lcg * 1664525u + 1013904223u; return (int)((g_lcg >> 8) % (uint32_t)n); }

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "--over-limit")) {
        const int blocks = std::atoi(argv[2]);
        const int n = check_row(blocks_row(blocks, 520), 520);
        std::printf("span_runs_check: spans %d runs %d limit %d failures %ld\n", blocks + 1, n, kRunCap, g_bad);
        return g_bad ? 1 : 0;
    }
    if (argc >= 3 && (argc - 3) % 3 == 0 && !std::strcmp(argv[1], "--row")) {
        const int W = std::atoi(argv[2]);
        std::vector<Span> sp;
        for (int i = 3; i + 2 < argc; i += 3) sp.push_back({ std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), (i / 3) & 1 });
        bool ok = W >= 1 && W <= 65535 && (int)sp.size() <= kRunSpanCap;
        for (const Span &s : sp) ok = ok && 0 <= s.lo && s.lo < s.hi && s.hi <= W && s.id >= 0 && s.id <= 32767;
        if (!ok) { std::printf("span_runs_check: --row takes W and up to %d spans 0 <= lo < hi <= W\n", kRunSpanCap); return 2; }
        const int n = check_row(sp, W);
        std::printf("span_runs_check: spans %d runs %d limit %d failures %ld\n", (int)sp.size(), n, kRunCap, g_bad);
        return g_bad ? 1 : 0;
    }

    // ---- pack / unpack at their limits
    for (int start : {0, 1, 255, 256, 65535}) for (int gap : {0, 1}) {
        const uint32_t w = run_pack_start(start, gap);
        CHECK(run_start(w) == start && run_gap(w) == gap);
    }
    for (int id : {0, 1, 32767}) for (int u : {0, 1}) { const uint32_t w = span_pack_id(id, u); CHECK(span_id(w) == id && span_unsafe_bit(w) == u); }
    for (int start : {0, 65535}) for (int slot : {0, 62}) for (int gap : {0, 1}) for (int u : {0, 1}) {
        const uint32_t e = run_ent(start, slot, gap, u);
        CHECK(run_ent_start(e) == start && run_ent_slot(e) == slot && run_ent_gap(e) == gap && run_ent_unsafe(e) == u && !(e & kRunEntStarts));
    }

    // ---- tables
    CHECK(check_row({}, 1) == 1);                                                       // no span: one gap run
    CHECK(check_row({}, 520) == 1);
    CHECK(check_row({ {0, 520, 3, 0} }, 520) == 1);                                     // one span over the whole row, ending at W
    CHECK(check_row({ {10, 500, 2, 0}, {100, 200, 5, 1} }, 520) == 5);                  // a higher id inside a lower one: the lower is split
    CHECK(check_row({ {100, 200, 2, 0}, {10, 500, 5, 0} }, 520) == 3);                  // the lower one wholly hidden
    CHECK(check_row({ {100, 200, 2, 0}, {100, 200, 5, 0} }, 520) == 3);                 // equal starts and equal ends
    CHECK(check_row({ {0, 100, 1, 0}, {300, 520, 2, 0} }, 520) == 3);                   // a gap in the middle
    CHECK(check_row({ {5, 100, 1, 0}, {300, 515, 2, 0} }, 520) == 5);                   // gaps in the middle and at both ends
    CHECK(check_row({ {0, 1, 1, 0}, {519, 520, 2, 0}, {255, 256, 3, 0} }, 520) == 5);   // spans of one pixel
    CHECK(check_row({ {0, 100, 4, 0}, {50, 200, 4, 1} }, 520) == 2);                    // one triangle twice, overlapping: one run, unsafe
    CHECK(check_row({ {0, 100, 4, 0}, {100, 200, 4, 0} }, 520) == 2);                   // ... abutting: still one run
    CHECK(check_row({ {0, 100, 4, 0}, {100, 200, 5, 0}, {200, 300, 4, 0} }, 300) == 3); // ... on both sides of another
    for (int edge : {255, 256, 257, 64, 63, 65, 511, 512, 513})                         // boundaries on, before and behind window and piece edges
        CHECK(check_row({ {0, edge, 1, 0}, {edge, 600, 2, 1} }, 600) == 2);
    CHECK(check_row({ {0, 600, 1, 0}, {255, 257, 2, 0}, {256, 257, 3, 0} }, 600) == 4);
    {   // 63 abutting spans: 63 runs; with a gap at the end 64: the limit itself
        std::vector<Span> sp;
        for (int i = 0; i < 63; i++) sp.push_back({ 8 * i, 8 * i + 8, i + 1, i & 1 });
        CHECK(check_row(sp, 504) == 63);
        CHECK(check_row(sp, 505) == 64);
        sp[0].lo = 1;                                                                   // and a gap in front: one over
        CHECK(check_row(sp, 505) == 65);
    }
    CHECK(check_row(blocks_row(31, 520), 520) == 63);
    CHECK(check_row(blocks_row(32, 520), 520) == 65);                                   // fewer than 64 spans, more runs than the limit
    CHECK(check_row(blocks_row(40, 520), 520) == 81);
    {   // 63 separated one-pixel spans: 127 runs, every candidate position in use
        std::vector<Span> sp;
        for (int i = 0; i < 63; i++) sp.push_back({ 2 * i + 1, 2 * i + 2, 63 - i, 0 });
        CHECK(check_row(sp, 600) == 127);
    }

    // ---- seeded random rows: 0 .. 63 spans, overlapping and nested, duplicate ids, shared starts and ends, one-pixel spans, spans ending at W
    for (int it = 0; it < 1500; it++) {
        const int W = 1 + rnd(it % 3 == 0 ? 40 : 600), cnt = rnd(it % 5 == 0 ? 64 : 12), ids = 1 + rnd(it % 2 ? 8 : 200);
        std::vector<Span> sp;
        for (int i = 0; i < cnt; i++) {
            int lo = rnd(W), hi;
            if (i && rnd(4) == 0) lo = sp[rnd(i)].lo;                                   // an equal start
            switch (rnd(6)) {
            case 0: hi = W; break;                                                      // ends at W
            case 1: hi = lo + 1; break;                                                 // one pixel
            case 2: hi = i ? sp[rnd(i)].hi : W; break;                                  // an equal end
            default: hi = lo + 1 + rnd(W - lo); break;
            }
            if (hi <= lo) hi = lo + 1;
            sp.push_back({ lo, hi, rnd(ids), rnd(3) == 0 });
        }
        check_row(sp, W);
    }

    std::printf("span_runs_check: checks %ld failures %ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
