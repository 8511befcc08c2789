// hg_span_runs.h -- the run form of a cached row: the build of the span cache turns the overlapping spans the self-span prologue
// left in a row's LDS block into disjoint runs, sorted by start, covering [0, W), each with its winner -- the largest triangle id, the last writer
// of :852-858 -- or none (a gap run).  A pixel's run is then found by counting run starts instead of testing every span that reaches its window.
// Here: the record words, the resolve (plain functions over the row's arrays, one call per lane and phase: the kernel calls them from 64 lanes, a
// host program for lanes 0 .. 63 in turn) and the window lookup.  Plain C++, no runtime: tests/cpp/span_runs_check.cpp drives it.
#pragma once
#include "hg_span_cache.h"

namespace hg {

constexpr int kRunCap = 64;                     // runs of a row: one per lane of the wave that walks it (and one LDS record slot each)
constexpr int kRunSpanCap = 63;                 // spans of a row the resolve takes (the packed block's capacity): lane 63 holds candidate position 0
constexpr int kRunCands = 2 * 64;               // candidate positions: lane i < cnt has lo[i] and hi[i] (if < W), lane 63 has 0

// ------------------------------------------------------------------------------------------------ record words
// A run record has the size of a span record (kSpanRecWords*) and the same words 1 and 2; word 0 is
//   start | gap << 16 (cells [start, next run's start) of the row; start <= 65535), id << 1 | unsafe bit (span_pack_id), m0, m1
// A gap run has no triangle: id 0, unsafe, and NaN in every matrix entry -- its record IS the row's "no triangle" record.
HG_SC_FN uint32_t run_pack_start(int start, int gap) { return (uint32_t)start | ((uint32_t)(gap & 1) << 16); }
HG_SC_FN int run_start(uint32_t w) { return (int)(w & 0xffffu); }
HG_SC_FN int run_gap(uint32_t w) { return (int)((w >> 16) & 1u); }

// A run in the resolve's LDS lists: start | slot << 16 | gap << 22 | unsafe << 23 (slot: the winner's slot in the row's block, 0 .. 62);
// a candidate also has bit 24 "starts a run".
HG_SC_FN uint32_t run_ent(int start, int slot, int gap, int unsafe) { return (uint32_t)start | ((uint32_t)slot << 16) | ((uint32_t)gap << 22) | ((uint32_t)unsafe << 23); }
HG_SC_FN int run_ent_start(uint32_t e) { return (int)(e & 0xffffu); }
HG_SC_FN int run_ent_slot(uint32_t e) { return (int)((e >> 16) & 63u); }
HG_SC_FN int run_ent_gap(uint32_t e) { return (int)((e >> 22) & 1u); }
HG_SC_FN int run_ent_unsafe(uint32_t e) { return (int)((e >> 23) & 1u); }
constexpr uint32_t kRunEntStarts = 1u << 24, kRunEntMask = kRunEntStarts - 1;

// ------------------------------------------------------------------------------------------------ the resolve (build time; all pairs: it runs once per frame set)
// lo, hi, key: the row's slots [0, cnt), cnt <= kRunSpanCap, 0 <= lo < hi <= W; key = id << ks | low bits, bit 0 the span's unsafe bit.
// The slots of the largest keys among the spans that hold cell x (*at) and cell x - 1 (*before), -1 where none does: one pass over the row.
HG_SC_FN void run_winners(const int *lo, const int *hi, const int *key, int cnt, int x, int *at, int *before)
{
    int a = -1, ak = 0, b = -1, bk = 0;
    for (int i = 0; i < cnt; i++) {
        const int l = lo[i], h = hi[i], k = key[i];
        if (l <= x && x < h && (a < 0 || k > ak)) { a = i; ak = k; }
        if (l < x && x <= h && (b < 0 || k > bk)) { b = i; bk = k; }
    }
    *at = a; *before = b;
}

// candidate c of the row: its position, false if it has none
HG_SC_FN bool run_cand_pos(const int *lo, const int *hi, int cnt, int W, int c, int *pos)
{
    const int i = c >> 1;
    if (i < cnt) { *pos = (c & 1) ? hi[i] : lo[i]; return *pos < W; }
    *pos = 0;
    return c == 2 * 63;
}

// Phase 1, lane `lane`: its two candidates.  A candidate starts a run when the winner at it differs (by triangle id) from the winner one cell
// before it and no earlier candidate has the same position.  A run's unsafe bit is the OR over every slot of the winner's id in the row: two
// slots of one triangle hold the same record, either may win, and the run may continue under the other.
HG_SC_FN void run_candidates(const int *lo, const int *hi, const int *key, int cnt, int W, int ks, int lane, uint32_t *cand)
{
    for (int b = 0; b < 2; b++) {
        const int c = 2 * lane + b;
        int pos;
        uint32_t e = 0;
        if (run_cand_pos(lo, hi, cnt, W, c, &pos)) {
            int wa, wb;
            run_winners(lo, hi, key, cnt, pos, &wa, &wb);
            const int ida = wa < 0 ? -1 : key[wa] >> ks;
            const int idb = pos == 0 ? -2 : wb < 0 ? -1 : key[wb] >> ks;       // (cell 0 always starts a run)
            if (ida != idb) {                                   // (the winners first: most candidates of a crowded row end here)
                bool dup = false;
                const int c_end = c < 2 * cnt ? c : 2 * cnt;    // (earlier candidates: slots' ends; position 0 is the last one)
                for (int c2 = 0; c2 < c_end && !dup; c2++) {
                    int p2;
                    dup = run_cand_pos(lo, hi, cnt, W, c2, &p2) && p2 == pos;
                }
                if (!dup) {
                    int unsafe = wa < 0 ? 1 : 0;
                    for (int i = 0; i < cnt; i++) unsafe |= ((key[i] >> ks) == ida) ? (key[i] & 1) : 0;
                    e = run_ent(pos, wa < 0 ? 0 : wa, wa < 0 ? 1 : 0, unsafe) | kRunEntStarts;
                }
            }
        }
        cand[c] = e;
    }
}

// Phase 2, lane `lane`, once every lane's phase 1 is visible: a run's place is the number of run starts below it.  Returns the row's number of
// runs (the same in every lane); beyond kRunCap nothing is written and the row stays in span form.  (Candidates live in [0, 2 cnt) and at 2 * 63.)
HG_SC_FN int run_place(const uint32_t *cand, int cnt, int lane, uint32_t *runs)
{
    const uint32_t zero = cand[2 * 63];                 // position 0: always a start, below every other
    int n = (zero & kRunEntStarts) ? 1 : 0;
    for (int c = 0; c < 2 * cnt; c++) n += (cand[c] & kRunEntStarts) ? 1 : 0;
    if (n > kRunCap) return n;
    for (int b = 0; b < 2; b++) {
        const uint32_t e = cand[2 * lane + b];
        if (!(e & kRunEntStarts)) continue;
        int rank = (2 * lane + b != 2 * 63 && (zero & kRunEntStarts) && run_ent_start(e) > 0) ? 1 : 0;
        for (int c = 0; c < 2 * cnt; c++) rank += ((cand[c] & kRunEntStarts) && run_ent_start(cand[c]) < run_ent_start(e)) ? 1 : 0;
        runs[rank] = e & kRunEntMask;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------ the lookup (use time)
// Window [c0, c0 + 256) of a row with run starts start[0 .. nruns): the run that holds c0, and the mask of the runs that start inside the
// window behind c0.  (The kernel: lane i keeps start[i], two ballots.)
HG_SC_FN void run_window(const int *start, int nruns, int c0, int *first, uint64_t *interior)
{
    uint64_t le = 0, lt = 0;
    for (int i = 0; i < nruns; i++) {
        le |= (uint64_t)(start[i] <= c0) << i;
        lt |= (uint64_t)(start[i] < c0 + 256) << i;
    }
    *first = __builtin_popcountll(le) - 1;
    *interior = lt & ~le;
}
// the run of cell x of that window: first + the number of interior run starts s <= x
HG_SC_FN int run_index(const int *start, int first, uint64_t interior, int x)
{
    int idx = first;
    for (uint64_t m = interior; m; m &= m - 1) idx += x >= start[__builtin_ctzll(m)] ? 1 : 0;
    return idx;
}
// Every run that overlaps a window owns at least one of its cells: the window's decisions are those of its runs.
HG_SC_FN uint64_t run_range(int first, uint64_t interior) { return interior | ((uint64_t)1 << first); }
HG_SC_FN bool run_window_safe(uint64_t unsafe_mask, uint64_t range) { return (unsafe_mask & range) == 0; }     // unsafe_mask: the unsafe bits of the row's runs (gaps are unsafe)
HG_SC_FN bool run_window_empty(uint64_t gap_mask, int first, uint64_t interior) { return interior == 0 && ((gap_mask >> first) & 1) != 0; }

} // namespace hg
