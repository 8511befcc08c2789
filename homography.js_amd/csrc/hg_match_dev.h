// hg_match_dev.h -- the one text of the matching rules (include/hgwarp.h, "matching descriptors") that the three kernels of hg_k_match.hip
// share: the tile sizes, the byte mask that keeps a row's padding out of a distance, the running two-nearest record with its merge -- a
// total order, so any tiling and any fold order give the same record --, its packed in-lane form, and the acceptance tests.  Needs
// hg_math.h only, so a host check can include it.
#pragma once
#include "hg_math.h"

namespace hg {

constexpr int kMatchTQ = 64;            // queries per workgroup of k_match_bits / k_match_u8 (a tile of one frame); the tests read this line
constexpr int kMatchTT = 64;            // train rows per LDS tile of both kernels; the tests read this line
constexpr int kMatchFinishBlock = 256;  // lanes of k_match_finish: queries per scan step
constexpr uint32_t kMatchNone = 0xffffffffu;   // "no distance yet": above every distance (at most 512 * 255 * 255 < 2^25)

// The bytes of the 32-bit word at byte offset `off` of a row that are data (below desc_bytes), as a mask over the little-endian word.
HG_HD uint32_t match_word_mask(int desc_bytes, int off)
{
    const int v = desc_bytes - off;
    return v >= 4 ? 0xffffffffu : (v <= 0 ? 0u : ((1u << (8 * v)) - 1u));
}

// The two nearest of the rows seen so far: d1 the smallest distance, j1 the LOWEST row that attains it, d2 the second entry of the ascending
// multiset of distances (kMatchNone while fewer than two rows were seen; j1 = -1 and d1 = kMatchNone before the first).
struct MatchTop2 { uint32_t d1; int32_t j1; uint32_t d2; };

HG_HD MatchTop2 match_top2_empty() { return MatchTop2{kMatchNone, -1, kMatchNone}; }
HG_HD MatchTop2 match_top2_one(uint32_t d, int32_t j) { return MatchTop2{d, j, kMatchNone}; }

// a := the two nearest of the union of what a and b have seen (disjoint sets of rows).  The nearest is the minimum of (d1, j1) in
// lexicographic order; the second distance is the second of {a.d1, a.d2, b.d1, b.d2}, of which a.d1 <= a.d2 and b.d1 <= b.d2 are known:
// min(max(a.d1, b.d1), min(a.d2, b.d2)).  Commutative and associative: the order of the folds does not matter.
HG_HD void match_merge(MatchTop2 &a, const MatchTop2 &b)
{
    const uint32_t hi1 = a.d1 > b.d1 ? a.d1 : b.d1, lo2 = a.d2 < b.d2 ? a.d2 : b.d2;
    const bool take_b = b.d1 < a.d1 || (b.d1 == a.d1 && (uint32_t)b.j1 < (uint32_t)a.j1);      // (j1 = -1 is above every row)
    a.d2 = hi1 < lo2 ? hi1 : lo2;
    if (take_b) { a.d1 = b.d1; a.j1 = b.j1; }
}

// A lane's running two nearest as packed words k = (d << shift) | j, j below 2^shift: rows differ in j, so the words differ, and the smaller
// word is the smaller (d, j) in lexicographic order -- the nearest is the smallest word, d2 the distance of the second smallest.  Three
// operations per row (a minimum and a median of three) where match_merge takes eight.  The words must stay below kMatchNone: bits use
// shift 16 over all train rows (d <= 4096), bytes shift 6 within one tile (d < 2^25).
struct MatchKeys2 { uint32_t k1, k2; };                        // k1 <= k2

HG_HD MatchKeys2 match_keys2_empty() { return MatchKeys2{kMatchNone, kMatchNone}; }
HG_HD void match_push(MatchKeys2 &t, uint32_t k)
{
    const uint32_t lo = t.k1 < k ? t.k1 : k, hi = t.k1 < k ? k : t.k1;
    t.k2 = t.k2 < hi ? t.k2 : hi;                                // (the median of k1 <= k2 and k)
    t.k1 = lo;
}
// The record of the words pushed, j0 added to their row numbers.
HG_HD MatchTop2 match_unpack(const MatchKeys2 &t, int shift, int32_t j0)
{
    MatchTop2 r = match_top2_empty();
    if (t.k1 != kMatchNone) { r.d1 = t.k1 >> shift; r.j1 = j0 + (int32_t)(t.k1 & ((1u << shift) - 1u)); }
    if (t.k2 != kMatchNone) r.d2 = t.k2 >> shift;
    return r;
}

// The word a train row keeps of its best query: the smallest (d, i) in lexicographic order is the smallest word, whoever offers it first.
HG_HD unsigned long long match_key(uint32_t d, uint32_t i) { return ((unsigned long long)d << 32) | (unsigned long long)i; }

// The distance cap and the ratio test of a query whose two nearest are t, over ct >= 1 train rows.  rr = ratio for HG_DESC_BITS, ratio * ratio
// (rounded once, on the host) for HG_DESC_U8; ratio_on = 0 switches the test off; with ct == 1 there is no second distance and it passes.
HG_HD bool match_passes(const MatchTop2 &t, int ct, uint32_t max_distance, int ratio_on, double rr)
{
    if (t.d1 > max_distance) return false;
    if (ratio_on && ct >= 2) return (double)t.d1 < rr * (double)t.d2;
    return true;
}

} // namespace hg
