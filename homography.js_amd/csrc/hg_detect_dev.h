// hg_detect_dev.h -- the one text of the keypoint rules (include/hgwarp.h, "detecting and describing keypoints") that the three kernels of
// hg_k_detect.hip and the host (hg_describe_pattern, hg_detect_layout) share: the luma, the Harris response in integers, the total order of
// the candidates, the direction table with the bin choice, and the rule that generates the sampling pattern.  Integer arithmetic only.
// Needs hg_math.h only, so a host check can include it.
#pragma once
#include "hg_math.h"

namespace hg {

constexpr int kDetectMargin = 16;       // a keypoint keeps this distance from every border of its plane
constexpr int kDetectBins = 32;         // direction bins
constexpr int kDetectTests = 256;       // bits of a descriptor
constexpr int kDetectTile = 32;         // k_detect_cells: side of a sub-tile of a cell; the tests read this line
constexpr int kDetectBlock = 256;       // lanes of k_detect_cells (one 2 x 2 block of a sub-tile each) and of k_detect_compact
constexpr int kDetectMaxPerCell = 16;
constexpr int kDetectDiscR = 15;        // radius of the orientation disc: the deepest reach of the feature

// L of an interleaved RGBA pixel (alpha ignored).
HG_HD int32_t detect_luma(uint32_t r, uint32_t g, uint32_t b) { return (int32_t)((77u * r + 150u * g + 29u * b + 128u) >> 8); }

// Harris with k = 1 / 16 from the window sums A = sum Ix Ix, C = sum Iy Iy, B = sum Ix Iy (each below 2^26 in magnitude): |R| < 2^56.
HG_HD int64_t detect_response(int32_t A, int32_t C, int32_t B)
{
    const int64_t a = A, c = C, b = B;
    return 16 * (a * c - b * b) - (a + c) * (a + c);
}

// The total order of the candidates: larger R first, among equal R the lower flat index.
HG_HD bool detect_beats(int64_t ra, int32_t ia, int64_t rb, int32_t ib) { return ra > rb || (ra == rb && ia < ib); }

// cos of bin k in Q14 (k taken mod 32); sin of bin k = cos of bin k + 24.
HG_HD int32_t detect_cos(int k)
{
    k &= 31;
    if (k > 16) k = 32 - k;                                      // c_{32 - k} = c_k
    const bool neg = k > 8;
    if (neg) k = 16 - k;                                         // c_{16 - k} = -c_k
    const int32_t c = k == 0 ? 16384 : k == 1 ? 16069 : k == 2 ? 15137 : k == 3 ? 13623 : k == 4 ? 11585 : k == 5 ? 9102 : k == 6 ? 6270 : k == 7 ? 3196 : 0;
    return neg ? -c : c;
}
HG_HD int32_t detect_sin(int k) { return detect_cos(k + 24); }

// The bin of the intensity centroid (m10, m01): the k that maximises m10 c_k + m01 s_k, the lowest k among equals (a flat patch: 0).
HG_HD int detect_bin(int32_t m10, int32_t m01)
{
    int best = 0;
    int64_t best_v = (int64_t)m10 * detect_cos(0) + (int64_t)m01 * detect_sin(0);
    for (int k = 1; k < kDetectBins; k++) {
        const int64_t v = (int64_t)m10 * detect_cos(k) + (int64_t)m01 * detect_sin(k);
        if (v > best_v) { best_v = v; best = k; }
    }
    return best;
}

HG_HD uint32_t detect_mix(uint32_t a)
{
    a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
    return a;
}

// The point a word of the walk proposes: two sums of four 3-bit fields, each -14..14; false when it lies outside the disc of radius 12.
HG_HD bool detect_walk_point(uint32_t w, int &x, int &y)
{
    x = (int)((w & 7u) + ((w >> 3) & 7u) + ((w >> 6) & 7u) + ((w >> 9) & 7u)) - 14;
    y = (int)(((w >> 12) & 7u) + ((w >> 15) & 7u) + ((w >> 18) & 7u) + ((w >> 21) & 7u)) - 14;
    return x * x + y * y <= 144;
}

// Test b of the base pattern: {ax, ay, bx, by}.
HG_HD void detect_base_test(int b, int8_t out[4])
{
    const uint32_t key = detect_mix(detect_mix(0x9e3779b9u) + (uint32_t)b);
    int ax = 0, ay = 0, x, y;
    bool have_a = false;
    for (uint32_t t = 0;; t++) {
        if (!detect_walk_point(detect_mix(key + t), x, y)) continue;
        if (!have_a) { ax = x; ay = y; have_a = true; continue; }
        if (x == ax && y == ay) continue;
        out[0] = (int8_t)ax; out[1] = (int8_t)ay; out[2] = (int8_t)x; out[3] = (int8_t)y;
        return;
    }
}

// A pattern point under bin k, with arithmetic shifts: every result lies in -12..12.
HG_HD void detect_rotate(int x, int y, int k, int8_t &ox, int8_t &oy)
{
    const int32_t c = detect_cos(k), s = detect_sin(k);
    ox = (int8_t)((x * c - y * s + 8192) >> 14);
    oy = (int8_t)((x * s + y * c + 8192) >> 14);
}

} // namespace hg
