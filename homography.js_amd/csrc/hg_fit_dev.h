// hg_fit_dev.h -- the one text of the fitting rules (include/hgwarp.h, "fitting transforms to matches") that host and device share: the
// sample draw (hg_fit_sample_indices computes it on the host, k_fit_hypotheses on the device), the validity of a sample, the minimal solve and
// the inlier test.  Needs hg_math.h only, so a host check can include it.
#pragma once
#include "hg_math.h"

namespace hg {

constexpr int kFitTile = 256;           // matches per LDS tile of k_fit_score (one per lane of its workgroup); the tests read this line
constexpr int kFitHypBlock = 256;       // hypotheses per workgroup of k_fit_score
constexpr int kFitDraws = 16;           // draws per hypothesis before it is given up

HG_HD int fit_k(int kind) { return kind == 1 ? 4 : 3; }

HG_HD uint32_t fit_mix(uint32_t a)
{
    a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
    return a;
}

// The K distinct indices of hypothesis h of frame f, drawn by the header's rule; false (and -1 everywhere) when count < K or the 16 draws
// hold fewer than K distinct values.  idx[3] = -1 for affine.
HG_HD bool fit_draw(int K, uint32_t seed, uint32_t f, uint32_t h, int32_t count, int32_t idx[4])
{
    idx[0] = idx[1] = idx[2] = idx[3] = -1;
    if (count < K) return false;
    const uint32_t k = fit_mix(fit_mix(fit_mix(seed + 0x9e3779b9u) + f) + h);
    int got = 0;
    for (int t = 0; t < kFitDraws && got < K; t++) {
        const int32_t i = (int32_t)(uint32_t)(((uint64_t)fit_mix(k + (uint32_t)t) * (uint64_t)(uint32_t)count) >> 32);
        const bool seen = (got > 0 && idx[0] == i) || (got > 1 && idx[1] == i) || (got > 2 && idx[2] == i);
        if (seen) continue;
        if (got == 0) idx[0] = i; else if (got == 1) idx[1] = i; else if (got == 2) idx[2] = i; else idx[3] = i;
        got++;
    }
    if (got < K) { idx[0] = idx[1] = idx[2] = idx[3] = -1; return false; }
    return true;
}

// Caller-given indices: every one of the first K inside [0, count), no two equal.
HG_HD bool fit_sample_ok(int K, const int32_t idx[4], int32_t count)
{
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        if (a >= K) continue;
        ok = ok && idx[a] >= 0 && idx[a] < count;
#pragma unroll
        for (int b = 0; b < 4; b++) if (b < a) ok = ok && idx[a] != idx[b];
    }
    return ok;
}

HG_HD bool fit_finite(double v) { return fabs(v) < INFINITY; }           // (NaN compares false)

// The minimal solve on K matches (x, y, u, v), from -> to: solve_projective_regs resp. solve_affine widened (slots 6, 7 = 0).  false when any
// entry is not finite (collinear or coincident points).
HG_HD bool fit_minimal(int kind, const float *s, const float *d, double m[8])
{
    if (kind == 1) {
        solve_projective_regs(s, d, m);
    } else {
        float o[6];
        solve_affine(s, d, o);
#pragma unroll
        for (int k = 0; k < 6; k++) m[k] = o[k];
        m[6] = 0.0; m[7] = 0.0;
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) ok = ok && fit_finite(m[k]);
    return ok;
}

// A match with a coordinate that is not finite is never an inlier: its x becomes NaN where it is staged, so that e below is NaN.
HG_HD bool fit_match_finite(float x, float y, float u, float v)
{
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(u) < INFINITY && fabsf(v) < INFINITY;
}

// e = (px - u)(px - u) + (py - v)(py - v) <= thr2, every step rounded on its own (contraction is off); NaN is no inlier.
template <int KIND>
HG_HD bool fit_inlier(const double *m, float x, float y, float u, float v, double thr2)
{
    double px, py;
    if (KIND == 1) apply_projective(m, (double)x, (double)y, px, py); else apply_affine(m, (double)x, (double)y, px, py);
    const double dx = px - (double)u, dy = py - (double)v;
    const double e = (dx * dx) + (dy * dy);
    return e <= thr2;
}

} // namespace hg
