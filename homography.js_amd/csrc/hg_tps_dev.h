// hg_tps_dev.h -- the one text of the thin-plate rules (include/hgwarp.h, "thin-plate splines") that host and device share: the sizes, the
// layout of a frame's record, the kernel U, the evaluation of a spline at a position and the lattice of the stepped field.  Needs hg_math.h
// only, so a host check can include it.
#pragma once
#include "hg_math.h"

namespace hg {

constexpr int kTpsMaxPoints = 1024;     // HG_TPS_MAX_POINTS
constexpr int kTpsHead = 16;            // doubles in front of a record's points
constexpr int kTpsMaxM = kTpsMaxPoints + 3;
constexpr int kTpsLdsCap = 5184;        // doubles of LDS the solve's matrix may take: M x M stays in LDS while M * M <= this (M <= 72, N <= 69); the tests read this line
constexpr int kTpsSolveBlock = 256;     // lanes of the solve's workgroup, matrix in LDS
constexpr int kTpsSolveBlockBig = 1024; // ... matrix in the caller's scratch
constexpr uint64_t kTpsNaN = 0x7ff8000000000000ull;   // every slot of a failed frame's record

enum : int32_t { kTpsOk = 0, kTpsSingular = 1, kTpsBadInput = 2 };

// One frame of a field call: the window, where its field starts (bytes from d_field) and where its nodes start (bytes from d_scratch).
struct TpsFrame { int32_t x_off, y_off, obj_w, obj_h; uint64_t out_off, node_off; };

// from / to: n_from_sets resp. n_to_sets lists of n_points (x, y) float32; records: F x (16 + 4 n_points) doubles; scratch: F x M x M doubles
// where the matrix does not fit LDS, else unused.
struct TpsSolveArgs {
    const float *from; int n_from_sets; const float *to; int n_to_sets; int n_points, n_frames; double lambda;
    double *records; int32_t *status; double *scratch;
};
// frames: F records on the device; W, H: the source's size; step 1: nodes unused.  (The kernels take records, frames and the output as
// __restrict__ parameters of their own: that is what lets the compiler read the record through scalar loads.)
struct TpsFieldArgs {
    const double *records; int n_points; const TpsFrame *frames; int n_frames, max_w, max_h; int W, H, step; uint8_t *field; uint8_t *nodes;
};

HG_HD int tps_record_doubles(int n_points) { return kTpsHead + 4 * n_points; }
HG_HD bool tps_in_lds(int n_points) { return (n_points + 3) * (n_points + 3) <= kTpsLdsCap; }
HG_HD bool tps_finite(double v) { return fabs(v) < INFINITY; }          // (NaN compares false)

// The natural logarithm of a positive finite q, good to about 2 ulp (measured against the library's over 1e7 values: EXPERIMENTS.md,
// "Thin-plate"), in about half the instructions of the library's: q = m 2^e with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1) by a
// reciprocal with two Newton steps and a corrected quotient, log m = 2 s + s z P(z), z = s s, P = 2/3 + 2 z / 5 + ... + 2 z^8 / 19 (the next
// term is below 3e-17 of the result), and e ln 2 added in two parts.  m - 1 is exact, so the result keeps its relative accuracy around
// q = 1, where e is 0.  Explicit fma: this is the one place of the spline's arithmetic that is not bound to separate roundings.
// +Infinity gives NaN (the sum it would enter is lost either way); NaN stays NaN.
HG_HD double tps_log(double q)
{
    int e;
    double m = frexp(q, &e);                                 // m in [1/2, 1), subnormals included
    if (m < 0.70710678118654752) { m = m + m; e -= 1; }
    const double a = m - 1.0, b = m + 1.0;
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __builtin_amdgcn_rcp(b);
#else
    double r = 1.0 / b;
#endif
    r = fma(fma(-b, r, 1.0), r, r);
    r = fma(fma(-b, r, 1.0), r, r);
    double s = a * r;
    s = fma(fma(-b, s, a), r, s);
    const double z = s * s;
    double p = 2.0 / 19.0;
    p = fma(p, z, 2.0 / 17.0); p = fma(p, z, 2.0 / 15.0); p = fma(p, z, 2.0 / 13.0); p = fma(p, z, 2.0 / 11.0);
    p = fma(p, z, 2.0 / 9.0); p = fma(p, z, 2.0 / 7.0); p = fma(p, z, 2.0 / 5.0); p = fma(p, z, 2.0 / 3.0);
    const double ed = (double)e;
    const double lo = fma(ed, 1.9082149292705877e-10, (s * z) * p);     // ln 2 = 0.693147180369123816490 + 1.9082149292705877e-10: the first part has 32 bits, so e times it is exact
    return fma(ed, 6.93147180369123816490e-01, (s + s) + lo);
}

// U(q) = q log q for q = r^2 (that is r^2 log r^2, twice the textbook kernel), U(0) = 0.
// Written without a branch: q == 0 gives 0 * log(1) = 0, so the log chains of several positions interleave.
HG_HD double tps_u(double q) { return q * tps_log(q > 0.0 ? q : 1.0); }

// The lattice of a stepped field over a window of n pixels along one axis: nodes at k * step, k = 0 .. tps_nodes - 1; the last one lies at or
// beyond the last pixel and there are always two, so every pixel has a node on either side.
HG_HD int tps_nodes(int n, int step) { const int k = (n + step - 2) / step + 1; return k < 2 ? 2 : k; }

// P positions through one record, term by term in index order: every position's chain is its own, so the log chains of the P overlap.  The
// record is read at addresses that do not depend on the lane.  sx = tx + (((a0x + a1x x') + a2x y') + sum_i wx_i U(q_i)), sy alike.
template <int P>
HG_HD void tps_eval(const double *__restrict__ rec, int n_points, const double *X, const double *Y, double *sx, double *sy)
{
    const double cx = rec[0], cy = rec[1], s = rec[2];
    double xn[P], yn[P], ax[P], ay[P];
#pragma unroll
    for (int p = 0; p < P; p++) { xn[p] = (X[p] - cx) * s; yn[p] = (Y[p] - cy) * s; ax[p] = 0.0; ay[p] = 0.0; }
    const double *__restrict__ pt = rec + kTpsHead;
    for (int i = 0; i < n_points; i++) {
        const double dx = pt[4 * i], dy = pt[4 * i + 1], wx = pt[4 * i + 2], wy = pt[4 * i + 3];
#pragma unroll
        for (int p = 0; p < P; p++) {
            const double ex = xn[p] - dx, ey = yn[p] - dy;
            const double u = tps_u(ex * ex + ey * ey);
            ax[p] = ax[p] + wx * u;
            ay[p] = ay[p] + wy * u;
        }
    }
#pragma unroll
    for (int p = 0; p < P; p++) {
        sx[p] = rec[3] + (((rec[8] + rec[10] * xn[p]) + rec[12] * yn[p]) + ax[p]);
        sy[p] = rec[4] + (((rec[9] + rec[11] * xn[p]) + rec[13] * yn[p]) + ay[p]);
    }
}

// A pixel of the stepped field from its four nodes (n00 = row above / left column), fx, fy in [0, 1]: exactly this expression.
HG_HD double tps_blend(double n00, double n01, double n10, double n11, double fx, double fy)
{
    return (n00 * (1.0 - fx) + n01 * fx) * (1.0 - fy) + (n10 * (1.0 - fx) + n11 * fx) * fy;
}

} // namespace hg
