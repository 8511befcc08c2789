// hg_align_dev.h -- the one text of the alignment rules (include/hgwarp.h, "refining transforms on the pixels") that host and device share:
// the normalisation of a matrix and its way back, the pass's arithmetic for one sample (warp, validity, the 12 taps, residual, Jacobian
// row), the solve, the displacement of the rectangle's corners and the level conversion of hg_align_scale_matrix.  Needs hg_math.h only, so a
// host check can include it.
#pragma once
#include "hg_math.h"

namespace hg {

constexpr int kAlignChunk = 8192;       // samples per workgroup of k_align_accumulate (32 per lane); the tests read this line
constexpr int kAlignBlock = 256;        // lanes per workgroup of both kernels
constexpr int kAlignSums = 66;          // doubles of a pass's record at P = 10: 55 of the triangle, 10 of J^T r, sum r r
constexpr int kAlignRec = kAlignSums + 1;   // a chunk's partial record: the sums, then the valid count (a double: exact)

HG_HD int align_p(int kind, int photometric) { return (kind == 1 ? 8 : 6) + (photometric ? 2 : 0); }
HG_HD bool align_finite(double v) { return fabs(v) < INFINITY; }           // (NaN compares false)

// c = ((W - 1) / 2, (H - 1) / 2), s = 2 / max(W, H) of both sides, and the corners of the sample rectangle.
struct AlignGeom {
    double cfx, cfy, sf, ctx, cty, st;
    double x0, y0, x1, y1;              // rx, ry, rx + rw - 1, ry + rh - 1
};

HG_HD AlignGeom align_geom(int Wf, int Hf, int Wt, int Ht, int rx, int ry, int rw, int rh)
{
    AlignGeom g;
    g.cfx = (double)(Wf - 1) / 2.0; g.cfy = (double)(Hf - 1) / 2.0; g.sf = 2.0 / (double)(Wf > Hf ? Wf : Hf);
    g.ctx = (double)(Wt - 1) / 2.0; g.cty = (double)(Ht - 1) / 2.0; g.st = 2.0 / (double)(Wt > Ht ? Wt : Ht);
    g.x0 = (double)rx; g.y0 = (double)ry; g.x1 = (double)(rx + rw - 1); g.y1 = (double)(ry + rh - 1);
    return g;
}

// The 3 x 3 row-major form of a matrix in the fit's layouts (projective h0..h7, h8 = 1; affine x' = m0 x + m2 y + m4, y' = m1 x + m3 y + m5).
HG_HD void align_to3x3(int kind, const double *m, double *a)
{
    if (kind == 1) { for (int k = 0; k < 8; k++) a[k] = m[k]; a[8] = 1.0; }
    else { a[0] = m[0]; a[1] = m[2]; a[2] = m[4]; a[3] = m[1]; a[4] = m[3]; a[5] = m[5]; a[6] = 0.0; a[7] = 0.0; a[8] = 1.0; }
}

// H' = T_to M T_from^-1 divided through by its last entry: h[0..7], row-major (h[8] == 1; affine: h[6] = h[7] = 0 exactly).
HG_HD void align_normalise(int kind, const double *m, const AlignGeom &g, double *h)
{
    double a[9], b[9];
    align_to3x3(kind, m, a);
    for (int r = 0; r < 3; r++) {                              // M T_from^-1, T_from^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1]
        b[3 * r + 0] = a[3 * r + 0] / g.sf;
        b[3 * r + 1] = a[3 * r + 1] / g.sf;
        b[3 * r + 2] = ((a[3 * r + 0] * g.cfx) + (a[3 * r + 1] * g.cfy)) + a[3 * r + 2];
    }
    for (int c = 0; c < 3; c++) {                              // T_to ., T_to = [s 0 -s cx; 0 s -s cy; 0 0 1]
        a[0 + c] = (b[0 + c] - (g.ctx * b[6 + c])) * g.st;
        a[3 + c] = (b[3 + c] - (g.cty * b[6 + c])) * g.st;
        a[6 + c] = b[6 + c];
    }
    for (int k = 0; k < 8; k++) h[k] = a[k] / a[8];
    if (kind != 1) { h[6] = 0.0; h[7] = 0.0; }
}

// M = T_to^-1 H' T_from divided through by its last entry, in the input's layout (affine: slots 6 and 7 zero).
HG_HD void align_denormalise(int kind, const double *h, const AlignGeom &g, double *m)
{
    double gt[9], hm[9];
    for (int r = 0; r < 3; r++) {
        const double h0 = h[3 * r + 0], h1 = h[3 * r + 1], h2 = r == 2 ? 1.0 : h[3 * r + 2];
        gt[3 * r + 0] = h0 * g.sf;
        gt[3 * r + 1] = h1 * g.sf;
        gt[3 * r + 2] = (h2 - (h0 * (g.sf * g.cfx))) - (h1 * (g.sf * g.cfy));
    }
    for (int c = 0; c < 3; c++) {
        hm[0 + c] = (gt[0 + c] / g.st) + (g.ctx * gt[6 + c]);
        hm[3 + c] = (gt[3 + c] / g.st) + (g.cty * gt[6 + c]);
        hm[6 + c] = gt[6 + c];
    }
    if (kind == 1) {
        for (int k = 0; k < 8; k++) m[k] = hm[k] / hm[8];
    } else {
        m[0] = hm[0]; m[2] = hm[1]; m[4] = hm[2]; m[1] = hm[3]; m[3] = hm[4]; m[5] = hm[5]; m[6] = 0.0; m[7] = 0.0;
    }
}

// The image in TO pixels of the FROM pixel (x, y) under the normalised iterate h: steps 1 and 2 of the pass.  D comes back too.
template <int KIND>
HG_HD void align_warp(const double *h, const AlignGeom &g, double x, double y, double &xn, double &yn, double &D, double &un, double &vn, double &u, double &v)
{
    xn = (x - g.cfx) * g.sf;
    yn = (y - g.cfy) * g.sf;
    D = KIND == 1 ? ((h[6] * xn) + (h[7] * yn)) + 1.0 : 1.0;
    un = (((h[0] * xn) + (h[1] * yn)) + h[2]) / D;
    vn = (((h[3] * xn) + (h[4] * yn)) + h[5]) / D;
    u = (un / g.st) + g.ctx;
    v = (vn / g.st) + g.cty;
}

HG_HD bool align_valid(double u, double v, double D, int Wt, int Ht)
{
    return align_finite(u) && align_finite(v) && D > 0.0 && u >= 1.0 && u < (double)(Wt - 2) && v >= 1.0 && v < (double)(Ht - 2);
}

HG_HD double align_blend(double p00, double p01, double p10, double p11, double fx, double fy)
{
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    return (((p00 * gx) + (p01 * fx)) * gy) + (((p10 * gx) + (p11 * fx)) * fy);
}

// Steps 4 and 5 at a VALID (u, v) of a luma plane of row length Wt: I and the central differences in TO pixels (12 taps: the 4 x 4 block
// around (floor u, floor v) without its corners).
HG_HD void align_taps(const uint8_t *__restrict__ to, int Wt, double u, double v, double &I, double &dx, double &dy)
{
    const double fu = floor(u), fv = floor(v);
    const double fx = u - fu, fy = v - fv;
    const int x0 = (int)fu, y0 = (int)fv;
    const uint8_t *r0 = to + (size_t)(y0 - 1) * (size_t)Wt + (size_t)(x0 - 1), *r1 = r0 + Wt, *r2 = r1 + Wt, *r3 = r2 + Wt;
    const double a1 = r0[1], a2 = r0[2];
    const double b0 = r1[0], b1 = r1[1], b2 = r1[2], b3 = r1[3];
    const double c0 = r2[0], c1 = r2[1], c2 = r2[2], c3 = r2[3];
    const double d1 = r3[1], d2 = r3[2];
    I = align_blend(b1, b2, c1, c2, fx, fy);
    dx = (align_blend(b2, b3, c2, c3, fx, fy) - align_blend(b0, b1, c0, c1, fx, fy)) / 2.0;
    dy = (align_blend(c1, c2, d1, d2, fx, fy) - align_blend(a1, a2, b1, b2, fx, fy)) / 2.0;
}

// Steps 5 to 7 from the taps: the residual and the Jacobian row J[0 .. P) of a valid sample with FROM luma a.
template <int KIND, int PHOTO>
HG_HD void align_row(const AlignGeom &g, double a, double gain, double bias, double xn, double yn, double D, double un, double vn, double I, double dx, double dy,
                     double &r, double *J)
{
    const double jx = (dx / g.st) / D, jy = (dy / g.st) / D;
    r = PHOTO ? ((gain * a) + bias) - I : a - I;
    if (KIND == 1) {
        const double w = -((jx * un) + (jy * vn));
        J[0] = jx * xn; J[1] = jx * yn; J[2] = jx; J[3] = jy * xn; J[4] = jy * yn; J[5] = jy; J[6] = w * xn; J[7] = w * yn;
    } else {
        J[0] = jx * xn; J[1] = jy * xn; J[2] = jx * yn; J[3] = jy * yn; J[4] = jx; J[5] = jy;
    }
    if (PHOTO) { J[KIND == 1 ? 8 : 6] = -a; J[KIND == 1 ? 9 : 7] = -1.0; }
}

// Parameter k of the update -> its slot in the row-major normalised iterate (affine: the affine slot order m0..m5).
HG_HD int align_slot(int kind, int k)
{
    if (kind == 1) return k;
    return k == 0 ? 0 : k == 1 ? 3 : k == 2 ? 1 : k == 3 ? 4 : k == 4 ? 2 : 5;
}

// Gaussian elimination with partial pivoting (first row with the largest magnitude) on the n x (n + 1) augmented system A (row stride ld),
// in one lane; the solution replaces the right-hand side.  A zero pivot leaves values that are not finite.  (The refit's routine.)
HG_HD void align_gauss(double *A, int n, int ld)
{
    for (int k = 0; k < n; k++) {
        int pk = k;
        double bestv = fabs(A[k * ld + k]);
        for (int j = k + 1; j < n; j++) { const double v = fabs(A[j * ld + k]); if (bestv < v) { bestv = v; pk = j; } }
        if (pk != k) for (int j = 0; j < n + 1; j++) { const double t = A[k * ld + j]; A[k * ld + j] = A[pk * ld + j]; A[pk * ld + j] = t; }
        const double akk = A[k * ld + k];
        for (int i = k + 1; i < n; i++) {
            const double l = A[i * ld + k] / akk;
            for (int j = k + 1; j < n + 1; j++) A[i * ld + j] -= l * A[k * ld + j];
        }
    }
    for (int i = n - 1; i >= 0; i--) {
        double x = A[i * ld + n];
        for (int j = i + 1; j < n; j++) x -= A[i * ld + j] * A[j * ld + n];
        A[i * ld + n] = x / A[i * ld + i];
    }
}

// The largest distance, in TO pixels, between the images of the rectangle's four corners under the normalised iterates ha and hb.
HG_HD double align_displacement(int kind, const double *ha, const double *hb, const AlignGeom &g)
{
    double best = 0.0;
    for (int k = 0; k < 4; k++) {
        const double x = (k & 1) ? g.x1 : g.x0, y = (k & 2) ? g.y1 : g.y0;
        double xn, yn, D, un, vn, ua, va, ub, vb;
        if (kind == 1) { align_warp<1>(ha, g, x, y, xn, yn, D, un, vn, ua, va); align_warp<1>(hb, g, x, y, xn, yn, D, un, vn, ub, vb); }
        else { align_warp<0>(ha, g, x, y, xn, yn, D, un, vn, ua, va); align_warp<0>(hb, g, x, y, xn, yn, D, un, vn, ub, vb); }
        const double du = ua - ub, dv = va - vb;
        const double d = sqrt((du * du) + (dv * dv));
        if (!(d <= best)) best = d;                            // (a NaN distance stays: it is never below eps)
    }
    return best;
}

// hg_align_scale_matrix: a position at level k is x_k = (x_0 + 0.5) 2^-k - 0.5, so with e = 2^(level_in - level_out) and o = (e - 1) / 2
// a position moves between the levels as x_out = e x_in + o, and M_out = S M_in S^-1 with S = [e 0 o; 0 e o; 0 0 1], divided through by
// its last entry (affine: the last row stays 0 0 1).
HG_HD void align_scale(int kind, const double *m, int level_in, int level_out, double *out)
{
    const int d = level_in - level_out;
    const double e = d >= 0 ? (double)((int64_t)1 << d) : 1.0 / (double)((int64_t)1 << -d);
    const double o = (e - 1.0) / 2.0, oi = ((1.0 / e) - 1.0) / 2.0;      // S^-1 = [1/e 0 oi; 0 1/e oi; 0 0 1]
    double a[9], b[9];
    align_to3x3(kind, m, a);
    for (int r = 0; r < 3; r++) {                              // M S^-1
        b[3 * r + 0] = a[3 * r + 0] / e;
        b[3 * r + 1] = a[3 * r + 1] / e;
        b[3 * r + 2] = ((a[3 * r + 0] * oi) + (a[3 * r + 1] * oi)) + a[3 * r + 2];
    }
    for (int c = 0; c < 3; c++) {                              // S .
        a[0 + c] = (e * b[0 + c]) + (o * b[6 + c]);
        a[3 + c] = (e * b[3 + c]) + (o * b[6 + c]);
        a[6 + c] = b[6 + c];
    }
    if (kind == 1) {
        for (int k = 0; k < 8; k++) out[k] = a[k] / a[8];
    } else {
        out[0] = a[0]; out[2] = a[1]; out[4] = a[2]; out[1] = a[3]; out[3] = a[4]; out[5] = a[5]; out[6] = 0.0; out[7] = 0.0;
    }
}

// What k_align_update keeps per frame between the passes (scratch of the context).
struct AlignState {
    double h[8];                        // the normalised iterate
    double gain, bias;
    double rms_first, rms_last;
    int32_t phase;                      // 0 iterating, 1 the final evaluation is pending, 2 stopped
    int32_t pending;                    // the status the final evaluation confirms (CONVERGED or MAX_ITER)
    int32_t updates, n_first;
};

struct AlignInfo { int32_t status, updates, n_valid_first, n_valid_last; double rms_first, rms_last, gain, bias; };
static_assert(sizeof(AlignInfo) == 48, "the header's 48 bytes");

} // namespace hg
