// hg_bundle_dev.h -- the one text of the bundle adjustment's rules (include/hgwarp.h, "adjusting a frame set over all pairs") that host and
// device share: the capacities, the layout of a pair record, the arithmetic of one slot (residual, validity, robust weight, the two Jacobian
// rows of both frames), the state the kernels keep between the rounds, the argument block and the two host helpers' 3 x 3 arithmetic.  The
// normalisation, the way back and the corner displacement are the alignment's (hg_align_dev.h) with both sides W x H.  Needs hg_math.h and
// hg_align_dev.h only, so a host check can include it.
#pragma once
#include "hg_align_dev.h"

#include <vector>

namespace hg {

constexpr int kBundleBlock = 256;       // lanes per workgroup of the pass, the assembly, the small solve and the decision
constexpr int kBundleChunk = 512;       // slots per workgroup of k_bundle_pass; the tests read this line
constexpr int kBundleTile = 128;        // slots of a chunk that lie in LDS at a time
constexpr int kBundleRec = 154;         // doubles of a record: (2 P + 1)(2 P + 2) / 2 sums and the count at P = 8 (affine: 92, the tail zero)
constexpr int kBundleLdsCap = 128;      // unknowns up to which the whole system lies in LDS: N <= this takes the small path; the tests read this line
constexpr int kBundlePanel = 32;        // columns of a panel of the blocked factorisation above it; the tests read this line
constexpr int kBundleMaxUnknowns = 2048;
constexpr double kBundleMaxCoord = 16777216.0;   // a coordinate beyond 2^24 in magnitude is no position (NaN fails the test too)
constexpr int kBundleBackBlock = 1024;  // lanes of the large path's back substitution

HG_HD int bundle_p(int kind) { return kind == 1 ? 8 : 6; }
// Entry (i, j), i <= j, of the upper triangle of an nv x nv symmetric matrix stored row by row.
HG_HD int bundle_tri(int nv, int i, int j) { return i * nv - (i * (i - 1)) / 2 + (j - i); }

// One slot.  ha, hb: the normalised iterates of the pair's frames (row-major h0..h7, h8 == 1; affine: h6 = h7 = 0).  in: the slot lies below
// counts[p] and its mask byte is not 0.  vx, vy (2 P + 1 values each): the x and the y row of [J_a | J_b | r].  False (and nothing
// written) for a slot that is not VALID.
template <int KIND>
HG_HD bool bundle_slot(const double *ha, const double *hb, const AlignGeom &g, float fx, float fy, float fu, float fv, bool in, double huber,
                       double *vx, double *vy, double &w, double &rho)
{
    constexpr int P = KIND == 1 ? 8 : 6;
    if (!in) return false;
    const double x = (double)fx, y = (double)fy, u = (double)fu, v = (double)fv;
    if (!(fabs(x) <= kBundleMaxCoord && fabs(y) <= kBundleMaxCoord && fabs(u) <= kBundleMaxCoord && fabs(v) <= kBundleMaxCoord)) return false;
    const double xn = (x - g.cfx) * g.sf, yn = (y - g.cfy) * g.sf, un = (u - g.cfx) * g.sf, vn = (v - g.cfy) * g.sf;
    const double Da = KIND == 1 ? ((ha[6] * xn) + (ha[7] * yn)) + 1.0 : 1.0;
    const double Db = KIND == 1 ? ((hb[6] * un) + (hb[7] * vn)) + 1.0 : 1.0;
    const double pax = (((ha[0] * xn) + (ha[1] * yn)) + ha[2]) / Da, pay = (((ha[3] * xn) + (ha[4] * yn)) + ha[5]) / Da;
    const double pbx = (((hb[0] * un) + (hb[1] * vn)) + hb[2]) / Db, pby = (((hb[3] * un) + (hb[4] * vn)) + hb[5]) / Db;
    if (!(align_finite(pax) && align_finite(pay) && align_finite(pbx) && align_finite(pby) && Da > 0.0 && Db > 0.0)) return false;
    const double rx = pax - pbx, ry = pay - pby;
    const double e = sqrt((rx * rx) + (ry * ry)) / g.sf;
    if (huber > 0.0 && e > huber) { w = huber / e; rho = ((2.0 * huber) * e) - (huber * huber); }
    else { w = 1.0; rho = e * e; }
    if (KIND == 1) {
        const double ax = xn / Da, ay = yn / Da, a1 = 1.0 / Da, bx = un / Db, by = vn / Db, b1 = 1.0 / Db;
        vx[0] = ax; vx[1] = ay; vx[2] = a1; vx[3] = 0.0; vx[4] = 0.0; vx[5] = 0.0; vx[6] = -((pax * xn) / Da); vx[7] = -((pax * yn) / Da);
        vy[0] = 0.0; vy[1] = 0.0; vy[2] = 0.0; vy[3] = ax; vy[4] = ay; vy[5] = a1; vy[6] = -((pay * xn) / Da); vy[7] = -((pay * yn) / Da);
        vx[8] = -bx; vx[9] = -by; vx[10] = -b1; vx[11] = 0.0; vx[12] = 0.0; vx[13] = 0.0; vx[14] = (pbx * un) / Db; vx[15] = (pbx * vn) / Db;
        vy[8] = 0.0; vy[9] = 0.0; vy[10] = 0.0; vy[11] = -bx; vy[12] = -by; vy[13] = -b1; vy[14] = (pby * un) / Db; vy[15] = (pby * vn) / Db;
    } else {
        vx[0] = xn; vx[1] = 0.0; vx[2] = yn; vx[3] = 0.0; vx[4] = 1.0; vx[5] = 0.0;
        vy[0] = 0.0; vy[1] = xn; vy[2] = 0.0; vy[3] = yn; vy[4] = 0.0; vy[5] = 1.0;
        vx[6] = -un; vx[7] = 0.0; vx[8] = -vn; vx[9] = 0.0; vx[10] = -1.0; vx[11] = 0.0;
        vy[6] = 0.0; vy[7] = -un; vy[8] = 0.0; vy[9] = -vn; vy[10] = 0.0; vy[11] = -1.0;
    }
    vx[2 * P] = rx; vy[2 * P] = ry;
    return true;
}

// Slot s of the row-major normalised iterate -> the parameter that lives there (-1: none).  The inverse of align_slot.
HG_HD int bundle_param(int kind, int s)
{
    if (kind == 1) return s;
    return s == 0 ? 0 : s == 3 ? 1 : s == 1 ? 2 : s == 4 ? 3 : s == 2 ? 4 : s == 5 ? 5 : -1;
}

// 3 x 3 helpers of hg_bundle_chain_from_pairs and hg_bundle_invert_matrix (row-major, plain doubles).
HG_HD void bundle_mul3(const double *a, const double *b, double *o)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) o[3 * r + c] = ((a[3 * r + 0] * b[0 + c]) + (a[3 * r + 1] * b[3 + c])) + (a[3 * r + 2] * b[6 + c]);
}
// The adjugate of a divided through by its last entry.
HG_HD void bundle_inv3(const double *a, double *o)
{
    double j[9];
    j[0] = (a[4] * a[8]) - (a[5] * a[7]); j[1] = (a[2] * a[7]) - (a[1] * a[8]); j[2] = (a[1] * a[5]) - (a[2] * a[4]);
    j[3] = (a[5] * a[6]) - (a[3] * a[8]); j[4] = (a[0] * a[8]) - (a[2] * a[6]); j[5] = (a[2] * a[3]) - (a[0] * a[5]);
    j[6] = (a[3] * a[7]) - (a[4] * a[6]); j[7] = (a[1] * a[6]) - (a[0] * a[7]); j[8] = (a[0] * a[4]) - (a[1] * a[3]);
    for (int k = 0; k < 9; k++) o[k] = j[k] / j[8];
}
// A 3 x 3 matrix divided through by its last entry, in the fit's layout of `kind` (affine: slots 6 and 7 zero).
HG_HD void bundle_from3x3(int kind, const double *a, double *m)
{
    if (kind == 1) { for (int k = 0; k < 8; k++) m[k] = a[k] / a[8]; }
    else { m[0] = a[0] / a[8]; m[2] = a[1] / a[8]; m[4] = a[2] / a[8]; m[1] = a[3] / a[8]; m[3] = a[4] / a[8]; m[5] = a[5] / a[8]; m[6] = 0.0; m[7] = 0.0; }
}

// What the kernels keep between the rounds (the head of the caller's scratch).
struct BundleState {
    double cost, lambda, rms_first;     // of the current iterate; the damping of the next solve
    int32_t cur;                        // which of the two iterate / record buffers is current
    int32_t done, sing;                 // the call has stopped; a pivot of this round's factorisation was not positive and finite
    int32_t fresh;                      // the current records have not been assembled yet
    int32_t rounds, accepted, n_cur, n_first;
};

struct BundleInfo { int32_t status, rounds, accepted, n_valid_first, n_valid_last, pad; double rms_first, rms_last, lambda_last; };
struct BundlePairInfo { int32_t n_valid_first, n_valid_last; double rms_first, rms_last; };
static_assert(sizeof(BundleInfo) == 48 && sizeof(BundlePairInfo) == 24, "the header's 48 and 24 bytes");

// n_free free frames, N = P n_free unknowns.  pairs4: (a, b, count, first chunk record) per pair.  work: (pair, chunk) per workgroup of the
// pass.  cls: 0 free, 1 fixed, 2 unanchored; fidx: the free index of a frame or -1; rowptr / ent: per free frame the records that touch it,
// in ascending pair index, as pair * 2 + side (0: the frame is a, 1: it is b).  iter: 2 x F x 8 normalised iterates; part: one record per
// workgroup of the pass; recs: 2 x n_pairs records; Hm: (N + 1) x N, row N the gradient; Wm: the same again (large path only).
struct BundleArgs {
    int kind, W, H, n_frames, n_pairs, n_points, n_work, n_free, N, n_iter;
    double eps, lambda0, huber;
    const float *matches; const uint8_t *mask;
    const int32_t *pairs4, *work, *cls, *fidx, *rowptr, *ent;
    int32_t *good;
    const double *mats_in; double *mats_out; uint8_t *info; double *sums;
    BundleState *state; double *iter, *part, *recs, *Hm, *Wm;
};

// The host-built lists of a call, in the order they are uploaded (one block of int32): pairs4, work, cls, fidx, rowptr, ent.  A frame is
// unanchored where union-find over the pairs with counts > 0 ties it to no fixed frame.
struct BundleLists { std::vector<int32_t> ints; size_t o_work, o_cls, o_fidx, o_rowptr, o_ent; int n_work, n_free; };

inline void bundle_build_lists(int n_frames, const uint8_t *fixed, const int32_t *pairs, int n_pairs, const int32_t *counts, int n_points, BundleLists &L)
{
    const int F = n_frames;
    std::vector<int> root((size_t)F);
    for (int f = 0; f < F; f++) root[(size_t)f] = f;
    auto find = [&](int f) { while (root[(size_t)f] != f) { root[(size_t)f] = root[(size_t)root[(size_t)f]]; f = root[(size_t)f]; } return f; };
    auto cnt = [&](int p) { return counts ? counts[p] : n_points; };
    for (int p = 0; p < n_pairs; p++)
        if (cnt(p) > 0) {
            const int ra = find(pairs[2 * p]), rb = find(pairs[2 * p + 1]);
            if (ra != rb) root[(size_t)(ra > rb ? ra : rb)] = ra > rb ? rb : ra;
        }
    std::vector<uint8_t> anchored((size_t)F, 0);
    for (int f = 0; f < F; f++) if (fixed[f]) anchored[(size_t)find(f)] = 1;
    std::vector<int32_t> &ints = L.ints;
    ints.clear();
    size_t n_work = 0;
    for (int p = 0; p < n_pairs; p++) {
        ints.push_back(pairs[2 * p]); ints.push_back(pairs[2 * p + 1]); ints.push_back(cnt(p)); ints.push_back((int32_t)n_work);
        n_work += (size_t)((cnt(p) + kBundleChunk - 1) / kBundleChunk);
    }
    L.n_work = (int)n_work;
    L.o_work = ints.size();
    for (int p = 0; p < n_pairs; p++)
        for (int k = 0; k < (cnt(p) + kBundleChunk - 1) / kBundleChunk; k++) { ints.push_back(p); ints.push_back(k); }
    L.o_cls = ints.size();
    L.n_free = 0;
    std::vector<int32_t> fidx((size_t)F, -1);
    for (int f = 0; f < F; f++) {
        const int cls = fixed[f] ? 1 : anchored[(size_t)find(f)] ? 0 : 2;
        ints.push_back(cls);
        if (cls == 0) fidx[(size_t)f] = L.n_free++;
    }
    L.o_fidx = ints.size();
    ints.insert(ints.end(), fidx.begin(), fidx.end());
    L.o_rowptr = ints.size();
    std::vector<std::vector<int32_t>> touch((size_t)L.n_free);
    for (int p = 0; p < n_pairs; p++)
        for (int side = 0; side < 2; side++) { const int fi = fidx[(size_t)pairs[2 * p + side]]; if (fi >= 0) touch[(size_t)fi].push_back(2 * p + side); }
    int32_t at = 0;
    for (int i = 0; i < L.n_free; i++) { ints.push_back(at); at += (int32_t)touch[(size_t)i].size(); }
    ints.push_back(at);
    L.o_ent = ints.size();
    for (int i = 0; i < L.n_free; i++) ints.insert(ints.end(), touch[(size_t)i].begin(), touch[(size_t)i].end());
    if (ints.size() & 1) ints.push_back(0);                    // (uploads go in 8-byte words)
}

} // namespace hg
