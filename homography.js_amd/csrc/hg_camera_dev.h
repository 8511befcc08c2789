// hg_camera_dev.h -- the one text of the camera rules (include/hgwarp.h, "camera models") that host and device share: the layout of a frame's
// record, the canvas position -> source position map of the three surfaces, the Brown-Conrady distortion, its fixed-point inverse and the
// source position -> canvas position map.  hg_camera_pack_record and hg_camera_limits run these functions on the host, the kernels of
// hg_k_camera.hip on the device.  Needs nothing but <math.h> and the HIP builtins, so a host check can include it.
// All arithmetic is f64, IEEE division and square root, contraction off, in the operation order of the header's text.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_CAM_HD __host__ __device__ __forceinline__
#else
#define HG_CAM_HD inline
#endif

namespace hg {

constexpr int kCamRecord = 32;          // HG_CAMERA_RECORD_DOUBLES
constexpr int kCamUndistortIters = 20;  // HG_CAMERA_UNDISTORT_ITERS
constexpr int kCamPiece = 256;          // columns of a workgroup's piece: 64 lanes x 4 pixels
constexpr int kCamBandRows = 32;        // rows of a workgroup's band; the tests read this line
constexpr double kCamTwoPi = 6.283185307179586;      // 2 pi, rounded once
constexpr double kCamInverseTol = 1e-9; // how close the undistorted point, distorted again, must land
enum : int { kCamPlane = 0, kCamCylinder = 1, kCamSphere = 2 };
// slots of a record: R at 0..8 (row-major, camera <- world)
enum : int { kCamFx = 9, kCamFy = 10, kCamCx = 11, kCamCy = 12, kCamK1 = 13, kCamK2 = 14, kCamP1 = 15, kCamP2 = 16, kCamK3 = 17, kCamR2Max = 18, kCamAc = 19 };

// One frame of a field call: the window and where its field starts (bytes from d_field).  The size of the field calls' frame table entry.
struct CamFrame { int32_t x_off, y_off, obj_w, obj_h; uint64_t out_off, pad; };

// (The kernel takes records, frames and the output as __restrict__ parameters of its own: that is what lets the compiler read the record
// through scalar loads.)
struct CamFieldArgs {
    const double *records; const CamFrame *frames; int n_frames, max_w, max_h, n_pieces; int W, H; double scale, u0, v0; uint8_t *field;
};
struct CamPointArgs {
    const double *records; int n_frames, surface; double scale, u0, v0; const float *points; int n_pts, n_sets; float *out;
};

HG_CAM_HD int cam_pieces(int w) { return (int)(((int64_t)w + kCamPiece - 1) / kCamPiece); }
HG_CAM_HD int cam_bands(int h) { return (int)(((int64_t)h + kCamBandRows - 1) / kCamBandRows); }
HG_CAM_HD bool cam_finite(double v) { return fabs(v) < INFINITY; }          // (NaN compares false)

// A record with a NaN in any slot fails its frame.
HG_CAM_HD bool cam_record_bad(const double *__restrict__ rec)
{
    bool bad = false;
    for (int i = 0; i < kCamRecord; i++) bad = bad || !(rec[i] == rec[i]);
    return bad;
}

// The ray of the canvas position (U, V) is (sa cb, yb, ca cb): sa, ca depend on the column only, yb, cb on the row only.
//   PLANE     a, 1  and  b, 1          (the products with 1 are exact: the ray is (a, b, 1))
//   CYLINDER  sin a, cos a  and  b, 1
//   SPHERE    sin a, cos a  and  sin b, cos b
template <int S>
HG_CAM_HD void cam_col(double U, double scale, double u0, double &sa, double &ca)
{
    const double a = (U - u0) / scale;
    if (S == kCamPlane) { sa = a; ca = 1.0; }
    else { sa = sin(a); ca = cos(a); }
}
template <int S>
HG_CAM_HD void cam_row(double V, double scale, double v0, double &yb, double &cb)
{
    const double b = (V - v0) / scale;
    if (S == kCamSphere) { yb = sin(b); cb = cos(b); }
    else { yb = b; cb = 1.0; }
}

// The radial factor and the tangential terms at the undistorted point (xn, yn).
HG_CAM_HD void cam_lens(const double *__restrict__ rec, double xn, double yn, double &rad, double &tx, double &ty, double &r2)
{
    const double k1 = rec[kCamK1], k2 = rec[kCamK2], p1 = rec[kCamP1], p2 = rec[kCamP2], k3 = rec[kCamK3];
    r2 = xn * xn + yn * yn;
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    tx = ((2.0 * p1) * xn) * yn + p2 * (r2 + (2.0 * xn) * xn);
    ty = p1 * (r2 + (2.0 * yn) * yn) + ((2.0 * p2) * xn) * yn;
}

// Canvas -> source from the column and row terms.  Returns c.z > 0 && r2 <= r2_max; the test against the picture is the caller's.
HG_CAM_HD bool cam_project(const double *__restrict__ rec, double sa, double ca, double yb, double cb, double &sx, double &sy)
{
    const double x = sa * cb, y = yb, z = ca * cb;
    const double c0 = (rec[0] * x + rec[1] * y) + rec[2] * z;
    const double c1 = (rec[3] * x + rec[4] * y) + rec[5] * z;
    const double c2 = (rec[6] * x + rec[7] * y) + rec[8] * z;
    const double xn = c0 / c2, yn = c1 / c2;
    double rad, tx, ty, r2;
    cam_lens(rec, xn, yn, rad, tx, ty, r2);
    const double xd = xn * rad + tx, yd = yn * rad + ty;
    sx = rec[kCamFx] * xd + rec[kCamCx];
    sy = rec[kCamFy] * yd + rec[kCamCy];
    return c2 > 0.0 && r2 <= rec[kCamR2Max];
}

template <int S>
HG_CAM_HD bool cam_to_source_s(const double *__restrict__ rec, double scale, double u0, double v0, double U, double V, double &sx, double &sy)
{
    double sa, ca, yb, cb;
    cam_col<S>(U, scale, u0, sa, ca);
    cam_row<S>(V, scale, v0, yb, cb);
    return cam_project(rec, sa, ca, yb, cb, sx, sy);
}
HG_CAM_HD bool cam_to_source(const double *__restrict__ rec, int surface, double scale, double u0, double v0, double U, double V, double &sx, double &sy)
{
    if (surface == kCamPlane) return cam_to_source_s<kCamPlane>(rec, scale, u0, v0, U, V, sx, sy);
    if (surface == kCamCylinder) return cam_to_source_s<kCamCylinder>(rec, scale, u0, v0, U, V, sx, sy);
    return cam_to_source_s<kCamSphere>(rec, scale, u0, v0, U, V, sx, sy);
}

// The fixed-point inverse of the distortion: kCamUndistortIters rounds from (xd, yd), then the result distorted once more must land within
// kCamInverseTol of (xd, yd) in both parts and keep r2 <= r2_max.
HG_CAM_HD bool cam_undistort(const double *__restrict__ rec, double xd, double yd, double &xn, double &yn, double &r2)
{
    double rad, tx, ty;
    xn = xd; yn = yd;
    for (int it = 0; it < kCamUndistortIters; it++) {
        cam_lens(rec, xn, yn, rad, tx, ty, r2);
        xn = (xd - tx) / rad;
        yn = (yd - ty) / rad;
    }
    cam_lens(rec, xn, yn, rad, tx, ty, r2);
    const double xe = xn * rad + tx, ye = yn * rad + ty;
    return fabs(xe - xd) <= kCamInverseTol && fabs(ye - yd) <= kCamInverseTol && r2 <= rec[kCamR2Max];      // (NaN fails)
}

// Source -> canvas.  Returns the validity of the header's rule; (U, V) may hold a NaN or an infinity where it is false.
HG_CAM_HD bool cam_to_canvas(const double *__restrict__ rec, int surface, double scale, double u0, double v0, double x, double y, double &U, double &V)
{
    const double xd = (x - rec[kCamCx]) / rec[kCamFx], yd = (y - rec[kCamCy]) / rec[kCamFy];
    double xn, yn, r2;
    bool ok = cam_undistort(rec, xd, yd, xn, yn, r2);
    const double wx = (rec[0] * xn + rec[3] * yn) + rec[6];
    const double wy = (rec[1] * xn + rec[4] * yn) + rec[7];
    const double wz = (rec[2] * xn + rec[5] * yn) + rec[8];
    double a, b;
    if (surface == kCamPlane) {
        ok = ok && wz > 0.0;
        a = wx / wz; b = wy / wz;
    } else {
        const double h = sqrt(wx * wx + wz * wz);
        a = atan2(wx, wz);
        b = surface == kCamCylinder ? wy / h : atan2(wy, h);
        a = rec[kCamAc] + remainder(a - rec[kCamAc], kCamTwoPi);
    }
    U = u0 + scale * a;
    V = v0 + scale * b;
    return ok;
}

} // namespace hg
