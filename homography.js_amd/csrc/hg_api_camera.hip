// hg_api_camera.hip -- the C ABI, part 13: camera models (hg_camera_pack_record, hg_camera_limits, hg_camera_focals_from_matrix,
// hg_camera_rotation_from_matrix, hg_field_camera_frames_device, hg_points_camera_to_source_frames_device,
// hg_points_camera_to_canvas_frames_device).  Geometry of its own, like the splines: no image, mesh or frame set is needed, and the warp
// paths' taps (hg_last_*_kernel), the sampling mode, the plan of the last warp, what the policy learned and every staged frame set stay as
// they were.  The host calls run the per-position rules of hg_camera_dev.h, the text the kernels run.
#include "hg_ctx.h"
#include "hg_camera_dev.h"

#include <cmath>

constexpr int kCamMaxFrames = 4096;

// ------------------------------------------------------------------------------------------------ host only
extern "C" int hg_camera_pack_record(const double *R, double fx, double fy, double cx, double cy, const double *dist, int W, int H, double *record)
{
    if (!R || !record) return fail(nullptr, HG_ERR_INVALID, "hg_camera_pack_record: R / record is NULL");
    if (W < 1 || H < 1) return fail(nullptr, HG_ERR_INVALID, "hg_camera_pack_record: W and H must be >= 1");
    bool finite = cam_finite(fx) && cam_finite(fy) && cam_finite(cx) && cam_finite(cy);
    for (int i = 0; i < 9; i++) finite = finite && cam_finite(R[i]);
    for (int i = 0; dist && i < 5; i++) finite = finite && cam_finite(dist[i]);
    if (!finite) return fail(nullptr, HG_ERR_INVALID, "hg_camera_pack_record: every number must be finite");
    if (!(fx > 0.0) || !(fy > 0.0)) return fail(nullptr, HG_ERR_INVALID, "hg_camera_pack_record: fx and fy must be > 0");
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
        const double g = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j];         // (R^T R)_ij
        if (!(std::fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-6)) return fail(nullptr, HG_ERR_INVALID, "hg_camera_pack_record: R is not orthonormal (|R^T R - I| > 1e-6)");
    }
    double rec[kCamRecord] = {};
    for (int i = 0; i < 9; i++) rec[i] = R[i];
    rec[kCamFx] = fx; rec[kCamFy] = fy; rec[kCamCx] = cx; rec[kCamCy] = cy;
    if (dist) { rec[kCamK1] = dist[0]; rec[kCamK2] = dist[1]; rec[kCamP1] = dist[2]; rec[kCamP2] = dist[3]; rec[kCamK3] = dist[4]; }
    rec[kCamR2Max] = INFINITY;
    rec[kCamAc] = std::atan2(R[6], R[8]);                    // w = R^T (0, 0, 1) = (R6, R7, R8)
    if (dist) {
        const double w = (double)W, h = (double)H;
        const double px[8] = {0.0, w, 0.0, w, w / 2.0, w / 2.0, 0.0, w}, py[8] = {0.0, 0.0, h, h, 0.0, h, h / 2.0, h / 2.0};
        double top = 0.0;
        for (int k = 0; k < 8; k++) {
            double xn, yn, r2;
            if (!cam_undistort(rec, (px[k] - cx) / fx, (py[k] - cy) / fy, xn, yn, r2))
                return fail(nullptr, HG_ERR_INVALID, "hg_camera_pack_record: the distortion is too strong for this picture (a corner or an edge midpoint has no inverse)");
            top = std::max(top, r2);
        }
        rec[kCamR2Max] = 1.05 * top;
    }
    std::memcpy(record, rec, sizeof rec);
    return HG_OK;
}

static bool cam_surface_ok(int s) { return s == kCamPlane || s == kCamCylinder || s == kCamSphere; }

// the first of the limits, shared by every call: the surface, (a field's format,) scale, u0, v0
static int check_cam_surface(hg_ctx *c, int surface)
{
    if (!cam_surface_ok(surface)) return fail(c, HG_ERR_INVALID, "camera: unknown surface (HG_SURFACE_PLANE, HG_SURFACE_CYLINDER or HG_SURFACE_SPHERE)");
    return HG_OK;
}
static int check_cam_canvas(hg_ctx *c, double scale, double u0, double v0)
{
    if (!cam_finite(scale) || !(scale > 0.0)) return fail(c, HG_ERR_INVALID, "camera: scale must be finite and > 0");
    if (!cam_finite(u0) || !cam_finite(v0)) return fail(c, HG_ERR_INVALID, "camera: u0 and v0 must be finite");
    return HG_OK;
}

extern "C" int hg_camera_limits(const double *record, int W, int H, int surface, double scale, double u0, double v0, int32_t *out)
{
    HG_TRY(check_cam_surface(nullptr, surface));
    HG_TRY(check_cam_canvas(nullptr, scale, u0, v0));
    if (W < 1 || H < 1) return fail(nullptr, HG_ERR_INVALID, "hg_camera_limits: W and H must be >= 1");
    if (!record || !out) return fail(nullptr, HG_ERR_INVALID, "hg_camera_limits: record / out is NULL");
    if (cam_record_bad(record)) return fail(nullptr, HG_ERR_INVALID, "hg_camera_limits: the record holds a NaN");
    double lo_u = INFINITY, hi_u = -INFINITY, lo_v = INFINITY, hi_v = -INFINITY;
    auto take = [&](double x, double y) {
        double U, V;
        if (!cam_to_canvas(record, surface, scale, u0, v0, x, y, U, V) || !cam_finite(U) || !cam_finite(V)) return;
        lo_u = std::min(lo_u, U); hi_u = std::max(hi_u, U); lo_v = std::min(lo_v, V); hi_v = std::max(hi_v, V);
    };
    for (int i = 0; i <= W; i++) { take((double)i, 0.0); take((double)i, (double)H); }
    for (int j = 0; j <= H; j++) { take(0.0, (double)j); take((double)W, (double)j); }
    if (!(lo_u <= hi_u)) return fail(nullptr, HG_ERR_INVALID, "hg_camera_limits: no border position of the picture is valid");
    if (surface != kCamPlane) {
        // the poles (0, +-1, 0): the border's image does not enclose a pole that lies inside the picture
        for (int s = -1; s <= 1; s += 2) {
            double sx, sy;
            const bool in = cam_project(record, 0.0, 0.0, (double)s, 1.0, sx, sy);
            if (!(in && sx >= 0 && sx < (double)W && sy >= 0 && sy < (double)H)) continue;
            if (surface == kCamCylinder) return fail(nullptr, HG_ERR_INVALID, "hg_camera_limits: the picture holds a pole, which a cylinder sends to infinity");
            lo_u = std::min(lo_u, u0 + scale * (record[kCamAc] - kCamTwoPi / 2.0));
            hi_u = std::max(hi_u, u0 + scale * (record[kCamAc] + kCamTwoPi / 2.0));
            const double vp = v0 + scale * ((double)s * (kCamTwoPi / 4.0));
            lo_v = std::min(lo_v, vp); hi_v = std::max(hi_v, vp);
        }
    }
    const double x0 = std::floor(lo_u) - 1.0, x1 = std::ceil(hi_u) + 1.0, y0 = std::floor(lo_v) - 1.0, y1 = std::ceil(hi_v) + 1.0;
    const double lim = (double)(1 << 26), w = x1 - x0 + 1.0, h = y1 - y0 + 1.0;
    if (std::fabs(x0) > lim || std::fabs(y0) > lim || w * h > 2147483648.0)
        return fail(nullptr, HG_ERR_INVALID, "hg_camera_limits: the window is beyond what hg_geom accepts (offsets up to 2^26, 2^31 pixels)");
    out[0] = (int32_t)x0; out[1] = (int32_t)y0; out[2] = (int32_t)w; out[3] = (int32_t)h;
    return HG_OK;
}

// One focal length from its two candidates num1 / den1 and num2 / den2: the one with the larger denominator magnitude; ok iff it is > 0
// and finite (0 / 0 is a NaN and fails).
static void cam_focal(double n1, double d1, double n2, double d2, double *f, int *ok)
{
    const double v = std::fabs(d1) > std::fabs(d2) ? n1 / d1 : n2 / d2;
    *ok = (v > 0.0 && cam_finite(v)) ? 1 : 0;
    *f = *ok ? std::sqrt(v) : 0.0;
}

extern "C" int hg_camera_focals_from_matrix(const double *h, double *f_from, double *f_to, int *ok_from, int *ok_to)
{
    if (!h || !f_from || !f_to || !ok_from || !ok_to) return fail(nullptr, HG_ERR_INVALID, "hg_camera_focals_from_matrix: a pointer is NULL");
    for (int i = 0; i < 9; i++) if (!cam_finite(h[i])) return fail(nullptr, HG_ERR_INVALID, "hg_camera_focals_from_matrix: every entry must be finite");
    // H = K_to R K_from^-1, K = diag(f, f, 1): R ~ K_to^-1 H K_from has columns 0 and 1 orthogonal and of equal length (f_to) and rows 0 and
    // 1 orthogonal and of equal length (f_from).
    cam_focal(-(h[0] * h[1] + h[3] * h[4]), h[6] * h[7], ((h[0] * h[0] + h[3] * h[3]) - h[1] * h[1]) - h[4] * h[4], (h[7] - h[6]) * (h[7] + h[6]), f_to, ok_to);
    cam_focal(-(h[2] * h[5]), h[0] * h[3] + h[1] * h[4], h[5] * h[5] - h[2] * h[2], ((h[0] * h[0] + h[1] * h[1]) - h[3] * h[3]) - h[4] * h[4], f_from, ok_from);
    return HG_OK;
}

static double cam_det3(const double *m)
{
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

extern "C" int hg_camera_rotation_from_matrix(const double *h, const double *k_from, const double *k_to, double *R)
{
    if (!h || !k_from || !k_to || !R) return fail(nullptr, HG_ERR_INVALID, "hg_camera_rotation_from_matrix: a pointer is NULL");
    bool finite = true;
    for (int i = 0; i < 9; i++) finite = finite && cam_finite(h[i]);
    for (int i = 0; i < 4; i++) finite = finite && cam_finite(k_from[i]) && cam_finite(k_to[i]);
    if (!finite) return fail(nullptr, HG_ERR_INVALID, "hg_camera_rotation_from_matrix: every number must be finite");
    if (!(k_from[0] > 0.0) || !(k_from[1] > 0.0) || !(k_to[0] > 0.0) || !(k_to[1] > 0.0))
        return fail(nullptr, HG_ERR_INVALID, "hg_camera_rotation_from_matrix: fx and fy must be > 0");
    // A = H K_from: column 0 times fx, column 1 times fy, column 2 = cx col0 + cy col1 + col2
    double A[9], M[9];
    for (int r = 0; r < 3; r++) {
        A[3 * r] = h[3 * r] * k_from[0];
        A[3 * r + 1] = h[3 * r + 1] * k_from[1];
        A[3 * r + 2] = (h[3 * r] * k_from[2] + h[3 * r + 1] * k_from[3]) + h[3 * r + 2];
    }
    // M = K_to^-1 A: row 0 = (row0 - cx row2) / fx, row 1 = (row1 - cy row2) / fy
    for (int j = 0; j < 3; j++) {
        M[j] = (A[j] - k_to[2] * A[6 + j]) / k_to[0];
        M[3 + j] = (A[3 + j] - k_to[3] * A[6 + j]) / k_to[1];
        M[6 + j] = A[6 + j];
    }
    const double det = cam_det3(M);
    if (!(det > 0.0) || !cam_finite(det)) return fail(nullptr, HG_ERR_INVALID, "hg_camera_rotation_from_matrix: det(K_to^-1 H K_from) must be finite and > 0");
    const double s = std::cbrt(det);
    for (int i = 0; i < 9; i++) M[i] = M[i] / s;
    for (int it = 0; it < 30; it++) {                        // R <- (R + R^-T) / 2, R^-T = the cofactor matrix / det
        const double d = cam_det3(M);
        const double C[9] = { M[4] * M[8] - M[5] * M[7], M[5] * M[6] - M[3] * M[8], M[3] * M[7] - M[4] * M[6],
                              M[2] * M[7] - M[1] * M[8], M[0] * M[8] - M[2] * M[6], M[1] * M[6] - M[0] * M[7],
                              M[1] * M[5] - M[2] * M[4], M[2] * M[3] - M[0] * M[5], M[0] * M[4] - M[1] * M[3] };
        for (int i = 0; i < 9; i++) M[i] = 0.5 * (M[i] + C[i] / d);
    }
    for (int i = 0; i < 9; i++) if (!cam_finite(M[i])) return fail(nullptr, HG_ERR_INVALID, "hg_camera_rotation_from_matrix: the polar iteration did not stay finite");
    std::memcpy(R, M, sizeof M);
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ device
static int check_cam_frames(hg_ctx *c, int n_frames)
{
    if (n_frames < 0 || n_frames > kCamMaxFrames) return fail(c, HG_ERR_INVALID, "camera: n_frames must be 0..4096");
    return HG_OK;
}

extern "C" int hg_field_camera_frames_device(hg_ctx *c, const double *d_records, const hg_geom *geoms, int n_frames, int W, int H, int surface,
                                             double scale, double u0, double v0, int fmt, const size_t *field_offsets, void *d_field)
{
    HG_TRY(check_cam_surface(c, surface));
    HG_TRY(check_field_fmt(c, fmt));
    HG_TRY(check_cam_canvas(c, scale, u0, v0));
    if (W < 1 || H < 1) return fail(c, HG_ERR_INVALID, "hg_field_camera_frames_device: W and H must be >= 1");
    HG_TRY(check_cam_frames(c, n_frames));
    if (n_frames > 0 && !geoms) return fail(c, HG_ERR_INVALID, "camera: geoms is NULL");
    if (n_frames == 0) return HG_OK;
    std::vector<FrameDesc> fds;
    HG_TRY(fill_frames(c, fds, geoms, nullptr, n_frames));   // (the window limits of every frame)
    HG_TRY(check_field_fmt(c, fmt, W, H));
    FieldTable<CamFrame> t;
    HG_TRY(field_table(c, geoms, (size_t)n_frames, fmt, field_offsets, &t));
    if (t.extent == 0) return HG_OK;                         // (every frame is empty)
    const int mw = t.max_w, mh = t.max_h;
    if ((int64_t)cam_pieces(mw) * cam_bands(mh) >= ((int64_t)1 << 31))
        return fail(c, HG_ERR_INVALID, "hg_field_camera_frames_device: the widest and the tallest window together span 2^31 tiles or more");
    if (!d_records || !d_field) return fail(c, HG_ERR_INVALID, "hg_field_camera_frames_device: d_records / d_field is NULL");
    if (misaligned(d_records, 8) || misaligned(d_field, field_px_bytes(fmt)))
        return fail(c, HG_ERR_INVALID, "hg_field_camera_frames_device: d_records must be aligned to 8 bytes, d_field to its pixel size");
    HG_TRY(bind(c));
    HG_TRY(settle_pending_on(c, d_field, t.extent));
    static_assert(sizeof(CamFrame) == sizeof(FrameDesc), "the field calls' frame table carries either record");
    HG_TRY(ensure(c, c->d_field_frames, (size_t)n_frames));
    HG_TRY(upload_frame_table(c, c->d_field_frames, t.recs.data(), sizeof(CamFrame) * (size_t)n_frames));
    CamFieldArgs a{d_records, reinterpret_cast<const CamFrame *>(c->d_field_frames.p), n_frames, mw, mh, cam_pieces(mw), W, H, scale, u0, v0,
                   static_cast<uint8_t *>(d_field)};
    HG_TRY(time_begin(c));
    launch_camera_field(a, fmt, surface, c->stream);
    HG_TRY(time_end(c));
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

static int camera_points(hg_ctx *c, const char *who, bool to_source, const double *d_records, int n_frames, int surface, double scale, double u0,
                         double v0, const void *d_points, int n_pts, int n_sets, void *d_out)
{
    HG_TRY(check_cam_surface(c, surface));
    HG_TRY(check_cam_canvas(c, scale, u0, v0));
    HG_TRY(check_cam_frames(c, n_frames));
    if (n_pts < 0 || n_pts > (1 << 24)) return fail(c, HG_ERR_INVALID, std::string(who) + ": n_pts must be 0..2^24");
    if (n_sets < 1) return fail(c, HG_ERR_INVALID, std::string(who) + ": n_sets must be >= 1");
    if (n_frames == 0 || n_pts == 0) return HG_OK;
    if (!d_records || !d_points || !d_out) return fail(c, HG_ERR_INVALID, std::string(who) + ": d_records / d_points / d_out is NULL");
    if (misaligned(d_records, 8) || misaligned(d_points, 8) || misaligned(d_out, 8))
        return fail(c, HG_ERR_INVALID, std::string(who) + ": d_records / d_points / d_out must be aligned to 8 bytes");
    HG_TRY(bind(c));
    HG_TRY(settle_pending_on(c, d_out, (size_t)n_frames * (size_t)n_pts * 8));
    CamPointArgs a{d_records, n_frames, surface, scale, u0, v0, static_cast<const float *>(d_points), n_pts, n_sets, static_cast<float *>(d_out)};
    launch_camera_points(a, to_source, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

extern "C" int hg_points_camera_to_source_frames_device(hg_ctx *c, const double *d_records, int n_frames, int surface, double scale, double u0,
                                                        double v0, const void *d_points, int n_pts, int n_sets, void *d_out)
{
    return camera_points(c, "hg_points_camera_to_source_frames_device", true, d_records, n_frames, surface, scale, u0, v0, d_points, n_pts, n_sets, d_out);
}

extern "C" int hg_points_camera_to_canvas_frames_device(hg_ctx *c, const double *d_records, int n_frames, int surface, double scale, double u0,
                                                        double v0, const void *d_points, int n_pts, int n_sets, void *d_out)
{
    return camera_points(c, "hg_points_camera_to_canvas_frames_device", false, d_records, n_frames, surface, scale, u0, v0, d_points, n_pts, n_sets, d_out);
}
