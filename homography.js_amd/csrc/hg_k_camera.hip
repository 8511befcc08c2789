// hg_k_camera.hip -- frame sets projected onto a plane, a cylinder or a sphere from a camera model (include/hgwarp.h, "camera models";
// DESIGN.md §4.22).
//   k_camera_field   the source field of the cameras.  A workgroup takes one frame, a piece of kCamPiece columns and a band of kCamBandRows
//                    rows.  The azimuth depends on the column only and the elevation on the row only: lane t evaluates the column term
//                    (sin, cos) of column t of the piece ONCE, the first kCamBandRows lanes the row terms of the band, all into LDS; a
//                    lane then keeps the terms of its four consecutive columns in registers and walks the band's rows (wave w takes rows w,
//                    w + 4, ...): per pixel two table reads, the 3 x 3 product, two divisions, the polynomial and a share of one quad
//                    store.  Transcendental calls per workgroup: 2 (kCamPiece + kCamBandRows) for 8192 pixels; PLANE has none at all.
//   k_camera_points  point lists, one position per lane, canvas -> source (no test against the picture) or source -> canvas.
// Pixels and points go through the one cam_project of hg_camera_dev.h with the same arguments, f64 with contraction off: a point on a pixel
// repeats the field's bits.  The record is read at lane-independent addresses (scalar loads).  Field values are stored through field_px and
// field_store_quad (hg_field_dev.h), non-temporal.  The kernels need those two headers only, so a host check compiles this file behind a
// thread-index shim (tests/cpp/camera_check.cpp); the launchers are compiled under hipcc only.
#ifdef __HIPCC__
#include "hg_kernels.h"
#endif
#include "hg_camera_dev.h"
#include "hg_field_dev.h"

namespace hg {

static_assert(kCamPiece == 256 && kCamBandRows <= kCamPiece && kCamBandRows % 4 == 0, "one lane per column of the piece; the band's rows come from the first lanes");

// ------------------------------------------------------------------------------------------------ k_camera_field
template <int FMT, int S>
__global__ __launch_bounds__(kCamPiece) void k_camera_field(CamFieldArgs a, const double *__restrict__ records, const CamFrame *__restrict__ frames,
                                                            uint8_t *__restrict__ out)
{
    __shared__ double s_col[2][kCamPiece];
    __shared__ double s_row[2][kCamBandRows];
    const int f = blockIdx.y;
    const CamFrame fd = frames[f];
    const int band = blockIdx.x / a.n_pieces, piece = blockIdx.x - band * a.n_pieces;      // (pieces x bands of the largest window, flat)
    const int64_t c0l = (int64_t)piece * kCamPiece, r0l = (int64_t)band * kCamBandRows;
    if (c0l >= fd.obj_w || r0l >= fd.obj_h) return;          // (the whole workgroup: no barrier is left waiting; empty windows too)
    const int c0 = (int)c0l, r0 = (int)r0l;
    const int t = threadIdx.x;
    {
        double sa, ca;
        cam_col<S>((double)((int64_t)c0 + t + fd.x_off), a.scale, a.u0, sa, ca);
        s_col[0][t] = sa; s_col[1][t] = ca;
        if (t < kCamBandRows) {
            double yb, cb;
            cam_row<S>((double)((int64_t)r0 + t + fd.y_off), a.scale, a.v0, yb, cb);
            s_row[0][t] = yb; s_row[1][t] = cb;
        }
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int OW = fd.obj_w, cq = c0 + 4 * lane;
    if (cq >= OW) return;                                    // the tail: nothing is written past the row
    const double *__restrict__ rec = records + (size_t)f * kCamRecord;
    const bool bad = cam_record_bad(rec);
    const double bw = (double)a.W, bh = (double)a.H, n_src_px = bw * bh;
    double sa[4], ca[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { sa[k] = s_col[0][4 * lane + k]; ca[k] = s_col[1][4 * lane + k]; }
    constexpr int PX = FMT == 0 ? 4 : 8;
    uint8_t *__restrict__ frame = out + fd.out_off;
    const bool vec_ok = ((OW & 3) == 0) && ((reinterpret_cast<uintptr_t>(frame) & 15) == 0);
    const int rend = min(kCamBandRows, fd.obj_h - r0);
    for (int rr = wave; rr < rend; rr += 4) {
        const double yb = s_row[0][rr], cb = S == kCamSphere ? s_row[1][rr] : 1.0;
        int vx[4], vy[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double sx, sy;
            const bool in = cam_project(rec, sa[k], ca[k], yb, cb, sx, sy);
            const bool cov = !bad && in && sx >= 0 && sx < bw && sy >= 0 && sy < bh;        // (NaN fails)
            field_px<FMT>(cov, sx, sy, bw, n_src_px, vx[k], vy[k]);
        }
        field_store_quad<FMT>(frame + (uint64_t)(r0 + rr) * (uint64_t)OW * PX, cq, OW, vec_ok, vx, vy);
    }
}

// ------------------------------------------------------------------------------------------------ k_camera_points
// Frame f reads list f % n_sets and writes n_pts pairs at f * n_pts.  A position that is not finite, a record with a NaN, a position the
// direction's validity rule refuses and a result with a NaN part hold 0x7fc00000 in both words.
template <bool TO_SOURCE>
__global__ __launch_bounds__(256) void k_camera_points(CamPointArgs a, const double *__restrict__ records, const float *__restrict__ points,
                                                       float *__restrict__ out)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_pts) return;                                // the tail: nothing is written past n_pts
    const double *__restrict__ rec = records + (size_t)f * kCamRecord;
    const v2f p = *reinterpret_cast<const v2f *>(points + 2 * ((size_t)(f % a.n_sets) * a.n_pts + i));
    const double X = (double)p.x, Y = (double)p.y;
    double rx = 0.0, ry = 0.0;
    bool ok = cam_finite(X) && cam_finite(Y) && !cam_record_bad(rec);
    if (ok) ok = TO_SOURCE ? cam_to_source(rec, a.surface, a.scale, a.u0, a.v0, X, Y, rx, ry) : cam_to_canvas(rec, a.surface, a.scale, a.u0, a.v0, X, Y, rx, ry);
    ok = ok && rx == rx && ry == ry;
    v2f v = { __int_as_float((int)kFieldNaN), __int_as_float((int)kFieldNaN) };
    if (ok) { v.x = (float)rx; v.y = (float)ry; }            // the one rounding to f32
    *reinterpret_cast<v2f *>(out + 2 * ((size_t)f * a.n_pts + i)) = v;
}

// ------------------------------------------------------------------------------------------------ launches
#ifdef __HIPCC__
template <int FMT>
static void launch_camera_field_fmt(const CamFieldArgs &a, int surface, dim3 grid, hipStream_t stream)
{
    const dim3 block(kCamPiece);
    if (surface == kCamPlane) hipLaunchKernelGGL((k_camera_field<FMT, kCamPlane>), grid, block, 0, stream, a, a.records, a.frames, a.field);
    else if (surface == kCamCylinder) hipLaunchKernelGGL((k_camera_field<FMT, kCamCylinder>), grid, block, 0, stream, a, a.records, a.frames, a.field);
    else hipLaunchKernelGGL((k_camera_field<FMT, kCamSphere>), grid, block, 0, stream, a, a.records, a.frames, a.field);
}

void launch_camera_field(const CamFieldArgs &a, int fmt, int surface, hipStream_t stream)
{
    if (a.n_frames <= 0 || a.max_h <= 0 || a.max_w <= 0) return;
    const dim3 grid((unsigned)((int64_t)a.n_pieces * cam_bands(a.max_h)), a.n_frames);      // (below 2^31: the API refuses beyond)
    if (fmt == 0) launch_camera_field_fmt<0>(a, surface, grid, stream);
    else launch_camera_field_fmt<1>(a, surface, grid, stream);
}

void launch_camera_points(const CamPointArgs &a, bool to_source, hipStream_t stream)
{
    if (a.n_frames <= 0 || a.n_pts <= 0) return;
    const dim3 grid((a.n_pts + 255) / 256, a.n_frames), block(256);
    if (to_source) hipLaunchKernelGGL(k_camera_points<true>, grid, block, 0, stream, a, a.records, a.points, a.out);
    else hipLaunchKernelGGL(k_camera_points<false>, grid, block, 0, stream, a, a.records, a.points, a.out);
}
#endif

} // namespace hg
