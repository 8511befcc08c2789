// hg_k_points.hip -- POINT LISTS through the warp geometry of a frame set: k_geo_points, k_pw_points_src, k_points_from_map, k_pw_points_out
// (include/hgwarp.h, hg_points_*).  Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  Geometry only, like the fields (hg_k_field.hip):
// fp64 coordinate math in the reference's operation order (contraction off), no source read at all, each result rounded once to f32.
// Grid of every kernel: blockIdx.y = frame, blockIdx.x = blocks of 256 points, one point per lane; frame f reads list f % n_sets and writes
// n_points pairs at f * n_points.  An unmapped point holds 0x7fc00000 in both words, the pattern of HG_FIELD_COORDS.
// MEASURED (EXPERIMENTS.md P.1, 64 4K frames): k_pw_points_src at 65536 points per frame and 5000 triangles is 33x SLOWER than the full-frame
// coords field call it stands in for (79 ms against 2.4 ms); also 3.5x slower at 65536 points / 200 triangles and 1.7x at 68 points / 5000
// triangles; it wins at 68 points / 200 triangles (0.22x).  Every wave walks every triangle, and with unsorted points the per-wave row
// reject removes next to nothing.  Not tuned here (bands, sorted lists: out of scope); dense lists should go through the field and a gather.
// Citations are file:line into the reference's Homography.js (v1.8.0).  Design notes: DESIGN.md §4.10.
#include "hg_dev.h"

namespace hg {

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr uint32_t kPointNaN = 0x7fc00000u;      // both words of an unmapped point (== kFieldNaN of hg_k_field.hip)
constexpr int kPtsBlock = 256;                   // points per workgroup
constexpr int kPtsTriChunk = 256;                // TriRange records k_pw_points_src stages in LDS per step (one per thread)

// The cell of a point: (Math.round(x), Math.round(y)), ties toward +Infinity (-0.5 belongs to cell 0), tested against [0, w) x [0, h) IN
// DOUBLES -- NaN fails every compare, floor(+-Inf) - (+-Inf) is NaN and leaves r infinite, 1e30 is simply too large -- and converted to
// integers only once it is known to lie inside.
__device__ __forceinline__ bool point_cell(float px, float py, double x0, double y0, double w, double h, int &cx, int &cy)
{
    const double x = (double)px, y = (double)py;
    double rx = floor(x), ry = floor(y);
    if (x - rx >= 0.5) rx += 1.0;                   // (x - floor(x) is exact)
    if (y - ry >= 0.5) ry += 1.0;
    rx -= x0; ry -= y0;                             // (integers below 2^31 minus integers below 2^31: exact)
    const bool in = rx >= 0.0 && rx < w && ry >= 0.0 && ry < h;
    cx = in ? (int)rx : 0; cy = in ? (int)ry : 0;
    return in;
}

__device__ __forceinline__ void point_store(float *__restrict__ out, size_t i, bool mapped, double x, double y)
{
    v2f v = { __int_as_float((int)kPointNaN), __int_as_float((int)kPointNaN) };
    if (mapped) { v.x = (float)x; v.y = (float)y; }     // the one rounding to f32
    *reinterpret_cast<v2f *>(out + 2 * i) = v;
}

// ------------------------------------------------------------------------------------------------ k_geo_points
// DIR 0, to source (:997-1011 at a position that need not be a pixel): the point (u, v) is in window coordinates; it maps iff its cell lies
// in the window and transform(inverse matrix, u + xOff, v + yOff) passes the coverage test :1001 -- for integer (u, v) k_geo_field's value.
// DIR 1, to output (:919-926): the point is in source pixels; it maps iff its cell lies in [0, W) x [0, H), the loop's domain, and the result
// is transform(forward matrix, px, py) - (xOff, yOff), the value :924 hands to Math.round, reported wherever it falls.
// apply_affine / apply_projective (hg_math.h) with IEEE divisions, as k_geo_field.  mats = F x 8 doubles.
template <int KIND, int DIR>
__global__ __launch_bounds__(kPtsBlock) void k_geo_points(const FrameDesc *__restrict__ frames, const double *__restrict__ mats, int W, int H,
                                                          const float *__restrict__ points, int n_points, int n_sets, float *__restrict__ out)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * kPtsBlock + threadIdx.x;
    if (i >= n_points) return;                               // the tail: nothing is written past n_points
    const FrameDesc fd = frames[f];
    double m[8];
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = mats[(size_t)f * 8 + k];
    const v2f p = *reinterpret_cast<const v2f *>(points + 2 * ((size_t)(f % n_sets) * n_points + i));
    const size_t o = (size_t)f * n_points + i;
    int cx, cy;
    double rx, ry;
    if (DIR == 0) {
        bool ok = point_cell(p.x, p.y, 0.0, 0.0, (double)fd.obj_w, (double)fd.obj_h, cx, cy);      // (an empty window holds no cell)
        const double x = (double)p.x + (double)fd.x_off, y = (double)p.y + (double)fd.y_off;
        if (KIND == 0) apply_affine(m, x, y, rx, ry); else apply_projective(m, x, y, rx, ry);      // :999
        ok = ok && rx >= 0 && rx < (double)W && ry >= 0 && ry < (double)H;                          // :1001 (NaN fails)
        point_store(out, o, ok, rx, ry);
    } else {
        const bool ok = point_cell(p.x, p.y, 0.0, 0.0, (double)W, (double)H, cx, cy);               // :919-920
        if (KIND == 0) apply_affine(m, (double)p.x, (double)p.y, rx, ry); else apply_projective(m, (double)p.x, (double)p.y, rx, ry);   // :923
        point_store(out, o, ok, rx - (double)fd.x_off, ry - (double)fd.y_off);                      // :924
    }
}

// ------------------------------------------------------------------------------------------------ k_pw_points_src
// To source, piecewise (:1042-1056 at a position that need not be a pixel), behind k_tri_setup and WITHOUT a map: the triangle of a point is
// the id the reference's map holds at the point's cell -- the largest id whose fillTriangle spans cover flat index r * objW + c, fill()'s
// wrap of negative indices included -- which is k_pw_field's resolve turned inside out: there a row's workgroup lists the spans of its row
// and every pixel takes the largest covering id; here a lane owns one cell and walks the triangles.
//   * The triangle loop is wave-uniform.  The TriRange records go through LDS, kPtsTriChunk at a time (one coalesced 16-byte load per
//     thread, then broadcast reads turned into scalar registers), the three edge equations of a triangle that survives the reject are read
//     at a uniform address (scalar loads), once per wave.
//   * The cheap reject comes first: with fused_row_spans' bounds, rows y of triangle t can reach output row r only for
//     (y - yOff) in [r - a, r - b] ("image" 0) or objH rows further up ("image" 1: negative indices wrapped by +len); a triangle none of
//     whose rows can reach the row of any lane of the wave costs one ballot.
//   * Each lane then evaluates span_cells for its rows of the triangle and keeps max(id) over the spans that contain its flat index.
// Then pw_coord (hg_dev.h): pw_pixel's arithmetic up to the coordinate and the bounds test :1047 with the frame's minSrc, applied to the
// point itself.  A frame k_tri_setup marked FRAME_IRREGULAR is skipped and redone by the host through the map (k_points_from_map); there
// is no span list, hence no overflow.  An empty window holds no cell: all its points are unmapped.
__global__ __launch_bounds__(kPtsBlock) void k_pw_points_src(PwMesh mesh, PwFrames fr, const float *__restrict__ points, int n_points, int n_sets,
                                                             float *__restrict__ out)
{
    const int f = blockIdx.y;
    const FrameDesc fd = fr.frames[f];
    const int i = blockIdx.x * kPtsBlock + threadIdx.x;
    const bool live = i < n_points;
    const size_t o = (size_t)f * n_points + (live ? i : 0);
    if (fd.obj_w <= 0 || fd.obj_h <= 0) {                    // (uniform over the workgroup, like every return in front of the barriers)
        if (live) point_store(out, o, false, 0.0, 0.0);
        return;
    }
    if (fr.status[f] & FRAME_IRREGULAR) return;              // written by k_tri_setup (previous kernel on this stream)

    __shared__ TriRange s_tr[kPtsTriChunk];
    const int T = mesh.n_tris, W = fd.obj_w;
    const int64_t len = (int64_t)W * fd.obj_h;
    v2f p = { 0.f, 0.f };
    if (live) p = *reinterpret_cast<const v2f *>(points + 2 * ((size_t)(f % n_sets) * n_points + i));
    int cx, cy;
    const bool in = point_cell(p.x, p.y, 0.0, 0.0, (double)W, (double)fd.obj_h, cx, cy) && live;
    const int64_t cell = (int64_t)cy * W + cx;
    const TriRange *__restrict__ trir = fr.trir + (size_t)f * T;
    const Seg *__restrict__ segs = fr.segs + (size_t)f * T * 3;
    int best = -1;
    for (int t0 = 0; t0 < T; t0 += kPtsTriChunk) {
        __syncthreads();                                     // (the previous chunk has been walked by every wave)
        if (t0 + (int)threadIdx.x < T) s_tr[threadIdx.x] = trir[t0 + threadIdx.x];
        __syncthreads();
        const int n = min(kPtsTriChunk, T - t0);
        for (int j = 0; j < n; j++) {
            TriRange tr;                                     // one LDS broadcast, moved to scalar registers: the loop's control flow is the wave's
            tr.y_min = __builtin_amdgcn_readfirstlane(s_tr[j].y_min); tr.y_end = __builtin_amdgcn_readfirstlane(s_tr[j].y_end);
            tr.a = __builtin_amdgcn_readfirstlane(s_tr[j].a); tr.b = __builtin_amdgcn_readfirstlane(s_tr[j].b);
            if (tr.y_end <= tr.y_min) continue;
            // the rows of this triangle that can reach the lane's output row, per image (fused_row_spans' enumeration)
            const int64_t top = (int64_t)tr.y_end - 1;
            int64_t ylo0 = (int64_t)cy - tr.a + fd.y_off, yhi0 = (int64_t)cy - tr.b + fd.y_off;
            int64_t ylo1 = ylo0 - fd.obj_h, yhi1 = yhi0 - fd.obj_h;
            if (ylo0 < tr.y_min) ylo0 = tr.y_min;
            if (yhi0 > top) yhi0 = top;
            if (ylo1 < tr.y_min) ylo1 = tr.y_min;
            if (yhi1 > top) yhi1 = top;
            const bool reach = in && (ylo0 <= yhi0 || ylo1 <= yhi1);
            if (!__any(reach)) continue;                     // the row-range reject: no span_cells, no edge equations
            const int t = t0 + j;
            const Seg sg[3] = { segs[3 * (size_t)t], segs[3 * (size_t)t + 1], segs[3 * (size_t)t + 2] };
            if (!reach) continue;
#pragma unroll 1
            for (int image = 0; image < 2; image++) {        // 0: indices >= 0;  1: negative indices wrapped by +len (= +objH rows)
                const int64_t ylo = image ? ylo1 : ylo0, yhi = image ? yhi1 : yhi0;
#pragma unroll 1
                for (int64_t y = ylo; y <= yhi; y++) {
                    int64_t k, fin;
                    span_cells(sg, (double)y, (double)fd.y_off, (double)W, len, k, fin);
                    if (cell >= k && cell < fin) best = max(best, t);      // "last writer wins" of the sequential fill loop :852-858 == largest id
                }
            }
        }
    }
    if (!live) return;
    const int2 ms = frame_min_src(mesh, fr, f);              // this frame's source minima
    const double bx0 = (double)ms.x, bx1 = (double)mesh.W + (double)ms.x;    // :1047
    const double by0 = (double)ms.y, by1 = (double)mesh.H + (double)ms.y;
    MatCache mc; mc.id = -1;
    double sx = 0.0, sy = 0.0;
    const bool cov = in && pw_coord(best, (double)p.x + (double)fd.x_off, (double)p.y + (double)fd.y_off, mc,
                                    fr.inv + (size_t)f * T * kInvStride, bx0, bx1, by0, by1, sx, sy);
    point_store(out, o, cov, sx, sy);
}

// ------------------------------------------------------------------------------------------------ k_points_from_map
// The redo of a flagged frame: k_map_fill (hg_k_map.hip) has materialised the frame's triangle map, the id of a point is map32 at its cell.
// points / out: the frame's own list and results.
__global__ __launch_bounds__(kPtsBlock) void k_points_from_map(PwMesh mesh, const float *__restrict__ invm, const int2 *__restrict__ min_src, FrameDesc fd,
                                                               const int32_t *__restrict__ map32, const float *__restrict__ points, int n_points,
                                                               float *__restrict__ out)
{
    const int i = blockIdx.x * kPtsBlock + threadIdx.x;
    if (i >= n_points) return;
    const v2f p = *reinterpret_cast<const v2f *>(points + 2 * (size_t)i);
    int cx, cy;
    const bool in = point_cell(p.x, p.y, 0.0, 0.0, (double)fd.obj_w, (double)fd.obj_h, cx, cy);
    const int tid = in ? map32[(int64_t)cy * fd.obj_w + cx] : -1;        // (the bounds check comes before the load)
    const int2 ms = min_src ? make_int2(__builtin_amdgcn_readfirstlane(min_src->x), __builtin_amdgcn_readfirstlane(min_src->y)) : make_int2(mesh.min_src_x, mesh.min_src_y);
    const double bx0 = (double)ms.x, bx1 = (double)mesh.W + (double)ms.x;
    const double by0 = (double)ms.y, by1 = (double)mesh.H + (double)ms.y;
    MatCache mc; mc.id = -1;
    double sx = 0.0, sy = 0.0;
    const bool cov = pw_coord(tid, (double)p.x + (double)fd.x_off, (double)p.y + (double)fd.y_off, mc, invm, bx0, bx1, by0, by1, sx, sy);
    point_store(out, (size_t)i, cov, sx, sy);
}

// ------------------------------------------------------------------------------------------------ k_pw_points_out
// To output, piecewise (:955-964 at a position that need not be a pixel): the cell of the point, relative to (minSrcX, minSrcY), must lie in
// the forward map [0, maxSrcX - minSrcX) x [0, maxSrcY - minSrcY) (:817-832, the map the forward warps build and cache) and hold an id > -1
// (:957-958, the Int16Array value); the result is that id's forward matrix (:785-804, f32 entries widened) applied to the point itself,
// minus the window's offsets (:962).  One gather from the map, six floats of fr.fwd, one store.
__global__ __launch_bounds__(kPtsBlock) void k_pw_points_out(const int32_t *__restrict__ fmap, const float *__restrict__ fwd, const FrameDesc *__restrict__ frames,
                                                             int T, int min_src_x, int min_src_y, int map_w, int map_h,
                                                             const float *__restrict__ points, int n_points, int n_sets, float *__restrict__ out)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * kPtsBlock + threadIdx.x;
    if (i >= n_points) return;
    const FrameDesc fd = frames[f];
    const v2f p = *reinterpret_cast<const v2f *>(points + 2 * ((size_t)(f % n_sets) * n_points + i));
    int mx, my;
    const bool in = point_cell(p.x, p.y, (double)min_src_x, (double)min_src_y, (double)map_w, (double)map_h, mx, my);
    const int t16 = in ? (int)(int16_t)fmap[(int64_t)my * map_w + mx] : -1;      // :957 (cell < 2^31: forward_limits)
    double nx = 0.0, ny = 0.0;
    if (t16 > -1) {                                                             // :958
        const float *mf = fwd + ((size_t)f * T + t16) * 6;
        const double m[6] = { mf[0], mf[1], mf[2], mf[3], mf[4], mf[5] };
        apply_affine(m, (double)p.x, (double)p.y, nx, ny);                      // :961
    }
    point_store(out, (size_t)f * n_points + i, t16 > -1, nx - (double)fd.x_off, ny - (double)fd.y_off);     // :962
}

// ------------------------------------------------------------------------------------------------ launchers
static dim3 points_grid(int n_points, int n_frames) { return dim3((unsigned)((n_points + kPtsBlock - 1) / kPtsBlock), (unsigned)n_frames); }

void launch_geo_points(int kind, int dir, const FrameDesc *frames, const double *mats, int n_frames, int W, int H, const float *points, int n_points,
                       int n_sets, float *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_points <= 0) return;
    const dim3 grid = points_grid(n_points, n_frames);
#define HG_GP(K, D) hipLaunchKernelGGL((k_geo_points<K, D>), grid, dim3(kPtsBlock), 0, stream, frames, mats, W, H, points, n_points, n_sets, out)
    if (kind == 0) { if (dir == 0) HG_GP(0, 0); else HG_GP(0, 1); }
    else           { if (dir == 0) HG_GP(1, 0); else HG_GP(1, 1); }
#undef HG_GP
}

void launch_pw_points_src(const PwMesh &mesh, const PwFrames &fr, const float *points, int n_points, int n_sets, float *out, hipStream_t stream)
{
    if (fr.n_frames <= 0 || n_points <= 0) return;
    hipLaunchKernelGGL(k_pw_points_src, points_grid(n_points, fr.n_frames), dim3(kPtsBlock), 0, stream, mesh, fr, points, n_points, n_sets, out);
}

void launch_points_from_map(const PwMesh &mesh, const PwFrames &fr, int f, const FrameDesc &fd, const int32_t *map32, const float *points,
                            int n_points, int n_sets, float *out, hipStream_t stream)
{
    if (n_points <= 0 || fd.obj_w <= 0 || fd.obj_h <= 0) return;
    const float *invm = fr.inv + (size_t)f * mesh.n_tris * kInvStride;
    const int2 *ms = fr.min_src ? fr.min_src + f : nullptr;
    hipLaunchKernelGGL(k_points_from_map, points_grid(n_points, 1), dim3(kPtsBlock), 0, stream, mesh, invm, ms, fd, map32,
                       points + 2 * (size_t)(f % n_sets) * n_points, n_points, out + 2 * (size_t)f * n_points);
}

void launch_pw_points_out(const int32_t *fmap, const float *fwd, const FrameDesc *frames, int n_frames, int T, int min_src_x, int min_src_y,
                          int map_w, int map_h, const float *points, int n_points, int n_sets, float *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_points <= 0) return;
    hipLaunchKernelGGL(k_pw_points_out, points_grid(n_points, n_frames), dim3(kPtsBlock), 0, stream, fmap, fwd, frames, T, min_src_x, min_src_y,
                       map_w, map_h, points, n_points, n_sets, out);
}

} // namespace hg
