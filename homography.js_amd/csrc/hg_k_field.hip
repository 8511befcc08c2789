// hg_k_field.hip -- the SOURCE FIELD of the inverse warps: k_geo_field, k_pw_field, k_field_from_map (include/hgwarp.h, HG_FIELD_*; the
// remaps that consume a field: hg_k_remap.hip).
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  The field kernels are write streams: fp64 coordinate math in the reference's
// operation order (contraction off), no source read at all; what they store is what the nearest loops would have indexed (HG_FIELD_INDEX)
// or the coordinate they would have rounded (HG_FIELD_COORDS).  Stores are non-temporal: a field is written once and must not evict the source.
// Citations are file:line into the reference's Homography.js (v1.8.0).  Design notes: DESIGN.md §4.9.
#include "hg_dev.h"
#include "hg_field_dev.h"

namespace hg {

// ------------------------------------------------------------------------------------------------ k_geo_field
// The field of _inverseGeometricWarp :997-1011 for all frames of a set in one launch (blockIdx.y = frame; frames == nullptr: one frame carried
// by value).  One wave per output row (4 rows per workgroup) walking 256-pixel windows; lane l owns pixels c0 + l + 64k, so every store
// instruction of the wave covers 64 consecutive pixels: 256 bytes of indices, 512 bytes of coordinates (one 8-byte store per lane).
// apply_affine / apply_projective (hg_math.h) with IEEE divisions: the same bits as every warp kernel's coordinate.  fd.out_off: where the
// frame's FIELD starts (the host stages the frame records with the field offsets in that place).
template <int KIND, int FMT>
__global__ __launch_bounds__(256) void k_geo_field(const FrameDesc *__restrict__ frames, const double *__restrict__ mats, GeoFieldOne one,
                                                   int W, int H, uint8_t *__restrict__ field)
{
    const int fz = blockIdx.y;
    const FrameDesc fd = frames ? frames[fz] : one.fd;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int OW = fd.obj_w;
    if (r >= fd.obj_h || OW <= 0) return;
    double m[8];
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = frames ? mats[(size_t)fz * 8 + k] : one.m[k];
    const int lane = threadIdx.x;
    const double y = (double)(r + fd.y_off);
    const double bw = (double)W, bh = (double)H, n_src_px = bw * bh;
    uint8_t *__restrict__ row = field + fd.out_off + (uint64_t)r * (uint64_t)OW * (FMT == 0 ? 4 : 8);
    for (int64_t c0 = 0; c0 < OW; c0 += 256) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t c = c0 + lane + 64 * k;
            if (c >= OW) continue;                           // the tail: nothing is written past obj_w
            const double x = (double)(c + fd.x_off);
            double sx, sy;
            if (KIND == 0) apply_affine(m, x, y, sx, sy); else apply_projective(m, x, y, sx, sy);     // :999
            const bool cov = sx >= 0 && sx < bw && sy >= 0 && sy < bh;                               // :1001 (NaN fails)
            int vx, vy;
            field_px<FMT>(cov, sx, sy, bw, n_src_px, vx, vy);
            if (FMT == 0) __builtin_nontemporal_store(vx, reinterpret_cast<int *>(row) + c);
            else { v2f v = { __int_as_float(vx), __int_as_float(vy) }; __builtin_nontemporal_store(v, reinterpret_cast<v2f *>(row) + c); }
        }
    }
}

// ------------------------------------------------------------------------------------------------ k_pw_field
// The field of _inversePiecewiseAffineWarp :1029-1058: k_pw_fused (hg_k_piecewise.hip) with another pixel body.  One workgroup per output
// row of one frame; the span prologue (every (triangle, source row) whose fillTriangle span can touch the row, clipped, into an LDS list) and
// the "largest covering id wins" resolve are that kernel's, and so is the flag protocol: a row of more than kRowSpanCap spans flags its frame
// FRAME_LDS_OVERFLOW, a frame k_tri_setup marked FRAME_IRREGULAR is skipped -- the host redoes both through the map (k_field_from_map).
// The pixel body is pw_pixel's arithmetic up to the coordinate and the bounds test :1047; it reads no source.
template <int FMT>
__device__ __forceinline__ void pw_field_px(int tid_raw, int x, double y, MatCache &mc, const float *__restrict__ invm, double w, double n_src_px,
                                            double bx0, double bx1, double by0, double by1, int &vx, int &vy)
{
    const int t16 = (int)(int16_t)tid_raw;          // Int16Array element conversion (ids >= 32768 wrap)
    bool cov = false;
    double sx = 0.0, sy = 0.0;
    if (t16 >= 0) {                                 // :1045
        if (t16 != mc.id) {
            const float4 lo = *reinterpret_cast<const float4 *>(invm + (size_t)t16 * kInvStride);
            const float2 hi = *reinterpret_cast<const float2 *>(invm + (size_t)t16 * kInvStride + 4);
            mc.m[0] = lo.x; mc.m[1] = lo.y; mc.m[2] = lo.z; mc.m[3] = lo.w; mc.m[4] = hi.x; mc.m[5] = hi.y;
            mc.id = t16;
        }
        const double xd = (double)x;
        sx = (mc.m[0] * xd) + (mc.m[2] * y) + mc.m[4];      // :1383
        sy = (mc.m[1] * xd) + (mc.m[3] * y) + mc.m[5];      // :1384
        cov = sx >= bx0 && sx < bx1 && sy >= by0 && sy < by1;   // :1047 (unrounded; NaN fails)
    }
    field_px<FMT>(cov, sx, sy, w, n_src_px, vx, vy);
}

template <int FMT>
__global__ __launch_bounds__(256) void k_pw_field(PwMesh mesh, PwFrames fr, uint8_t *__restrict__ field)
{
    const int f = blockIdx.y;
    const FrameDesc fd = fr.frames[f];
    const int r = blockIdx.x;
    if (r >= fd.obj_h || fd.obj_w <= 0) return;
    if (fr.status[f] & FRAME_IRREGULAR) return;      // written by k_tri_setup (previous kernel on this stream)

    __shared__ int s_lo[kRowSpanCap], s_hi[kRowSpanCap], s_id[kRowSpanCap];
    __shared__ int s_cnt;
    const int T = mesh.n_tris, W = fd.obj_w;
    const int64_t row0 = (int64_t)r * W;
    const int cnt = fused_row_spans(fr, f, T, fd, r, s_lo, s_hi, s_id, &s_cnt);
    if (cnt > kRowSpanCap) {                         // the frame is redone through the materialised map by the host
        if (threadIdx.x == 0) flag_frame(fr, f, FRAME_LDS_OVERFLOW);
        return;
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwin = (W + 255) >> 8;
    const float *__restrict__ invm = fr.inv + (size_t)f * T * kInvStride;
    constexpr int PX = FMT == 0 ? 4 : 8;
    uint8_t *__restrict__ orow = field + fd.out_off + (uint64_t)row0 * PX;
    const bool vec_ok = ((W & 3) == 0) && ((reinterpret_cast<uintptr_t>(field + fd.out_off) & 15) == 0);
    const double y = (double)(r + fd.y_off);
    const int2 ms = frame_min_src(mesh, fr, f);              // this frame's source minima
    const double bx0 = (double)ms.x, bx1 = (double)mesh.W + (double)ms.x;    // :1047
    const double by0 = (double)ms.y, by1 = (double)mesh.H + (double)ms.y;
    const double sw = (double)mesh.W, n_src_px = sw * (double)mesh.H;

    for (int w = wave; w < nwin; w += 4) {
        const int c0 = w << 8, cq = c0 + (lane << 2);
        int tid[4];
        fused_resolve_quad(s_lo, s_hi, s_id, cnt, c0, lane, tid);
        if (cq < W) {
            int vx[4], vy[4];
            MatCache mc; mc.id = -1;
#pragma unroll
            for (int k = 0; k < 4; k++)
                pw_field_px<FMT>(tid[k], cq + k + fd.x_off, y, mc, invm, sw, n_src_px, bx0, bx1, by0, by1, vx[k], vy[k]);
            field_store_quad<FMT>(orow, cq, W, vec_ok, vx, vy);
        }
    }
}

// ------------------------------------------------------------------------------------------------ k_field_from_map
// The redo of a flagged frame: k_map_fill (hg_k_map.hip) has materialised the frame's triangle map, this is the pixel loop :1042-1056 over it
// with the field body.  Block = 64 x 4 threads = 4 rows x 256 pixels, like k_pw_from_map.  `frame`: where this frame's field starts.
template <int FMT>
__global__ __launch_bounds__(256) void k_field_from_map(PwMesh mesh, const float *__restrict__ invm, const int2 *__restrict__ min_src, FrameDesc fd,
                                                        const int32_t *__restrict__ map32, uint8_t *__restrict__ frame)
{
    const int r = blockIdx.y * 4 + threadIdx.y;
    const int cq = (blockIdx.x * 64 + threadIdx.x) << 2;
    const int W = fd.obj_w;
    if (r >= fd.obj_h || cq >= W) return;
    const int64_t row0 = (int64_t)r * W;
    constexpr int PX = FMT == 0 ? 4 : 8;
    uint8_t *__restrict__ orow = frame + (uint64_t)row0 * PX;
    const bool vec_ok = ((W & 3) == 0) && ((reinterpret_cast<uintptr_t>(frame) & 15) == 0);
    const double y = (double)(r + fd.y_off);
    const int2 ms = min_src ? make_int2(__builtin_amdgcn_readfirstlane(min_src->x), __builtin_amdgcn_readfirstlane(min_src->y)) : make_int2(mesh.min_src_x, mesh.min_src_y);
    const double bx0 = (double)ms.x, bx1 = (double)mesh.W + (double)ms.x;
    const double by0 = (double)ms.y, by1 = (double)mesh.H + (double)ms.y;
    const double sw = (double)mesh.W, n_src_px = sw * (double)mesh.H;
    int vx[4], vy[4];
    MatCache mc; mc.id = -1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int tid = (cq + k < W) ? map32[row0 + cq + k] : -1;
        pw_field_px<FMT>(tid, cq + k + fd.x_off, y, mc, invm, sw, n_src_px, bx0, bx1, by0, by1, vx[k], vy[k]);
    }
    field_store_quad<FMT>(orow, cq, W, vec_ok, vx, vy);
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_geo_field(int kind, int fmt, const FrameDesc *frames, const double *mats, const GeoFieldOne &one, int n_frames, int max_h,
                      int W, int H, uint8_t *field, hipStream_t stream)
{
    if (n_frames <= 0 || max_h <= 0) return;
    dim3 grid((max_h + 3) / 4, n_frames);
#define HG_GF(K, F) hipLaunchKernelGGL((k_geo_field<K, F>), grid, dim3(64, 4), 0, stream, frames, mats, one, W, H, field)
    if (kind == 0) { if (fmt == 0) HG_GF(0, 0); else HG_GF(0, 1); }
    else           { if (fmt == 0) HG_GF(1, 0); else HG_GF(1, 1); }
#undef HG_GF
}

void launch_pw_field(const PwMesh &mesh, const PwFrames &fr, int fmt, uint8_t *field, hipStream_t stream)
{
    if (fr.n_frames <= 0 || fr.max_obj_h <= 0) return;
    dim3 grid(fr.max_obj_h, fr.n_frames);
    if (fmt == 0) hipLaunchKernelGGL(k_pw_field<0>, grid, dim3(256), 0, stream, mesh, fr, field);
    else          hipLaunchKernelGGL(k_pw_field<1>, grid, dim3(256), 0, stream, mesh, fr, field);
}

void launch_field_from_map(const PwMesh &mesh, const PwFrames &fr, int f, const FrameDesc &fd, const int32_t *map32, int fmt, uint8_t *field,
                           hipStream_t stream)
{
    if (fd.obj_w <= 0 || fd.obj_h <= 0) return;
    dim3 grid((fd.obj_w + 255) / 256, (fd.obj_h + 3) / 4);
    const float *invm = fr.inv + (size_t)f * mesh.n_tris * kInvStride;
    const int2 *ms = fr.min_src ? fr.min_src + f : nullptr;
    if (fmt == 0) hipLaunchKernelGGL(k_field_from_map<0>, grid, dim3(64, 4), 0, stream, mesh, invm, ms, fd, map32, field + fd.out_off);
    else          hipLaunchKernelGGL(k_field_from_map<1>, grid, dim3(64, 4), 0, stream, mesh, invm, ms, fd, map32, field + fd.out_off);
}

} // namespace hg
