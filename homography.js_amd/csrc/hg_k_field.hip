// hg_k_field.hip -- the SOURCE FIELD of the inverse warps and the remaps that consume it: k_geo_field, k_pw_field, k_field_from_map,
// k_remap_index, k_remap_bilinear_f32 and their whole-frame-set forms k_remap_index_frames, k_remap_bilinear_frames (include/hgwarp.h, HG_FIELD_*).
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  The field kernels are write streams: fp64 coordinate math in the reference's
// operation order (contraction off), no source read at all; what they store is what the nearest loops would have indexed (HG_FIELD_INDEX)
// or the coordinate they would have rounded (HG_FIELD_COORDS).  Stores are non-temporal: a field is written once and must not evict the source.
// Citations are file:line into the reference's Homography.js (v1.8.0).  Design notes: DESIGN.md §4.9.
#include "hg_dev.h"

namespace hg {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr uint32_t kFieldNaN = 0x7fc00000u;      // both words of an uncovered pixel of HG_FIELD_COORDS

// HG_FIELD_INDEX of a pixel that passed the coverage test: Math.round(sy) * W + Math.round(sx) (:1005 / :1049) where that lies in the array,
// else -1 (JS reads `undefined`, stored as 0).  In doubles: exact below 2^53, and a product beyond that is far outside [0, n_src_px) either way.
__device__ __forceinline__ int field_index(double sx, double sy, double w, double n_src_px)
{
    double rx = floor(sx), ry = floor(sy);
    if (sx - rx >= 0.5) rx += 1.0;
    if (sy - ry >= 0.5) ry += 1.0;
    const double idx = ry * w + rx;
    return (idx >= 0.0 && idx < n_src_px) ? (int)idx : -1;
}

// One pixel's field value: FMT 0 -> x = index; FMT 1 -> (x, y) = bit patterns of ((float)sx, (float)sy) or of the quiet NaN.
template <int FMT>
__device__ __forceinline__ void field_px(bool covered, double sx, double sy, double w, double n_src_px, int &x, int &y)
{
    if (FMT == 0) { x = covered ? field_index(sx, sy, w, n_src_px) : -1; y = 0; }
    else { x = covered ? __float_as_int((float)sx) : (int)kFieldNaN; y = covered ? __float_as_int((float)sy) : (int)kFieldNaN; }
}

// Four consecutive pixels of one row, starting at column cq (16-byte non-temporal stores where the row pitch and the frame's start allow it).
template <int FMT>
__device__ __forceinline__ void field_store_quad(uint8_t *__restrict__ row, int cq, int W, bool vec_ok, const int vx[4], const int vy[4])
{
    if (FMT == 0) {
        int *__restrict__ p = reinterpret_cast<int *>(row) + cq;
        if (vec_ok && cq + 3 < W) { v4i v = { vx[0], vx[1], vx[2], vx[3] }; __builtin_nontemporal_store(v, reinterpret_cast<v4i *>(p)); }
        else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (cq + k < W) __builtin_nontemporal_store(vx[k], p + k);
        }
    } else {
        int *__restrict__ p = reinterpret_cast<int *>(row) + 2 * (size_t)cq;
        if (vec_ok && cq + 3 < W) {
            v4i a = { vx[0], vy[0], vx[1], vy[1] }, b = { vx[2], vy[2], vx[3], vy[3] };
            __builtin_nontemporal_store(a, reinterpret_cast<v4i *>(p));
            __builtin_nontemporal_store(b, reinterpret_cast<v4i *>(p) + 1);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (cq + k < W) { __builtin_nontemporal_store(vx[k], p + 2 * k); __builtin_nontemporal_store(vy[k], p + 2 * k + 1); }
        }
    }
}

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

// ------------------------------------------------------------------------------------------------ remaps
// out[i] = 0 <= field[i] < n_src ? src[field[i]] : all-zero, pixels being opaque blocks of sizeof(T) bytes.  One pixel per lane, grid-stride;
// the range check comes before the load, so no read leaves [0, n_src) whatever the field holds.
template <typename T>
__global__ __launch_bounds__(256) void k_remap_index(const int32_t *__restrict__ fld, size_t n, const T *__restrict__ src, size_t n_src, T *__restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int32_t v = fld[i];
        T px = T();
        if (v >= 0 && (size_t)v < n_src) px = src[(size_t)v];
        out[i] = px;
    }
}

// Column / row of a tap: clamp(v, 0, n - 1) for an integer-valued finite float v, clamped in float first so that the conversion is defined
// for any magnitude (2147483520 is the largest float below 2^31).
__device__ __forceinline__ int remap_tap(float v, int n)
{
    return min((int)fminf(fmaxf(v, 0.0f), 2147483520.0f), n - 1);
}

// Bilinear remap of C interleaved f32 channels through a HG_FIELD_COORDS field.  A NaN or infinite coordinate gives zeros; otherwise
// x0 = floorf(sx), fx = sx - x0, taps clamp(x0, 0, W-1) and clamp(x0 + 1, 0, W-1) (the +1 in f32), rows alike, and blend4's operation order
// per channel in f32 (contraction off): v = (p00*(1-fx) + p01*fx)*(1-fy) + (p10*(1-fx) + p11*fx)*fy, stored as it is.
template <int C>
__global__ __launch_bounds__(256) void k_remap_bilinear_f32(const float *__restrict__ coords, size_t n, const float *__restrict__ src, int W, int H,
                                                            float *__restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float2 s = reinterpret_cast<const float2 *>(coords)[i];
        float v[C];
#pragma unroll
        for (int ch = 0; ch < C; ch++) v[ch] = 0.0f;
        if (fabsf(s.x) < INFINITY && fabsf(s.y) < INFINITY) {            // (NaN compares false)
            const float x0 = floorf(s.x), y0 = floorf(s.y);
            const float fx = s.x - x0, fy = s.y - y0, gx = 1.0f - fx, gy = 1.0f - fy;
            const int64_t c0 = remap_tap(x0, W), c1 = remap_tap(x0 + 1.0f, W);
            const int64_t r0 = (int64_t)remap_tap(y0, H) * W, r1 = (int64_t)remap_tap(y0 + 1.0f, H) * W;
            const float *__restrict__ p00 = src + (r0 + c0) * C, *__restrict__ p01 = src + (r0 + c1) * C;
            const float *__restrict__ p10 = src + (r1 + c0) * C, *__restrict__ p11 = src + (r1 + c1) * C;
#pragma unroll
            for (int ch = 0; ch < C; ch++) v[ch] = (p00[ch] * gx + p01[ch] * fx) * gy + (p10[ch] * gx + p11[ch] * fx) * fy;
        }
#pragma unroll
        for (int ch = 0; ch < C; ch++) out[i * C + ch] = v[ch];
    }
}

// ------------------------------------------------------------------------------------------------ remaps of whole frame sets
// One launch for all frames: block b belongs to the last frame whose blk0 <= b (a binary search over the device frame table, uniform over the
// block, so scalar loads) and covers blk_px consecutive pixels of that frame's flat list.  Empty frames own no block.
__device__ __forceinline__ RemapFrame remap_frame_of(const RemapFrame *__restrict__ frames, int n, uint32_t b)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (frames[mid].blk0 <= b) lo = mid; else hi = mid;
    }
    return frames[lo];
}

template <typename T>
__device__ __forceinline__ T remap_gather(int32_t v, const T *__restrict__ src, size_t n_src)
{
    T px = T();
    if (v >= 0 && (size_t)v < n_src) px = src[(size_t)v];    // the range check comes before the load
    return px;
}

// Four consecutive pixels in one store of 4 * sizeof(T) bytes (16 bytes at a time beyond that); p is aligned to min(16, 4 * sizeof(T)).
template <typename T>
__device__ __forceinline__ void remap_store_quad(T *__restrict__ p, const T q[4])
{
    if constexpr (sizeof(T) == 1)
        *reinterpret_cast<uint32_t *>(p) = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    else if constexpr (sizeof(T) == 2)
        *reinterpret_cast<uint2 *>(p) = make_uint2((uint32_t)q[0] | ((uint32_t)q[1] << 16), (uint32_t)q[2] | ((uint32_t)q[3] << 16));
    else if constexpr (sizeof(T) == 4)
        *reinterpret_cast<uint4 *>(p) = make_uint4(q[0], q[1], q[2], q[3]);
    else if constexpr (sizeof(T) == 8) {
        reinterpret_cast<uint4 *>(p)[0] = make_uint4(q[0].x, q[0].y, q[1].x, q[1].y);
        reinterpret_cast<uint4 *>(p)[1] = make_uint4(q[2].x, q[2].y, q[3].x, q[3].y);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = q[k];
    }
}

// k_remap_index for every frame of a set.  PACK: in a frame whose field start is 16-byte aligned and whose output start is aligned to the
// packed store (both hold under the default packings) a lane takes pixels 4j .. 4j+3 of the frame: one 16-byte field load, four range-checked
// gathers, one packed store; the last 1-3 pixels of a frame go one by one.  Other frames, and PACK = false, take one pixel per lane.
template <typename T, bool PACK>
__global__ __launch_bounds__(256) void k_remap_index_frames(const RemapFrame *__restrict__ frames, int n_frames, uint64_t blk_px,
                                                            const uint8_t *__restrict__ fld, const uint8_t *__restrict__ planes, size_t n_src,
                                                            size_t plane_stride, uint8_t *__restrict__ out)
{
    const RemapFrame fr = remap_frame_of(frames, n_frames, blockIdx.x);
    const int32_t *__restrict__ f = reinterpret_cast<const int32_t *>(fld + fr.fld_off);
    const T *__restrict__ src = reinterpret_cast<const T *>(planes + (size_t)fr.plane * plane_stride);
    T *__restrict__ o = reinterpret_cast<T *>(out + fr.out_off);
    const uint64_t p0 = (uint64_t)(blockIdx.x - fr.blk0) * blk_px;
    const uint64_t end = min(fr.n_px, p0 + blk_px);
    constexpr uintptr_t kOutMask = (sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) - 1;
    if (PACK && !(reinterpret_cast<uintptr_t>(f) & 15) && !(reinterpret_cast<uintptr_t>(o) & kOutMask)) {
        for (uint64_t i = p0 + threadIdx.x * 4; i < end; i += 1024) {
            if (i + 3 < end) {
                const v4i v = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(f + i));
                const T q[4] = { remap_gather(v.x, src, n_src), remap_gather(v.y, src, n_src), remap_gather(v.z, src, n_src), remap_gather(v.w, src, n_src) };
                remap_store_quad(o + i, q);
            } else {
                for (uint64_t k = i; k < end; k++) o[k] = remap_gather(f[k], src, n_src);
            }
        }
    } else {
        for (uint64_t i = p0 + threadIdx.x; i < end; i += 256) o[i] = remap_gather(f[i], src, n_src);
    }
}

// The C channels of one tap as floats.  u8 with 2 or 4 channels: one 2- / 4-byte load where the plane's start is aligned for it (wide).
template <typename E, int C>
__device__ __forceinline__ void remap_tap_load(const E *__restrict__ p, bool wide, float t[C])
{
    if constexpr (sizeof(E) == 1 && (C == 2 || C == 4)) {
        if (wide) {
            uint32_t w;
            if constexpr (C == 4) w = *reinterpret_cast<const uint32_t *>(p); else w = *reinterpret_cast<const uint16_t *>(p);
#pragma unroll
            for (int ch = 0; ch < C; ch++) t[ch] = (float)((w >> (8 * ch)) & 255u);
            return;
        }
    }
#pragma unroll
    for (int ch = 0; ch < C; ch++) t[ch] = (float)p[ch];
}

// k_remap_bilinear_f32's pixel for every frame of a set, and for 8-bit planes (E = uint8_t): taps and fractions as there, all in f32; the
// four taps of a channel converted to float and blended in the same operation order (contraction off), then
// out = (uint8)min(255, floor(v + 0.5f)) -- blend4's rounding; v >= 0 always -- and the channel bytes of the pixel leave in one store where
// there are 2 or 4 of them and the frame's output start is aligned for it.  One pixel per lane.  frames == nullptr: the frame `one`.
template <typename E, int C>
__global__ __launch_bounds__(256) void k_remap_bilinear_frames(const RemapFrame *__restrict__ frames, RemapFrame one, int n_frames, uint64_t blk_px,
                                                               const uint8_t *__restrict__ coords, const uint8_t *__restrict__ planes,
                                                               size_t plane_stride, int W, int H, uint8_t *__restrict__ out)
{
    const RemapFrame fr = frames ? remap_frame_of(frames, n_frames, blockIdx.x) : one;
    const float2 *__restrict__ cf = reinterpret_cast<const float2 *>(coords + fr.fld_off);
    const E *__restrict__ src = reinterpret_cast<const E *>(planes + (size_t)fr.plane * plane_stride);
    E *__restrict__ o = reinterpret_cast<E *>(out + fr.out_off);
    const uint64_t p0 = (uint64_t)(blockIdx.x - fr.blk0) * blk_px;
    const uint64_t end = min(fr.n_px, p0 + blk_px);
    constexpr bool kBytes = sizeof(E) == 1 && (C == 2 || C == 4);
    const bool src_wide = kBytes && !(reinterpret_cast<uintptr_t>(src) & (C - 1));
    const bool out_wide = kBytes && !(reinterpret_cast<uintptr_t>(o) & (C - 1));
    for (uint64_t i = p0 + threadIdx.x; i < end; i += 256) {
        const float2 s = cf[i];
        float v[C];
#pragma unroll
        for (int ch = 0; ch < C; ch++) v[ch] = 0.0f;
        if (fabsf(s.x) < INFINITY && fabsf(s.y) < INFINITY) {            // (NaN compares false)
            const float x0 = floorf(s.x), y0 = floorf(s.y);
            const float fx = s.x - x0, fy = s.y - y0, gx = 1.0f - fx, gy = 1.0f - fy;
            const int64_t c0 = remap_tap(x0, W), c1 = remap_tap(x0 + 1.0f, W);
            const int64_t r0 = (int64_t)remap_tap(y0, H) * W, r1 = (int64_t)remap_tap(y0 + 1.0f, H) * W;
            float p00[C], p01[C], p10[C], p11[C];
            remap_tap_load<E, C>(src + (r0 + c0) * C, src_wide, p00);
            remap_tap_load<E, C>(src + (r0 + c1) * C, src_wide, p01);
            remap_tap_load<E, C>(src + (r1 + c0) * C, src_wide, p10);
            remap_tap_load<E, C>(src + (r1 + c1) * C, src_wide, p11);
#pragma unroll
            for (int ch = 0; ch < C; ch++) v[ch] = (p00[ch] * gx + p01[ch] * fx) * gy + (p10[ch] * gx + p11[ch] * fx) * fy;
        }
        if constexpr (sizeof(E) == 4) {
#pragma unroll
            for (int ch = 0; ch < C; ch++) o[i * C + ch] = v[ch];
        } else {
            uint32_t b[C];
#pragma unroll
            for (int ch = 0; ch < C; ch++) b[ch] = (uint32_t)fminf(255.0f, floorf(v[ch] + 0.5f));
            if constexpr (C == 4) {
                if (out_wide) { *reinterpret_cast<uint32_t *>(o + i * 4) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); continue; }
            } else if constexpr (C == 2) {
                if (out_wide) { *reinterpret_cast<uint16_t *>(o + i * 2) = (uint16_t)(b[0] | (b[1] << 8)); continue; }
            }
#pragma unroll
            for (int ch = 0; ch < C; ch++) o[i * C + ch] = (uint8_t)b[ch];
        }
    }
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

static unsigned remap_blocks(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 16384); }

void launch_remap_index(const int32_t *fld, size_t n, const void *src, size_t n_src, int pixel_bytes, void *out, hipStream_t stream)
{
    if (n == 0) return;
    const dim3 grid(remap_blocks(n));
#define HG_RI(T) hipLaunchKernelGGL(k_remap_index<T>, grid, dim3(256), 0, stream, fld, n, static_cast<const T *>(src), n_src, static_cast<T *>(out))
    switch (pixel_bytes) {
    case 1: HG_RI(uint8_t); break;
    case 2: HG_RI(uint16_t); break;
    case 4: HG_RI(uint32_t); break;
    case 8: HG_RI(uint2); break;
    case 16: HG_RI(uint4); break;
    default: break;                                          // (the caller refused it)
    }
#undef HG_RI
}

void launch_remap_bilinear_f32(const float *coords, size_t n, const float *src, int W, int H, int channels, float *out, hipStream_t stream)
{
    if (n == 0) return;
    const dim3 grid(remap_blocks(n));
#define HG_RB(C) hipLaunchKernelGGL(k_remap_bilinear_f32<C>, grid, dim3(256), 0, stream, coords, n, src, W, H, out)
    switch (channels) {
    case 1: HG_RB(1); break;
    case 2: HG_RB(2); break;
    case 3: HG_RB(3); break;
    case 4: HG_RB(4); break;
    default: break;
    }
#undef HG_RB
}

// Pixel sizes whose frames kernel carries the packed form: those for which it was measured to win (EXPERIMENTS.md F.4).  A build with
// -DHG_REMAP_PACK_ALL=1 (make EXTRA=...) carries it for every size, to measure again.
#ifndef HG_REMAP_PACK_ALL
#define HG_REMAP_PACK_ALL 0
#endif
constexpr bool remap_has_packed(size_t pixel_bytes) { return HG_REMAP_PACK_ALL || pixel_bytes == 1; }
bool remap_index_packs(int pixel_bytes) { return remap_has_packed((size_t)pixel_bytes); }

template <typename T>
static void launch_remap_index_frames_t(const RemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, bool packed, const uint8_t *field,
                                        const uint8_t *planes, size_t n_src, size_t plane_stride, uint8_t *out, hipStream_t stream)
{
    if constexpr (remap_has_packed(sizeof(T))) {
        if (packed) {
            hipLaunchKernelGGL((k_remap_index_frames<T, true>), dim3(n_blocks), dim3(256), 0, stream, frames, n_frames, blk_px, field, planes, n_src, plane_stride, out);
            return;
        }
    }
    hipLaunchKernelGGL((k_remap_index_frames<T, false>), dim3(n_blocks), dim3(256), 0, stream, frames, n_frames, blk_px, field, planes, n_src, plane_stride, out);
}

void launch_remap_index_frames(const RemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, bool packed, const uint8_t *field,
                               const uint8_t *planes, size_t n_src, size_t plane_stride, int pixel_bytes, uint8_t *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_blocks == 0) return;
#define HG_RF(T) launch_remap_index_frames_t<T>(frames, n_frames, n_blocks, blk_px, packed, field, planes, n_src, plane_stride, out, stream)
    switch (pixel_bytes) {
    case 1: HG_RF(uint8_t); break;
    case 2: HG_RF(uint16_t); break;
    case 4: HG_RF(uint32_t); break;
    case 8: HG_RF(uint2); break;
    case 16: HG_RF(uint4); break;
    default: break;                                          // (the caller refused it)
    }
#undef HG_RF
}

void launch_remap_bilinear_frames(const RemapFrame *frames, const RemapFrame &one, int n_frames, uint32_t n_blocks, uint64_t blk_px,
                                  const uint8_t *coords, const uint8_t *planes, size_t plane_stride, int W, int H, int elem, int channels,
                                  uint8_t *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_blocks == 0) return;
#define HG_BF(E, C) hipLaunchKernelGGL((k_remap_bilinear_frames<E, C>), dim3(n_blocks), dim3(256), 0, stream, frames, one, n_frames, blk_px, coords, planes, plane_stride, W, H, out)
#define HG_BE(E) switch (channels) { case 1: HG_BF(E, 1); break; case 2: HG_BF(E, 2); break; case 3: HG_BF(E, 3); break; case 4: HG_BF(E, 4); break; default: break; }
    if (elem == 0) HG_BE(float) else HG_BE(uint8_t)
#undef HG_BE
#undef HG_BF
}

} // namespace hg
