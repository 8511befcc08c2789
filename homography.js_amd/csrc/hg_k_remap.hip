// hg_k_remap.hip -- the remaps that consume a source field (include/hgwarp.h, hg_remap_*): k_remap_index, k_remap_bilinear_f32 and their
// whole-frame-set forms k_remap_index_frames, k_remap_bilinear_frames.
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  All arithmetic is f32 in the written order (contraction off); the numpy model of
// tests/hgtest/remap_frames.py follows it operation by operation.  Design notes: DESIGN.md §4.9.
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_remap_dev.h"

namespace hg {

typedef int v4i __attribute__((ext_vector_type(4)));

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

// Bilinear remap of C interleaved f32 channels through a HG_FIELD_COORDS field.  A NaN or infinite coordinate gives zeros; otherwise
// tri_sample's pixel -- its text once more, reading the taps in place: this kernel has no timing tool of its own, so it keeps its
// assembly --, stored as it is.
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
        if (remap_finite(s)) {
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

// k_remap_bilinear_f32's pixel for every frame of a set, and for 8-bit planes (E = uint8_t): the four taps of a channel converted to
// float as they are loaded (this kernel's measured order: EXPERIMENTS.md F.8), the blend rounded and stored by remap_px_store.  One pixel
// per lane.  frames == nullptr: the frame `one`.
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
        if (remap_finite(s)) tri_sample<E, C, float>(src, src_wide, W, H, s.x, s.y, v);
        remap_px_store<E, C>(o, i, out_wide, v);
    }
}

// ------------------------------------------------------------------------------------------------ launchers
#ifdef __HIPCC__
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
    for_elem_channels(elem, channels, [&](auto e, auto c) {
        hipLaunchKernelGGL((k_remap_bilinear_frames<decltype(e), decltype(c)::value>), dim3(n_blocks), dim3(256), 0, stream, frames, one, n_frames, blk_px,
                           coords, planes, plane_stride, W, H, out);
    });
}
#endif

} // namespace hg
