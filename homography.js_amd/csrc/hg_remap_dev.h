// hg_remap_dev.h -- the one text of the remap family's device helpers (hg_k_remap.hip, hg_k_pyramid.hip, hg_k_aniso.hip, hg_k_mosaic.hip, hg_k_bicubic.hip):
// the frame of a block, taps, pixel loads, the bilinear sample on one level, the field's footprint, the level choice and the store tail.
// Needs the records and the HIP qualifiers only -- from hg_dev.h under hipcc, from tests/cpp/hip_host_shim.h in the host checks, which
// compile the kernel files themselves.  All arithmetic is f32 in the written order (contraction off).  Design notes: DESIGN.md §4.9.
#pragma once
#include "hg_remap_records.h"
#include <type_traits>

namespace hg {

// One launch for all frames: block b belongs to the last frame whose blk0 <= b (a binary search over the device frame table, uniform over the
// block, so scalar loads) and covers blk_px consecutive pixels of that frame's flat list.  Empty frames own no block.
template <typename R>
__device__ __forceinline__ R remap_frame_of(const R *__restrict__ frames, int n, uint32_t b)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (frames[mid].blk0 <= b) lo = mid; else hi = mid;
    }
    return frames[lo];
}

// Column / row of a tap: clamp(v, 0, n - 1) for an integer-valued finite float v, clamped in float first so that the conversion is defined
// for any magnitude (2147483520 is the largest float below 2^31).
__device__ __forceinline__ int remap_tap(float v, int n)
{
    return min((int)fminf(fmaxf(v, 0.0f), 2147483520.0f), n - 1);
}

// Does the field cover the pixel?  An uncovered one holds a NaN or infinite word.
__device__ __forceinline__ bool remap_finite(float2 s) { return fabsf(s.x) < INFINITY && fabsf(s.y) < INFINITY; }      // (NaN compares false)

// Size of level k of a pyramid over n pixels: (n + 1) >> 1 applied k times = ceil(n / 2^k); k <= 31, n < 2^31.
__device__ __forceinline__ int pyr_size(int n, int k)
{
    return (int)(((uint32_t)n + ((1u << k) - 1u)) >> k);
}

// What a loaded channel is held as until the blend: bytes widened to uint32, floats as they are.
template <typename E> using remap_px_t = std::conditional_t<sizeof(E) == 1, uint32_t, float>;

// The C channels of one pixel as values of V.  Bytes with 2 or 4 channels: one 2- / 4-byte load where the pixel list's start is aligned
// for it (wide).
template <typename E, int C, typename V>
__device__ __forceinline__ void remap_px_load(const E *__restrict__ p, bool wide, V t[C])
{
    if constexpr (sizeof(E) == 1 && (C == 2 || C == 4)) {
        if (wide) {
            uint32_t w;
            if constexpr (C == 4) w = *reinterpret_cast<const uint32_t *>(p); else w = *reinterpret_cast<const uint16_t *>(p);
#pragma unroll
            for (int ch = 0; ch < C; ch++) t[ch] = (V)((w >> (8 * ch)) & 255u);
            return;
        }
    }
#pragma unroll
    for (int ch = 0; ch < C; ch++) t[ch] = (V)p[ch];
}

// The bilinear pixel of one level: W x H pixels at src, the coordinate (u, v) finite.  x0 = floorf(u), fx = u - x0, taps clamp(x0, 0, W-1)
// and clamp(x0 + 1, 0, W-1) (the +1 in f32), rows alike, and blend4's operation order per channel:
// r = (p00*(1-fx) + p01*fx)*(1-fy) + (p10*(1-fx) + p11*fx)*fy.  V: what the four taps wait as (remap_px_load).
template <typename E, int C, typename V = remap_px_t<E>>
__device__ __forceinline__ void tri_sample(const E *__restrict__ src, bool wide, int W, int H, float u, float v, float r[C])
{
    const float x0 = floorf(u), y0 = floorf(v);
    const float fx = u - x0, fy = v - y0, gx = 1.0f - fx, gy = 1.0f - fy;
    const int64_t c0 = remap_tap(x0, W), c1 = remap_tap(x0 + 1.0f, W);
    const int64_t r0 = (int64_t)remap_tap(y0, H) * W, r1 = (int64_t)remap_tap(y0 + 1.0f, H) * W;
    V p00[C], p01[C], p10[C], p11[C];
    remap_px_load<E, C>(src + (r0 + c0) * C, wide, p00);
    remap_px_load<E, C>(src + (r0 + c1) * C, wide, p01);
    remap_px_load<E, C>(src + (r1 + c0) * C, wide, p10);
    remap_px_load<E, C>(src + (r1 + c1) * C, wide, p11);
#pragma unroll
    for (int ch = 0; ch < C; ch++) r[ch] = ((float)p00[ch] * gx + (float)p01[ch] * fx) * gy + ((float)p10[ch] * gx + (float)p11[ch] * fx) * fy;
}

// Pixel t = col0 + (i - p0) of the rows from row0 on, in a frame obj_w pixels wide: its column and row.  (A block's pixels seldom pass 2^32.)
__device__ __forceinline__ void remap_px_xy(uint64_t t, uint64_t ow, uint64_t row0, uint64_t *px, uint64_t *py)
{
    const uint64_t dj = (t >> 32) ? t / ow : (uint64_t)((uint32_t)t / (uint32_t)ow);
    *px = t - dj * ow; *py = row0 + dj;
}

// The step from s to the first of the two neighbour candidates that exists and is finite: *dx, *dy and the squared length in source pixels;
// all three 0 without one.
__device__ __forceinline__ float remap_step(const float2 *__restrict__ cf, float2 s, bool has_a, uint64_t ia, bool has_b, uint64_t ib, float *dx, float *dy)
{
    float2 n = make_float2(INFINITY, INFINITY);
    if (has_a) n = cf[ia];
    if (!remap_finite(n) && has_b) n = cf[ib];
    *dx = 0.0f; *dy = 0.0f;
    if (!remap_finite(n)) return 0.0f;
    *dx = n.x - s.x; *dy = n.y - s.y;
    return *dx * *dx + *dy * *dy;
}

// The level(s) of a footprint q (a squared step): q <= 1: level 0 alone.  Else k = floor(log2(q)) >> 1 -- the exponent field of q --, level
// levels-1 alone if k reaches it, otherwise levels k and k+1 (n = 2) blended by w = (q / 4^k - 1) / 3, the weight of level k + 1.
struct RemapLevels { int k, n; float w; };
__device__ __forceinline__ RemapLevels remap_levels(float q, int levels)
{
    int k = 0, n = 1;
    float w = 0.0f;
    if (q > 1.0f) {
        const uint32_t qb = __float_as_uint(q);
        k = ((int)(qb >> 23) - 127) >> 1;                          // (+Inf: 64)
        if (k >= levels - 1) k = levels - 1;
        else { w = (__uint_as_float(qb - ((uint32_t)(2 * k) << 23)) - 1.0f) * 0.33333334f; n = 2; }      // ldexpf(q, -2k), exact
    }
    return RemapLevels{k, n, w};
}

// Pixel i of the output list o: f32 as it is; u8 as min(255, floor(v + 0.5f)) -- blend4's rounding; v >= 0 always --, the channel bytes in
// one store where there are 2 or 4 of them and the list's start is aligned for it (wide).  SIGNED: v may be negative (a filter with negative
// lobes); u8 is then min(255, max(0, floor(v + 0.5f))), so that the conversion to unsigned stays defined.
template <typename E, int C, bool SIGNED = false>
__device__ __forceinline__ void remap_px_store(E *__restrict__ o, uint64_t i, bool wide, const float v[C])
{
    if constexpr (sizeof(E) == 4) {
#pragma unroll
        for (int ch = 0; ch < C; ch++) o[i * C + ch] = v[ch];
    } else {
        uint32_t b[C];
#pragma unroll
        for (int ch = 0; ch < C; ch++) {
            if constexpr (SIGNED) b[ch] = (uint32_t)fminf(255.0f, fmaxf(0.0f, floorf(v[ch] + 0.5f)));
            else b[ch] = (uint32_t)fminf(255.0f, floorf(v[ch] + 0.5f));
        }
        if constexpr (C == 4) {
            if (wide) { *reinterpret_cast<uint32_t *>(o + i * 4) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); return; }
        } else if constexpr (C == 2) {
            if (wide) { *reinterpret_cast<uint16_t *>(o + i * 2) = (uint16_t)(b[0] | (b[1] << 8)); return; }
        }
#pragma unroll
        for (int ch = 0; ch < C; ch++) o[i * C + ch] = (uint8_t)b[ch];
    }
}

// The (element, channels) instantiation of a launch: f(E(), std::integral_constant<int, C>()) with E = float (elem 0) or uint8_t and
// C = channels (1..4; the callers refused anything else).
template <typename F>
void for_elem_channels(int elem, int channels, F f)
{
    auto by_channels = [&](auto e) {
        switch (channels) {
        case 1: f(e, std::integral_constant<int, 1>()); break;
        case 2: f(e, std::integral_constant<int, 2>()); break;
        case 3: f(e, std::integral_constant<int, 3>()); break;
        case 4: f(e, std::integral_constant<int, 4>()); break;
        default: break;
        }
    };
    if (elem == 0) by_channels(float()); else by_channels(uint8_t());
}

} // namespace hg
