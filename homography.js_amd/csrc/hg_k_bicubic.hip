// hg_k_bicubic.hip -- the bicubic remap on the field seam (include/hgwarp.h, hg_remap_bicubic_frames_device): k_remap_bicubic_frames gathers
// a plane through a HG_FIELD_COORDS field as k_remap_bilinear_frames does, but blends 4 x 4 clamped taps with the weights of a (B, C) cubic
// (Catmull-Rom, Mitchell, B-spline), so that an enlargement keeps its edges and curves.
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  All arithmetic is f32 in the written order (contraction off); the numpy model of
// tests/hgtest/bicubic.py follows it operation by operation.  Design notes: DESIGN.md §4.9, figures: EXPERIMENTS.md F.9.
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_remap_dev.h"

namespace hg {

// The four weights of the fraction t in [0, 1): the taps lie 1 + t, t, 1 - t and 2 - t away.
__device__ __forceinline__ float cubic_near(const CubicCoef &k, float x) { return (((k.p3 * x) + k.p2) * x) * x + k.p0; }
__device__ __forceinline__ float cubic_far(const CubicCoef &k, float x) { return ((((k.q3 * x) + k.q2) * x) + k.q1) * x + k.q0; }
__device__ __forceinline__ void cubic_weights(const CubicCoef &k, float t, float w[4])
{
    w[0] = cubic_far(k, 1.0f + t);
    w[1] = cubic_near(k, t);
    w[2] = cubic_near(k, 1.0f - t);
    w[3] = cubic_far(k, 2.0f - t);
}

// Which instantiations keep the row loop rolled: those with 3 or 4 channels, where the unrolled form costs waves (all eight timed in both
// forms: EXPERIMENTS.md F.9).  A build with -DHG_BICUBIC_ROLL=1 (make EXTRA=...) rolls it everywhere, =0 nowhere, to measure again.
#ifndef HG_BICUBIC_ROLL
#define HG_BICUBIC_ROLL -1
#endif
constexpr bool bicubic_rolls(int channels)
{
    return HG_BICUBIC_ROLL >= 0 ? HG_BICUBIC_ROLL != 0 : channels >= 3;
}

// One pixel per lane over the frame's flat list: the grid, the block search and the records are k_remap_bilinear_frames'.  A NaN or infinite
// coordinate gives zeros.  Otherwise the four tap columns x0-1 .. x0+2 and rows y0-1 .. y0+2 are clamped into the plane one by one (the sums
// in f32, clamped in float before the conversion), and the rows are folded one at a time: the four taps of row n are loaded, blended into
// h_n = ((p0*wx0 + p1*wx1) + p2*wx2) + p3*wx3 and added into r = ((h_0*wy0 + h_1*wy1) + h_2*wy2) + h_3*wy3 before the next row's loads are
// needed.  With 1 or 2 channels the row loop is unrolled: the compiler then issues the sixteen loads of a pixel ahead of the blend, at 8
// waves per SIMD all the same.  With 3 or 4 channels that order would cost waves (16 x C taps live), so the loop stays rolled (4 x C taps
// live, 8 waves); the row's tap and weight are then formed inside the loop from the uniform n, by the same operations.  The cubic's negative lobes can take r below 0: the byte store clamps on both sides.
template <typename E, int C>
__global__ __launch_bounds__(256) void k_remap_bicubic_frames(const RemapFrame *__restrict__ frames, int n_frames, uint64_t blk_px, CubicCoef k,
                                                              const uint8_t *__restrict__ coords, const uint8_t *__restrict__ planes,
                                                              size_t plane_stride, int W, int H, uint8_t *__restrict__ out)
{
    const RemapFrame fr = remap_frame_of(frames, n_frames, blockIdx.x);
    const float2 *__restrict__ cf = reinterpret_cast<const float2 *>(coords + fr.fld_off);
    const E *__restrict__ src = reinterpret_cast<const E *>(planes + (size_t)fr.plane * plane_stride);
    E *__restrict__ o = reinterpret_cast<E *>(out + fr.out_off);
    const uint64_t p0 = (uint64_t)(blockIdx.x - fr.blk0) * blk_px;
    const uint64_t end = min(fr.n_px, p0 + blk_px);
    constexpr bool kBytes = sizeof(E) == 1 && (C == 2 || C == 4);
    const bool src_wide = kBytes && !(reinterpret_cast<uintptr_t>(src) & (C - 1));
    const bool out_wide = kBytes && !(reinterpret_cast<uintptr_t>(o) & (C - 1));
    constexpr int kRowUnroll = bicubic_rolls(C) ? 1 : 4;
    for (uint64_t i = p0 + threadIdx.x; i < end; i += 256) {
        const float2 s = cf[i];
        float v[C];
#pragma unroll
        for (int ch = 0; ch < C; ch++) v[ch] = 0.0f;
        if (remap_finite(s)) {
            const float x0 = floorf(s.x), y0 = floorf(s.y);
            float wx[4];
            cubic_weights(k, s.x - x0, wx);
            const float fy = s.y - y0;
            const int64_t c0 = remap_tap(x0 - 1.0f, W), c1 = remap_tap(x0, W), c2 = remap_tap(x0 + 1.0f, W), c3 = remap_tap(x0 + 2.0f, W);
#pragma unroll kRowUnroll
            for (int n = 0; n < 4; n++) {
                // (n is uniform, or a constant where the loop is unrolled: the selects are scalar or gone; y0 + 0.0f clamps to the tap of y0)
                const float wy = n == 0 ? cubic_far(k, 1.0f + fy) : n == 1 ? cubic_near(k, fy) : n == 2 ? cubic_near(k, 1.0f - fy) : cubic_far(k, 2.0f - fy);
                const int64_t r = (int64_t)remap_tap(y0 + (float)(n - 1), H) * W;
                float t0[C], t1[C], t2[C], t3[C];
                remap_px_load<E, C>(src + (r + c0) * C, src_wide, t0);
                remap_px_load<E, C>(src + (r + c1) * C, src_wide, t1);
                remap_px_load<E, C>(src + (r + c2) * C, src_wide, t2);
                remap_px_load<E, C>(src + (r + c3) * C, src_wide, t3);
#pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    const float h = ((t0[ch] * wx[0] + t1[ch] * wx[1]) + t2[ch] * wx[2]) + t3[ch] * wx[3];
                    v[ch] = n == 0 ? h * wy : v[ch] + h * wy;
                }
            }
        }
        remap_px_store<E, C, true>(o, i, out_wide, v);
    }
}

// ------------------------------------------------------------------------------------------------ launcher
#ifdef __HIPCC__
void launch_remap_bicubic_frames(const RemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, const CubicCoef &k,
                                 const uint8_t *coords, const uint8_t *planes, size_t plane_stride, int W, int H, int elem, int channels,
                                 uint8_t *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_blocks == 0) return;
    for_elem_channels(elem, channels, [&](auto e, auto c) {
        hipLaunchKernelGGL((k_remap_bicubic_frames<decltype(e), decltype(c)::value>), dim3(n_blocks), dim3(256), 0, stream, frames, n_frames, blk_px, k,
                           coords, planes, plane_stride, W, H, out);
    });
}
#endif

} // namespace hg
