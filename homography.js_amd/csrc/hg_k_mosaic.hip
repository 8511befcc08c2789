// hg_k_mosaic.hip -- the frames of a set blended into one canvas on the field seam (include/hgwarp.h, hg_mosaic_frames_device):
// k_mosaic_frames gathers, per canvas pixel, the pixels of every frame whose window holds it and whose HG_FIELD_COORDS field covers it.
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  All arithmetic is f32 in the written order (contraction off); the numpy model of
// tests/hgtest/mosaic.py follows it operation by operation.  Design notes: DESIGN.md §4.11, figures: EXPERIMENTS.md F.7.
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_mosaic_dev.h"

namespace hg {

// Channel c of a contributor as the blend takes it: p_c, or with GAIN q_c = g * p_c on the exposure channels (alpha, channel 3 of 4, as it is).
template <bool GAIN, int C, typename V>
__device__ __forceinline__ float mos_value(float g, int c, V p)
{
    if constexpr (GAIN) { if (c < mos_stat_channels(C)) return g * (float)p; }
    return (float)p;
}
// What LAST and a lone contributor of a gained mosaic store of q_c: itself, or the byte min(255, floor(q_c + 0.5f)) as every u8 result is
// rounded (an unscaled byte comes back as it was).
template <typename E>
__device__ __forceinline__ remap_px_t<E> mos_stored(float q)
{
    if constexpr (sizeof(E) == 4) return q; else return (uint32_t)fminf(255.0f, floorf(q + 0.5f));
}

// One canvas pixel per lane, 64 columns x 4 rows per block (one wave per row: its loads from one frame row are contiguous); block b owns
// tile (b % tiles_x, b / tiles_x).  A gather: the frame table is walked by the whole block, frames whose window misses the tile are
// skipped from their record, no lane writes a pixel another lane reads and there are no atomics -- the sum below runs in ascending frame
// order on every run.  mode 0 (last) walks descending and a lane leaves at its first contributor, whose pixel it copies.  modes 1
// (mean) and 2 (feather): acc_c = acc_c + w * p_c and wsum = wsum + w in ascending f; exactly one contributor stores that pixel as it
// is, more store acc_c / wsum (u8: min(255, floor(r + 0.5f))).  No contributor: zeros, weight 0.  The accumulators, the first
// contributor's pixel and the count live in registers; nothing is indexed at run time.
// GAIN (hg_mosaic_frames_gain_device; an instantiation of its own, the plain one's code is what it was): gains[f] is frame f's factor, one
// per record of the table.  A contributor's exposure channels become q_c = g_f * p_c (one f32 multiply; alpha, channel 3 of 4, passes as
// it is) before anything else: LAST and a lone contributor store q_c (u8: min(255, floor(q_c + 0.5f))), the sum takes w * q_c.
template <typename E, int C, bool GAIN = false>
__global__ __launch_bounds__(256) void k_mosaic_frames(const MosaicFrame4 *__restrict__ frames, int n_quads, const uint8_t *__restrict__ coords,
                                                       const uint8_t *__restrict__ pixels, int W, int H, int mode, float feather,
                                                       int cx, int cy, int cw, int ch, uint32_t tiles_x, uint8_t *__restrict__ canvas,
                                                       float *__restrict__ weight, const float *__restrict__ gains = nullptr)
{
    using V = remap_px_t<E>;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t i0 = (int64_t)tx * 64, j0 = (int64_t)ty * 4;
    const int64_t X0 = cx + i0, Y0 = cy + j0, X1 = min(X0 + 64, (int64_t)cx + cw), Y1 = min(Y0 + 4, (int64_t)cy + ch);
    const int64_t i = i0 + threadIdx.x, j = j0 + threadIdx.y;
    if (i >= cw || j >= ch) return;
    const int64_t X = cx + i, Y = cy + j;
    V r[C];                                                      // what is stored: the channels as loaded, or the rounded quotient
#pragma unroll
    for (int c = 0; c < C; c++) r[c] = 0;
    float wsum = 0.0f;
    if (mode == 0) {
        for (int q = n_quads - 1; q >= 0 && wsum == 0.0f; q--) {
            const MosaicFrame4 quad = frames[q];
#pragma unroll
            for (int k = 3; k >= 0; k--) {
                const MosaicFrame &fr = quad.f[k];
                if (wsum != 0.0f || !mos_hits(fr, X0, X1, Y0, Y1)) continue;
                float2 s;
                V p[C];
                if (!mos_fetch<E, C>(fr, X, Y, coords, pixels, &s, p)) continue;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    if constexpr (GAIN) r[c] = mos_stored<E>(mos_value<GAIN, C>(gains[q * 4 + k], c, p[c])); else r[c] = p[c];
                }
                wsum = 1.0f;
            }
        }
    } else {
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 0.0f;
        int n = 0;
        const float fw = (float)W, fh = (float)H;
        for (int q = 0; q < n_quads; q++) {
            const MosaicFrame4 quad = frames[q];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const MosaicFrame &fr = quad.f[k];
                if (!mos_hits(fr, X0, X1, Y0, Y1)) continue;
                float2 s;
                V p[C];
                if (!mos_fetch<E, C>(fr, X, Y, coords, pixels, &s, p)) continue;
                float g = 1.0f;
                if constexpr (GAIN) g = gains[q * 4 + k];
                float w = 1.0f;
                if (mode == 2) {
                    const float dx = fminf(s.x + 1.0f, fw - s.x), dy = fminf(s.y + 1.0f, fh - s.y);
                    w = fmaxf(fminf(fminf(dx, dy), feather), 0x1p-10f);
                }
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float x = mos_value<GAIN, C>(g, c, p[c]);   // p_c, or q_c
                    acc[c] = acc[c] + w * x;
                    if (n == 0) { if constexpr (GAIN) r[c] = mos_stored<E>(x); else r[c] = p[c]; }
                }
                wsum = wsum + w;
                n++;
            }
        }
        if (n > 1) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float q = acc[c] / wsum;
                if constexpr (sizeof(E) == 4) r[c] = q; else r[c] = (uint32_t)fminf(255.0f, floorf(q + 0.5f));
            }
        }
    }
    const uint64_t k = (uint64_t)j * (uint64_t)cw + (uint64_t)i;
    if (weight) __builtin_nontemporal_store(wsum, weight + k);
    E *__restrict__ o = reinterpret_cast<E *>(canvas) + k * C;
    if constexpr (sizeof(E) == 1 && C == 4) {
        if (!(reinterpret_cast<uintptr_t>(canvas) & 3)) { __builtin_nontemporal_store(r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24), reinterpret_cast<uint32_t *>(o)); return; }
    } else if constexpr (sizeof(E) == 1 && C == 2) {
        if (!(reinterpret_cast<uintptr_t>(canvas) & 1)) { __builtin_nontemporal_store((uint16_t)(r[0] | (r[1] << 8)), reinterpret_cast<uint16_t *>(o)); return; }
    }
#pragma unroll
    for (int c = 0; c < C; c++) __builtin_nontemporal_store((E)r[c], o + c);
}

// ------------------------------------------------------------------------------------------------ launcher
#ifdef __HIPCC__
void launch_mosaic_frames(const MosaicFrame4 *frames, int n_quads, const uint8_t *coords, const uint8_t *pixels, int W, int H, int elem, int channels,
                          int mode, float feather, int cx, int cy, int cw, int ch, uint8_t *canvas, float *weight, const float *gains, hipStream_t stream)
{
    if (cw <= 0 || ch <= 0) return;
    const uint32_t tiles_x = (uint32_t)(((int64_t)cw + 63) / 64);
    const uint64_t n_blocks = (uint64_t)tiles_x * (uint64_t)(((int64_t)ch + 3) / 4);      // (< 2^31 for a canvas of at most 2^31 pixels)
    for_elem_channels(elem, channels, [&](auto e, auto c) {
        if (gains)
            hipLaunchKernelGGL((k_mosaic_frames<decltype(e), decltype(c)::value, true>), dim3((uint32_t)n_blocks), dim3(64, 4), 0, stream, frames, n_quads, coords,
                               pixels, W, H, mode, feather, cx, cy, cw, ch, tiles_x, canvas, weight, gains);
        else
            hipLaunchKernelGGL((k_mosaic_frames<decltype(e), decltype(c)::value>), dim3((uint32_t)n_blocks), dim3(64, 4), 0, stream, frames, n_quads, coords, pixels,
                               W, H, mode, feather, cx, cy, cw, ch, tiles_x, canvas, weight, (const float *)nullptr);
    });
}
#endif

} // namespace hg
