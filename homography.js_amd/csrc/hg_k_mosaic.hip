// hg_k_mosaic.hip -- the frames of a set blended into one canvas on the field seam (include/hgwarp.h, hg_mosaic_frames_device):
// k_mosaic_frames gathers, per canvas pixel, the pixels of every frame whose window holds it and whose HG_FIELD_COORDS field covers it.
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  All arithmetic is f32 in the written order (contraction off); the numpy model of
// tests/hgtest/mosaic.py follows it operation by operation.  Design notes: DESIGN.md §4.11, figures: EXPERIMENTS.md F.7.
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_remap_dev.h"

namespace hg {

// Does the window of `fr` meet the canvas tile [X0, X1) x [Y0, Y1) of destination space?  Everything here is uniform over the block: the
// test runs on the scalar side, from the record alone.
__device__ __forceinline__ bool mos_hits(const MosaicFrame &fr, int64_t X0, int64_t X1, int64_t Y0, int64_t Y1)
{
    return fr.obj_w > 0 && fr.obj_h > 0 && fr.x_off < X1 && (int64_t)fr.x_off + fr.obj_w > X0 && fr.y_off < Y1 && (int64_t)fr.y_off + fr.obj_h > Y0;
}

// Frame `fr` at destination position (X, Y): false unless the window holds the position and the field covers it there (both coordinate
// words finite); else the coordinate in *s and the pixel's channels in p.  Bytes with 2 or 4 channels move as one load where the frame's
// start is aligned for it (uniform per frame).
template <typename E, int C>
__device__ __forceinline__ bool mos_fetch(const MosaicFrame &fr, int64_t X, int64_t Y, const uint8_t *__restrict__ coords,
                                          const uint8_t *__restrict__ pixels, float2 *s, remap_px_t<E> p[C])
{
    const int64_t u = X - fr.x_off, v = Y - fr.y_off;
    if (u < 0 || u >= fr.obj_w || v < 0 || v >= fr.obj_h) return false;
    const uint64_t k = (uint64_t)v * (uint64_t)fr.obj_w + (uint64_t)u;       // (< 2^31)
    *s = reinterpret_cast<const float2 *>(coords + fr.fld_off)[k];
    if (!remap_finite(*s)) return false;
    const E *__restrict__ px = reinterpret_cast<const E *>(pixels + fr.pix_off);
    const bool wide = sizeof(E) == 1 && (C == 2 || C == 4) && !(reinterpret_cast<uintptr_t>(px) & (C - 1));
    remap_px_load<E, C>(px + k * C, wide, p);
    return true;
}

// One canvas pixel per lane, 64 columns x 4 rows per block (one wave per row: its loads from one frame row are contiguous); block b owns
// tile (b % tiles_x, b / tiles_x).  A gather: the frame table is walked by the whole block, frames whose window misses the tile are
// skipped from their record, no lane writes a pixel another lane reads and there are no atomics -- the sum below runs in ascending frame
// order on every run.  mode 0 (last) walks descending and a lane leaves at its first contributor, whose pixel it copies.  modes 1
// (mean) and 2 (feather): acc_c = acc_c + w * p_c and wsum = wsum + w in ascending f; exactly one contributor stores that pixel as it
// is, more store acc_c / wsum (u8: min(255, floor(r + 0.5f))).  No contributor: zeros, weight 0.  The accumulators, the first
// contributor's pixel and the count live in registers; nothing is indexed at run time.
template <typename E, int C>
__global__ __launch_bounds__(256) void k_mosaic_frames(const MosaicFrame4 *__restrict__ frames, int n_quads, const uint8_t *__restrict__ coords,
                                                       const uint8_t *__restrict__ pixels, int W, int H, int mode, float feather,
                                                       int cx, int cy, int cw, int ch, uint32_t tiles_x, uint8_t *__restrict__ canvas,
                                                       float *__restrict__ weight)
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
                for (int c = 0; c < C; c++) r[c] = p[c];
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
                float w = 1.0f;
                if (mode == 2) {
                    const float dx = fminf(s.x + 1.0f, fw - s.x), dy = fminf(s.y + 1.0f, fh - s.y);
                    w = fmaxf(fminf(fminf(dx, dy), feather), 0x1p-10f);
                }
#pragma unroll
                for (int c = 0; c < C; c++) {
                    acc[c] = acc[c] + w * (float)p[c];
                    if (n == 0) r[c] = p[c];
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
                          int mode, float feather, int cx, int cy, int cw, int ch, uint8_t *canvas, float *weight, hipStream_t stream)
{
    if (cw <= 0 || ch <= 0) return;
    const uint32_t tiles_x = (uint32_t)(((int64_t)cw + 63) / 64);
    const uint64_t n_blocks = (uint64_t)tiles_x * (uint64_t)(((int64_t)ch + 3) / 4);      // (< 2^31 for a canvas of at most 2^31 pixels)
    for_elem_channels(elem, channels, [&](auto e, auto c) {
        hipLaunchKernelGGL((k_mosaic_frames<decltype(e), decltype(c)::value>), dim3((uint32_t)n_blocks), dim3(64, 4), 0, stream, frames, n_quads, coords, pixels, W, H,
                           mode, feather, cx, cy, cw, ch, tiles_x, canvas, weight);
    });
}
#endif

} // namespace hg
