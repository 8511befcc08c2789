// hg_k_multiband.hip -- the multi-band mosaic (include/hgwarp.h, hg_mosaic_multiband_device; Burt & Adelson's pyramid blend as Brown &
// Lowe's section 7 uses it): k_mb_label ranks the contributors of every canvas pixel, k_mb_seed turns coverage and labels into one flag byte
// per frame-grid pixel, k_mb_reduce builds one level of every frame's image and weight pyramids per launch, k_mb_blend blends one level of
// Laplacians over the canvas grid and collapses it onto the level below, coarse to fine.  Hand-written HIP for gfx950 (MI355X / CDNA4),
// wave64, no atomics, no scratch.  Every launch covers ALL frames through the table of MbFrame records: 2 + (L - 1) + L launches whatever F
// is.  All arithmetic is f32 in the written order (contraction off); the numpy model of tests/hgtest/multiband.py follows it operation by
// operation.  The shared rules: hg_multiband_dev.h.  Design notes: DESIGN.md §4.16, figures: EXPERIMENTS.md "Multi-band".
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_multiband_dev.h"

namespace hg {

// Channel c of a frame pixel as level 0 takes it: q_c = g * p_c on the exposure channels, p_c on the alpha of a 4-channel frame.  A gain
// of 1.0f (no gains) leaves the value as it is.
template <int C, typename V>
__device__ __forceinline__ float mb_value(float g, int c, V p)
{
    return c < mos_stat_channels(C) ? g * (float)p : (float)p;
}

// The C channels of pixel k of frame `fr` (the caller knows that the frame contributes there).
template <typename E, int C>
__device__ __forceinline__ void mb_pixel(const MbFrame &fr, uint64_t k, const uint8_t *__restrict__ pixels, float v[C])
{
    const E *__restrict__ px = reinterpret_cast<const E *>(pixels + fr.m.pix_off);
    const bool wide = sizeof(E) == 1 && (C == 2 || C == 4) && !(reinterpret_cast<uintptr_t>(px) & (C - 1));
    remap_px_t<E> p[C];
    remap_px_load<E, C>(px + k * C, wide, p);
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = mb_value<C>(fr.gain, c, p[c]);
}

// ------------------------------------------------------------------------------------------------ step 1: the labels
// The mosaic's gather without pixel loads: one canvas pixel per lane, 64 columns x 4 rows per block, the quad table walked by the whole
// block in ascending order, frames whose window misses the tile skipped from their record.  The label is the contributor with the largest
// rank, the lowest index among equals (a later frame must be strictly larger); -1 without one.
__global__ __launch_bounds__(256) void k_mb_label(const MosaicFrame4 *__restrict__ frames, int n_quads, const uint8_t *__restrict__ coords, int W, int H,
                                                  float feather, int cx, int cy, int cw, int ch, uint32_t tiles_x, int32_t *__restrict__ labels)
{
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t i0 = (int64_t)tx * 64, j0 = (int64_t)ty * 4;
    const int64_t X0 = cx + i0, Y0 = cy + j0, X1 = min(X0 + 64, (int64_t)cx + cw), Y1 = min(Y0 + 4, (int64_t)cy + ch);
    const int64_t i = i0 + threadIdx.x, j = j0 + threadIdx.y;
    if (i >= cw || j >= ch) return;
    const int64_t X = cx + i, Y = cy + j;
    const float fw = (float)W, fh = (float)H;
    int32_t label = -1;
    float best = 0.0f;                                         // (every rank is >= 2^-10)
    for (int q = 0; q < n_quads; q++) {
        const MosaicFrame4 quad = frames[q];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const MosaicFrame &fr = quad.f[k];
            if (!mos_hits(fr, X0, X1, Y0, Y1)) continue;
            float2 s;
            uint64_t at;
            if (!mos_covers(fr, X, Y, coords, &s, &at)) continue;
            const float w = mb_rank(s, fw, fh, feather);
            if (w > best) { best = w; label = q * 4 + k; }
        }
    }
    labels[(uint64_t)j * (uint64_t)cw + (uint64_t)i] = label;
}

// ------------------------------------------------------------------------------------------------ step 3: the flag bytes
// Four consecutive grid pixels of one frame per lane, 1024 per block; block b belongs to the last frame whose blk0[0] <= b.  A grid pixel
// outside the canvas gets 0 and reads nothing; inside, MB_CONTRIBUTES from the frame's coordinate and MB_IS_LABEL from the label map.
__global__ __launch_bounds__(256) void k_mb_seed(const MbFrame *__restrict__ frames, int n_frames, const uint8_t *__restrict__ coords, MbCanvas cv,
                                                 const int32_t *__restrict__ labels, uint8_t *__restrict__ work)
{
    const MbFrame &fr = frames[mb_frame_of(frames, n_frames, 0, blockIdx.x)];
    const uint64_t n = (uint64_t)fr.gw * (uint64_t)fr.gh;
    const uint64_t p0 = ((uint64_t)(blockIdx.x - fr.blk0[0]) * 256 + threadIdx.x) * 4;
    if (p0 >= n) return;
    uint32_t word = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint64_t p = p0 + t;
        if (p >= n) break;
        const uint64_t ly = p / (uint32_t)fr.gw;
        const int64_t x = fr.gx + (int64_t)(p - ly * (uint32_t)fr.gw), y = fr.gy + (int64_t)ly;
        if (x < 0 || x >= cv.cw || y < 0 || y >= cv.ch) continue;
        float2 s;
        uint64_t at;
        if (!mos_covers(fr.m, cv.cx + x, cv.cy + y, coords, &s, &at)) continue;
        const uint32_t flag = MB_CONTRIBUTES | (labels[(uint64_t)y * (uint64_t)cv.cw + (uint64_t)x] == fr.index ? MB_IS_LABEL : 0u);
        word |= flag << (8 * t);
    }
    uint8_t *__restrict__ o = work + fr.flag_off + p0;
    if (p0 + 4 <= n) { *reinterpret_cast<uint32_t *>(o) = word; return; }     // (flag_off is a multiple of 256)
    for (uint64_t t = 0; p0 + t < n; t++) o[t] = (uint8_t)(word >> (8 * t));
}

// ------------------------------------------------------------------------------------------------ step 4: reduce
// Level lv of every frame from level lv - 1, images and weights alike: 32 x 8 outputs per block, one per lane; block b belongs to the last
// frame whose blk0[lv] <= b and owns tile b - blk0[lv] of its level-lv grid.  The 67 x 19 input tile -- outputs (x, y) read inputs
// 2x - 2 .. 2x + 2 -- is staged in LDS for the C channels and the weight, 0.0f outside the frame's grid; the row sums of its 19 rows at the
// 32 output columns go to LDS too, and every lane adds five of them.  FIRST (lv == 1): the input is the frame's own pixels, gained, where
// the flag byte says MB_CONTRIBUTES (the window holds such a pixel), and the weight is 1.0f where it says MB_IS_LABEL.
template <typename E, int C, bool FIRST>
__global__ __launch_bounds__(256) void k_mb_reduce(const MbFrame *__restrict__ frames, int n_frames, int lv, MbCanvas cv, const uint8_t *__restrict__ pixels,
                                                   uint8_t *__restrict__ work)
{
    __shared__ float tile[C + 1][kMbInH][kMbInW + 1];
    __shared__ float rows[C + 1][kMbInH][kMbTileW];
    const MbFrame &fr = frames[mb_frame_of(frames, n_frames, lv, blockIdx.x)];
    const int iw = fr.gw >> (lv - 1), ih = fr.gh >> (lv - 1), ow = iw >> 1, oh = ih >> 1;
    const uint32_t tiles_x = (uint32_t)(ow + kMbTileW - 1) / kMbTileW, b = blockIdx.x - fr.blk0[lv];
    const int ox0 = (int)(b % tiles_x) * kMbTileW, oy0 = (int)(b / tiles_x) * kMbTileH;
    const int ix0 = 2 * ox0 - 2, iy0 = 2 * oy0 - 2;
    const int tid = threadIdx.y * kMbTileW + threadIdx.x;
    const float *__restrict__ src_i = reinterpret_cast<const float *>(work + fr.img_off[FIRST ? 1 : lv - 1]);      // (FIRST: not read)
    const float *__restrict__ src_m = reinterpret_cast<const float *>(work + fr.msk_off[FIRST ? 1 : lv - 1]);
    for (int e = tid; e < kMbInH * kMbInW; e += 256) {
        const int r = e / kMbInW, q = e - r * kMbInW;
        const int x = ix0 + q, y = iy0 + r;
        float v[C], m = 0.0f;
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = 0.0f;
        if (x >= 0 && x < iw && y >= 0 && y < ih) {
            const uint64_t at = (uint64_t)y * (uint64_t)iw + (uint64_t)x;
            if constexpr (FIRST) {
                const uint32_t flag = work[fr.flag_off + at];
                if (flag & MB_CONTRIBUTES) {
                    const int64_t u = (int64_t)cv.cx + fr.gx + x - fr.m.x_off, w = (int64_t)cv.cy + fr.gy + y - fr.m.y_off;
                    mb_pixel<E, C>(fr, (uint64_t)w * (uint64_t)fr.m.obj_w + (uint64_t)u, pixels, v);
                }
                m = (flag & MB_IS_LABEL) ? 1.0f : 0.0f;
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) v[c] = src_i[at * C + c];
                m = src_m[at];
            }
        }
#pragma unroll
        for (int c = 0; c < C; c++) tile[c][r][q] = v[c];
        tile[C][r][q] = m;
    }
    __syncthreads();
    for (int e = tid; e < kMbInH * kMbTileW; e += 256) {
        const int r = e / kMbTileW, x = e - r * kMbTileW;
#pragma unroll
        for (int p = 0; p <= C; p++) {
            const float *t = &tile[p][r][2 * x];
            rows[p][r][x] = mb_sum5(t[0], t[1], t[2], t[3], t[4]);
        }
    }
    __syncthreads();
    const int ox = ox0 + (int)threadIdx.x, oy = oy0 + (int)threadIdx.y;
    if (ox >= ow || oy >= oh) return;
    const uint64_t at = (uint64_t)oy * (uint64_t)ow + (uint64_t)ox;
    float *__restrict__ dst_i = reinterpret_cast<float *>(work + fr.img_off[lv]);
    float *__restrict__ dst_m = reinterpret_cast<float *>(work + fr.msk_off[lv]);
    const int r0 = 2 * (int)threadIdx.y, xx = (int)threadIdx.x;
#pragma unroll
    for (int p = 0; p <= C; p++) {
        const float o = mb_sum5(rows[p][r0][xx], rows[p][r0 + 1][xx], rows[p][r0 + 2][xx], rows[p][r0 + 3][xx], rows[p][r0 + 4][xx]) * 0.00390625f;
        if (p < C) dst_i[at * C + p] = o; else dst_m[at] = o;
    }
}

// ------------------------------------------------------------------------------------------------ steps 6 and 7: blend, collapse, store
// Level k of the canvas grid, one position per lane, the mosaic's tile (64 x 4) and walk: the frame table in ascending order by the whole
// block, frames whose level-k grid misses the tile skipped from their record on the scalar side.  Per frame the weight is read first; the
// image value and the up to nine taps of the level above are read only where it is not 0.0f.  Levels >= 1 cover the whole canvas grid and
// store R_k in the work area.  LAST (k == 0) covers the canvas pixels only: the weight is the flag bit MB_IS_LABEL and the image the
// frame's own pixel, gained; it rounds and stores canvas and weight with nontemporal stores, zeros where no frame owns the pixel.
template <typename E, int C, bool LAST>
__global__ __launch_bounds__(256) void k_mb_blend(const MbFrame *__restrict__ frames, int n_frames, int k, MbCanvas cv, const uint8_t *__restrict__ pixels,
                                                  uint8_t *__restrict__ work, uint32_t tiles_x, uint8_t *__restrict__ canvas, float *__restrict__ weight)
{
    const int wk = LAST ? cv.cw : cv.pw >> k, hk = LAST ? cv.ch : cv.ph >> k, org = LAST ? 0 : cv.A >> k;      // this launch's raster; its origin in level coordinates is -org
    const bool top = k == cv.L - 1;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t i0 = (int64_t)tx * 64, j0 = (int64_t)ty * 4;
    const int64_t x0 = i0 - org, y0 = j0 - org, x1 = min(i0 + 64, (int64_t)wk) - org, y1 = min(j0 + 4, (int64_t)hk) - org;
    const int64_t i = i0 + threadIdx.x, j = j0 + threadIdx.y;
    if (i >= wk || j >= hk) return;
    const int64_t x = i - org, y = j - org;
    float num[C], den = 0.0f;
#pragma unroll
    for (int c = 0; c < C; c++) num[c] = 0.0f;
    for (int f = 0; f < n_frames; f++) {
        const MbFrame &fr = frames[f];
        const int64_t gx = fr.gx >> k, gy = fr.gy >> k, gw = fr.gw >> k, gh = fr.gh >> k;      // (gx, gy: multiples of A, so the shift is exact)
        if (gx >= x1 || gx + gw <= x0 || gy >= y1 || gy + gh <= y0) continue;
        const int64_t lx = x - gx, ly = y - gy;
        if (lx < 0 || lx >= gw || ly < 0 || ly >= gh) continue;
        const uint64_t at = (uint64_t)ly * (uint64_t)gw + (uint64_t)lx;
        float w, v[C];
        if constexpr (LAST) {
            if (!(work[fr.flag_off + at] & MB_IS_LABEL)) continue;
            w = 1.0f;
            const int64_t u = (int64_t)cv.cx + x - fr.m.x_off, t = (int64_t)cv.cy + y - fr.m.y_off;      // (the label's frame contributes here)
            mb_pixel<E, C>(fr, (uint64_t)t * (uint64_t)fr.m.obj_w + (uint64_t)u, pixels, v);
        } else {
            w = reinterpret_cast<const float *>(work + fr.msk_off[k])[at];
            if (w == 0.0f) continue;
            const float *__restrict__ im = reinterpret_cast<const float *>(work + fr.img_off[k]);
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = im[at * C + c];
        }
        if (!top) {
            float e[C];
            mb_expand<C>(reinterpret_cast<const float *>(work + fr.img_off[k + 1]), (int)(gw >> 1), (int)(gh >> 1), (int)lx, (int)ly, e);
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = v[c] - e[c];
        }
#pragma unroll
        for (int c = 0; c < C; c++) num[c] = num[c] + w * v[c];
        den = den + w;
    }
    float r[C];
#pragma unroll
    for (int c = 0; c < C; c++) r[c] = den > 0.0f ? num[c] / den : 0.0f;
    if (!top) {
        float e[C];
        mb_expand<C>(reinterpret_cast<const float *>(work + cv.r_off[k + 1]), cv.pw >> (k + 1), cv.ph >> (k + 1), (int)(x + (cv.A >> k)), (int)(y + (cv.A >> k)), e);
#pragma unroll
        for (int c = 0; c < C; c++) r[c] = r[c] + e[c];
    }
    const uint64_t at = (uint64_t)j * (uint64_t)wk + (uint64_t)i;
    if constexpr (!LAST) {
        float *__restrict__ o = reinterpret_cast<float *>(work + cv.r_off[k]) + at * C;
#pragma unroll
        for (int c = 0; c < C; c++) o[c] = r[c];
    } else {
        const bool owned = den > 0.0f;                            // at level 0 den counts the frames whose label this is: 1.0f or none
        if (weight) __builtin_nontemporal_store(owned ? 1.0f : 0.0f, weight + at);
        E *__restrict__ o = reinterpret_cast<E *>(canvas) + at * C;
        if constexpr (sizeof(E) == 4) {
#pragma unroll
            for (int c = 0; c < C; c++) __builtin_nontemporal_store(owned ? r[c] : 0.0f, o + c);
        } else {
            uint32_t q[C];
#pragma unroll
            for (int c = 0; c < C; c++) q[c] = owned ? (uint32_t)fminf(255.0f, fmaxf(0.0f, floorf(r[c] + 0.5f))) : 0u;
            if constexpr (C == 4) {
                if (!(reinterpret_cast<uintptr_t>(canvas) & 3)) { __builtin_nontemporal_store(q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24), reinterpret_cast<uint32_t *>(o)); return; }
            } else if constexpr (C == 2) {
                if (!(reinterpret_cast<uintptr_t>(canvas) & 1)) { __builtin_nontemporal_store((uint16_t)(q[0] | (q[1] << 8)), reinterpret_cast<uint16_t *>(o)); return; }
            }
#pragma unroll
            for (int c = 0; c < C; c++) __builtin_nontemporal_store((E)q[c], o + c);
        }
    }
}

// ------------------------------------------------------------------------------------------------ launcher
#ifdef __HIPCC__
static uint32_t mb_tiles(int w, int h, uint32_t *tiles_x)
{
    *tiles_x = (uint32_t)(((int64_t)w + 63) / 64);
    return (uint32_t)((uint64_t)*tiles_x * (uint64_t)(((int64_t)h + 3) / 4));
}

void launch_multiband(const MbArgs &a, hipStream_t stream)
{
    const MbCanvas &cv = a.cv;
    if (cv.cw <= 0 || cv.ch <= 0) return;
    uint32_t tiles_x = 0;
    const uint32_t canvas_blocks = mb_tiles(cv.cw, cv.ch, &tiles_x);
    hipLaunchKernelGGL(k_mb_label, dim3(canvas_blocks), dim3(64, 4), 0, stream, a.quads, a.n_quads, a.coords, a.W, a.H, a.feather, cv.cx, cv.cy, cv.cw, cv.ch, tiles_x,
                       a.labels);
    if (a.blocks[0]) hipLaunchKernelGGL(k_mb_seed, dim3(a.blocks[0]), dim3(256), 0, stream, a.frames, a.n_frames, a.coords, cv, a.labels, a.work);
    for_elem_channels(a.elem, a.channels, [&](auto e, auto c) {
        using E = decltype(e);
        constexpr int C = decltype(c)::value;
        for (int lv = 1; lv < cv.L; lv++) {
            if (!a.blocks[lv]) continue;
            if (lv == 1) hipLaunchKernelGGL((k_mb_reduce<E, C, true>), dim3(a.blocks[lv]), dim3(kMbTileW, kMbTileH), 0, stream, a.frames, a.n_frames, lv, cv, a.pixels, a.work);
            else hipLaunchKernelGGL((k_mb_reduce<float, C, false>), dim3(a.blocks[lv]), dim3(kMbTileW, kMbTileH), 0, stream, a.frames, a.n_frames, lv, cv, a.pixels, a.work);
        }
        for (int k = cv.L - 1; k >= 1; k--) {
            uint32_t tx = 0;
            const uint32_t nb = mb_tiles(cv.pw >> k, cv.ph >> k, &tx);
            hipLaunchKernelGGL((k_mb_blend<float, C, false>), dim3(nb), dim3(64, 4), 0, stream, a.frames, a.n_frames, k, cv, a.pixels, a.work, tx, a.canvas, a.weight);
        }
        hipLaunchKernelGGL((k_mb_blend<E, C, true>), dim3(canvas_blocks), dim3(64, 4), 0, stream, a.frames, a.n_frames, 0, cv, a.pixels, a.work, tiles_x, a.canvas, a.weight);
    });
}
#endif

} // namespace hg
