// hg_k_pyramid.hip -- minification filtering on the field seam (include/hgwarp.h, hg_pyramid_* / hg_remap_trilinear_frames_device):
// k_pyr_down builds one level of a plane's mip pyramid from the level below it, k_remap_trilinear_frames gathers a plane and its pyramid
// through a HG_FIELD_COORDS field, choosing the level(s) of every pixel from the field's own footprint.
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  All arithmetic is f32 in the written order (contraction off); the numpy model of
// tests/hgtest/trilinear.py follows it operation by operation.  Design notes: DESIGN.md §4.9, figures: EXPERIMENTS.md F.5.
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_remap_dev.h"

namespace hg {

// ------------------------------------------------------------------------------------------------ one pyramid level
// Level k (Wd x Hd) from level k - 1 (Ws x Hs) of every plane: pixel (x, y) averages the pixels at columns min(2x, Ws-1), min(2x+1, Ws-1)
// and rows alike -- u8: ((a + b) + (c + d) + 2) >> 2; f32: ((a + b) + (c + d)) * 0.25f.  One output pixel per lane, 64 x 4 pixels per
// block; rows beyond gridDim.y * 4 and planes beyond gridDim.z are strided over.  Reads stay inside [0, Ws) x [0, Hs) by the clamps.
template <typename E, int C>
__global__ __launch_bounds__(256) void k_pyr_down(const uint8_t *__restrict__ src, size_t src_stride, int Ws, int Hs, uint8_t *__restrict__ dst,
                                                  size_t dst_stride, int Wd, int Hd, int n_planes)
{
    using V = remap_px_t<E>;
    constexpr bool kBytes = sizeof(E) == 1 && (C == 2 || C == 4);
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= Wd) return;
    const int64_t c0 = min(2 * (int64_t)x, (int64_t)Ws - 1), c1 = min(2 * (int64_t)x + 1, (int64_t)Ws - 1);
    for (int pl = blockIdx.z; pl < n_planes; pl += gridDim.z) {
        const E *__restrict__ s = reinterpret_cast<const E *>(src + (size_t)pl * src_stride);
        E *__restrict__ d = reinterpret_cast<E *>(dst + (size_t)pl * dst_stride);
        const bool s_wide = kBytes && !(reinterpret_cast<uintptr_t>(s) & (C - 1));
        const bool d_wide = kBytes && !(reinterpret_cast<uintptr_t>(d) & (C - 1));
        for (int64_t y = (int64_t)blockIdx.y * 4 + threadIdx.y; y < Hd; y += (int64_t)gridDim.y * 4) {
            const int64_t r0 = min(2 * y, (int64_t)Hs - 1) * Ws, r1 = min(2 * y + 1, (int64_t)Hs - 1) * Ws;
            V a[C], b[C], c[C], e[C];
            remap_px_load<E, C>(s + (r0 + c0) * C, s_wide, a);
            remap_px_load<E, C>(s + (r0 + c1) * C, s_wide, b);
            remap_px_load<E, C>(s + (r1 + c0) * C, s_wide, c);
            remap_px_load<E, C>(s + (r1 + c1) * C, s_wide, e);
            E *__restrict__ o = d + (y * Wd + x) * C;
            if constexpr (sizeof(E) == 4) {
#pragma unroll
                for (int ch = 0; ch < C; ch++) o[ch] = ((a[ch] + b[ch]) + (c[ch] + e[ch])) * 0.25f;
            } else {
                uint32_t v[C];
#pragma unroll
                for (int ch = 0; ch < C; ch++) v[ch] = ((a[ch] + b[ch]) + (c[ch] + e[ch]) + 2u) >> 2;
                if constexpr (C == 4) {
                    if (d_wide) { *reinterpret_cast<uint32_t *>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24); continue; }
                } else if constexpr (C == 2) {
                    if (d_wide) { *reinterpret_cast<uint16_t *>(o) = (uint16_t)(v[0] | (v[1] << 8)); continue; }
                }
#pragma unroll
                for (int ch = 0; ch < C; ch++) o[ch] = (uint8_t)v[ch];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the trilinear remap
// The coordinate of (sx, sy) on level k >= 1: ((s + 0.5) * 2^-k) - 0.5, and that level of the pyramid at pyr.
template <typename E, int C>
__device__ __forceinline__ void tri_sample_level(const E *__restrict__ plane, bool plane_wide, const uint8_t *__restrict__ pyr, bool pyr_wide,
                                                 const uint64_t *__restrict__ lvl_off, int W, int H, int k, float2 s, float r[C])
{
    if (k == 0) { tri_sample<E, C>(plane, plane_wide, W, H, s.x, s.y, r); return; }
    const float inv = __uint_as_float((uint32_t)(127 - k) << 23);
    const float u = ((s.x + 0.5f) * inv) - 0.5f, v = ((s.y + 0.5f) * inv) - 0.5f;
    tri_sample<E, C>(reinterpret_cast<const E *>(pyr + lvl_off[k]), pyr_wide, pyr_size(W, k), pyr_size(H, k), u, v, r);
}

// One pixel per lane over the frame's flat list, read as obj_w x obj_h.  The footprint of pixel (i, j) comes from the field itself: the
// squared step to the horizontal neighbour ((i+1, j), else (i-1, j)) and to the vertical one, the larger of the two being q.  The
// neighbours are LOADED, not exchanged between lanes: the vertical one lies obj_w pixels away in any case, the horizontal one is the
// next lane's cache line, and an exchange would need every lane of the wave alive at frame and row ends.  q <= 1: level 0 alone (the
// bilinear frames remap, bit for bit).  Else k = floor(log2(q)) >> 1 -- the exponent field of q --, level levels-1 alone if k reaches it,
// otherwise levels k and k+1 blended by t = (q / 4^k - 1) / 3.  lvl_off: byte offsets of levels 1 .. levels-1 inside a pyramid.
template <typename E, int C>
__global__ __launch_bounds__(256) void k_remap_trilinear_frames(const TriRemapFrame *__restrict__ frames, int n_frames, uint64_t blk_px,
                                                                const uint64_t *__restrict__ lvl_off, int levels,
                                                                const uint8_t *__restrict__ coords, const uint8_t *__restrict__ planes,
                                                                const uint8_t *__restrict__ pyrs, int W, int H, uint8_t *__restrict__ out)
{
    const TriRemapFrame fr = remap_frame_of(frames, n_frames, blockIdx.x);
    const float2 *__restrict__ cf = reinterpret_cast<const float2 *>(coords + fr.fld_off);
    const E *__restrict__ src = reinterpret_cast<const E *>(planes + fr.plane_off);
    const uint8_t *__restrict__ pyr = pyrs + fr.pyr_off;           // (never read with levels == 1)
    E *__restrict__ o = reinterpret_cast<E *>(out + fr.out_off);
    const uint64_t p0 = (uint64_t)(blockIdx.x - fr.blk0) * blk_px;
    const uint64_t end = min(fr.n_px, p0 + blk_px);
    constexpr bool kBytes = sizeof(E) == 1 && (C == 2 || C == 4);
    const bool src_wide = kBytes && !(reinterpret_cast<uintptr_t>(src) & (C - 1));
    const bool pyr_wide = kBytes && !(reinterpret_cast<uintptr_t>(pyr) & (C - 1));      // (level offsets are multiples of 256)
    const bool out_wide = kBytes && !(reinterpret_cast<uintptr_t>(o) & (C - 1));
    const uint64_t ow = fr.obj_w, oh = fr.obj_h;
    const uint64_t row0 = p0 / ow, col0 = p0 - row0 * ow;        // (uniform over the block)
    for (uint64_t i = p0 + threadIdx.x; i < end; i += 256) {
        uint64_t px, py;
        remap_px_xy(col0 + (i - p0), ow, row0, &px, &py);
        const float2 s = cf[i];
        float v[C];
#pragma unroll
        for (int ch = 0; ch < C; ch++) v[ch] = 0.0f;
        if (remap_finite(s)) {
            float dx, dy;                                          // (the steps' directions: the anisotropic kernel's business)
            const float qh = remap_step(cf, s, px + 1 < ow, i + 1, px >= 1, i - 1, &dx, &dy);
            const float qv = remap_step(cf, s, py + 1 < oh, i + ow, py >= 1, i - ow, &dx, &dy);
            const float q = fmaxf(qh, qv);
            const RemapLevels lv = remap_levels(q, levels);
            const int k = lv.k;
            const float w = lv.w;                                  // weight of level k + 1
            tri_sample_level<E, C>(src, src_wide, pyr, pyr_wide, lvl_off, W, H, k, s, v);
            if (lv.n == 2) {
                float hi[C];
                tri_sample_level<E, C>(src, src_wide, pyr, pyr_wide, lvl_off, W, H, k + 1, s, hi);
#pragma unroll
                for (int ch = 0; ch < C; ch++) v[ch] = v[ch] + (hi[ch] - v[ch]) * w;
            }
        }
        remap_px_store<E, C>(o, i, out_wide, v);
    }
}

// ------------------------------------------------------------------------------------------------ launchers
#ifdef __HIPCC__
void launch_pyr_down(const uint8_t *src, size_t src_stride, int Ws, int Hs, uint8_t *dst, size_t dst_stride, int Wd, int Hd, int n_planes,
                     int elem, int channels, hipStream_t stream)
{
    if (n_planes <= 0 || Wd <= 0 || Hd <= 0) return;
    const dim3 grid((unsigned)((Wd + 63) / 64), (unsigned)std::min((Hd + 3) / 4, 65535), (unsigned)std::min(n_planes, 65535));
    for_elem_channels(elem, channels, [&](auto e, auto c) {
        hipLaunchKernelGGL((k_pyr_down<decltype(e), decltype(c)::value>), grid, dim3(64, 4), 0, stream, src, src_stride, Ws, Hs, dst, dst_stride, Wd, Hd, n_planes);
    });
}

void launch_remap_trilinear_frames(const TriRemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, const uint64_t *lvl_off, int levels,
                                   const uint8_t *coords, const uint8_t *planes, const uint8_t *pyrs, int W, int H, int elem, int channels,
                                   uint8_t *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_blocks == 0) return;
    for_elem_channels(elem, channels, [&](auto e, auto c) {
        hipLaunchKernelGGL((k_remap_trilinear_frames<decltype(e), decltype(c)::value>), dim3(n_blocks), dim3(256), 0, stream, frames, n_frames, blk_px, lvl_off, levels,
                           coords, planes, pyrs, W, H, out);
    });
}
#endif

} // namespace hg
