// hg_mosaic_dev.h -- the one text of what the mosaic's kernels share (hg_k_mosaic.hip, hg_k_mosaic_stats.hip): the window test of a tile,
// the contributor rule (steps 1-3 of hg_mosaic_frames_device in include/hgwarp.h), alone and with the fetch of the contributor's pixel.  Needs
// hg_remap_dev.h only, so the host checks of tests/cpp compile it with the kernel files.
#pragma once
#include "hg_remap_dev.h"

namespace hg {

// Does the window of `fr` meet the canvas tile [X0, X1) x [Y0, Y1) of destination space?  Everything here is uniform over the block: the
// test runs on the scalar side, from the record alone.
__device__ __forceinline__ bool mos_hits(const MosaicFrame &fr, int64_t X0, int64_t X1, int64_t Y0, int64_t Y1)
{
    return fr.obj_w > 0 && fr.obj_h > 0 && fr.x_off < X1 && (int64_t)fr.x_off + fr.obj_w > X0 && fr.y_off < Y1 && (int64_t)fr.y_off + fr.obj_h > Y0;
}

// Is frame `fr` a CONTRIBUTOR at destination position (X, Y) -- does its window hold the position and does its field cover it there (both
// coordinate words finite)?  Then the coordinate in *s and the pixel's index within the frame in *k.  No pixel is read.
__device__ __forceinline__ bool mos_covers(const MosaicFrame &fr, int64_t X, int64_t Y, const uint8_t *__restrict__ coords, float2 *s, uint64_t *k)
{
    const int64_t u = X - fr.x_off, v = Y - fr.y_off;
    if (u < 0 || u >= fr.obj_w || v < 0 || v >= fr.obj_h) return false;
    *k = (uint64_t)v * (uint64_t)fr.obj_w + (uint64_t)u;                     // (< 2^31)
    *s = reinterpret_cast<const float2 *>(coords + fr.fld_off)[*k];
    return remap_finite(*s);
}

// Frame `fr` at destination position (X, Y): false unless it contributes there; else the coordinate in *s and the pixel's channels in p.
// Bytes with 2 or 4 channels move as one load where the frame's start is aligned for it (uniform per frame).  The contributor test is
// mos_covers' and stays written out here: routed through mos_covers, the compiler schedules k_mosaic_frames differently (7 % more
// instructions in six of the eight plain instantiations), and that kernel's code is to stay what it was.
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

// The channels that carry exposure (hg_mosaic_overlap_stats_device, hg_mosaic_frames_gain_device): all of them, but not the alpha of a
// 4-channel frame.
constexpr int mos_stat_channels(int C) { return C == 4 ? 3 : C; }

} // namespace hg
