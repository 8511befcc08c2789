// hg_remap_records.h -- the device records of the remap family (hg_k_remap.hip, hg_k_pyramid.hip, hg_k_aniso.hip, hg_k_mosaic.hip, hg_k_bicubic.hip): what
// the host stages and the kernels read.  Plain C++ over <cstdint>, no HIP types: the host checks of tests/cpp include this very file.
#pragma once
#include <cstdint>

namespace hg {

// The remaps of a whole frame set in one launch.  A frame is a flat list of n_px pixels: its field at fld_off and its output at out_off
// (bytes), read from plane `plane`; blocks [blk0, next frame's blk0) of the grid cover it, blk_px pixels each (a multiple of 1024), so the
// frame of a block is found by a binary search over blk0 -- empty frames own no block.
struct RemapFrame { uint64_t fld_off, out_off, n_px; uint32_t blk0, plane; };
static_assert(sizeof(RemapFrame) == 32, "the table is staged in 8-byte words and passed by value");

// A frame of the trilinear remap: RemapFrame's flat list read as obj_w x obj_h, its plane at plane_off and that plane's pyramid at pyr_off
// (bytes from the bases the kernel gets).
struct TriRemapFrame { uint64_t fld_off, out_off, n_px, plane_off, pyr_off; uint32_t blk0, obj_w, obj_h, pad; };
static_assert(sizeof(TriRemapFrame) % 8 == 0, "the table is staged in 8-byte words");

// The bicubic remap's kernel (hg_k_bicubic.hip; include/hgwarp.h hg_remap_bicubic_frames_device): the seven polynomial coefficients of the
// (B, C) cubic, computed once per call on the host in double and rounded once to f32; passed by value.
// near(x) = (((p3*x) + p2)*x)*x + p0 on [0, 1], far(x) = ((((q3*x) + q2)*x) + q1)*x + q0 on [1, 2].
struct CubicCoef { float p3, p2, p0, q3, q2, q1, q0; };

// The mosaic (hg_k_mosaic.hip; include/hgwarp.h hg_mosaic_frames_device).  A frame: its HG_FIELD_COORDS field at fld_off and its pixels at
// pix_off (bytes from the bases the kernel gets), row-major obj_w x obj_h, pixel (i, j) at destination position (x_off + i, y_off + j).
struct MosaicFrame { uint64_t fld_off, pix_off; int32_t x_off, y_off, obj_w, obj_h; };
// The table goes four records at a time (one round trip of scalar loads per four window tests): the last quad is filled with empty frames.
struct MosaicFrame4 { MosaicFrame f[4]; };
static_assert(sizeof(MosaicFrame4) == 128, "the table is staged in 8-byte words");

// The multi-band mosaic (hg_k_multiband.hip; include/hgwarp.h hg_mosaic_multiband_device).
constexpr int kMbMaxBands = 8;
constexpr int kMbSeedPx = 1024;                               // grid pixels per block of k_mb_seed: 4 per lane
constexpr int kMbTileW = 32, kMbTileH = 8;                    // the output tile of k_mb_reduce; its input tile with the halo:
constexpr int kMbInW = 2 * kMbTileW + 3, kMbInH = 2 * kMbTileH + 3;
// A frame that TAKES PART (its window meets the canvas): the mosaic's record, its level-0 grid in canvas-relative coordinates -- aligned to
// A = 2^(L-1) with a margin of A, so level k's grid is this one shifted right by k --, where its flag bytes and its levels 1..L-1 of I (C
// floats per pixel) and M lie in the work area, its gain, its index in the caller's list (what a label names), and its first block in the
// seed launch (blk0[0]) and in the reduce launch that writes level k (blk0[k]).
struct MbFrame {
    MosaicFrame m;
    int32_t gx, gy, gw, gh;
    uint64_t flag_off;
    float gain; int32_t index;
    uint64_t img_off[kMbMaxBands], msk_off[kMbMaxBands];      // (entry 0 unused: level 0 is the frame's own pixels and the flag bytes)
    uint32_t blk0[kMbMaxBands];
};
static_assert(sizeof(MbFrame) == 224, "the table is staged in 8-byte words");
// The canvas window, the size of level 0 of its grid (origin (-A, -A)), the band count, A, and where levels 1..L-1 of R lie in the work area.
struct MbCanvas { int32_t cx, cy, cw, ch, pw, ph, L, A; uint64_t r_off[kMbMaxBands]; };

} // namespace hg
