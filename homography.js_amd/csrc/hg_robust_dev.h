// hg_robust_dev.h -- the one text of the robust mosaic's rules (hg_k_robust.hip; include/hgwarp.h hg_mosaic_robust_device): the staging cap,
// the value of a contributor (step 2), the two ranks a mode asks for and the result from the ranked values (step 4).  Integers only, but
// for the one f32 multiply of a gain and the one of `trim`.  Needs hg_mosaic_dev.h only, so the host check of tests/cpp compiles it with
// the kernel file.
#pragma once
#include "hg_mosaic_dev.h"

namespace hg {

// The modes, as include/hgwarp.h numbers them (HG_ROBUST_*).
constexpr int ROB_MEDIAN = 0, ROB_TRIMMED = 1, ROB_MIN = 2, ROB_MAX = 3;

// The staging cap L_max: a tile that at most this many frames hit keeps every lane's contributors in LDS, one 32-bit word per slot and lane
// (1 KiB per slot and block of 256 lanes); a tile that more frames hit walks its list in global memory once per round instead.  LDS is what
// bounds the waves a CU holds here, so a launch takes no more slots than its frame set can fill: rob_cap.  The choice: DESIGN.md §4.20, the
// runs: EXPERIMENTS.md "Robust mosaic".  (A/B builds: make VARIANT=_l32 EXTRA=-DHG_ROBUST_LMAX=32.)
#ifndef HG_ROBUST_LMAX
#define HG_ROBUST_LMAX 64
#endif
constexpr uint32_t ROB_LMAX = HG_ROBUST_LMAX;
static_assert(ROB_LMAX >= 2 && ROB_LMAX <= 128, "the staging area is ROB_LMAX KiB of the 160 KiB a CU has, and a block must fit");
// The slots a launch over n_frames records allocates: no tile is hit by more frames than there are, and 16 / 32 / 64 slots leave room for
// 9 / 4 / 2 blocks on a CU.
constexpr uint32_t rob_cap(int n_frames) { return n_frames <= 16 && ROB_LMAX >= 16 ? 16u : n_frames <= 32 && ROB_LMAX >= 32 ? 32u : ROB_LMAX; }
// How far the walk over a lane's LDS column is unrolled (reads in flight).
#ifndef HG_ROBUST_UNROLL
#define HG_ROBUST_UNROLL 1
#endif

// A value every lane of the wave holds alike (an entry of the block's list, read from LDS), said so: the frame's record is then read on
// the scalar side, as the mosaic reads it.
__device__ __forceinline__ uint32_t rob_uniform(uint32_t v)
{
#ifdef __HIPCC__
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}

// Step 2: the byte of a gained exposure channel, min(255, floor(g * (float)p + 0.5f)) -- what mos_stored<uint8_t> (hg_k_mosaic.hip) stores
// of q = g * p, the same operations in the same order.  A byte again BEFORE it is ranked.
__device__ __forceinline__ uint32_t rob_gained(float g, uint32_t p)
{
    return (uint32_t)fminf(255.0f, floorf(g * (float)p + 0.5f));
}

// The C bytes of a contributor as one word, channel c in bits 8c..8c+7.
template <int C>
__device__ __forceinline__ uint32_t rob_pack(const uint32_t p[C])
{
    uint32_t w = 0;
#pragma unroll
    for (int c = 0; c < C; c++) w |= p[c] << (8 * c);
    return w;
}
__device__ __forceinline__ uint32_t rob_byte(uint32_t w, int c) { return (w >> (8 * c)) & 255u; }

// Step 4: the two ranks (0-based, lo <= hi) of the n >= 1 ascending values a mode reads.  MIN, MAX and an odd MEDIAN read one value
// (lo == hi); an even MEDIAN its two middle ones; TRIMMED the bounds t and n - 1 - t of what it keeps, t = min((int)(trim * (float)n),
// (n - 1) / 2) with the product as one f32 multiply, truncated (trim in [0, 0.5): the product is below 128).
__device__ __forceinline__ void rob_ranks(int mode, float trim, uint32_t n, uint32_t *lo, uint32_t *hi)
{
    if (mode == ROB_MIN) { *lo = 0; *hi = 0; }
    else if (mode == ROB_MAX) { *lo = n - 1; *hi = n - 1; }
    else if (mode == ROB_MEDIAN) { *lo = (n - 1) >> 1; *hi = n >> 1; }
    else {
        const uint32_t t = min((uint32_t)(int)(trim * (float)n), (n - 1) >> 1);
        *lo = t; *hi = n - 1 - t;
    }
}

// Step 4 for MIN, MAX and MEDIAN from a = s_lo and b = s_hi: with lo == hi (a + a + 1) >> 1 is a.
__device__ __forceinline__ uint32_t rob_middle(uint32_t a, uint32_t b) { return (a + b + 1) >> 1; }

// Step 4 for TRIMMED: S = s_lo + ... + s_hi over m = hi - lo + 1 values, then (2 S + m) / (2 m) in integer division (S <= 256 * 255; the
// compiler's expansion of the unsigned division is exact).
__device__ __forceinline__ uint32_t rob_trimmed(uint32_t S, uint32_t m) { return (2 * S + m) / (2 * m); }

} // namespace hg
