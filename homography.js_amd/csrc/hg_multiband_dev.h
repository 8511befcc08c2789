// hg_multiband_dev.h -- the one text of what the multi-band mosaic's kernels and its host path share (hg_k_multiband.hip,
// hg_api_multiband.hip; include/hgwarp.h hg_mosaic_multiband_device): the records of the frame table, the rank of a contributor, the 5-tap
// sum of the reduce, the 1-D rule of the expand and the expansion of one position.  Needs hg_mosaic_dev.h only, so the host check of
// tests/cpp compiles it with the kernel file.  All arithmetic is f32 in the written order (contraction off); the numpy model of
// tests/hgtest/multiband.py follows it operation by operation.
#pragma once
#include "hg_mosaic_dev.h"

namespace hg {

// (The records MbFrame and MbCanvas and the tile constants: hg_remap_records.h.)  The flag byte of a frame-grid pixel.
enum : uint32_t { MB_CONTRIBUTES = 1, MB_IS_LABEL = 2 };

// The frame of block b in launch `lv` (0: seed, k: the reduce that writes level k): the last one whose blk0[lv] <= b; uniform over the block.
__device__ __forceinline__ int mb_frame_of(const MbFrame *__restrict__ frames, int n, int lv, uint32_t b)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (frames[mid].blk0[lv] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// The rank of a contributor: HG_MOSAIC_FEATHER's weight (step 6 of hg_mosaic_frames_device), the same expression, cap and floor.
__device__ __forceinline__ float mb_rank(float2 s, float fw, float fh, float feather)
{
    const float dx = fminf(s.x + 1.0f, fw - s.x), dy = fminf(s.y + 1.0f, fh - s.y);
    return fmaxf(fminf(fminf(dx, dy), feather), 0x1p-10f);
}

// The 5-tap sum of the reduce, along a row and then along the column of the row sums (the caller scales by 1 / 256 once).
__device__ __forceinline__ float mb_sum5(float t0, float t1, float t2, float t3, float t4)
{
    return ((t0 + t4) + (t1 + t3) * 4.0f) + t2 * 6.0f;
}

// The 1-D rule of the expand at position x of level k from level k + 1: x even, i = x / 2: a, b, c = T[i-1], T[i], T[i+1]; x odd,
// i = (x - 1) / 2: b, c = T[i], T[i+1] (a is not read).
__device__ __forceinline__ float mb_expand1(bool odd, float a, float b, float c)
{
    return odd ? (b + c) * 0.5f : ((a + c) + b * 6.0f) * 0.125f;
}

// expand(T)(lx, ly) for the C interleaved channels of T, w x h pixels of level k + 1 (0.0f outside); (lx, ly) >= 0 is the position of
// level k relative to the grid's origin, which is even, so parity is the position's own.  Horizontally on the at most three rows the
// vertical rule needs, then vertically.
template <int C>
__device__ __forceinline__ void mb_expand(const float *__restrict__ T, int w, int h, int lx, int ly, float out[C])
{
    const int i = lx >> 1, j = ly >> 1;
    const bool ox = (lx & 1) != 0, oy = (ly & 1) != 0;
    float r[3][C];
#pragma unroll
    for (int dj = 0; dj < 3; dj++) {
        const int row = j - 1 + dj;
        const bool row_in = row >= 0 && row < h && !(dj == 0 && oy);
#pragma unroll
        for (int c = 0; c < C; c++) {
            float t[3];
#pragma unroll
            for (int di = 0; di < 3; di++) {
                const int col = i - 1 + di;
                t[di] = 0.0f;
                if (row_in && col >= 0 && col < w && !(di == 0 && ox)) t[di] = T[((uint64_t)row * (uint64_t)w + (uint64_t)col) * C + c];
            }
            r[dj][c] = mb_expand1(ox, t[0], t[1], t[2]);
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) out[c] = mb_expand1(oy, r[0][c], r[1][c], r[2][c]);
}

} // namespace hg
