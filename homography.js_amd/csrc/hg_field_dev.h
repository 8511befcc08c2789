// hg_field_dev.h -- what the kernels that WRITE a source field share (hg_k_field.hip, hg_k_tps.hip): the value of one pixel in both formats
// (include/hgwarp.h, HG_FIELD_INDEX / HG_FIELD_COORDS) and the quad store.  Needs nothing but the HIP builtins, so a host check can include
// it behind a shim.
#pragma once
#include <math.h>
#include <stdint.h>

namespace hg {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr uint32_t kFieldNaN = 0x7fc00000u;      // both words of an uncovered pixel of HG_FIELD_COORDS

// HG_FIELD_INDEX of a pixel that passed the coverage test: Math.round(sy) * W + Math.round(sx) (:1005 / :1049) where that lies in the array,
// else -1 (JS reads `undefined`, stored as 0).  In doubles: exact below 2^53, and a product beyond that is far outside [0, n_src_px) either way.
__device__ __forceinline__ int field_index(double sx, double sy, double w, double n_src_px)
{
    double rx = floor(sx), ry = floor(sy);
    if (sx - rx >= 0.5) rx += 1.0;
    if (sy - ry >= 0.5) ry += 1.0;
    const double idx = ry * w + rx;
    return (idx >= 0.0 && idx < n_src_px) ? (int)idx : -1;
}

// One pixel's field value: FMT 0 -> x = index; FMT 1 -> (x, y) = bit patterns of ((float)sx, (float)sy) or of the quiet NaN.
template <int FMT>
__device__ __forceinline__ void field_px(bool covered, double sx, double sy, double w, double n_src_px, int &x, int &y)
{
    if (FMT == 0) { x = covered ? field_index(sx, sy, w, n_src_px) : -1; y = 0; }
    else { x = covered ? __float_as_int((float)sx) : (int)kFieldNaN; y = covered ? __float_as_int((float)sy) : (int)kFieldNaN; }
}

// Four consecutive pixels of one row, starting at column cq (16-byte non-temporal stores where the row pitch and the frame's start allow it).
template <int FMT>
__device__ __forceinline__ void field_store_quad(uint8_t *__restrict__ row, int cq, int W, bool vec_ok, const int vx[4], const int vy[4])
{
    if (FMT == 0) {
        int *__restrict__ p = reinterpret_cast<int *>(row) + cq;
        if (vec_ok && cq + 3 < W) { v4i v = { vx[0], vx[1], vx[2], vx[3] }; __builtin_nontemporal_store(v, reinterpret_cast<v4i *>(p)); }
        else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (cq + k < W) __builtin_nontemporal_store(vx[k], p + k);
        }
    } else {
        int *__restrict__ p = reinterpret_cast<int *>(row) + 2 * (size_t)cq;
        if (vec_ok && cq + 3 < W) {
            v4i a = { vx[0], vy[0], vx[1], vy[1] }, b = { vx[2], vy[2], vx[3], vy[3] };
            __builtin_nontemporal_store(a, reinterpret_cast<v4i *>(p));
            __builtin_nontemporal_store(b, reinterpret_cast<v4i *>(p) + 1);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (cq + k < W) { __builtin_nontemporal_store(vx[k], p + 2 * k); __builtin_nontemporal_store(vy[k], p + 2 * k + 1); }
        }
    }
}

} // namespace hg
