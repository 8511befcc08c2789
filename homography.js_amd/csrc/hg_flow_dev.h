// hg_flow_dev.h -- the one text of the dense-flow rules (include/hgwarp.h, "dense optical flow"): the per-pixel arithmetic of
// hg_k_flow.hip, the tile constants and the argument blocks of its kernels.  Needs the remap helpers and the HIP qualifiers only -- from hg_dev.h
// under hipcc, from tests/cpp/hip_host_shim.h in the host check, which compiles the kernel file itself.  Window sums are integers (their order
// is free); everything floating is f32 or f64 in the written order, IEEE division, contraction off.
#pragma once
#include "hg_remap_dev.h"

namespace hg {

constexpr int kFlowTileW = 32, kFlowTileH = 16, kFlowBlock = 256;      // the output tile of k_flow_iter and its workgroup
constexpr int kFlowMaxRadius = 7, kFlowMaxLevels = 12, kFlowMaxIter = 32;

// One level of one call: T = TO's level, F = FROM's level, both W x H one-byte planes; frame f reads to + (f % n_to_sets) * to_stride and
// from + f * from_stride; its flow lies at f * W * H pairs of flow_in / flow_out.  good (or nullptr): one byte per pixel, frames W * H apart.
struct FlowIterArgs {
    const uint8_t *to; size_t to_stride; int n_to_sets; const uint8_t *from; size_t from_stride; int W, H, radius; double min_eig, max_update;
    const float2 *flow_in; float2 *flow_out; uint8_t *good;
};
// The flow of a level (W x H) from the level below it (Wc x Hc), all frames.
struct FlowUpArgs { const float2 *coarse; int Wc, Hc; float2 *fine; int W, H; };
// The outputs at level 0.  offs: one 16-byte record {out_off, 0} per frame (the byte offset of the frame's field, and of its flow pairs);
// field / flow / residual may be nullptr (not wanted).
struct FlowOff { uint64_t out_off, pad; };
struct FlowFinishArgs {
    const uint8_t *to; size_t to_stride; int n_to_sets; const uint8_t *from; size_t from_stride; int W, H; const float2 *flow; const FlowOff *offs;
    uint8_t *field, *flow_out, *residual;
};
// (The chained field, hg_field_compose_frames_device, takes the bilinear frames remap's table and arguments: no block of its own.)

// Pixels of the window |dx|, |dy| <= R around (x, y) that lie inside the W x H plane.
__device__ __forceinline__ int flow_window_n(int x, int y, int W, int H, int R)
{
    return (min(x + R, W - 1) - max(x - R, 0) + 1) * (min(y + R, H - 1) - max(y - R, 0) + 1);
}

// The good test on the window sums (all below 2^53, so the doubles are exact): trace > 0, det > 0 and det >= (4 n min_eig) trace.
// *det: the determinant as a double.
__device__ __forceinline__ bool flow_good(int64_t gxx, int64_t gxy, int64_t gyy, int n, double min_eig, double *det)
{
    const int64_t trace = gxx + gyy, d = gxx * gyy - gxy * gxy;
    *det = (double)d;
    return trace > 0 && d > 0 && (double)d >= ((4.0 * (double)n) * min_eig) * (double)trace;
}

// The bilinear sample of a one-byte plane at (u, v), by the remap rule.
__device__ __forceinline__ float flow_sample(const uint8_t *__restrict__ plane, int W, int H, float u, float v)
{
    float s;
    tri_sample<uint8_t, 1, float>(plane, false, W, H, u, v, &s);
    return s;
}

// eq of a pixel: the residual at its own flow, linearised back to a zero flow, in sixteenths.
__device__ __forceinline__ int64_t flow_eq(float s, int t, int gx, int gy, float u, float v)
{
    const float e = s - (float)t;
    const double e0 = (double)e - (((double)gx * (double)u) + ((double)gy * (double)v)) / 2.0;
    return (int64_t)llrint(16.0 * e0);
}

// One component of the window's common flow, -((a bx' - b by') / det) / 8, and the capped step towards it.
__device__ __forceinline__ double flow_solve(int64_t a, int64_t p, int64_t b, int64_t q, double det)
{
    return -((((double)a * (double)p) - ((double)b * (double)q)) / det) / 8.0;
}
__device__ __forceinline__ float flow_step(float u, double U, double cap)
{
    double d = U - (double)u;
    d = d < -cap ? -cap : (d > cap ? cap : d);
    return (float)((double)u + d);
}

// The residual byte: min(255, floor(|e| + 0.5f)).
__device__ __forceinline__ uint8_t flow_residual(float s, int t)
{
    return (uint8_t)fminf(255.0f, floorf(fabsf(s - (float)t) + 0.5f));
}

} // namespace hg
