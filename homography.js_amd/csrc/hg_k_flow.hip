// hg_k_flow.hip -- dense optical flow between plane pairs, pyramidal Lucas-Kanade (include/hgwarp.h, "dense optical flow").
//   k_flow_up       the flow of a level from the level below it: the f32 bilinear remap's blend of the (u, v) pairs, times 2
//   k_flow_iter     one Jacobi iteration of one level, one workgroup per tile of kFlowTileW x kFlowTileH pixels of one frame: T with a halo of
//                   radius + 1 goes into LDS, every pixel of the tile plus halo gets its gradients and its eq (four taps of F at its own flow),
//                   the five window sums are formed separably in LDS -- rows, then columns --, and every pixel of the tile solves its 2 x 2
//                   system and writes the new flow into the other buffer.  G is re-formed from the same tile instead of being stored
//   k_flow_finish   field, flow pairs and residual of level 0
//   k_field_compose_frames   the chained field of hg_field_compose_frames_device: the bilinear frames remap of a 2-channel f32 plane with the
//                   NaN pattern wherever a coordinate or a result is not finite
// Window sums are integers: no order, no atomics, no cross-workgroup reduction; two runs give the same bits.  The rules live in hg_flow_dev.h.
// The kernels need that header only, so a host check compiles this file behind a thread-index shim (tests/cpp/flow_check.cpp); the launchers
// are compiled under hipcc only.
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_flow_dev.h"

namespace hg {

// ------------------------------------------------------------------------------------------------ k_flow_up
// One pixel per lane, 64 x 4 pixels per block, blockIdx.z = the frame.
__global__ __launch_bounds__(256) void k_flow_up(FlowUpArgs a)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const size_t f = blockIdx.z;
    const float cx = ((float)x + 0.5f) * 0.5f - 0.5f, cy = ((float)y + 0.5f) * 0.5f - 0.5f;
    float r[2];
    tri_sample<float, 2, float>(reinterpret_cast<const float *>(a.coarse + f * (size_t)a.Wc * (size_t)a.Hc), false, a.Wc, a.Hc, cx, cy, r);
    a.fine[f * (size_t)a.W * (size_t)a.H + (size_t)y * a.W + x] = make_float2(r[0] * 2.0f, r[1] * 2.0f);
}

// ------------------------------------------------------------------------------------------------ k_flow_iter
// RMAX sizes the LDS (3: 30 KB, 7: 45 KB); the radius itself is a.radius <= RMAX.  The tile plus halo is hw x hh pixels from (x0 - R, y0 - R);
// pixels of it outside the plane carry zeros, which is the clipping of the window.  T is loaded with clamped coordinates one pixel further
// out, so the one-sided border gradients are the plain difference of two LDS bytes.
template <int RMAX>
__global__ __launch_bounds__(kFlowBlock) void k_flow_iter(FlowIterArgs a)
{
    constexpr int HW = kFlowTileW + 2 * RMAX, HH = kFlowTileH + 2 * RMAX;
    __shared__ uint8_t s_t[(HH + 2) * (HW + 2)];
    __shared__ int16_t s_gx[HH * HW], s_gy[HH * HW];
    __shared__ int64_t s_eq[HH * HW];
    __shared__ int32_t r_xx[HH * kFlowTileW], r_xy[HH * kFlowTileW], r_yy[HH * kFlowTileW];
    __shared__ int64_t r_bx[HH * kFlowTileW], r_by[HH * kFlowTileW];
    const int W = a.W, H = a.H, R = a.radius, tid = threadIdx.x;
    const int hw = kFlowTileW + 2 * R, hh = kFlowTileH + 2 * R, tw = hw + 2;
    const int x0 = blockIdx.x * kFlowTileW, y0 = blockIdx.y * kFlowTileH;
    const size_t f = blockIdx.z, n_px = (size_t)W * (size_t)H;
    const uint8_t *__restrict__ T = a.to + (f % (size_t)a.n_to_sets) * a.to_stride;
    const uint8_t *__restrict__ F = a.from + f * a.from_stride;
    const float2 *__restrict__ fin = a.flow_in + f * n_px;

    for (int i = tid; i < (hh + 2) * tw; i += kFlowBlock) {
        const int ly = i / tw, lx = i - ly * tw;
        const int qx = min(max(x0 - R - 1 + lx, 0), W - 1), qy = min(max(y0 - R - 1 + ly, 0), H - 1);
        s_t[i] = T[(size_t)qy * W + qx];
    }
    __syncthreads();
    for (int i = tid; i < hh * hw; i += kFlowBlock) {
        const int ly = i / hw, lx = i - ly * hw;
        const int qx = x0 - R + lx, qy = y0 - R + ly;
        int gx = 0, gy = 0;
        int64_t eq = 0;
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
            const int c = (ly + 1) * tw + lx + 1;
            gx = (int)s_t[c + 1] - (int)s_t[c - 1];
            gy = (int)s_t[c + tw] - (int)s_t[c - tw];
            const float2 uv = fin[(size_t)qy * W + qx];
            const float s = flow_sample(F, W, H, (float)qx + uv.x, (float)qy + uv.y);
            eq = flow_eq(s, (int)s_t[c], gx, gy, uv.x, uv.y);
        }
        s_gx[i] = (int16_t)gx; s_gy[i] = (int16_t)gy; s_eq[i] = eq;
    }
    __syncthreads();
    for (int i = tid; i < hh * kFlowTileW; i += kFlowBlock) {
        const int ly = i / kFlowTileW, cx = i - ly * kFlowTileW;
        int32_t xx = 0, xy = 0, yy = 0;
        int64_t bx = 0, by = 0;
        for (int k = 0; k <= 2 * R; k++) {
            const int j = ly * hw + cx + k;
            const int32_t gx = s_gx[j], gy = s_gy[j];
            const int64_t eq = s_eq[j];
            xx += gx * gx; xy += gx * gy; yy += gy * gy;
            bx += (int64_t)gx * eq; by += (int64_t)gy * eq;
        }
        r_xx[i] = xx; r_xy[i] = xy; r_yy[i] = yy; r_bx[i] = bx; r_by[i] = by;
    }
    __syncthreads();
    for (int i = tid; i < kFlowTileH * kFlowTileW; i += kFlowBlock) {
        const int ty = i / kFlowTileW, tx = i - ty * kFlowTileW;
        const int x = x0 + tx, y = y0 + ty;
        if (x >= W || y >= H) continue;
        int64_t xx = 0, xy = 0, yy = 0, bx = 0, by = 0;
        for (int k = 0; k <= 2 * R; k++) {
            const int j = (ty + k) * kFlowTileW + tx;
            xx += r_xx[j]; xy += r_xy[j]; yy += r_yy[j]; bx += r_bx[j]; by += r_by[j];
        }
        const size_t p = (size_t)y * W + x;
        float2 uv = fin[p];
        double det;
        const bool good = flow_good(xx, xy, yy, flow_window_n(x, y, W, H, R), a.min_eig, &det);
        if (good) {
            uv.x = flow_step(uv.x, flow_solve(yy, bx, xy, by, det), a.max_update);
            uv.y = flow_step(uv.y, flow_solve(xx, by, xy, bx, det), a.max_update);
        }
        a.flow_out[f * n_px + p] = uv;
        if (a.good) a.good[f * n_px + p] = good ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ k_flow_finish
// One pixel per lane, 64 x 4 pixels per block, blockIdx.z = the frame.
__global__ __launch_bounds__(256) void k_flow_finish(FlowFinishArgs a)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const size_t f = blockIdx.z, n_px = (size_t)a.W * (size_t)a.H, p = (size_t)y * a.W + x;
    const float2 uv = a.flow[f * n_px + p];
    const float sx = (float)x + uv.x, sy = (float)y + uv.y;
    const uint64_t off = a.offs[f].out_off;
    if (a.field) {
        const bool covered = sx >= 0.0f && sx < (float)a.W && sy >= 0.0f && sy < (float)a.H;      // (NaN fails)
        const float nan = __uint_as_float(0x7fc00000u);
        reinterpret_cast<float2 *>(a.field + off)[p] = covered ? make_float2(sx, sy) : make_float2(nan, nan);
    }
    if (a.flow_out) reinterpret_cast<float2 *>(a.flow_out + off)[p] = uv;
    if (a.residual) {
        const uint8_t *__restrict__ T = a.to + (f % (size_t)a.n_to_sets) * a.to_stride;
        a.residual[f * n_px + p] = flow_residual(flow_sample(a.from + f * a.from_stride, a.W, a.H, sx, sy), (int)T[p]);
    }
}

// ------------------------------------------------------------------------------------------------ k_field_compose_frames
// k_remap_bilinear_frames<float, 2> over the inner field of the frame, with another tail: a pixel whose outer coordinate is not finite, or
// whose blend has a part that is not finite (an inner tap that is NaN or infinite), holds the NaN pattern in both words.
__global__ __launch_bounds__(256) void k_field_compose_frames(const RemapFrame *__restrict__ frames, int n_frames, uint64_t blk_px,
                                                              const uint8_t *__restrict__ outer, const uint8_t *__restrict__ inner, size_t inner_stride,
                                                              int W, int H, uint8_t *__restrict__ out)
{
    const RemapFrame fr = remap_frame_of(frames, n_frames, blockIdx.x);
    const float2 *__restrict__ cf = reinterpret_cast<const float2 *>(outer + fr.fld_off);
    const float *__restrict__ src = reinterpret_cast<const float *>(inner + (size_t)fr.plane * inner_stride);
    float2 *__restrict__ o = reinterpret_cast<float2 *>(out + fr.out_off);
    const uint64_t p0 = (uint64_t)(blockIdx.x - fr.blk0) * blk_px;
    const uint64_t end = min(fr.n_px, p0 + blk_px);
    const float nan = __uint_as_float(0x7fc00000u);
    for (uint64_t i = p0 + threadIdx.x; i < end; i += 256) {
        const float2 s = cf[i];
        float2 r = make_float2(nan, nan);
        if (remap_finite(s)) {
            float v[2];
            tri_sample<float, 2, float>(src, false, W, H, s.x, s.y, v);
            if (remap_finite(make_float2(v[0], v[1]))) r = make_float2(v[0], v[1]);
        }
        o[i] = r;
    }
}

// ------------------------------------------------------------------------------------------------ launchers
#ifdef __HIPCC__
void launch_flow_up(const FlowUpArgs &a, int n_frames, hipStream_t stream)
{
    if (n_frames <= 0) return;
    hipLaunchKernelGGL(k_flow_up, dim3((unsigned)((a.W + 63) / 64), (unsigned)((a.H + 3) / 4), (unsigned)n_frames), dim3(64, 4), 0, stream, a);
}

void launch_flow_iter(const FlowIterArgs &a, int n_frames, hipStream_t stream)
{
    if (n_frames <= 0) return;
    const dim3 grid((unsigned)((a.W + kFlowTileW - 1) / kFlowTileW), (unsigned)((a.H + kFlowTileH - 1) / kFlowTileH), (unsigned)n_frames);
    if (a.radius <= 3) hipLaunchKernelGGL(k_flow_iter<3>, grid, dim3(kFlowBlock), 0, stream, a);
    else hipLaunchKernelGGL(k_flow_iter<kFlowMaxRadius>, grid, dim3(kFlowBlock), 0, stream, a);
}

void launch_flow_finish(const FlowFinishArgs &a, int n_frames, hipStream_t stream)
{
    if (n_frames <= 0) return;
    hipLaunchKernelGGL(k_flow_finish, dim3((unsigned)((a.W + 63) / 64), (unsigned)((a.H + 3) / 4), (unsigned)n_frames), dim3(64, 4), 0, stream, a);
}

void launch_field_compose_frames(const RemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, const uint8_t *outer, const uint8_t *inner,
                                 size_t inner_stride, int W, int H, uint8_t *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_blocks == 0) return;
    hipLaunchKernelGGL(k_field_compose_frames, dim3(n_blocks), dim3(256), 0, stream, frames, n_frames, blk_px, outer, inner, inner_stride, W, H, out);
}
#endif

} // namespace hg
