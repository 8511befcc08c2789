// hg_api_flow.hip -- the C ABI, part 12: dense optical flow and chained fields (hg_flow_layout, hg_flow_dense_frames_device,
// hg_field_compose_frames_device).  The flow call is work of its own, like the aligner: it needs no image, mesh or frame set, and leaves the
// warp paths' taps (hg_last_*_kernel), the sampling mode, the plan of the last warp, what the policy learned and every staged frame set as it
// found them.  Scratch comes from the caller (hg_flow_layout), as multiband's does; nothing is waited for between levels or iterations.
#include "hg_ctx.h"
#include "hg_flow_dev.h"

#include <cmath>

constexpr int kFlowMaxSide = 32768, kFlowMaxFrames = 4096;

namespace {

// Where everything lies in the scratch of one call (bytes from d_scratch, each part at the 256-byte grain): the luma copies of 4-channel
// planes (every FROM plane, then the TO planes), the pyramids of both plane sets in hg_pyramid_layout's layout, one after the other, and two
// flow buffers per level (n_frames x Wk x Hk pairs each).
struct FlowPlan {
    size_t luma_from = 0, luma_to = 0, pyr_from = 0, pyr_to = 0, pyr_stride = 0, lvl[32] = {}, flow[kFlowMaxLevels][2] = {}, total = 0;
    int w[kFlowMaxLevels] = {}, h[kFlowMaxLevels] = {};
};

int check_flow_shape(hg_ctx *c, int W, int H, int channels, int levels)
{
    if (W < 1 || W > kFlowMaxSide || H < 1 || H > kFlowMaxSide || (int64_t)W * H > ((int64_t)1 << 30))
        return fail(c, HG_ERR_INVALID, "flow: W and H must be 1..32768 and W * H <= 2^30");
    if (channels != 1 && channels != 4) return fail(c, HG_ERR_INVALID, "flow: channels must be 1 or 4");
    if (levels < 1 || levels > std::min(hg_pyramid_levels(W, H), kFlowMaxLevels))
        return fail(c, HG_ERR_INVALID, "flow: levels must be 1..min(hg_pyramid_levels(W, H), 12)");
    return HG_OK;
}

int check_flow_sets(hg_ctx *c, int n_frames, int n_to_sets)
{
    if (n_frames < 0 || n_frames > kFlowMaxFrames) return fail(c, HG_ERR_INVALID, "flow: n_frames must be 0..4096");
    if (n_to_sets < 1 || n_to_sets > std::max(n_frames, 1)) return fail(c, HG_ERR_INVALID, "flow: n_to_sets must be 1..max(n_frames, 1)");
    return HG_OK;
}

void plan_flow(int W, int H, int channels, int n_frames, int n_to_sets, int levels, FlowPlan *p)
{
    const size_t F = (size_t)n_frames, S = (size_t)n_to_sets, n_px = (size_t)W * (size_t)H;
    size_t off = 0;
    if (channels == 4) {
        p->luma_from = off; off += pad256(F * n_px);
        p->luma_to = off; off += pad256(S * n_px);
    }
    hg_pyramid_layout(W, H, HG_ELEM_U8, 1, levels, p->lvl, &p->pyr_stride);      // (the shape was checked: cannot fail)
    p->pyr_from = off; off += F * p->pyr_stride;
    p->pyr_to = off; off += S * p->pyr_stride;
    for (int k = 0; k < levels; k++) {
        p->w[k] = W; p->h[k] = H;
        for (int b = 0; b < 2; b++) { p->flow[k][b] = off; off += pad256(F * (size_t)W * (size_t)H * 8); }
        W = (W + 1) >> 1; H = (H + 1) >> 1;
    }
    p->total = off;
}

} // namespace

extern "C" int hg_flow_layout(int W, int H, int channels, int n_frames, int n_to_sets, int levels, size_t *scratch_bytes)
{
    HG_TRY(check_flow_shape(nullptr, W, H, channels, levels));
    HG_TRY(check_flow_sets(nullptr, n_frames, n_to_sets));
    if (!scratch_bytes) return fail(nullptr, HG_ERR_INVALID, "hg_flow_layout: scratch_bytes is NULL");
    FlowPlan p;
    plan_flow(W, H, channels, n_frames, n_to_sets, levels, &p);
    *scratch_bytes = p.total;
    return HG_OK;
}

extern "C" int hg_flow_dense_frames_device(hg_ctx *c, const void *d_from, int n_frames, size_t from_stride_bytes, const void *d_to, int n_to_sets,
                                           size_t to_stride_bytes, int W, int H, int channels, int levels, int n_iter, int radius, double min_eig,
                                           double max_update, const size_t *field_offsets, void *d_field, void *d_flow, void *d_residual,
                                           void *d_good, void *d_scratch)
{
    // (the shape: needs no device)
    HG_TRY(check_flow_shape(c, W, H, channels, levels));
    if (n_iter < 1 || n_iter > kFlowMaxIter) return fail(c, HG_ERR_INVALID, "flow: n_iter must be 1..32");
    if (radius < 1 || radius > kFlowMaxRadius) return fail(c, HG_ERR_INVALID, "flow: radius must be 1..7");
    if (!(min_eig >= 0.0) || !(min_eig < INFINITY)) return fail(c, HG_ERR_INVALID, "flow: min_eig must be finite and >= 0");
    if (!(max_update > 0.0) || !(max_update <= 4.0)) return fail(c, HG_ERR_INVALID, "flow: max_update must lie in (0, 4]");
    HG_TRY(check_flow_sets(c, n_frames, n_to_sets));
    const size_t n_px = (size_t)W * (size_t)H, F = (size_t)n_frames;
    if (from_stride_bytes < n_px * (size_t)channels || to_stride_bytes < n_px * (size_t)channels)
        return fail(c, HG_ERR_INVALID, "flow: a plane stride must be >= W * H * channels");
    HG_TRY(bind(c));
    if (n_frames == 0) return HG_OK;
    std::vector<FlowOff> offs(F);
    size_t off = 0;
    for (size_t f = 0; f < F; f++) {
        offs[f] = FlowOff{field_offsets ? field_offsets[f] : off, 0};
        if (offs[f].out_off & 7) return fail(c, HG_ERR_INVALID, "field offsets must be multiples of the field's pixel size (4 or 8 bytes)");
        off += pad256(n_px * 8);
    }
    if (!d_from || !d_to || !d_field || !d_scratch) return fail(c, HG_ERR_INVALID, "hg_flow_dense_frames_device: d_from / d_to / d_field / d_scratch is NULL");
    if (misaligned(d_field, 8) || misaligned(d_flow, 8) || misaligned(d_scratch, 16))
        return fail(c, HG_ERR_INVALID, "hg_flow_dense_frames_device: d_field / d_flow must be aligned to 8 bytes, d_scratch to 16 bytes");
    HG_TRY(hg_sync(c));                                      // queued runs: settled first, as the aligner does
    FlowPlan p;
    plan_flow(W, H, channels, n_frames, n_to_sets, levels, &p);
    uint8_t *ws = static_cast<uint8_t *>(d_scratch);
    // the table of field offsets: through the field calls' staging, stream-ordered
    static_assert(sizeof(FlowOff) * 2 == sizeof(FrameDesc), "the field calls' frame table carries either record");
    HG_TRY(ensure(c, c->d_field_frames, (F + 1) / 2));
    HG_TRY(upload_frame_table(c, c->d_field_frames, offs.data(), sizeof(FlowOff) * F));
    // level 0 of both sides: the caller's planes, or their luma copies
    const uint8_t *from = static_cast<const uint8_t *>(d_from), *to = static_cast<const uint8_t *>(d_to);
    size_t from_stride = from_stride_bytes, to_stride = to_stride_bytes;
    if (channels == 4) {
        launch_align_luma(from, from_stride_bytes, W, H, n_frames, ws + p.luma_from, c->stream);
        launch_align_luma(to, to_stride_bytes, W, H, n_to_sets, ws + p.luma_to, c->stream);
        from = ws + p.luma_from; from_stride = n_px;
        to = ws + p.luma_to; to_stride = n_px;
    }
    // the pyramids: one launch per level and side, each reading the level before it
    const uint8_t *lf[kFlowMaxLevels], *lt[kFlowMaxLevels];
    size_t sf[kFlowMaxLevels], st[kFlowMaxLevels];
    lf[0] = from; sf[0] = from_stride; lt[0] = to; st[0] = to_stride;
    for (int k = 1; k < levels; k++) {
        uint8_t *df = ws + p.pyr_from + p.lvl[k], *dt = ws + p.pyr_to + p.lvl[k];
        launch_pyr_down(lf[k - 1], sf[k - 1], p.w[k - 1], p.h[k - 1], df, p.pyr_stride, p.w[k], p.h[k], n_frames, HG_ELEM_U8, 1, c->stream);
        launch_pyr_down(lt[k - 1], st[k - 1], p.w[k - 1], p.h[k - 1], dt, p.pyr_stride, p.w[k], p.h[k], n_to_sets, HG_ELEM_U8, 1, c->stream);
        lf[k] = df; sf[k] = p.pyr_stride; lt[k] = dt; st[k] = p.pyr_stride;
    }
    // the walk
    const float2 *cur = nullptr;
    for (int k = levels - 1; k >= 0; k--) {
        float2 *a = reinterpret_cast<float2 *>(ws + p.flow[k][0]), *b = reinterpret_cast<float2 *>(ws + p.flow[k][1]);
        if (k == levels - 1) HIP_TRY(c, hipMemsetAsync(a, 0, F * (size_t)p.w[k] * (size_t)p.h[k] * 8, c->stream));
        else launch_flow_up(FlowUpArgs{cur, p.w[k + 1], p.h[k + 1], a, p.w[k], p.h[k]}, n_frames, c->stream);
        for (int it = 0; it < n_iter; it++) {
            const bool last = k == 0 && it == n_iter - 1;
            launch_flow_iter(FlowIterArgs{lt[k], st[k], n_to_sets, lf[k], sf[k], p.w[k], p.h[k], radius, min_eig, max_update, a, b,
                                          last ? static_cast<uint8_t *>(d_good) : nullptr}, n_frames, c->stream);
            std::swap(a, b);
        }
        cur = a;
    }
    launch_flow_finish(FlowFinishArgs{lt[0], st[0], n_to_sets, lf[0], sf[0], W, H, cur, reinterpret_cast<const FlowOff *>(c->d_field_frames.p),
                                      static_cast<uint8_t *>(d_field), static_cast<uint8_t *>(d_flow), static_cast<uint8_t *>(d_residual)}, n_frames, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

extern "C" int hg_field_compose_frames_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_outer, const size_t *outer_offsets,
                                              const void *d_inner, int Wi, int Hi, int n_inner, size_t inner_stride_bytes, void *d_out,
                                              const size_t *out_offsets)
{
    return remap_flat_frames(c, "hg_field_compose_frames_device", geoms, n_frames, d_outer, outer_offsets, d_inner, Wi, Hi, n_inner, inner_stride_bytes,
                             HG_ELEM_F32, 2, d_out, out_offsets, nullptr, true);
}
