// hg_api_multiband.hip -- the C ABI, part 11: the multi-band mosaic of a frame set (hg_mosaic_multiband_layout,
// hg_mosaic_multiband_device).  Like the plain mosaic the call needs no image, mesh or staged frame set, is independent of the sampling
// mode, and leaves the warp paths' taps (hg_last_*_kernel), the plan of the last warp, what the policy learned and every staged frame set
// as it found them.  The library allocates nothing: every intermediate lives in the caller's work area, whose layout is mb_plan's.
#include "hg_ctx.h"

#include <cmath>

namespace {

int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

// What both entries derive from the windows: the mosaic's quad table, the records of the frames that take part, the canvas record, the
// block counts of the seed and reduce launches, and the work area.  The parts of the work area, each 256-byte aligned, in this order:
// the labels (one int32 per canvas pixel; used when d_labels is NULL); the flag bytes of every taking-part frame's level-0 grid, in
// frame order; per taking-part frame, for k = 1..L-1, level k of I (channels floats per pixel) and then level k of M (one float per
// pixel); levels 1..L-1 of R on the canvas grid.  An empty canvas needs nothing.
struct MbPlan {
    std::vector<MosaicFrame4> quads;
    std::vector<MbFrame> frames;
    MbCanvas cv{};
    uint32_t blocks[kMbMaxBands] = {0};
    size_t labels_off = 0, total = 0;
};

int mb_plan(hg_ctx *c, const std::string &fn, const hg_geom *geoms, int n_frames, const size_t *field_offsets, const size_t *frame_offsets, size_t es,
            size_t px, hg_geom canvas, int channels, int L, MbPlan *plan)
{
    std::vector<FrameDesc> lim;                               // (the window limits of the canvas and of every frame)
    const size_t zero = 0;
    HG_TRY(fill_frames(c, lim, &canvas, &zero, 1));
    if (n_frames > 0) HG_TRY(fill_frames(c, lim, geoms, nullptr, n_frames));
    plan->quads.assign(((size_t)n_frames + 3) / 4, MosaicFrame4{});      // (the fill of the last quad: empty frames)
    const int64_t A = (int64_t)1 << (L - 1), cw = canvas.obj_w, ch = canvas.obj_h;
    const bool empty = frame_px(cw, ch) == 0;
    MbCanvas &cv = plan->cv;
    cv = MbCanvas{};
    cv.cx = canvas.x_off; cv.cy = canvas.y_off; cv.cw = canvas.obj_w; cv.ch = canvas.obj_h; cv.L = L; cv.A = (int32_t)A;
    size_t off = 0;
    auto part = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    if (!empty) {
        cv.pw = (int32_t)(A * ceil_div(cw, A) + 2 * A); cv.ph = (int32_t)(A * ceil_div(ch, A) + 2 * A);
        plan->labels_off = part((size_t)cw * (size_t)ch * 4);
    }
    size_t foff = 0, poff = 0;
    for (int f = 0; f < n_frames; f++) {
        const hg_geom &g = geoms[f];
        MosaicFrame &r = plan->quads[(size_t)f / 4].f[f % 4];
        r = MosaicFrame{field_offsets ? field_offsets[f] : foff, frame_offsets ? frame_offsets[f] : poff, g.x_off, g.y_off, g.obj_w, g.obj_h};
        if (r.fld_off & 7) return fail(c, HG_ERR_INVALID, "field offsets must be multiples of the field's pixel size (8 bytes)");
        if (r.pix_off & (es - 1)) return fail(c, HG_ERR_INVALID, fn + ": frame offsets must be multiples of the element size");
        foff += pad256(frame_px(g.obj_w, g.obj_h) * 8);
        poff += pad256(frame_px(g.obj_w, g.obj_h) * px);
        if (empty || frame_px(g.obj_w, g.obj_h) == 0) continue;
        // window ∩ canvas in canvas-relative coordinates
        const int64_t a0 = std::max<int64_t>(g.x_off, cv.cx) - cv.cx, a1 = std::min<int64_t>((int64_t)g.x_off + g.obj_w, (int64_t)cv.cx + cw) - cv.cx;
        const int64_t b0 = std::max<int64_t>(g.y_off, cv.cy) - cv.cy, b1 = std::min<int64_t>((int64_t)g.y_off + g.obj_h, (int64_t)cv.cy + ch) - cv.cy;
        if (a0 >= a1 || b0 >= b1) continue;
        MbFrame m{};
        m.m = r;
        m.index = f;
        m.gain = 1.0f;
        m.gx = (int32_t)(A * (floor_div(a0, A) - 1)); m.gy = (int32_t)(A * (floor_div(b0, A) - 1));
        m.gw = (int32_t)(A * (ceil_div(a1, A) + 1) - m.gx); m.gh = (int32_t)(A * (ceil_div(b1, A) + 1) - m.gy);
        plan->frames.push_back(m);
    }
    uint64_t blk[kMbMaxBands] = {0};
    for (MbFrame &m : plan->frames) m.flag_off = part((size_t)m.gw * (size_t)m.gh);
    for (MbFrame &m : plan->frames) {
        m.blk0[0] = (uint32_t)blk[0];
        blk[0] += ((uint64_t)m.gw * (uint64_t)m.gh + kMbSeedPx - 1) / kMbSeedPx;
        for (int k = 1; k < L; k++) {
            const uint64_t w = (uint64_t)(m.gw >> k), h = (uint64_t)(m.gh >> k);
            m.img_off[k] = part((size_t)(w * h) * (size_t)channels * 4);
            m.msk_off[k] = part((size_t)(w * h) * 4);
            m.blk0[k] = (uint32_t)blk[k];
            blk[k] += ((w + kMbTileW - 1) / kMbTileW) * ((h + kMbTileH - 1) / kMbTileH);
        }
    }
    for (int k = 0; k < L; k++) {
        if (blk[k] > 0x7fffffffull) return fail(c, HG_ERR_INVALID, fn + ": the frame grids need more than 2^31 - 1 blocks in one launch");
        plan->blocks[k] = (uint32_t)blk[k];
    }
    if (!empty)
        for (int k = 1; k < L; k++) cv.r_off[k] = part((size_t)(cv.pw >> k) * (size_t)(cv.ph >> k) * (size_t)channels * 4);
    plan->total = off;
    return HG_OK;
}

} // namespace

extern "C" int hg_mosaic_multiband_layout(const hg_geom *geoms, int n_frames, hg_geom canvas, int channels, int n_bands, size_t *work_bytes)
{
    const std::string fn("hg_mosaic_multiband_layout");
    if (!work_bytes) return fail(nullptr, HG_ERR_INVALID, fn + ": work_bytes is NULL");
    if (n_frames < 0 || n_frames > 65535) return fail(nullptr, HG_ERR_INVALID, fn + ": n_frames must be 0..65535");
    if (channels < 1 || channels > 4) return fail(nullptr, HG_ERR_INVALID, fn + ": channels must be 1..4");
    if (n_bands < 1 || n_bands > kMbMaxBands) return fail(nullptr, HG_ERR_INVALID, fn + ": n_bands must be 1..8");
    if (n_frames > 0 && !geoms) return fail(nullptr, HG_ERR_INVALID, fn + ": NULL pointer");
    MbPlan plan;
    HG_TRY(mb_plan(nullptr, fn, geoms, n_frames, nullptr, nullptr, 1, (size_t)channels, canvas, channels, n_bands, &plan));
    *work_bytes = plan.total;
    return HG_OK;
}

extern "C" int hg_mosaic_multiband_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                          const void *d_frames, const size_t *frame_offsets, int elem, int channels, int W, int H, float feather,
                                          int n_bands, hg_geom canvas, void *d_canvas, float *d_weight, int32_t *d_labels, const float *gains,
                                          void *d_work, size_t work_bytes)
{
    HG_TRY(bind(c));
    const std::string fn("hg_mosaic_multiband_device");
    if (n_frames < 0 || n_frames > 65535) return fail(c, HG_ERR_INVALID, fn + ": n_frames must be 0..65535");
    if (!d_canvas) return fail(c, HG_ERR_INVALID, fn + ": d_canvas is NULL");
    if (elem != HG_ELEM_F32 && elem != HG_ELEM_U8) return fail(c, HG_ERR_INVALID, fn + ": unknown elem (HG_ELEM_F32 or HG_ELEM_U8)");
    if (channels < 1 || channels > 4 || W < 1 || H < 1) return fail(c, HG_ERR_INVALID, fn + ": channels must be 1..4, W and H >= 1");
    if (!(feather > 0.0f)) return fail(c, HG_ERR_INVALID, fn + ": feather must be > 0 (+Inf: uncapped)");
    if (n_bands < 1 || n_bands > kMbMaxBands) return fail(c, HG_ERR_INVALID, fn + ": n_bands must be 1..8");
    if (n_frames > 0 && (!geoms || !d_coords || !d_frames)) return fail(c, HG_ERR_INVALID, fn + ": NULL pointer");
    const size_t es = elem == HG_ELEM_F32 ? 4 : 1, px = es * (size_t)channels;
    if (misaligned(d_coords, 8) || misaligned(d_frames, es) || misaligned(d_canvas, es) || misaligned(d_weight, 4) || misaligned(d_labels, 4))
        return fail(c, HG_ERR_INVALID, fn + ": d_coords must be aligned to 8 bytes, d_frames / d_canvas to the element size, d_weight / d_labels to 4");
    if (n_frames == 0) gains = nullptr;
    for (int f = 0; gains && f < n_frames; f++)
        if (!(gains[f] > 0.0f) || !std::isfinite(gains[f])) return fail(c, HG_ERR_INVALID, fn + ": every gain must be finite and > 0");
    MbPlan plan;
    HG_TRY(mb_plan(c, fn, geoms, n_frames, field_offsets, frame_offsets, es, px, canvas, channels, n_bands, &plan));
    const size_t n_px = frame_px(canvas.obj_w, canvas.obj_h);
    if (n_px == 0) return HG_OK;
    if (!d_work || misaligned(d_work, 256) || work_bytes < plan.total)
        return fail(c, HG_ERR_INVALID, fn + ": d_work must be aligned to 256 bytes and hold what hg_mosaic_multiband_layout returns");
    if (gains)
        for (MbFrame &m : plan.frames) m.gain = gains[m.index];
    HG_TRY(settle_pending_on(c, d_canvas, n_px * px));
    if (d_weight) HG_TRY(settle_pending_on(c, d_weight, n_px * 4));
    if (d_labels) HG_TRY(settle_pending_on(c, d_labels, n_px * 4));
    HG_TRY(settle_pending_on(c, d_work, plan.total));
    // the quads and, behind them, the records of the frames that take part: ONE staged upload
    const size_t q_bytes = plan.quads.size() * sizeof(MosaicFrame4), f_bytes = plan.frames.size() * sizeof(MbFrame);
    const MosaicFrame4 *d_quads = nullptr;
    const MbFrame *d_recs = nullptr;
    if (q_bytes + f_bytes) {
        HG_TRY(ensure(c, c->d_mb_table, (q_bytes + f_bytes) / 8));
        HG_TRY(upload_frame_table(c, c->d_mb_table.p, plan.quads.data(), q_bytes, plan.frames.data(), f_bytes));
        d_quads = reinterpret_cast<const MosaicFrame4 *>(c->d_mb_table.p);
        d_recs = reinterpret_cast<const MbFrame *>(reinterpret_cast<const uint8_t *>(c->d_mb_table.p) + q_bytes);
    }
    uint8_t *work = static_cast<uint8_t *>(d_work);
    MbArgs a{d_quads, (int)plan.quads.size(), d_recs, (int)plan.frames.size(), plan.cv, {0}, static_cast<const uint8_t *>(d_coords),
             static_cast<const uint8_t *>(d_frames), W, H, elem, channels, feather, work, d_labels ? d_labels : reinterpret_cast<int32_t *>(work + plan.labels_off),
             static_cast<uint8_t *>(d_canvas), d_weight};
    for (int k = 0; k < kMbMaxBands; k++) a.blocks[k] = plan.blocks[k];
    launch_multiband(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}
