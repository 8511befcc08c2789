// hg_api_tps.hip -- the C ABI, part 10: thin-plate splines (hg_tps_layout, hg_tps_solve_frames_device, hg_tps_field_layout,
// hg_field_tps_frames_device, hg_points_tps_frames_device).  Geometry of its own, like a fit: no image, mesh or frame set is needed, and the
// warp paths' taps (hg_last_*_kernel), the sampling mode, the plan of the last warp, what the policy learned and every staged frame set stay
// as they were.  Scratch comes from the caller (hg_tps_layout, hg_tps_field_layout), as multiband's does.
#include "hg_ctx.h"
#include "hg_tps_dev.h"

#include <cmath>

constexpr int kTpsMaxFrames = 4096;

static bool tps_step_ok(int step) { return step == 1 || step == 2 || step == 4 || step == 8 || step == 16 || step == 32; }

static int check_tps_shape(hg_ctx *c, int n_points, int n_frames)
{
    if (n_points < 3 || n_points > kTpsMaxPoints) return fail(c, HG_ERR_INVALID, "tps: n_points must be 3..1024");
    if (n_frames < 0 || n_frames > kTpsMaxFrames) return fail(c, HG_ERR_INVALID, "tps: n_frames must be 0..4096");
    return HG_OK;
}

extern "C" int hg_tps_layout(int n_points, int n_frames, size_t *record_bytes_per_frame, size_t *solve_scratch_bytes)
{
    HG_TRY(check_tps_shape(nullptr, n_points, n_frames));
    const size_t M = (size_t)n_points + 3;
    if (record_bytes_per_frame) *record_bytes_per_frame = (size_t)tps_record_doubles(n_points) * 8;
    if (solve_scratch_bytes) *solve_scratch_bytes = tps_in_lds(n_points) ? 0 : (size_t)n_frames * M * M * 8;
    return HG_OK;
}

extern "C" int hg_tps_solve_frames_device(hg_ctx *c, const void *d_from, int n_from_sets, const void *d_to, int n_to_sets, int n_points,
                                          int n_frames, double lambda, double *d_records, int32_t *d_status, void *d_scratch)
{
    HG_TRY(check_tps_shape(c, n_points, n_frames));
    if (n_from_sets < 1 || n_to_sets < 1) return fail(c, HG_ERR_INVALID, "hg_tps_solve_frames_device: n_from_sets / n_to_sets must be >= 1");
    if (!(lambda >= 0.0) || !(lambda < INFINITY)) return fail(c, HG_ERR_INVALID, "hg_tps_solve_frames_device: lambda must be finite and >= 0");
    if (n_frames == 0) return HG_OK;
    const bool scratch = !tps_in_lds(n_points);
    if (!d_from || !d_to || !d_records || !d_status || (scratch && !d_scratch))
        return fail(c, HG_ERR_INVALID, "hg_tps_solve_frames_device: d_from / d_to / d_records / d_status / d_scratch is NULL");
    if (misaligned(d_from, 8) || misaligned(d_to, 8) || misaligned(d_records, 8) || misaligned(d_scratch, 8))
        return fail(c, HG_ERR_INVALID, "hg_tps_solve_frames_device: d_from / d_to / d_records / d_scratch must be aligned to 8 bytes");
    if (misaligned(d_status, 4)) return fail(c, HG_ERR_INVALID, "hg_tps_solve_frames_device: d_status must be aligned to 4 bytes");
    HG_TRY(bind(c));
    HG_TRY(hg_sync(c));                                      // queued runs: settled first, as the fit does
    TpsSolveArgs a{static_cast<const float *>(d_from), n_from_sets, static_cast<const float *>(d_to), n_to_sets, n_points, n_frames, lambda,
                   d_records, d_status, static_cast<double *>(d_scratch)};
    launch_tps_solve(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// The node lattices of the frames, packed at the 256-byte grain: *offs (n entries, may be NULL) and the total.
static int tps_node_layout(const hg_geom *geoms, int n_frames, int step, std::vector<size_t> *offs, size_t *total)
{
    size_t off = 0;
    if (offs) offs->assign((size_t)n_frames, 0);
    for (int f = 0; f < n_frames; f++) {
        if (offs) (*offs)[(size_t)f] = off;
        if (step > 1 && geoms[f].obj_w > 0 && geoms[f].obj_h > 0)
            off += pad256((size_t)tps_nodes(geoms[f].obj_w, step) * (size_t)tps_nodes(geoms[f].obj_h, step) * 16);
    }
    *total = off;
    return HG_OK;
}

static int check_tps_field_shape(hg_ctx *c, const hg_geom *geoms, int n_frames, int step)
{
    if (n_frames < 0 || n_frames > kTpsMaxFrames) return fail(c, HG_ERR_INVALID, "tps: n_frames must be 0..4096");
    if (!tps_step_ok(step)) return fail(c, HG_ERR_INVALID, "tps: step must be 1, 2, 4, 8, 16 or 32");
    if (n_frames > 0 && !geoms) return fail(c, HG_ERR_INVALID, "tps: geoms is NULL");
    return HG_OK;
}

extern "C" int hg_tps_field_layout(const hg_geom *geoms, int n_frames, int step, size_t *scratch_bytes)
{
    HG_TRY(check_tps_field_shape(nullptr, geoms, n_frames, step));
    if (!scratch_bytes) return fail(nullptr, HG_ERR_INVALID, "hg_tps_field_layout: scratch_bytes is NULL");
    return tps_node_layout(geoms, n_frames, step, nullptr, scratch_bytes);
}

extern "C" int hg_field_tps_frames_device(hg_ctx *c, const double *d_records, int n_points, const hg_geom *geoms, int n_frames, int W, int H,
                                          int fmt, int step, const size_t *field_offsets, void *d_field, void *d_scratch)
{
    HG_TRY(check_tps_shape(c, n_points, n_frames));
    HG_TRY(check_tps_field_shape(c, geoms, n_frames, step));
    HG_TRY(check_field_fmt(c, fmt));
    if (W < 1 || H < 1) return fail(c, HG_ERR_INVALID, "hg_field_tps_frames_device: W and H must be >= 1");
    HG_TRY(check_field_fmt(c, fmt, W, H));
    if (n_frames == 0) return HG_OK;
    std::vector<FrameDesc> fds;
    HG_TRY(fill_frames(c, fds, geoms, nullptr, n_frames));   // (the window limits of every frame)
    std::vector<size_t> node_offs;
    size_t node_bytes = 0;
    HG_TRY(tps_node_layout(geoms, n_frames, step, &node_offs, &node_bytes));
    FieldTable<TpsFrame> t;
    HG_TRY(field_table(c, geoms, (size_t)n_frames, fmt, field_offsets, &t));
    for (int f = 0; f < n_frames; f++) t.recs[(size_t)f].node_off = node_offs[(size_t)f];
    if (t.extent == 0) return HG_OK;                         // (every frame is empty)
    if (!d_records || !d_field || (node_bytes > 0 && !d_scratch)) return fail(c, HG_ERR_INVALID, "hg_field_tps_frames_device: d_records / d_field / d_scratch is NULL");
    if (misaligned(d_records, 8) || misaligned(d_field, field_px_bytes(fmt)) || misaligned(d_scratch, 16))
        return fail(c, HG_ERR_INVALID, "hg_field_tps_frames_device: d_records must be aligned to 8 bytes, d_field to its pixel size, d_scratch to 16 bytes");
    HG_TRY(bind(c));
    HG_TRY(settle_pending_on(c, d_field, t.extent));
    static_assert(sizeof(TpsFrame) == sizeof(FrameDesc), "the field calls' frame table carries either record");
    HG_TRY(ensure(c, c->d_field_frames, (size_t)n_frames));
    HG_TRY(upload_frame_table(c, c->d_field_frames, t.recs.data(), sizeof(TpsFrame) * (size_t)n_frames));
    TpsFieldArgs a{d_records, n_points, reinterpret_cast<const TpsFrame *>(c->d_field_frames.p), n_frames, t.max_w, t.max_h, W, H, step,
                   static_cast<uint8_t *>(d_field), static_cast<uint8_t *>(d_scratch)};
    HG_TRY(time_begin(c));
    launch_tps_field(a, fmt, c->stream);
    HG_TRY(time_end(c));
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

extern "C" int hg_points_tps_frames_device(hg_ctx *c, const double *d_records, int n_points, int n_frames, const void *d_points, int n_pts,
                                           int n_sets, void *d_out)
{
    HG_TRY(check_tps_shape(c, n_points, n_frames));
    if (n_pts < 0 || n_pts > (1 << 24)) return fail(c, HG_ERR_INVALID, "hg_points_tps_frames_device: n_pts must be 0..2^24");
    if (n_sets < 1) return fail(c, HG_ERR_INVALID, "hg_points_tps_frames_device: n_sets must be >= 1");
    if (n_frames == 0 || n_pts == 0) return HG_OK;
    if (!d_records || !d_points || !d_out) return fail(c, HG_ERR_INVALID, "hg_points_tps_frames_device: d_records / d_points / d_out is NULL");
    if (misaligned(d_records, 8) || misaligned(d_points, 8) || misaligned(d_out, 8))
        return fail(c, HG_ERR_INVALID, "hg_points_tps_frames_device: d_records / d_points / d_out must be aligned to 8 bytes");
    HG_TRY(bind(c));
    HG_TRY(settle_pending_on(c, d_out, (size_t)n_frames * (size_t)n_pts * 8));
    launch_tps_points(d_records, n_points, n_frames, static_cast<const float *>(d_points), n_pts, n_sets, static_cast<float *>(d_out), c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}
