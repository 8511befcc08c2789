// hg_api_field.hip -- the C ABI, part 6: the source field of the inverse warps (HG_FIELD_INDEX / HG_FIELD_COORDS) and the two single-plane
// remaps through a field (hg_remap_index_device, hg_remap_bilinear_f32_device).  The remaps of whole frame sets are in hg_api_remap.hip, the
// mosaics in hg_api_mosaic.hip.
// A field call computes where the inverse loops would read, never what: it needs the source's SIZE only, is independent of the sampling
// mode, and leaves the warp paths' taps (hg_last_*_kernel) and the piecewise layout state as it found them.
#include "hg_ctx.h"

extern "C" int hg_pack_field_offsets(const hg_geom *g, int n, int fmt, size_t *offsets, size_t *total)
{
    if (!g || n < 0 || !field_fmt_ok(fmt) || !offsets || !total) return fail(nullptr, HG_ERR_INVALID, "hg_pack_field_offsets: bad arguments");
    pack_offsets(g, n, field_px_bytes(fmt), offsets, total);
    return HG_OK;
}

// What every field call checks first: the format, and that the source has a size -- below 2^31 pixels for the index format.
static int check_field_source(hg_ctx *c, int fmt)
{
    HG_TRY(check_field_fmt(c, fmt));
    if (!c->d_img || c->W <= 0 || c->H <= 0) return fail(c, HG_ERR_STATE, "no source image: a field needs its size (hg_set_image)");
    return check_field_fmt(c, fmt, c->W, c->H);
}

// The frame records of `frames` with the FIELD offsets in out_off (offs, or packed as hg_pack_field_offsets does), on the host in *t and on
// the device in c->d_field_frames (upload_frame_table).
static int stage_field_frames(hg_ctx *c, const std::vector<FrameDesc> &frames, int fmt, const size_t *offs, FieldTable<FrameDesc> *t)
{
    HG_TRY(field_table(c, frames.data(), frames.size(), fmt, offs, t));
    HG_TRY(ensure(c, c->d_field_frames, frames.size()));
    return upload_frame_table(c, c->d_field_frames, t->recs.data(), sizeof(FrameDesc) * frames.size());
}

// ------------------------------------------------------------------------------------------------ affine / projective
// settle_pending_on the extent of a field.
static int settle_field_conflicts(hg_ctx *c, const void *d_field, const std::vector<FrameDesc> &recs, int fmt)
{
    size_t extent = 0;
    for (const FrameDesc &d : recs)
        if (frame_px(d.obj_w, d.obj_h)) extent = std::max(extent, (size_t)d.out_off + frame_px(d.obj_w, d.obj_h) * field_px_bytes(fmt));
    return settle_pending_on(c, d_field, extent);
}

extern "C" int hg_field_inverse_geometric_device(hg_ctx *c, int kind, const double *m, hg_geom geom, int fmt, void *d_field)
{
    HG_TRY(bind(c));
    if ((kind != HG_AFFINE && kind != HG_PROJECTIVE) || !m || !d_field) return fail(c, HG_ERR_INVALID, "hg_field_inverse_geometric: bad arguments");
    HG_TRY(check_field_source(c, fmt));
    std::vector<FrameDesc> one;
    const size_t zero = 0;
    HG_TRY(fill_frames(c, one, &geom, &zero, 1));            // (the window limits of every frame)
    if (geom.obj_w <= 0 || geom.obj_h <= 0) return HG_OK;
    HG_TRY(settle_field_conflicts(c, d_field, one, fmt));
    GeoFieldOne g;
    g.fd = one[0];
    for (int k = 0; k < 8; k++) g.m[k] = k < (kind == HG_AFFINE ? 6 : 8) ? m[k] : 0.0;
    HG_TRY(time_begin(c));
    launch_geo_field(kind, fmt, nullptr, nullptr, g, 1, geom.obj_h, c->W, c->H, static_cast<uint8_t *>(d_field), c->stream);
    HG_TRY(time_end(c));
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

extern "C" int hg_field_inverse_geometric(hg_ctx *c, int kind, const double *m, hg_geom geom, int fmt, void *out_host)
{
    HG_TRY(bind(c));
    if (!out_host) return fail(c, HG_ERR_INVALID, "out is NULL");
    HG_TRY(check_field_fmt(c, fmt));
    const size_t bytes = frame_px(geom.obj_w, geom.obj_h) * field_px_bytes(fmt);
    HG_TRY(ensure(c, c->d_field_tmp, std::max(bytes, (size_t)8)));
    HG_TRY(hg_field_inverse_geometric_device(c, kind, m, geom, fmt, c->d_field_tmp));
    if (bytes == 0) return HG_OK;
    HIP_TRY(c, hipMemcpyAsync(out_host, c->d_field_tmp, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

extern "C" int hg_field_inverse_geometric_frames_device(hg_ctx *c, int fmt, const size_t *offs, void *d_field)
{
    HG_TRY(bind(c));
    if (!d_field) return fail(c, HG_ERR_INVALID, "d_field is NULL");
    HG_TRY(check_field_source(c, fmt));
    if (c->geo_frames.empty()) return fail(c, HG_ERR_STATE, "no frames: call hg_geometric_set_frames first");
    FieldTable<FrameDesc> t;
    HG_TRY(stage_field_frames(c, c->geo_frames, fmt, offs, &t));
    HG_TRY(settle_pending_on(c, d_field, t.extent));
    // frames given as point sets: the matrices are solved on the device, as at the head of every warp of the set (:994)
    if (c->geo_from_points)
        launch_solve_frames(c->geo_kind, c->d_geo_pts, c->d_geo_pts + c->geo_frames.size() * 8, c->d_geo_frames, c->d_mats, c->d_geo_plain,
                            (int)c->geo_frames.size(), c->stream);
    HG_TRY(time_begin(c));
    launch_geo_field(c->geo_kind, fmt, c->d_field_frames, c->d_mats, GeoFieldOne{}, (int)t.recs.size(), t.max_h, c->W, c->H, static_cast<uint8_t *>(d_field), c->stream);
    HG_TRY(time_end(c));
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ piecewise affine
// General path, settled inside the call (like a bilinear piecewise warp): queued warp runs are settled first and keep their own results;
// k_tri_setup + k_pw_field over the whole set; frames the kernel flagged (a row beyond kRowSpanCap spans, irregular triangles) are redone
// through the materialised map before the call returns and counted in hg_redone_frames.  The plan of the last warp (c->pw_plan), what the
// policy learned (c->pw_learned), the status ring and the kernel taps are not touched: the next warp of the set lays itself out as before.
extern "C" int hg_field_inverse_piecewise_frames_device(hg_ctx *c, int fmt, const size_t *offs, void *d_field)
{
    HG_TRY(bind(c));
    if (!d_field) return fail(c, HG_ERR_INVALID, "d_field is NULL");
    HG_TRY(check_field_fmt(c, fmt));
    HG_TRY(check_pw_state(c));
    HG_TRY(check_field_source(c, fmt));
    HG_TRY(hg_sync(c));                                      // queued warp runs: settled against their own status sets and staged frame sets
    const size_t F = c->pw_frames.size();
    FieldTable<FrameDesc> t;
    HG_TRY(stage_field_frames(c, c->pw_frames, fmt, offs, &t));
    PwMesh mesh = mesh_of(c);
    PwFrames fr = frames_of(c);
    fr.frames = c->d_field_frames;                           // the same windows, field offsets
    fr.status = c->solve.status; fr.host_flag = nullptr;         // a status set of this call's own, read right below
    fr.two_round = nullptr;                                  // (outside the frame set's step numbering, like the deferred redo)
    fr.self_spans = 0; fr.band_ent = nullptr; fr.band_cnt = nullptr; fr.n_bands = 0;     // k_tri_setup without candidate bands
    uint8_t *field = static_cast<uint8_t *>(d_field);
    HIP_TRY(c, hipMemsetAsync(c->solve.status, 0, sizeof(int32_t) * F, c->stream));
    launch_tri_setup(mesh, fr, c->stream);
    HG_TRY(time_begin(c));
    launch_pw_field(mesh, fr, fmt, field, c->stream);
    HG_TRY(time_end(c));
    HIP_TRY(c, hipGetLastError());
    std::vector<int32_t> status(F);
    HIP_TRY(c, hipMemcpyAsync(status.data(), c->solve.status, sizeof(int32_t) * F, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    bool redone = false;
    for (size_t f = 0; f < F; f++) {
        if (status[f] == FRAME_OK) continue;
        const FrameDesc &fd = t.recs[f];
        if (fd.obj_w <= 0 || fd.obj_h <= 0) continue;
        HG_TRY(ensure(c, c->d_map32, (size_t)fd.obj_w * fd.obj_h));
        launch_map_build(mesh, fr, (int)f, fd, c->d_map32, c->stream);      // (k_tri_setup's edge equations and row ranges of frame f)
        launch_field_from_map(mesh, fr, (int)f, fd, c->d_map32, fmt, field, c->stream);
        HIP_TRY(c, hipGetLastError());
        c->pw_redone++; c->pw_last_flag = status[f];
        redone = true;
    }
    if (redone) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

extern "C" int hg_field_inverse_piecewise(hg_ctx *c, int fmt, void *out_host)
{
    HG_TRY(bind(c));
    if (!out_host) return fail(c, HG_ERR_INVALID, "out is NULL");
    HG_TRY(check_field_fmt(c, fmt));
    HG_TRY(check_pw_state(c));
    if (c->pw_frames.size() != 1) return fail(c, HG_ERR_STATE, "this call needs exactly one prepared frame (hg_piecewise_prepare)");
    const FrameDesc &fd = c->pw_frames[0];
    const size_t bytes = frame_px(fd.obj_w, fd.obj_h) * field_px_bytes(fmt);
    HG_TRY(ensure(c, c->d_field_tmp, std::max(bytes, (size_t)8)));
    const size_t zero = 0;
    HG_TRY(hg_field_inverse_piecewise_frames_device(c, fmt, &zero, c->d_field_tmp));
    if (bytes == 0) return HG_OK;
    HIP_TRY(c, hipMemcpy(out_host, c->d_field_tmp, bytes, hipMemcpyDeviceToHost));
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ remaps
extern "C" int hg_remap_index_device(hg_ctx *c, const void *d_field, size_t n_px, const void *d_src, size_t n_src_px, int pixel_bytes, void *d_out)
{
    HG_TRY(bind(c));
    if (pixel_bytes != 1 && pixel_bytes != 2 && pixel_bytes != 4 && pixel_bytes != 8 && pixel_bytes != 16)
        return fail(c, HG_ERR_INVALID, "hg_remap_index_device: pixel_bytes must be 1, 2, 4, 8 or 16");
    if (n_px == 0) return HG_OK;
    if (!d_field || !d_out || (!d_src && n_src_px > 0)) return fail(c, HG_ERR_INVALID, "hg_remap_index_device: NULL pointer");
    if (misaligned(d_field, 4) || misaligned(d_src, (size_t)pixel_bytes) || misaligned(d_out, (size_t)pixel_bytes))
        return fail(c, HG_ERR_INVALID, "hg_remap_index_device: d_src / d_out must be aligned to pixel_bytes, d_field to 4 bytes");
    launch_remap_index(static_cast<const int32_t *>(d_field), n_px, d_src, n_src_px, pixel_bytes, d_out, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

extern "C" int hg_remap_bilinear_f32_device(hg_ctx *c, const void *d_coords, size_t n_px, const float *d_src, int W, int H, int channels, float *d_out)
{
    HG_TRY(bind(c));
    if (channels < 1 || channels > 4 || W < 1 || H < 1) return fail(c, HG_ERR_INVALID, "hg_remap_bilinear_f32_device: channels must be 1..4, W and H >= 1");
    if (n_px == 0) return HG_OK;
    if (!d_coords || !d_src || !d_out) return fail(c, HG_ERR_INVALID, "hg_remap_bilinear_f32_device: NULL pointer");
    if (misaligned(d_coords, 8) || misaligned(d_src, 4) || misaligned(d_out, 4))
        return fail(c, HG_ERR_INVALID, "hg_remap_bilinear_f32_device: d_coords must be aligned to 8 bytes, d_src / d_out to 4");
    launch_remap_bilinear_f32(static_cast<const float *>(d_coords), n_px, d_src, W, H, channels, d_out, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}
