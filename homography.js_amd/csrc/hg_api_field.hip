// hg_api_field.hip -- the C ABI, part 6: the source field of the inverse warps (HG_FIELD_INDEX / HG_FIELD_COORDS), the remaps through it and
// the mosaic of a frame set (hg_mosaic_frames_device).
// A field call computes where the inverse loops would read, never what: it needs the source's SIZE only, is independent of the sampling
// mode, and leaves the warp paths' taps (hg_last_*_kernel) and the piecewise layout state as it found them.
#include "hg_ctx.h"

#include <cmath>

static bool field_fmt_ok(int fmt) { return fmt == HG_FIELD_INDEX || fmt == HG_FIELD_COORDS; }
static size_t field_px_bytes(int fmt) { return fmt == HG_FIELD_INDEX ? 4 : 8; }

extern "C" int hg_pack_field_offsets(const hg_geom *g, int n, int fmt, size_t *offsets, size_t *total)
{
    if (!g || n < 0 || !field_fmt_ok(fmt) || !offsets || !total) return fail(nullptr, HG_ERR_INVALID, "hg_pack_field_offsets: bad arguments");
    pack_offsets(g, n, field_px_bytes(fmt), offsets, total);
    return HG_OK;
}

// What every field call checks first: the format, and that the source has a size -- below 2^31 pixels for the index format.
static int check_field_source(hg_ctx *c, int fmt)
{
    if (!field_fmt_ok(fmt)) return fail(c, HG_ERR_INVALID, "unknown field format (HG_FIELD_INDEX or HG_FIELD_COORDS)");
    if (!c->d_img || c->W <= 0 || c->H <= 0) return fail(c, HG_ERR_STATE, "no source image: a field needs its size (hg_set_image)");
    if (fmt == HG_FIELD_INDEX && (int64_t)c->W * c->H >= ((int64_t)1 << 31))
        return fail(c, HG_ERR_INVALID, "HG_FIELD_INDEX: the source has 2^31 pixels or more (an int32 cannot index it)");
    return HG_OK;
}

// A frame table (a multiple of 8 bytes) to the device: copied into page-locked staging and uploaded stream-ordered, like the frame sets
// themselves (no GPU wait unless the upload that used the staging slot four calls ago is still queued).
static int upload_frame_table(hg_ctx *c, void *d_dst, const void *src, size_t bytes)
{
    StageSlot *gs = nullptr;
    HG_TRY(c->field_stage.acquire(c, bytes, "field frame staging", &gs));
    std::memcpy(gs->h, src, bytes);
    HG_TRY(upload_staged(c, d_dst, gs->h, bytes));
    return c->field_stage.commit(c, gs);
}

// The frame records of `frames` with the FIELD offsets in out_off (offs, or packed as hg_pack_field_offsets does), on the host in *recs and on
// the device in c->d_field_frames (upload_frame_table).
static int stage_field_frames(hg_ctx *c, const std::vector<FrameDesc> &frames, int fmt, const size_t *offs, std::vector<FrameDesc> *recs)
{
    const size_t F = frames.size(), px = field_px_bytes(fmt);
    *recs = frames;
    size_t off = 0;
    for (size_t f = 0; f < F; f++) {
        FrameDesc &d = (*recs)[f];
        d.out_off = offs ? offs[f] : off;
        if (d.out_off & (px - 1)) return fail(c, HG_ERR_INVALID, "field offsets must be multiples of the field's pixel size (4 or 8 bytes)");
        off += pad256(frame_px(d.obj_w, d.obj_h) * px);
    }
    HG_TRY(ensure(c, c->d_field_frames, F));
    return upload_frame_table(c, c->d_field_frames, recs->data(), sizeof(FrameDesc) * F);
}

// A queued run's deferred redo must not land later on what this call writes: queued runs whose output overlaps [ptr, ptr + bytes) are
// settled first.
static int settle_pending_on(hg_ctx *c, const void *ptr, size_t bytes)
{
    if (c->pw_pending_out.empty() && c->fwd_pending.empty()) return HG_OK;
    return settle_output_conflicts(c, ptr, bytes, 0);
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
    if (!field_fmt_ok(fmt)) return fail(c, HG_ERR_INVALID, "unknown field format (HG_FIELD_INDEX or HG_FIELD_COORDS)");
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
    std::vector<FrameDesc> recs;
    HG_TRY(stage_field_frames(c, c->geo_frames, fmt, offs, &recs));
    HG_TRY(settle_field_conflicts(c, d_field, recs, fmt));
    int mh = 0;
    for (const FrameDesc &d : recs) if (d.obj_w > 0) mh = std::max(mh, d.obj_h);
    // frames given as point sets: the matrices are solved on the device, as at the head of every warp of the set (:994)
    if (c->geo_from_points)
        launch_solve_frames(c->geo_kind, c->d_geo_pts, c->d_geo_pts + c->geo_frames.size() * 8, c->d_geo_frames, c->d_mats, c->d_geo_plain,
                            (int)c->geo_frames.size(), c->stream);
    HG_TRY(time_begin(c));
    launch_geo_field(c->geo_kind, fmt, c->d_field_frames, c->d_mats, GeoFieldOne{}, (int)recs.size(), mh, c->W, c->H, static_cast<uint8_t *>(d_field), c->stream);
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
    if (!field_fmt_ok(fmt)) return fail(c, HG_ERR_INVALID, "unknown field format (HG_FIELD_INDEX or HG_FIELD_COORDS)");
    HG_TRY(check_pw_state(c));
    HG_TRY(check_field_source(c, fmt));
    HG_TRY(hg_sync(c));                                      // queued warp runs: settled against their own status sets and staged frame sets
    const size_t F = c->pw_frames.size();
    std::vector<FrameDesc> recs;
    HG_TRY(stage_field_frames(c, c->pw_frames, fmt, offs, &recs));
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
        const FrameDesc &fd = recs[f];
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
    if (!field_fmt_ok(fmt)) return fail(c, HG_ERR_INVALID, "unknown field format (HG_FIELD_INDEX or HG_FIELD_COORDS)");
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
    const uintptr_t mask = (uintptr_t)pixel_bytes - 1;
    if ((reinterpret_cast<uintptr_t>(d_field) & 3) || (reinterpret_cast<uintptr_t>(d_src) & mask) || (reinterpret_cast<uintptr_t>(d_out) & mask))
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
    if ((reinterpret_cast<uintptr_t>(d_coords) & 7) || (reinterpret_cast<uintptr_t>(d_src) & 3) || (reinterpret_cast<uintptr_t>(d_out) & 3))
        return fail(c, HG_ERR_INVALID, "hg_remap_bilinear_f32_device: d_coords must be aligned to 8 bytes, d_src / d_out to 4");
    launch_remap_bilinear_f32(static_cast<const float *>(d_coords), n_px, d_src, W, H, channels, d_out, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ remaps of whole frame sets
extern "C" int hg_pack_plane_offsets(const hg_geom *g, int n, size_t px_bytes, size_t *offsets, size_t *total)
{
    if (!g || n < 0 || px_bytes < 1 || !offsets || !total) return fail(nullptr, HG_ERR_INVALID, "hg_pack_plane_offsets: bad arguments");
    pack_offsets(g, n, px_bytes, offsets, total);
    return HG_OK;
}

static bool misaligned(const void *p, size_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }      // (align: a power of two)

// The frame table of a frames remap: flat lists of obj_w * obj_h pixels, fields of fld_px bytes per pixel at foffs (NULL: packed as
// hg_pack_field_offsets does), outputs of out_px bytes per pixel at ooffs (NULL: packed as hg_pack_plane_offsets does; else multiples of
// out_align, a power of two), frame f on plane f % n_planes.  *extent: the bytes the call writes from d_out on.
static int remap_frame_table(hg_ctx *c, const hg_geom *geoms, int n, size_t fld_px, const size_t *foffs, size_t out_px, size_t out_align,
                             const size_t *ooffs, int n_planes, std::vector<RemapFrame> *recs, size_t *extent)
{
    recs->resize((size_t)n);
    size_t foff = 0, ooff = 0;
    *extent = 0;
    for (int f = 0; f < n; f++) {
        RemapFrame &r = (*recs)[(size_t)f];
        r.n_px = frame_px(geoms[f].obj_w, geoms[f].obj_h);
        r.fld_off = foffs ? foffs[f] : foff;
        r.out_off = ooffs ? ooffs[f] : ooff;
        r.blk0 = 0; r.plane = (uint32_t)(f % n_planes);
        if (r.fld_off & (fld_px - 1)) return fail(c, HG_ERR_INVALID, "field offsets must be multiples of the field's pixel size (4 or 8 bytes)");
        if (r.out_off & (out_align - 1)) return fail(c, HG_ERR_INVALID, "output offsets must be multiples of pixel_bytes (index) or of the element size (bilinear)");
        foff += pad256((size_t)r.n_px * fld_px);
        ooff += pad256((size_t)r.n_px * out_px);
        if (r.n_px) *extent = std::max(*extent, (size_t)r.out_off + (size_t)r.n_px * out_px);
    }
    return HG_OK;
}

// Blocks of blk_px pixels over the frames, in frame order: blk0 of every record, the grid size.  blk_px starts at base_px (a multiple of 1024)
// and doubles until the grid fits 2^30 blocks (only sets far beyond any memory get there).
static void assign_remap_blocks(std::vector<RemapFrame> &recs, uint64_t base_px, uint64_t *blk_px, uint32_t *n_blocks)
{
    for (uint64_t px = base_px;; px *= 2) {
        uint64_t b = 0;
        for (RemapFrame &r : recs) {
            r.blk0 = (uint32_t)b;
            b += (r.n_px + px - 1) / px;
            if (b > ((uint64_t)1 << 30)) break;
        }
        if (b <= ((uint64_t)1 << 30)) { *blk_px = px; *n_blocks = (uint32_t)b; return; }
    }
}

// Settle what could still land on the output, then put the table on the device.
static int stage_remap_frames(hg_ctx *c, const std::vector<RemapFrame> &recs, const void *d_out, size_t extent)
{
    HG_TRY(settle_pending_on(c, d_out, extent));
    HG_TRY(ensure(c, c->d_remap_frames, recs.size()));
    return upload_frame_table(c, c->d_remap_frames, recs.data(), sizeof(RemapFrame) * recs.size());
}

extern "C" int hg_remap_index_frames_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_field, const size_t *field_offsets,
                                            const void *d_planes, size_t n_src_px, int n_planes, size_t plane_stride_bytes, int pixel_bytes,
                                            void *d_out, const size_t *out_offsets)
{
    HG_TRY(bind(c));
    if (pixel_bytes != 1 && pixel_bytes != 2 && pixel_bytes != 4 && pixel_bytes != 8 && pixel_bytes != 16)
        return fail(c, HG_ERR_INVALID, "hg_remap_index_frames_device: pixel_bytes must be 1, 2, 4, 8 or 16");
    if (n_planes < 1) return fail(c, HG_ERR_INVALID, "hg_remap_index_frames_device: n_planes must be >= 1");
    if (n_frames < 0 || n_frames > 65535) return fail(c, HG_ERR_INVALID, "hg_remap_index_frames_device: n_frames must be 0..65535");
    if (n_frames == 0) return HG_OK;
    if (!geoms || !d_field || !d_out || (!d_planes && n_src_px > 0)) return fail(c, HG_ERR_INVALID, "hg_remap_index_frames_device: NULL pointer");
    const size_t px = (size_t)pixel_bytes;
    if (misaligned(d_field, 4) || misaligned(d_planes, px) || misaligned(d_out, px) || (plane_stride_bytes & (px - 1)))
        return fail(c, HG_ERR_INVALID, "hg_remap_index_frames_device: d_planes / d_out / plane_stride_bytes must be aligned to pixel_bytes, d_field to 4 bytes");
    std::vector<RemapFrame> recs;
    size_t extent = 0;
    HG_TRY(remap_frame_table(c, geoms, n_frames, 4, field_offsets, px, px, out_offsets, n_planes, &recs, &extent));
    if (extent == 0) return HG_OK;                           // (every frame is empty)
    const bool packed = remap_index_packs(pixel_bytes) && c->opt_remap_pack != 0;      // (option "remap_pack" 0: one pixel per lane, for measurements)
    uint64_t blk_px = 0; uint32_t n_blocks = 0;
    assign_remap_blocks(recs, packed ? 4096 : 1024, &blk_px, &n_blocks);
    HG_TRY(stage_remap_frames(c, recs, d_out, extent));
    launch_remap_index_frames(c->d_remap_frames, n_frames, n_blocks, blk_px, packed, static_cast<const uint8_t *>(d_field),
                              static_cast<const uint8_t *>(d_planes), n_src_px, plane_stride_bytes, pixel_bytes, static_cast<uint8_t *>(d_out), c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ mip pyramids and the trilinear remap
extern "C" int hg_pyramid_levels(int W, int H)
{
    if (W < 1 || H < 1) return 0;
    int n = 1;
    for (; W > 1 || H > 1; n++) { W = (W + 1) >> 1; H = (H + 1) >> 1; }
    return n;
}

static bool plane_fmt_ok(int elem, int channels) { return (elem == HG_ELEM_F32 || elem == HG_ELEM_U8) && channels >= 1 && channels <= 4; }

// offs[k], k = 1 .. levels - 1, and the bytes of one pyramid (levels already checked against hg_pyramid_levels).
static size_t pyramid_offsets(int W, int H, size_t px_bytes, int levels, size_t *offs)
{
    size_t off = 0;
    offs[0] = 0;
    for (int k = 1; k < levels; k++) {
        W = (W + 1) >> 1; H = (H + 1) >> 1;
        offs[k] = off;
        off += pad256((size_t)W * (size_t)H * px_bytes);
    }
    return off;
}

extern "C" int hg_pyramid_layout(int W, int H, int elem, int channels, int levels, size_t *offsets, size_t *total)
{
    if (!plane_fmt_ok(elem, channels) || levels < 1 || levels > hg_pyramid_levels(W, H) || !offsets || !total)
        return fail(nullptr, HG_ERR_INVALID, "hg_pyramid_layout: bad arguments");
    *total = pyramid_offsets(W, H, (elem == HG_ELEM_F32 ? 4 : 1) * (size_t)channels, levels, offsets);
    return HG_OK;
}

// What the pyramid calls check of the pyramids of a plane set (written: the call writes them, so every pyramid needs its room);
// *total: the bytes of one pyramid, offs: its level offsets (room for 32).
static int check_pyramid(hg_ctx *c, const char *who, int W, int H, int elem, int channels, int levels, const void *d_pyr, size_t pyr_stride_bytes,
                         bool written, size_t *offs, size_t *total)
{
    if (levels < 1 || levels > hg_pyramid_levels(W, H)) return fail(c, HG_ERR_INVALID, std::string(who) + ": levels must lie in 1..hg_pyramid_levels(W, H)");
    const size_t es = elem == HG_ELEM_F32 ? 4 : 1;
    *total = pyramid_offsets(W, H, es * (size_t)channels, levels, offs);
    if (levels == 1) return HG_OK;                           // (no pyramid is read or written)
    if (!d_pyr) return fail(c, HG_ERR_INVALID, std::string(who) + ": d_pyr is NULL with levels > 1");
    if (misaligned(d_pyr, es) || (pyr_stride_bytes & (es - 1))) return fail(c, HG_ERR_INVALID, std::string(who) + ": d_pyr / pyr_stride_bytes must be aligned to the element size");
    if (written && pyr_stride_bytes < *total) return fail(c, HG_ERR_INVALID, std::string(who) + ": pyr_stride_bytes is smaller than one pyramid (hg_pyramid_layout's total)");
    return HG_OK;
}

extern "C" int hg_pyramid_build_device(hg_ctx *c, const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                                       int levels, void *d_pyr, size_t pyr_stride_bytes)
{
    HG_TRY(bind(c));
    if (!plane_fmt_ok(elem, channels) || W < 1 || H < 1) return fail(c, HG_ERR_INVALID, "hg_pyramid_build_device: elem must be HG_ELEM_F32 or HG_ELEM_U8, channels 1..4, W and H >= 1");
    if (n_planes < 1) return fail(c, HG_ERR_INVALID, "hg_pyramid_build_device: n_planes must be >= 1");
    size_t offs[32], total = 0;
    HG_TRY(check_pyramid(c, "hg_pyramid_build_device", W, H, elem, channels, levels, d_pyr, pyr_stride_bytes, true, offs, &total));
    if (levels == 1) return HG_OK;
    const size_t es = elem == HG_ELEM_F32 ? 4 : 1;
    if (!d_planes) return fail(c, HG_ERR_INVALID, "hg_pyramid_build_device: d_planes is NULL");
    if (misaligned(d_planes, es) || (plane_stride_bytes & (es - 1))) return fail(c, HG_ERR_INVALID, "hg_pyramid_build_device: d_planes / plane_stride_bytes must be aligned to the element size");
    const uint8_t *src = static_cast<const uint8_t *>(d_planes);
    uint8_t *pyr = static_cast<uint8_t *>(d_pyr);
    size_t src_stride = plane_stride_bytes;
    int ws = W, hs = H;
    for (int k = 1; k < levels; k++) {                       // one launch per level, each reading the level before it
        const int wd = (ws + 1) >> 1, hd = (hs + 1) >> 1;
        launch_pyr_down(src, src_stride, ws, hs, pyr + offs[k], pyr_stride_bytes, wd, hd, n_planes, elem, channels, c->stream);
        src = pyr + offs[k]; src_stride = pyr_stride_bytes; ws = wd; hs = hd;
    }
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ bilinear, bicubic, trilinear and anisotropic remaps of whole frame sets
// What the bilinear, bicubic, trilinear and anisotropic frames remaps (who: the entry point's name) check of their arguments; lvl (room for 32): the
// level offsets of one pyramid.  levels == 1: no pyramid, d_pyr is not looked at.  The pointers only matter with frames to remap.
static int check_remap_frames(hg_ctx *c, const std::string &who, const hg_geom *geoms, int n_frames, const void *d_coords, const void *d_planes, int W, int H,
                              int n_planes, size_t plane_stride_bytes, int elem, int channels, const void *d_out, const void *d_pyr, size_t pyr_stride_bytes,
                              int levels, size_t *lvl)
{
    if (elem != HG_ELEM_F32 && elem != HG_ELEM_U8) return fail(c, HG_ERR_INVALID, who + ": unknown elem (HG_ELEM_F32 or HG_ELEM_U8)");
    if (channels < 1 || channels > 4 || W < 1 || H < 1) return fail(c, HG_ERR_INVALID, who + ": channels must be 1..4, W and H >= 1");
    if (n_planes < 1) return fail(c, HG_ERR_INVALID, who + ": n_planes must be >= 1");
    if (n_frames < 0 || n_frames > 65535) return fail(c, HG_ERR_INVALID, who + ": n_frames must be 0..65535");
    size_t total = 0;
    HG_TRY(check_pyramid(c, who.c_str(), W, H, elem, channels, levels, d_pyr, pyr_stride_bytes, false, lvl, &total));
    if (n_frames == 0) return HG_OK;
    if (!geoms || !d_coords || !d_planes || !d_out) return fail(c, HG_ERR_INVALID, who + ": NULL pointer");
    const size_t es = elem == HG_ELEM_F32 ? 4 : 1;
    if (misaligned(d_coords, 8) || misaligned(d_planes, es) || misaligned(d_out, es) || (plane_stride_bytes & (es - 1)))
        return fail(c, HG_ERR_INVALID, who + ": d_coords must be aligned to 8 bytes, d_planes / d_out / plane_stride_bytes to the element size");
    return HG_OK;
}

// The bilinear and the bicubic frames remap (who: the entry point's name): one check, one table, one staging; cubic == nullptr launches the
// bilinear kernel, otherwise the bicubic one with those coefficients.  compose (hg_api_flow.hip; elem HG_ELEM_F32, channels 2, no cubic): the
// planes are inner fields and the chained-field kernel takes the bilinear one's place.
int remap_flat_frames(hg_ctx *c, const char *who, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                      const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                      void *d_out, const size_t *out_offsets, const CubicCoef *cubic, bool compose)
{
    HG_TRY(bind(c));
    size_t lvl[32];
    HG_TRY(check_remap_frames(c, who, geoms, n_frames, d_coords, d_planes, W, H, n_planes, plane_stride_bytes, elem, channels, d_out, nullptr, 0, 1, lvl));
    if (n_frames == 0) return HG_OK;
    const size_t es = elem == HG_ELEM_F32 ? 4 : 1;
    std::vector<RemapFrame> recs;
    size_t extent = 0;
    if (compose && misaligned(d_out, 8)) return fail(c, HG_ERR_INVALID, std::string(who) + ": d_out must be aligned to 8 bytes");      // (a field)
    HG_TRY(remap_frame_table(c, geoms, n_frames, 8, field_offsets, es * (size_t)channels, compose ? 8 : es, out_offsets, n_planes, &recs, &extent));
    if (extent == 0) return HG_OK;
    uint64_t blk_px = 0; uint32_t n_blocks = 0;
    assign_remap_blocks(recs, 1024, &blk_px, &n_blocks);
    HG_TRY(stage_remap_frames(c, recs, d_out, extent));
    const uint8_t *co = static_cast<const uint8_t *>(d_coords), *pl = static_cast<const uint8_t *>(d_planes);
    if (compose) launch_field_compose_frames(c->d_remap_frames, n_frames, n_blocks, blk_px, co, pl, plane_stride_bytes, W, H, static_cast<uint8_t *>(d_out), c->stream);
    else if (cubic) launch_remap_bicubic_frames(c->d_remap_frames, n_frames, n_blocks, blk_px, *cubic, co, pl, plane_stride_bytes, W, H, elem, channels, static_cast<uint8_t *>(d_out), c->stream);
    else launch_remap_bilinear_frames(c->d_remap_frames, RemapFrame{}, n_frames, n_blocks, blk_px, co, pl, plane_stride_bytes, W, H, elem, channels, static_cast<uint8_t *>(d_out), c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

extern "C" int hg_remap_bilinear_frames_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                               const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                                               void *d_out, const size_t *out_offsets)
{
    return remap_flat_frames(c, "hg_remap_bilinear_frames_device", geoms, n_frames, d_coords, field_offsets, d_planes, W, H, n_planes, plane_stride_bytes,
                             elem, channels, d_out, out_offsets, nullptr, false);
}

// The coefficients of the (B, C) cubic: in double from (double)B and (double)C in the header's written order, each rounded once to f32.
static CubicCoef cubic_coefficients(float Bf, float Cf)
{
    const double B = (double)Bf, C = (double)Cf;
    CubicCoef k;
    k.p3 = (float)(((12.0 - 9.0 * B) - 6.0 * C) / 6.0);
    k.p2 = (float)(((-18.0 + 12.0 * B) + 6.0 * C) / 6.0);
    k.p0 = (float)((6.0 - 2.0 * B) / 6.0);
    k.q3 = (float)((-B - 6.0 * C) / 6.0);
    k.q2 = (float)((6.0 * B + 30.0 * C) / 6.0);
    k.q1 = (float)((-12.0 * B - 48.0 * C) / 6.0);
    k.q0 = (float)((8.0 * B + 24.0 * C) / 6.0);
    return k;
}

extern "C" int hg_remap_bicubic_frames_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                              const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                                              void *d_out, const size_t *out_offsets, float B, float C)
{
    if (!(B >= 0.0f && B <= 1.0f)) return fail(c, HG_ERR_INVALID, "hg_remap_bicubic_frames_device: B must lie in [0, 1]");      // (a NaN compares false)
    if (!(C >= 0.0f && C <= 1.0f)) return fail(c, HG_ERR_INVALID, "hg_remap_bicubic_frames_device: C must lie in [0, 1]");
    const CubicCoef k = cubic_coefficients(B, C);
    return remap_flat_frames(c, "hg_remap_bicubic_frames_device", geoms, n_frames, d_coords, field_offsets, d_planes, W, H, n_planes, plane_stride_bytes,
                             elem, channels, d_out, out_offsets, &k, false);
}

extern "C" int hg_remap_bilinear_u8_device(hg_ctx *c, const void *d_coords, size_t n_px, const uint8_t *d_src, int W, int H, int channels, uint8_t *d_out)
{
    HG_TRY(bind(c));
    if (channels < 1 || channels > 4 || W < 1 || H < 1) return fail(c, HG_ERR_INVALID, "hg_remap_bilinear_u8_device: channels must be 1..4, W and H >= 1");
    if (n_px == 0) return HG_OK;
    if (!d_coords || !d_src || !d_out) return fail(c, HG_ERR_INVALID, "hg_remap_bilinear_u8_device: NULL pointer");
    if (misaligned(d_coords, 8)) return fail(c, HG_ERR_INVALID, "hg_remap_bilinear_u8_device: d_coords must be aligned to 8 bytes");
    std::vector<RemapFrame> one(1);
    one[0] = RemapFrame{0, 0, (uint64_t)n_px, 0, 0};
    uint64_t blk_px = 0; uint32_t n_blocks = 0;
    assign_remap_blocks(one, 1024, &blk_px, &n_blocks);
    launch_remap_bilinear_frames(nullptr, one[0], 1, n_blocks, blk_px, static_cast<const uint8_t *>(d_coords), d_src, 0, W, H, HG_ELEM_U8, channels, d_out, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// The trilinear and the anisotropic frames remap (who: the entry point's name): one table, one staging; max_aniso == 0 launches the
// trilinear kernel, 1..16 the anisotropic one.
static int remap_mip_frames(hg_ctx *c, const std::string &who, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                            const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                            void *d_out, const size_t *out_offsets, const void *d_pyr, size_t pyr_stride_bytes, int levels, int max_aniso)
{
    HG_TRY(bind(c));
    size_t lvl[32] = {0};
    HG_TRY(check_remap_frames(c, who, geoms, n_frames, d_coords, d_planes, W, H, n_planes, plane_stride_bytes, elem, channels, d_out, d_pyr, pyr_stride_bytes, levels, lvl));
    if (n_frames == 0) return HG_OK;
    const size_t es = elem == HG_ELEM_F32 ? 4 : 1;
    std::vector<RemapFrame> recs;
    size_t extent = 0;
    HG_TRY(remap_frame_table(c, geoms, n_frames, 8, field_offsets, es * (size_t)channels, es, out_offsets, n_planes, &recs, &extent));
    if (extent == 0) return HG_OK;
    uint64_t blk_px = 0; uint32_t n_blocks = 0;
    assign_remap_blocks(recs, 1024, &blk_px, &n_blocks);
    HG_TRY(settle_pending_on(c, d_out, extent));
    // the device table: 32 level offsets, then one record per frame
    const size_t words = 32 + (size_t)n_frames * (sizeof(TriRemapFrame) / 8);
    HG_TRY(ensure(c, c->d_tri_table, words));
    StageSlot *gs = nullptr;
    HG_TRY(c->field_stage.acquire(c, words * 8, "field frame staging", &gs));
    uint64_t *tab = reinterpret_cast<uint64_t *>(gs->h);
    for (int k = 0; k < 32; k++) tab[k] = lvl[k];
    TriRemapFrame *tf = reinterpret_cast<TriRemapFrame *>(tab + 32);
    for (int f = 0; f < n_frames; f++) {
        const RemapFrame &r = recs[(size_t)f];
        tf[f] = TriRemapFrame{r.fld_off, r.out_off, r.n_px, (uint64_t)r.plane * plane_stride_bytes, (uint64_t)r.plane * pyr_stride_bytes, r.blk0,
                              (uint32_t)std::max(geoms[f].obj_w, 0), (uint32_t)std::max(geoms[f].obj_h, 0), 0};
    }
    HG_TRY(upload_staged(c, c->d_tri_table, gs->h, words * 8));
    HG_TRY(c->field_stage.commit(c, gs));
    const TriRemapFrame *d_frames = reinterpret_cast<const TriRemapFrame *>(c->d_tri_table.p + 32);
    const uint8_t *co = static_cast<const uint8_t *>(d_coords), *pl = static_cast<const uint8_t *>(d_planes), *py = static_cast<const uint8_t *>(d_pyr);
    if (max_aniso == 0) launch_remap_trilinear_frames(d_frames, n_frames, n_blocks, blk_px, c->d_tri_table, levels, co, pl, py, W, H, elem, channels, static_cast<uint8_t *>(d_out), c->stream);
    else launch_remap_aniso_frames(d_frames, n_frames, n_blocks, blk_px, c->d_tri_table, levels, max_aniso, co, pl, py, W, H, elem, channels, static_cast<uint8_t *>(d_out), c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

extern "C" int hg_remap_trilinear_frames_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                                const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                                                void *d_out, const size_t *out_offsets, const void *d_pyr, size_t pyr_stride_bytes, int levels)
{
    return remap_mip_frames(c, "hg_remap_trilinear_frames_device", geoms, n_frames, d_coords, field_offsets, d_planes, W, H, n_planes, plane_stride_bytes,
                            elem, channels, d_out, out_offsets, d_pyr, pyr_stride_bytes, levels, 0);
}

extern "C" int hg_remap_aniso_frames_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                            const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                                            void *d_out, const size_t *out_offsets, const void *d_pyr, size_t pyr_stride_bytes, int levels, int max_aniso)
{
    if (max_aniso < 1 || max_aniso > 16) return fail(c, HG_ERR_INVALID, "hg_remap_aniso_frames_device: max_aniso must lie in 1..16");
    return remap_mip_frames(c, "hg_remap_aniso_frames_device", geoms, n_frames, d_coords, field_offsets, d_planes, W, H, n_planes, plane_stride_bytes,
                            elem, channels, d_out, out_offsets, d_pyr, pyr_stride_bytes, levels, max_aniso);
}

// ------------------------------------------------------------------------------------------------ the mosaic
// What the mosaic's entries share: the hg_geom limits of the canvas and of every frame, and the frame table -- quads of records, the last one
// filled with empty frames -- from the geoms and the offsets (given, or packed for `px` bytes per pixel of `es`-byte elements).
static int mosaic_table(hg_ctx *c, const char *what, const hg_geom *geoms, int n_frames, const size_t *field_offsets, const size_t *frame_offsets,
                        size_t es, size_t px, hg_geom canvas, std::vector<MosaicFrame4> *quads)
{
    std::vector<FrameDesc> lim;                               // (the window limits of the canvas and of every frame)
    const size_t zero = 0;
    HG_TRY(fill_frames(c, lim, &canvas, &zero, 1));
    if (n_frames > 0) HG_TRY(fill_frames(c, lim, geoms, nullptr, n_frames));
    quads->assign(((size_t)n_frames + 3) / 4, MosaicFrame4{});     // (the fill of the last quad: empty frames)
    size_t foff = 0, poff = 0;
    for (int f = 0; f < n_frames; f++) {
        const hg_geom &g = geoms[f];
        MosaicFrame &r = (*quads)[(size_t)f / 4].f[f % 4];
        r = MosaicFrame{field_offsets ? field_offsets[f] : foff, frame_offsets ? frame_offsets[f] : poff, g.x_off, g.y_off, g.obj_w, g.obj_h};
        if (r.fld_off & 7) return fail(c, HG_ERR_INVALID, "field offsets must be multiples of the field's pixel size (8 bytes)");
        if (r.pix_off & (es - 1)) return fail(c, HG_ERR_INVALID, std::string(what) + ": frame offsets must be multiples of the element size");
        foff += pad256(frame_px(g.obj_w, g.obj_h) * 8);
        poff += pad256(frame_px(g.obj_w, g.obj_h) * px);
    }
    return HG_OK;
}

// The table, and behind it one gain per record if there are gains (an array of its own: the records keep their 32 bytes), to
// c->d_mosaic_frames in ONE staged upload.  *d_gains: where the gains lie on the device, or nullptr.
static int upload_mosaic_table(hg_ctx *c, const std::vector<MosaicFrame4> &quads, const float *gains, int n_frames, const float **d_gains)
{
    const size_t n_quads = quads.size(), gain_quads = gains ? (n_quads * 4 * sizeof(float) + sizeof(MosaicFrame4) - 1) / sizeof(MosaicFrame4) : 0;
    *d_gains = nullptr;
    if (n_quads == 0) return HG_OK;
    HG_TRY(ensure(c, c->d_mosaic_frames, n_quads + gain_quads));
    if (!gains) return upload_frame_table(c, c->d_mosaic_frames, quads.data(), sizeof(MosaicFrame4) * n_quads);
    std::vector<MosaicFrame4> blob(n_quads + gain_quads, MosaicFrame4{});
    std::copy(quads.begin(), quads.end(), blob.begin());
    float *g = reinterpret_cast<float *>(blob.data() + n_quads);
    for (size_t f = 0; f < n_quads * 4; f++) g[f] = f < (size_t)n_frames ? gains[f] : 1.0f;      // (the fill's frames are empty)
    *d_gains = reinterpret_cast<const float *>(c->d_mosaic_frames.p + n_quads);
    return upload_frame_table(c, c->d_mosaic_frames, blob.data(), sizeof(MosaicFrame4) * blob.size());
}

static int mosaic_frames(hg_ctx *c, const char *what, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                         const void *d_frames, const size_t *frame_offsets, int elem, int channels, int W, int H, int mode, float feather,
                         hg_geom canvas, void *d_canvas, float *d_weight, const float *gains)
{
    HG_TRY(bind(c));
    const std::string fn(what);
    if (n_frames < 0 || n_frames > 65535) return fail(c, HG_ERR_INVALID, fn + ": n_frames must be 0..65535");
    if (!d_canvas) return fail(c, HG_ERR_INVALID, fn + ": d_canvas is NULL");
    if (elem != HG_ELEM_F32 && elem != HG_ELEM_U8) return fail(c, HG_ERR_INVALID, fn + ": unknown elem (HG_ELEM_F32 or HG_ELEM_U8)");
    if (mode != HG_MOSAIC_LAST && mode != HG_MOSAIC_MEAN && mode != HG_MOSAIC_FEATHER)
        return fail(c, HG_ERR_INVALID, fn + ": unknown mode (HG_MOSAIC_LAST, HG_MOSAIC_MEAN or HG_MOSAIC_FEATHER)");
    if (channels < 1 || channels > 4 || W < 1 || H < 1) return fail(c, HG_ERR_INVALID, fn + ": channels must be 1..4, W and H >= 1");
    if (mode == HG_MOSAIC_FEATHER && !(feather > 0.0f)) return fail(c, HG_ERR_INVALID, fn + ": feather must be > 0 (+Inf: uncapped)");
    if (n_frames > 0 && (!geoms || !d_coords || !d_frames)) return fail(c, HG_ERR_INVALID, fn + ": NULL pointer");
    const size_t es = elem == HG_ELEM_F32 ? 4 : 1, px = es * (size_t)channels;
    if (misaligned(d_coords, 8) || misaligned(d_frames, es) || misaligned(d_canvas, es) || misaligned(d_weight, 4))
        return fail(c, HG_ERR_INVALID, fn + ": d_coords must be aligned to 8 bytes, d_frames / d_canvas to the element size, d_weight to 4");
    for (int f = 0; gains && f < n_frames; f++)
        if (!(gains[f] > 0.0f) || !std::isfinite(gains[f])) return fail(c, HG_ERR_INVALID, fn + ": every gain must be finite and > 0");
    std::vector<MosaicFrame4> quads;
    HG_TRY(mosaic_table(c, what, geoms, n_frames, field_offsets, frame_offsets, es, px, canvas, &quads));
    const size_t n_px = frame_px(canvas.obj_w, canvas.obj_h);
    if (n_px == 0) return HG_OK;
    HG_TRY(settle_pending_on(c, d_canvas, n_px * px));
    if (d_weight) HG_TRY(settle_pending_on(c, d_weight, n_px * 4));
    const float *d_gains = nullptr;
    HG_TRY(upload_mosaic_table(c, quads, gains, n_frames, &d_gains));
    launch_mosaic_frames(c->d_mosaic_frames, (int)quads.size(), static_cast<const uint8_t *>(d_coords), static_cast<const uint8_t *>(d_frames), W, H, elem, channels,
                         mode, feather, canvas.x_off, canvas.y_off, canvas.obj_w, canvas.obj_h, static_cast<uint8_t *>(d_canvas), d_weight, d_gains, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

extern "C" int hg_mosaic_frames_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                       const void *d_frames, const size_t *frame_offsets, int elem, int channels, int W, int H,
                                       int mode, float feather, hg_geom canvas, void *d_canvas, float *d_weight)
{
    return mosaic_frames(c, "hg_mosaic_frames_device", geoms, n_frames, d_coords, field_offsets, d_frames, frame_offsets, elem, channels, W, H, mode, feather,
                         canvas, d_canvas, d_weight, nullptr);
}

extern "C" int hg_mosaic_frames_gain_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                            const void *d_frames, const size_t *frame_offsets, int elem, int channels, int W, int H,
                                            int mode, float feather, hg_geom canvas, void *d_canvas, float *d_weight, const float *gains)
{
    return mosaic_frames(c, "hg_mosaic_frames_gain_device", geoms, n_frames, d_coords, field_offsets, d_frames, frame_offsets, elem, channels, W, H, mode,
                         feather, canvas, d_canvas, d_weight, n_frames > 0 ? gains : nullptr);
}

// ------------------------------------------------------------------------------------------------ the robust mosaic
// The mosaic's entry with an order statistic for a blend: its checks in its order (those that do not apply -- elem, W, H, feather -- left
// out), then this entry's own.  u8 only.
extern "C" int hg_mosaic_robust_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                       const void *d_frames, const size_t *frame_offsets, int channels, int mode, float trim, const float *gains,
                                       hg_geom canvas, void *d_canvas, float *d_weight)
{
    HG_TRY(bind(c));
    const char *what = "hg_mosaic_robust_device";
    const std::string fn(what);
    if (n_frames < 0 || n_frames > 65535) return fail(c, HG_ERR_INVALID, fn + ": n_frames must be 0..256");
    if (!d_canvas) return fail(c, HG_ERR_INVALID, fn + ": d_canvas is NULL");
    if (channels < 1 || channels > 4) return fail(c, HG_ERR_INVALID, fn + ": channels must be 1..4");
    if (n_frames > 0 && (!geoms || !d_coords || !d_frames)) return fail(c, HG_ERR_INVALID, fn + ": NULL pointer");
    if (misaligned(d_coords, 8) || misaligned(d_weight, 4)) return fail(c, HG_ERR_INVALID, fn + ": d_coords must be aligned to 8 bytes, d_weight to 4");
    std::vector<MosaicFrame4> quads;
    if (const int rc = mosaic_table(c, what, geoms, n_frames, field_offsets, frame_offsets, 1, (size_t)channels, canvas, &quads))
        return c->err.find(fn) == std::string::npos ? fail(c, rc, fn + ": " + c->err) : rc;       // (the shared checks do not all name their caller)
    if (n_frames > 256) return fail(c, HG_ERR_INVALID, fn + ": n_frames must be 0..256");
    if (mode != HG_ROBUST_MEDIAN && mode != HG_ROBUST_TRIMMED && mode != HG_ROBUST_MIN && mode != HG_ROBUST_MAX)
        return fail(c, HG_ERR_INVALID, fn + ": unknown mode (HG_ROBUST_MEDIAN, HG_ROBUST_TRIMMED, HG_ROBUST_MIN or HG_ROBUST_MAX)");
    if (mode == HG_ROBUST_TRIMMED && !(trim >= 0.0f && trim < 0.5f)) return fail(c, HG_ERR_INVALID, fn + ": trim must lie in [0, 0.5)");
    if (n_frames == 0) gains = nullptr;
    for (int f = 0; gains && f < n_frames; f++)
        if (!(gains[f] > 0.0f) || !std::isfinite(gains[f])) return fail(c, HG_ERR_INVALID, fn + ": every gain must be finite and > 0");
    const size_t n_px = frame_px(canvas.obj_w, canvas.obj_h);
    if (n_px == 0) return HG_OK;
    HG_TRY(settle_pending_on(c, d_canvas, n_px * (size_t)channels));
    if (d_weight) HG_TRY(settle_pending_on(c, d_weight, n_px * 4));
    const float *d_gains = nullptr;
    HG_TRY(upload_mosaic_table(c, quads, gains, n_frames, &d_gains));
    launch_mosaic_robust(c->d_mosaic_frames, n_frames, static_cast<const uint8_t *>(d_coords), static_cast<const uint8_t *>(d_frames), channels, mode, trim,
                         canvas.x_off, canvas.y_off, canvas.obj_w, canvas.obj_h, static_cast<uint8_t *>(d_canvas), d_weight, d_gains, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ exposure: overlap statistics and the gain solve
extern "C" int hg_mosaic_overlap_stats_device(hg_ctx *c, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                                              const void *d_frames, const size_t *frame_offsets, int channels, hg_geom canvas, uint64_t *d_stats)
{
    HG_TRY(bind(c));
    const char *what = "hg_mosaic_overlap_stats_device";
    const std::string fn(what);
    if (n_frames < 0 || n_frames > 256) return fail(c, HG_ERR_INVALID, fn + ": n_frames must be 0..256");
    if (channels < 1 || channels > 4) return fail(c, HG_ERR_INVALID, fn + ": channels must be 1..4");
    if (n_frames > 0 && (!geoms || !d_coords || !d_frames || !d_stats)) return fail(c, HG_ERR_INVALID, fn + ": NULL pointer");
    if (misaligned(d_coords, 8) || misaligned(d_stats, 8)) return fail(c, HG_ERR_INVALID, fn + ": d_coords and d_stats must be aligned to 8 bytes");
    std::vector<MosaicFrame4> quads;
    HG_TRY(mosaic_table(c, what, geoms, n_frames, field_offsets, frame_offsets, 1, (size_t)channels, canvas, &quads));
    if (n_frames == 0) return HG_OK;
    const size_t bytes = (size_t)n_frames * (size_t)n_frames * 2 * sizeof(uint64_t);
    HG_TRY(settle_pending_on(c, d_stats, bytes));
    HIP_TRY(c, hipMemsetAsync(d_stats, 0, bytes, c->stream));
    if (frame_px(canvas.obj_w, canvas.obj_h) == 0) return HG_OK;
    const float *none = nullptr;
    HG_TRY(upload_mosaic_table(c, quads, nullptr, n_frames, &none));
    launch_mosaic_stats(c->d_mosaic_frames, n_frames, static_cast<const uint8_t *>(d_coords), static_cast<const uint8_t *>(d_frames), channels, canvas.x_off,
                        canvas.y_off, canvas.obj_w, canvas.obj_h, d_stats, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// Host only, no context: the normal equations of Brown & Lowe's gain error over the frames that cover anything, solved by a Cholesky
// factorisation in double, in index order.
extern "C" int hg_mosaic_solve_gains(const uint64_t *stats, int n_frames, int channels, double sigma_n, double sigma_g, float *gains)
{
    const std::string fn("hg_mosaic_solve_gains");
    if (n_frames < 0 || n_frames > 256) return fail(nullptr, HG_ERR_INVALID, fn + ": n_frames must be 0..256");
    if (channels < 1 || channels > 4) return fail(nullptr, HG_ERR_INVALID, fn + ": channels must be 1..4");
    if (!std::isfinite(sigma_n) || !std::isfinite(sigma_g) || !(sigma_n > 0.0) || !(sigma_g > 0.0))
        return fail(nullptr, HG_ERR_INVALID, fn + ": sigma_n and sigma_g must be finite and > 0");
    if (n_frames == 0) return HG_OK;
    if (!stats || !gains) return fail(nullptr, HG_ERR_INVALID, fn + ": NULL pointer");
    const size_t F = (size_t)n_frames;
    const double k = channels == 4 ? 3.0 : (double)channels, alpha = 1.0 / (sigma_n * sigma_n), beta = 1.0 / (sigma_g * sigma_g);
    auto N = [&](size_t a, size_t b) { return stats[(a * F + b) * 2]; };
    auto I = [&](size_t a, size_t b) { return (double)stats[(a * F + b) * 2 + 1] / (k * (double)N(a, b)); };      // (asked where N > 0 only)
    for (size_t a = 0; a < F; a++)
        for (size_t b = a + 1; b < F; b++)
            if (N(a, b) != N(b, a)) return fail(nullptr, HG_ERR_INVALID, fn + ": the statistics are not symmetric in N");
    std::vector<size_t> live;                                 // the frames that cover anything, ascending
    for (size_t a = 0; a < F; a++) { gains[a] = 1.0f; if (N(a, a) > 0) live.push_back(a); }
    const size_t n = live.size();
    std::vector<double> A(n * n, 0.0), rhs(n, 0.0);
    for (size_t r = 0; r < n; r++) {
        const size_t a = live[r];
        double cover = 0.0, diag = 0.0;
        for (size_t q = 0; q < n; q++) {
            const size_t b = live[q];
            if (N(a, b) == 0) continue;
            const double nab = (double)N(a, b);
            cover += nab;
            if (b == a) continue;
            diag += nab * I(a, b) * I(a, b);
            A[r * n + q] = -2.0 * alpha * nab * I(a, b) * I(b, a);
        }
        A[r * n + r] = beta * cover + 2.0 * alpha * diag;
        rhs[r] = beta * cover;
    }
    // A = L L^T (the lower triangle, in place), then L y = rhs and L^T g = y
    for (size_t j = 0; j < n; j++) {
        double d = A[j * n + j];
        for (size_t q = 0; q < j; q++) d -= A[j * n + q] * A[j * n + q];
        if (!(d > 0.0) || !std::isfinite(d)) return fail(nullptr, HG_ERR_INVALID, fn + ": the system is not positive definite");
        const double l = std::sqrt(d);
        A[j * n + j] = l;
        for (size_t i = j + 1; i < n; i++) {
            double v = A[i * n + j];
            for (size_t q = 0; q < j; q++) v -= A[i * n + q] * A[j * n + q];
            A[i * n + j] = v / l;
        }
    }
    for (size_t i = 0; i < n; i++) {
        double v = rhs[i];
        for (size_t q = 0; q < i; q++) v -= A[i * n + q] * rhs[q];
        rhs[i] = v / A[i * n + i];
    }
    for (size_t i = n; i-- > 0;) {
        double v = rhs[i];
        for (size_t q = i + 1; q < n; q++) v -= A[q * n + i] * rhs[q];
        rhs[i] = v / A[i * n + i];
    }
    for (size_t r = 0; r < n; r++) {
        const float g = (float)rhs[r];
        if (!std::isfinite(g) || !(g > 0.0f)) {
            for (size_t a = 0; a < F; a++) gains[a] = 1.0f;
            return fail(nullptr, HG_ERR_INVALID, fn + ": the solution has a gain that is not finite and positive");
        }
        gains[live[r]] = g;
    }
    return HG_OK;
}
