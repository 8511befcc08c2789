// hg_api_points.hip -- the C ABI, part 7: point lists through the warp geometry of a frame set (hg_points_to_source_*, hg_points_to_output_*).
// Like a field call a points call is geometry only: it needs the source's SIZE, is independent of the sampling mode, and leaves the warp
// paths' taps (hg_last_*_kernel), the plan of the last warp and what the policy learned as it found them.  Every entry point follows its
// field counterpart (hg_api_field.hip, hg_api_forward.hip) in what it demands of the context, what it settles first and what it stages.
#include "hg_ctx.h"

constexpr int kMaxPoints = 1 << 24;              // points per list

// What every points call checks first.  *work: false when there is nothing to do (n_points == 0: HG_OK, nothing is touched).
static int check_points_args(hg_ctx *c, const void *d_points, int n_points, int n_sets, const void *d_out, bool *work)
{
    *work = false;
    if (n_points < 0 || n_points > kMaxPoints) return fail(c, HG_ERR_INVALID, "n_points must be 0..2^24");
    if (n_sets < 1) return fail(c, HG_ERR_INVALID, "n_sets must be >= 1");
    if (n_points == 0) return HG_OK;
    if (!d_points || !d_out) return fail(c, HG_ERR_INVALID, "d_points / d_out is NULL");
    if (misaligned(d_points, 8) || misaligned(d_out, 8))
        return fail(c, HG_ERR_INVALID, "d_points / d_out must be aligned to 8 bytes (interleaved x,y float32)");
    *work = true;
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ to source
extern "C" int hg_points_to_source_geometric_frames_device(hg_ctx *c, const void *d_points, int n_points, int n_sets, void *d_out)
{
    HG_TRY(bind(c));
    bool work = false;
    HG_TRY(check_points_args(c, d_points, n_points, n_sets, d_out, &work));
    if (!work) return HG_OK;
    if (!c->d_img || c->W <= 0 || c->H <= 0) return fail(c, HG_ERR_STATE, "no source image: the coverage test needs its size (hg_set_image)");
    if (c->geo_frames.empty()) return fail(c, HG_ERR_STATE, "no frames: call hg_geometric_set_frames first");
    const size_t F = c->geo_frames.size();
    HG_TRY(settle_pending_on(c, d_out, F * (size_t)n_points * 8));      // (as the fields do)
    // frames given as point sets: the matrices are solved on the device, as at the head of every warp of the set (:994)
    if (c->geo_from_points)
        launch_solve_frames(c->geo_kind, c->d_geo_pts, c->d_geo_pts + F * 8, c->d_geo_frames, c->d_mats, c->d_geo_plain, (int)F, c->stream);
    HG_TRY(time_begin(c));
    launch_geo_points(c->geo_kind, 0, c->d_geo_frames, c->d_mats, (int)F, c->W, c->H, static_cast<const float *>(d_points), n_points, n_sets,
                      static_cast<float *>(d_out), c->stream);
    HG_TRY(time_end(c));
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// General path, settled inside the call like hg_field_inverse_piecewise_frames_device: queued warp runs are settled first and keep their own
// results; k_tri_setup (flagging into a status set of this call's own) + k_pw_points_src over the whole set; a frame k_tri_setup flagged
// irregular is redone through the materialised map before the call returns and counted in hg_redone_frames.  There is no LDS span list and
// hence no overflow flag.  The plan of the last warp, what the policy learned, the status ring and the kernel taps are not touched.
extern "C" int hg_points_to_source_piecewise_frames_device(hg_ctx *c, const void *d_points, int n_points, int n_sets, void *d_out)
{
    HG_TRY(bind(c));
    bool work = false;
    HG_TRY(check_points_args(c, d_points, n_points, n_sets, d_out, &work));
    if (!work) return HG_OK;
    HG_TRY(check_pw_state(c));
    if (c->W <= 0 || c->H <= 0) return fail(c, HG_ERR_STATE, "no source image: the bounds test needs its size (hg_set_image)");
    HG_TRY(hg_sync(c));                                      // queued warp runs: settled against their own status sets and staged frame sets
    const size_t F = c->pw_frames.size();
    PwMesh mesh = mesh_of(c);
    PwFrames fr = frames_of(c);
    fr.status = c->solve.status; fr.host_flag = nullptr;         // a status set of this call's own, read right below
    fr.two_round = nullptr;                                  // (outside the frame set's step numbering, like the deferred redo)
    fr.self_spans = 0; fr.band_ent = nullptr; fr.band_cnt = nullptr; fr.n_bands = 0;     // k_tri_setup without candidate bands
    const float *pts = static_cast<const float *>(d_points);
    float *out = static_cast<float *>(d_out);
    HIP_TRY(c, hipMemsetAsync(c->solve.status, 0, sizeof(int32_t) * F, c->stream));
    launch_tri_setup(mesh, fr, c->stream);
    HG_TRY(time_begin(c));
    launch_pw_points_src(mesh, fr, pts, n_points, n_sets, out, c->stream);
    HG_TRY(time_end(c));
    HIP_TRY(c, hipGetLastError());
    std::vector<int32_t> status(F);
    HIP_TRY(c, hipMemcpyAsync(status.data(), c->solve.status, sizeof(int32_t) * F, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    bool redone = false;
    for (size_t f = 0; f < F; f++) {
        if (status[f] == FRAME_OK) continue;
        const FrameDesc &fd = c->pw_frames[f];
        if (fd.obj_w <= 0 || fd.obj_h <= 0) continue;        // (the kernel has written this frame: an empty window holds no cell)
        HG_TRY(ensure(c, c->d_map32, (size_t)fd.obj_w * fd.obj_h));
        launch_map_build(mesh, fr, (int)f, fd, c->d_map32, c->stream);      // (k_tri_setup's edge equations and row ranges of frame f)
        launch_points_from_map(mesh, fr, (int)f, fd, c->d_map32, pts, n_points, n_sets, out, c->stream);
        HIP_TRY(c, hipGetLastError());
        c->pw_redone++; c->pw_last_flag = status[f];
        redone = true;
    }
    if (redone) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ to output
// The limits and refusals of hg_field_forward_geometric_batch_device; queued runs are settled first (hg_sync), then the call is asynchronous:
// the matrices and the windows' offsets go up in one block (the scratch of the tile-binned forward kernels: no staged set is touched).
extern "C" int hg_points_to_output_geometric_batch_device(hg_ctx *c, int kind, const double *m, const hg_geom *geoms, int n_frames,
                                                          const void *d_points, int n_points, int n_sets, void *d_out)
{
    HG_TRY(bind(c));
    bool work = false;
    HG_TRY(check_points_args(c, d_points, n_points, n_sets, d_out, &work));
    if (!work) return HG_OK;
    if ((kind != HG_AFFINE && kind != HG_PROJECTIVE) || !m || !geoms || n_frames <= 0)
        return fail(c, HG_ERR_INVALID, "hg_points_to_output_geometric: bad arguments");
    if (!c->d_img) return fail(c, HG_ERR_STATE, "no source image: call hg_set_image first");
    if ((int64_t)c->W * c->H >= ((int64_t)1 << 31) || c->H > 65535)
        return fail(c, HG_ERR_INVALID, "the source image has 2^31 pixels or more, or more than 65535 rows: not supported by the forward path");
    std::vector<FrameDesc> fds;
    HG_TRY(fill_frames(c, fds, geoms, nullptr, n_frames));   // (the window limits of every frame; 65535 frames)
    HG_TRY(hg_sync(c));
    const size_t n = (size_t)n_frames, m_bytes = sizeof(double) * 8 * n, bytes = m_bytes + sizeof(FrameDesc) * n;
    HG_TRY(ensure(c, c->d_fwd_par, bytes));
    std::vector<uint8_t> blob(bytes);
    std::memcpy(blob.data(), m, m_bytes);
    std::memcpy(blob.data() + m_bytes, fds.data(), sizeof(FrameDesc) * n);
    HIP_TRY(c, hipMemcpyAsync(c->d_fwd_par, blob.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));             // caller / local memory is not retained
    launch_geo_points(kind, 1, reinterpret_cast<const FrameDesc *>(c->d_fwd_par + m_bytes), reinterpret_cast<const double *>(c->d_fwd_par.p), n_frames,
                      c->W, c->H, static_cast<const float *>(d_points), n_points, n_sets, static_cast<float *>(d_out), c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}

// Steps (A) and (B) of hg_field_forward_piecewise_batch_device (forward_piecewise_stage: limits, queued runs settled, the forward map built or
// reused, the frame set staged, k_tri_setup), then one launch; nothing to redo, asynchronous on the ctx stream.
extern "C" int hg_points_to_output_piecewise_batch_device(hg_ctx *c, const float *dst_points, int max_src_x, int max_src_y, const hg_geom *geoms,
                                                          int n_frames, const void *d_points, int n_points, int n_sets, void *d_out)
{
    HG_TRY(bind(c));
    bool work = false;
    HG_TRY(check_points_args(c, d_points, n_points, n_sets, d_out, &work));
    if (!work) return HG_OK;
    if (!dst_points || !geoms || n_frames <= 0) return fail(c, HG_ERR_INVALID, "hg_points_to_output_piecewise: bad arguments");
    int64_t map_w = 0, map_h = 0;
    HG_TRY(forward_piecewise_stage(c, dst_points, max_src_x, max_src_y, geoms, nullptr, n_frames, true, &map_w, &map_h));
    if (map_w <= 0 || map_h <= 0) map_w = map_h = 0;         // (an empty source box: no map, no cell)
    launch_pw_points_out(c->d_fmap, c->solve.fwd, c->d_pw_frames, n_frames, c->n_tris, c->min_src_x, c->min_src_y, (int)map_w, (int)map_h,
                         static_cast<const float *>(d_points), n_points, n_sets, static_cast<float *>(d_out), c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}
