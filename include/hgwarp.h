/*
 * hgwarp.h -- C ABI of libhgwarp.so, the MI355X (gfx950) inverse-warp engine that sits behind the Homography.js
 * `Homography` class for its per-pixel hot path.
 *
 * The reference (Eric-Canas/Homography.js v1.8.0) has no FFI seam: the seam is the ES-module class itself.  Each
 * entry point below therefore names the reference *function* it replaces (file:line into the reference's
 * Homography.js).  The bindings that call this ABI are
 *     homography.js_amd/csrc/hgwarp_napi.c   (N-API addon used by the drop-in JS class homography.js_amd/js/Homography.mjs)
 *     homography.js_amd/hgwarp.py            (ctypes; used by tests/, bench.py and __graft_entry__.py)
 * and INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns an int status (HG_OK == 0); hg_last_error() gives the text of the last failure;
 *   - plain pointers + sizes, no C++/torch types; caller memory is never retained after return unless the function
 *     name ends in `_device` and says "aliased";
 *   - one hg_ctx per Homography instance; a ctx is bound to one GPU and one HIP stream and is not thread-safe;
 *     distinct ctxs are independent;
 *   - images are RGBA8, row-major, 4*W*H bytes (Uint8ClampedArray of an ImageData, reference :297-299);
 *   - points are interleaved x,y float32 (the reference's Float32Array, :220/:339); triangles are 3 uint32 vertex ids
 *     each (Delaunator's `.triangles`, :1217); per-triangle matrices are 6 float32 [a,b,c,d,e,f] with
 *     x' = a*x + c*y + e, y' = b*x + d*y + f (:1297-1304);
 *   - functions ending in `_device` take/leave data in GPU memory and are asynchronous on the ctx stream
 *     (hg_sync() waits and reports deferred errors); the others are synchronous like the reference's warp();
 *   - there is NO CPU fallback: without a usable gfx950 device hg_create() fails and nothing warps.
 */
#ifndef HGWARP_H
#define HGWARP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_VERSION 100          /* 0.1.0 (sampling modes are detected by the presence of hg_set_sampling, source fields by that of hg_field_inverse_geometric,
                                   the forward source fields by that of hg_field_forward_geometric, point lists by that of
                                   hg_points_to_source_geometric_frames_device, mip pyramids and the trilinear remap by that of hg_pyramid_build_device,
                                   the anisotropic remap by that of hg_remap_aniso_frames_device, mosaics by the presence of hg_mosaic_frames_device,
                                   the bicubic remap by that of hg_remap_bicubic_frames_device, exposure gains of a mosaic by that of
                                   hg_mosaic_overlap_stats_device, fitting transforms to matches by that of hg_fit_matches_frames_device);
                                   matching descriptors by the presence of hg_match_descriptors_frames_device, keypoints by the presence of
                                   hg_detect_describe_frames_device, multi-band mosaics by the presence of hg_mosaic_multiband_device, robust mosaics
                                   by the presence of hg_mosaic_robust_device, adjusting a frame set over all pairs by the presence of
                                   hg_bundle_adjust_frames_device, thin-plate splines
                                   by the presence of hg_tps_solve_frames_device, dense optical flow by the presence of
                                   hg_flow_dense_frames_device, camera models by the presence of hg_field_camera_frames_device,
                                   refining transforms on the pixels by the presence of
                                   hg_align_refine_frames_device */

enum {
    HG_OK = 0,
    HG_ERR_INVALID = 1,         /* bad argument (NULL pointer, negative size, unknown kind) */
    HG_ERR_HIP = 2,             /* a HIP runtime call failed (text in hg_last_error) */
    HG_ERR_NO_DEVICE = 3,       /* no usable GPU / device id out of range */
    HG_ERR_STATE = 4,           /* call order: image / mesh / prepared frame missing */
    HG_ERR_NOMEM = 5,
    HG_ERR_RANGE = 6            /* a reference-state warp whose map names a triangle without a matrix: the reference's loop throws a
                                   TypeError there (`matrix[0]` of undefined, :1383) */
};

enum { HG_AFFINE = 0, HG_PROJECTIVE = 1 };

/* Sampling modes of the inverse warps (hg_set_sampling).  Not part of the reference, which always copies the nearest pixel. */
enum { HG_SAMPLE_NEAREST = 0, HG_SAMPLE_BILINEAR = 1 };

/* Formats of the SOURCE FIELD of an inverse warp (hg_field_*): for every output pixel, which source pixel the nearest loop reads
 * (HG_FIELD_INDEX, one int32) or where it looks (HG_FIELD_COORDS, two float32).  Not part of the reference. */
enum { HG_FIELD_INDEX = 0, HG_FIELD_COORDS = 1 };
/* Element types of the planes a bilinear remap reads and writes (hg_remap_bilinear_frames_device). */
enum { HG_ELEM_F32 = 0, HG_ELEM_U8 = 1 };

typedef struct hg_ctx hg_ctx;

/* Output window of one frame, the reference's (_xOutputOffset, _yOutputOffset, _objectiveWidth, _objectiveHeight).
 * Accepted: up to 2^31 pixels, offsets up to 2^26 in magnitude, at most 65535 frames per set (HG_ERR_INVALID beyond);
 * obj_w / obj_h <= 0 = empty frame. */
typedef struct hg_geom { int32_t x_off, y_off, obj_w, obj_h; } hg_geom;

/* ------------------------------------------------------------------------------------------------ library / context */
int hg_version(void);
int hg_device_count(int *count);
/* Replaces `new Homography()` (:78) for the device side: owns a stream and the device buffers. */
int hg_create(int device_id, hg_ctx **ctx);
/* Same, but launches on a stream owned by the caller (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream). */
int hg_create_on_stream(int device_id, void *hip_stream, hg_ctx **ctx);
void hg_destroy(hg_ctx *ctx);
/* Text of the last error on this ctx (or, with ctx == NULL, of the last failed hg_create / host call of this thread). */
const char *hg_last_error(const hg_ctx *ctx);
/* Waits for the ctx stream; returns the first deferred error of the asynchronous `_device` calls since the last sync.
 * Also settles queued piecewise runs: hg_warp_inverse_piecewise_frames_device calls are queued back to back (up to 63
 * before the library syncs by itself); a frame whose mesh is denser than the fast path's row lists (or whose spans are
 * irregular) is only flagged by the kernel and is redone here, through the materialised map, into the output buffer of
 * the call that flagged it (from the frame set that call was given: a staged copy, newer sets may have gone up since).  Queued
 * calls that wrote overlapping bytes are settled in call order: a later call's frame goes back on top of an earlier call's redo,
 * and an earlier redo is skipped when a later call wrote exactly the same byte range (one buffer reused step after step).  The
 * same holds for queued hg_warp_forward_piecewise_batch_device calls (tile lists over capacity, triangles the tiles cannot bound).
 * A frame is final once hg_sync (or any synchronous call) has returned. */
int hg_sync(hg_ctx *ctx);
/* Sampling mode of the ctx (HG_ERR_INVALID for any other value; the default is HG_SAMPLE_NEAREST).
 *   HG_SAMPLE_NEAREST   the reference's Math.round(srcX) pixel copy (:1005-1007, :1048-1052), bit-identical to it.
 *   HG_SAMPLE_BILINEAR  opt-in, not the reference's.  The source coordinate (sx, sy) is computed exactly as in nearest mode (f64,
 *                       JS operation order) and the coverage test is unchanged (:1001; :1045-1047 with the minSrc bounds for
 *                       piecewise): a pixel is written iff nearest mode writes it, uncovered pixels stay all-zero.  Taps:
 *                       x0 = floor(sx), y0 = floor(sy), fx = (float)(sx - x0), fy = (float)(sy - y0); columns clamp(x0, 0, W-1) and
 *                       clamp(x0+1, 0, W-1), rows alike (piecewise indexes the source as the reference does: no minSrc subtraction).
 *                       No read leaves the image: nearest mode's wrap of the flat index does not exist here.  Blend: straight
 *                       (not premultiplied) RGBA, each channel in f32,
 *                           v = (p00*(1-fx) + p01*fx)*(1-fy) + (p10*(1-fx) + p11*fx)*fy,   out = (uint8)min(255, floor(v + 0.5f)),
 *                       so that where fx == fy == 0 the result equals the nearest one byte for byte.
 * The mode governs the INVERSE warps: single-frame, frame-set, batch and `_device` forms, per-frame sources (hg_set_images_device),
 * hg_warp_inverse_piecewise_via_map, hg_warp_inverse_piecewise_state and the hg_multi_* batches.  The forward (scatter) entry points
 * copy source pixels by definition and ignore it; so do the taps (hg_get_tri_map*, hg_get_matrices).  The mode in effect when a warp
 * entry point is called governs that warp, whichever mode its frame set was staged under; work already queued keeps the mode it was
 * queued with, including the frames hg_sync redoes through the map.  Bilinear piecewise warps run on the general kernel
 * (hg_last_piecewise_kernel() == 4) and are settled within the call.  Not an hg_set_option knob: it changes results. */
int hg_set_sampling(hg_ctx *ctx, int mode);
int hg_get_sampling(const hg_ctx *ctx, int *mode);
/* Device scratch/output helpers so that bindings without a device allocator (Node) can keep frames resident. */
int hg_device_alloc(hg_ctx *ctx, size_t bytes, void **dptr);
int hg_device_free(hg_ctx *ctx, void *dptr);
int hg_copy_to_host(hg_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
int hg_copy_to_device(hg_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
/* D2H queued on the ctx stream behind the warps issued so far; dst must stay alive until hg_sync().  A true asynchronous
 * DMA when dst is pinned memory from hg_host_alloc (page-locked, usable by every device). */
int hg_copy_to_host_async(hg_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
/* The same without settling queued runs first (purely stream-ordered): for callers that queue the copies of several devices
 * before waiting for any (hg_multi_*); frames a fused run only flagged are rewritten by the later hg_sync -- hg_redone_frames
 * tells -- and must then be copied again. */
int hg_enqueue_copy_to_host(hg_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
/* Host -> device on the context's COPY stream (a second stream owned by the ctx), not ordered with the warp stream until
 * hg_fence_copies(): the upload of frame f + 1's source overlaps frame f's D2H on the warp stream (full-duplex PCIe).  Pageable src:
 * returns once the caller's memory has been read.  hg_fence_copies: everything queued on the warp stream afterwards waits for the
 * uploads queued so far.  (The video loop `for (f) warp(image_f)`, README.md:121-137, through js/Homography.mjs warpBatch({images}).) */
int hg_upload_on_copy_stream(hg_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
int hg_fence_copies(hg_ctx *ctx);
/* Device -> host on the context's DOWNLOAD stream (a third stream owned by the ctx), ordered behind the warps issued so far and nothing
 * issued later: frame f comes down while frame f + 1 is warped and image f + 2 goes up.  Stream-ordered like hg_enqueue_copy_to_host (a
 * frame a fused run flagged is rewritten by the next hg_sync -- hg_redone_frames tells -- and is then downloaded again by the caller).
 * hg_fence_downloads: the host waits for the downloads queued so far (hg_sync does not wait for them). */
int hg_download_behind_warps(hg_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
int hg_fence_downloads(hg_ctx *ctx);
/* Everything queued on the ctx stream after this call waits for hip_event (a hipEvent_t recorded on any stream of any device):
 * orders warps behind the caller's own uploads / peer copies without blocking the host. */
int hg_stream_wait_event(hg_ctx *ctx, void *hip_event);
int hg_host_alloc(size_t bytes, void **ptr);
int hg_host_free(void *ptr);
int hg_ctx_device(const hg_ctx *ctx);

/* ------------------------------------------------------------------------------------------------ host-side solves
 * Tiny, run on the host in double precision with the reference's exact operation order; no GPU needed. */
/* affineMatrixFromTriangles :1265-1306 */
int hg_solve_affine(const float src[6], const float dst[6], float out[6]);
/* inverseAffineMatrix :1345-1365 */
int hg_invert_affine(const float m[6], float out[6]);
/* projectiveMatrixFromSquares :1320-1333 + numeric.js solve/LU/LUsolve :1650-1751; out = h0..h7 (h8 == 1) */
int hg_solve_projective(const float src[8], const float dst[8], double out[8]);
/* calculateTransformLimits :1503-1527; kind HG_AFFINE (m[0..5]) / HG_PROJECTIVE (m[0..7]); out = xOff,yOff,objW,objH
 * as doubles exactly as JS computes them (may be NaN/Inf for degenerate matrices). */
int hg_transform_limits(int kind, const double *m, double width, double height, double out[4]);
/* minmaxXYofArray(array, rounded=true) :1558-1589; out = round(minX), round(minY), round(maxX), round(maxY) */
int hg_minmax_xy(const float *points, int n_values, double out[4]);
/* Math.round (ties toward +Infinity), exposed so that bindings share one definition. */
double hg_js_round(double x);
/* Host Delaunay triangulation, where the reference calls `new Delaunator(points).triangles` (:1216-1218 <- :262, :742).
 * points = n_points interleaved x,y.  Writes up to `capacity` triangles (3 vertex ids each) and stores the total count in
 * *n_triangles; pass out_triangles = NULL to query the count (at most 2*n_points).  The algorithm is a restatement of
 * delaunator 5.0.0's (sweep-hull, its seed choice, sort, hull hash and flip order; orientation by an exact-sign predicate), so
 * the LIST is meant to equal delaunator's -- order and diagonals decide pixels where triangles meet -- but delaunator's
 * source is absent from the reference tree and no reference test pins it: "triangulation parity unpinned".  Identical
 * (order included) to js/delaunay.mjs.  HG_ERR_INVALID for non-finite input or a too-small buffer. */
int hg_triangulate(const float *points, int n_points, uint32_t *out_triangles, int capacity, int *n_triangles);

/* ------------------------------------------------------------------------------------------------ source image */
/* setImage, ImageData branch :297-299: uploads RGBA8 (the reference aliases caller memory and re-reads it on every
 * warp(); callers that mutate the buffer call this again). */
int hg_set_image(hg_ctx *ctx, const uint8_t *rgba, int width, int height);
/* Same, source already in GPU memory (aliased, not copied: it must stay alive and unchanged while warps run).
 * This is how a source texture received by an RCCL broadcast is attached without another copy. */
int hg_set_image_device(hg_ctx *ctx, const void *d_rgba, int width, int height);
/* The video case `for (f) { warp(frame_f) }` (README.md:121-137: every warp() gets its own image, setImage :290 per
 * frame): n_images sources of identical size, `stride_bytes` apart in GPU memory (aliased).  Frame f of a frame set
 * (hg_*_set_frames), and frame f of a batch of the forward (scatter-semantics) entry points hg_warp_forward_*_batch_device, then
 * reads image f % n_images; n_images == 1 is hg_set_image_device. */
int hg_set_images_device(hg_ctx *ctx, const void *d_rgba, int width, int height, int n_images, size_t stride_bytes);

/* ------------------------------------------------------------------------------------------------ affine / projective
 * _inverseGeometricWarp pixel loop :997-1011 (+ applyAffineTransformToPoint :1382 / applyProjectiveTransformToPoint
 * :1401).  `m` is the INVERSE matrix the reference obtains at :994 by re-solving with the point sets swapped
 * (hg_solve_affine(dst, src) widened to double, or hg_solve_projective(dst, src)): 6 resp. 8 doubles.
 * Output: 4*obj_w*obj_h bytes, every pixel written (0 where the reference leaves the zero-initialised buffer). */
int hg_warp_inverse_geometric(hg_ctx *ctx, int kind, const double *m, hg_geom geom, uint8_t *out_host);
int hg_warp_inverse_geometric_device(hg_ctx *ctx, int kind, const double *m, hg_geom geom, void *d_out);
/* The caller loop `setDestinyPoints(dst_f); warp()` (test/benchmark.js:107-110) for F frames in one launch:
 * m = F x 8 doubles (affine uses the first 6 of each 8), geoms = F windows, out_offsets = F byte offsets into d_out
 * (NULL: packed as hg_pack_offsets does).  set_frames uploads the per-frame inputs (kept until replaced);
 * frames_device runs all uploaded frames; batch_device = both. */
int hg_geometric_set_frames(hg_ctx *ctx, int kind, const double *m, const hg_geom *geoms, const size_t *out_offsets, int n_frames);
/* Same frame set given as POINT SETS: the reference obtains the inverse matrix at the head of every inverse warp by
 * re-solving with the swapped sets (:994 calculateTransformMatrix(dstPoints, srcPoints) -> projectiveMatrixFromSquares
 * :1320-1333 + numeric.js LU/LUsolve :1650-1751, or affineMatrixFromTriangles :1265-1306).  from / to = n_frames x 4 (or
 * 3) points x,y float32; the matrix of frame f maps from[f] -> to[f] (pass dst, src for the inverse warp).  Every
 * hg_warp_inverse_geometric_frames_device then runs the solves ON THE DEVICE (one lane per frame, the LU in its exact
 * operation order; bit patterns equal to hg_solve_projective / hg_solve_affine) followed by the pixel kernel. */
int hg_geometric_set_frames_points(hg_ctx *ctx, int kind, const float *from, const float *to, const hg_geom *geoms,
                                   const size_t *out_offsets, int n_frames);
/* Parity tap: the n_frames x 8 doubles the pixel kernel uses (device-solved when the frames were given as point sets). */
int hg_get_geometric_matrices(hg_ctx *ctx, double *out, int n_frames);
int hg_warp_inverse_geometric_frames_device(hg_ctx *ctx, void *d_out);
int hg_warp_inverse_geometric_batch_device(hg_ctx *ctx, int kind, const double *m, const hg_geom *geoms,
                                           const size_t *out_offsets, int n_frames, void *d_out);
/* Packed output layout for n frames: offsets[i] = start of frame i (256-byte aligned), *total = bytes needed. */
int hg_pack_offsets(const hg_geom *geoms, int n_frames, size_t *offsets, size_t *total);

/* ------------------------------------------------------------------------------------------------ piecewise affine
 * Source side of the mesh, kept across frames like the reference's cached _srcPoints/_triangles/_minSrcX/_minSrcY
 * (:742, :758).  min_src_x/min_src_y are the rounded source-point bbox minimum used by the bounds test :1047.
 * Coordinates (source and destiny) may be NaN but not infinite or beyond 2^24 in magnitude: HG_ERR_INVALID (the
 * reference's fillTriangle row loop would run for as many rows as the triangle is tall -- forever for Infinity). */
int hg_piecewise_set_mesh(hg_ctx *ctx, const float *src_points, int n_points, const uint32_t *triangles, int n_triangles,
                          int min_src_x, int min_src_y);
/* Per-frame destination side = what setDestinyPoints + the head of _inversePiecewiseAffineWarp recompute every frame:
 * _calculatePiecewiseAffineTransformMatrices :785-804 (affineMatrixFromTriangles per triangle, f32),
 * inverseAffineMatrix per triangle :1036-1038, and the edge equations / row ranges of fillTriangle :1111-1151.
 * All on the device; dst_points are n_points x,y float32 in pixel coordinates. */
int hg_piecewise_prepare(hg_ctx *ctx, const float *dst_points, hg_geom geom);
/* _inversePiecewiseAffineWarp :1029-1058 for the prepared frame.  The triangle-index map of
 * _buildInverseTrianglesCorrespondencesMatrix :845-861 is not materialised: each output row's triangle spans
 * (fillTriangle/predictXLimits, with TypedArray.fill index semantics) are rebuilt in LDS and resolved per pixel with
 * "largest covering id wins", which equals the reference's sequential overwrite. */
int hg_warp_inverse_piecewise(hg_ctx *ctx, uint8_t *out_host);
int hg_warp_inverse_piecewise_device(hg_ctx *ctx, void *d_out);
/* F frames (F destination point sets on the mesh set above) in one pass: dst_points = F x n_points x 2 float32.
 * set_frames uploads points + windows (kept until replaced; hg_piecewise_prepare == set_frames with one frame);
 * frames_device runs the per-frame solves and the warp for all uploaded frames; batch_device = both.
 * set_frames does NOT wait for the GPU (the reference's loop calls setDestinyPoints before every warp, test/benchmark.js:107-110,
 * Homography.js:337-380): the caller's arrays are copied into page-locked staging owned by the ctx before it returns, the
 * uploads are ordered behind the queued runs on the ctx stream, and every queued run keeps the staged copy of the set it
 * warped, so that frames it flagged can still be redone by hg_sync after newer sets went up.  Up to 63 set / run pairs
 * queue between two hg_sync calls; the 64th settles the queue by itself. */
int hg_piecewise_set_frames(hg_ctx *ctx, const float *dst_points, const hg_geom *geoms, const size_t *out_offsets, int n_frames);
int hg_warp_inverse_piecewise_frames_device(hg_ctx *ctx, void *d_out);
int hg_warp_inverse_piecewise_batch_device(hg_ctx *ctx, const float *dst_points, const hg_geom *geoms,
                                           const size_t *out_offsets, int n_frames, void *d_out);
/* Frame sets whose frames bring their own SOURCE points -- the reference's loop
 *     for (f) { h.setSourcePoints(src_f); h.setDestinyPoints(dst_f); out_f = h.warp(image_f); }
 * (one image per frame through hg_set_images_device: each frame's landmarks live in its own image).  src_points = n_frames x
 * n_points x,y float32, the source side of frame f; triangles and n_points stay those of hg_piecewise_set_mesh, which must have been
 * called (HG_ERR_STATE otherwise).  min_src = n_frames x {minSrcX, minSrcY} int32, the values the bounds test :1047 uses for that
 * frame, passed explicitly like hg_piecewise_set_mesh's (a binding that mirrors the reference's caches hands over what its state
 * holds, stale values included); NULL = as a fresh instance would: the rounded bounding-box minimum of the frame's own source points
 * (:758, the rule of hg_minmax_xy; hg_piecewise_frame_min_src is that rule for one frame, on the host).
 * Frame f == _inversePiecewiseAffineWarp :1029-1058 with _srcPoints = src_f, _dstPoints = dst_f, the mesh's triangles,
 * _minSrcX/Y = min_src[f], image f % n_images and window geoms[f]: bit-identical in nearest mode, the bilinear rules above otherwise.
 * Everything downstream treats such a set like any other: hg_warp_inverse_piecewise_frames_device runs it, sets queue 63 deep
 * without a wait, flagged frames are redone at hg_sync from the staged copy of their own set (source points and minima included), and
 * with one frame the single-frame forms and taps (hg_warp_inverse_piecewise, _via_map, hg_get_tri_map[_fused], hg_get_matrices)
 * describe that frame.  A later hg_piecewise_set_frames / hg_piecewise_prepare returns to the mesh-wide source side; the forward
 * (scatter) entry points always use it.  HG_ERR_INVALID: NULL src_points / dst_points / geoms, n_frames <= 0, a source coordinate that
 * is infinite or beyond 2^24 in magnitude (NaN stays legal); a refused call leaves the ctx without a frame set.
 * Layout policy: the fast kernels need every frame's minima inside their ranges (|min| < 2^22), else the whole set takes the general
 * kernel; the high-dword bounds form needs every frame's minima >= 0. */
int hg_piecewise_set_frames_src(hg_ctx *ctx, const float *src_points, const int32_t *min_src, const float *dst_points,
                                const hg_geom *geoms, const size_t *out_offsets, int n_frames);
int hg_warp_inverse_piecewise_src_batch_device(hg_ctx *ctx, const float *src_points, const int32_t *min_src, const float *dst_points,
                                               const hg_geom *geoms, const size_t *out_offsets, int n_frames, void *d_out);
int hg_piecewise_frame_min_src(const float *src_points, int n_points, int32_t out[2]);
/* Parity taps (debug / tests): the Int16Array map the reference would have built for the prepared frame
 * (len = obj_w*obj_h), via the materialising kernel (atomicMax rasteriser) or via the fused kernel's own lookup;
 * and the per-triangle forward / inverse matrices (n_triangles x 6 float32 each; either may be NULL). */
int hg_get_tri_map(hg_ctx *ctx, int16_t *out, size_t len);
int hg_get_tri_map_fused(hg_ctx *ctx, int16_t *out, size_t len);
int hg_get_matrices(hg_ctx *ctx, float *fwd, float *inv);
/* Same warp through the materialised map (map build kernel + map-reading warp kernel).  Always available; it is also
 * what the library itself re-runs for a frame whose rows overflow the fused kernel's LDS span list. */
int hg_warp_inverse_piecewise_via_map(hg_ctx *ctx, uint8_t *out_host);

/* ------------------------------------------------------------------------------------------------ source fields and remaps
 * The geometry of an inverse warp without its pixels: callers that hold a mask, a depth or flow map, a label image or float features
 * beside the picture send those planes through exactly the picture's geometry by a gather (hg_remap_*), or hand the field to their own
 * code.  A field is computed from the f64 source coordinate (sx, sy) of the loops :997-1011 / :1042-1056 -- JS operation order, contraction
 * off, the very value the warp kernels round -- and the coverage test of the loop (:1001; :1045-1047 with the frame's minSrc for piecewise).
 *   HG_FIELD_INDEX   one int32 per output pixel: the flat PIXEL index Math.round(sy) * W + Math.round(sx) the nearest loop reads (:1005 /
 *                    :1049; no minSrc subtraction) where the pixel passes the coverage test AND the index lies in [0, W*H); else -1 (no
 *                    triangle, a coordinate out of bounds or NaN, or an index outside the array, which JS reads as undefined -> 0).  Hence
 *                        out32[i] = idx[i] >= 0 ? img32[idx[i]] : 0
 *                    IS the nearest warp, byte for byte, the reference's wrap of sx in [W - 0.5, W) into the next row included.  With
 *                    hg_set_images_device the index of frame f is relative to image f % n_images.  A source of 2^31 pixels or more:
 *                    HG_ERR_INVALID for this format.
 *   HG_FIELD_COORDS  two float32 per output pixel, interleaved (sx, sy): the f64 coordinate rounded ONCE to f32, for every pixel that
 *                    passes the coverage test; every other pixel holds 0x7fc00000 (a quiet NaN, that exact pattern) in both words.  A
 *                    covered pixel whose index falls outside the array is still covered here: index >= 0 implies "not NaN", not the
 *                    other way round.  A coordinate just below W may round to W itself in f32 (likewise H): consumers clamp their taps,
 *                    as hg_remap_bilinear_f32_device does.
 * Both are independent of hg_set_sampling: the mode is neither read nor changed.  Field calls leave hg_last_piecewise_kernel / _variant /
 * _self, hg_last_geometric_kernel, hg_last_forward_kernel and the layout the policy learned for the mesh as they found them.
 * Layout: frame f is row-major obj_w x obj_h at field_offsets[f] bytes into d_field (NULL: packed as hg_pack_field_offsets does; the RGBA
 * out_offsets of the frame set play no part); offsets are multiples of the pixel size (4 / 8 bytes; HG_ERR_INVALID otherwise), d_field is
 * aligned to 16 bytes or more (any hg_device_alloc / hipMalloc pointer).  Bytes between frames are never written; empty frames write nothing.
 * HG_ERR_INVALID: unknown format, NULL pointers.  HG_ERR_STATE: no source image (its size is needed), no mesh, no frame set. */
/* Host only: offsets[i] = start of frame i's field (256-byte aligned), *total = bytes needed; 4 (index) or 8 (coords) bytes per pixel. */
int hg_pack_field_offsets(const hg_geom *geoms, int n_frames, int format, size_t *offsets, size_t *total);
/* The field of hg_warp_inverse_geometric(kind, m, geom): synchronous into host memory, or asynchronous into GPU memory.  Neither touches
 * a staged frame set. */
int hg_field_inverse_geometric(hg_ctx *ctx, int kind, const double *m, hg_geom geom, int format, void *out_host);
int hg_field_inverse_geometric_device(hg_ctx *ctx, int kind, const double *m, hg_geom geom, int format, void *d_field);
/* ... of the staged set of hg_geometric_set_frames[_points], all frames in one launch (point sets: the matrices are solved on the device
 * first, as at the head of every warp of the set).  Asynchronous. */
int hg_field_inverse_geometric_frames_device(hg_ctx *ctx, int format, const size_t *field_offsets, void *d_field);
/* The field of hg_warp_inverse_piecewise for the prepared frame (exactly one frame staged), into host memory. */
int hg_field_inverse_piecewise(hg_ctx *ctx, int format, void *out_host);
/* ... of the staged set of hg_piecewise_set_frames / _set_frames_src / hg_piecewise_prepare; per-frame source points and min_src are
 * honoured.  Runs on the general path and is SETTLED INSIDE THE CALL, as bilinear piecewise warps are: queued warp runs are settled first
 * (they keep their own results); a frame with a row of more than 1024 spans, or with irregular triangles, is only flagged by the kernel and
 * redone through the materialised map before the call returns (counted in hg_redone_frames).  The field is final on return. */
int hg_field_inverse_piecewise_frames_device(hg_ctx *ctx, int format, const size_t *field_offsets, void *d_field);
/* out[i] = 0 <= field[i] < n_src_px ? src[field[i]] : all-zero, for i < n_px, pixels being opaque blocks of pixel_bytes = 1, 2, 4, 8 or 16
 * bytes (anything else: HG_ERR_INVALID); d_src and d_out aligned to the block size, d_field (int32) to 4 bytes.  Asynchronous on the ctx
 * stream.  No read ever leaves [0, n_src_px), whatever the field holds: caller-made fields are legal.  With 4-byte pixels and the RGBA
 * source this is the nearest warp. */
int hg_remap_index_device(hg_ctx *ctx, const void *d_field, size_t n_px, const void *d_src, size_t n_src_px, int pixel_bytes, void *d_out);
/* Bilinear gather of `channels` (1..4) interleaved float32 planes of a W x H source (W, H >= 1) through a HG_FIELD_COORDS field (or any
 * caller-made (sx, sy) list; 8-byte aligned).  Asynchronous on the ctx stream.  Pixel i: if sx or sy is NaN or infinite every channel is 0;
 * otherwise x0 = floorf(sx), fx = sx - x0, tap columns clamp(x0, 0, W-1) and clamp(x0 + 1.0f, 0, W-1), rows alike -- clamped in float before
 * the integer conversion, so that 1e30 is a legal coordinate -- and per channel in f32, contraction off,
 *     v = (p00*(1-fx) + p01*fx)*(1-fy) + (p10*(1-fx) + p11*fx)*fy,
 * stored as it is (no rounding, no clamping): the operation order of the bilinear sampling mode, so a float32 model matches bit for bit. */
int hg_remap_bilinear_f32_device(hg_ctx *ctx, const void *d_coords, size_t n_px, const float *d_src, int W, int H, int channels, float *d_out);
/* The same gather for 8-bit planes (a matte, a grey image, straight -- not premultiplied -- RGBA): taps and fractions are those of the f32
 * form, all in f32; each channel's four taps are converted to float and blended in the same operation order, contraction off, then
 *     out = (uint8)min(255, floor(v + 0.5f))          (the rounding of the bilinear sampling mode's blend4)
 * A NaN or infinite coordinate gives 0 in every channel.  d_coords is aligned to 8 bytes, d_src and d_out to nothing.  Asynchronous. */
int hg_remap_bilinear_u8_device(hg_ctx *ctx, const void *d_coords, size_t n_px, const uint8_t *d_src, int W, int H, int channels, uint8_t *d_out);
/* The remaps for a WHOLE FRAME SET in one launch: what a loop of n_frames single-list calls over the fields of a *_frames_device /
 * *_batch_device field call would do.  The geoms are passed explicitly and no staged frame set is consulted -- a forward field or a
 * caller-made one is as legal as an inverse one -- and only obj_w and obj_h of each are read: frame f is a flat list of obj_w * obj_h
 * pixels; a frame with obj_w <= 0 or obj_h <= 0 is empty and writes nothing.
 *   field_offsets  where frame f's field starts in d_field / d_coords, in bytes.  NULL: packed as hg_pack_field_offsets does for the format
 *                  the call reads; otherwise multiples of 4 (index) or 8 (coords).
 *   out_offsets    where frame f's output starts in d_out, in bytes.  NULL: packed as hg_pack_plane_offsets does with px_bytes =
 *                  pixel_bytes (index) or channels * element size (bilinear: 4 for HG_ELEM_F32, 1 for HG_ELEM_U8); otherwise multiples
 *                  of pixel_bytes resp. of the element size.
 *   planes         frame f reads plane f % n_planes (n_planes >= 1) at d_planes + (f % n_planes) * plane_stride_bytes: the rule
 *                  hg_set_images_device gives images.  plane_stride_bytes is a multiple of pixel_bytes resp. the element size; d_planes
 *                  and d_out are aligned as the single forms demand.
 * Per pixel the index form is exactly hg_remap_index_device with n_src_px pixels per plane -- no read leaves that plane's [0, n_src_px),
 * whatever the field holds --, the bilinear form exactly hg_remap_bilinear_f32_device (elem HG_ELEM_F32) or hg_remap_bilinear_u8_device
 * (HG_ELEM_U8), bit for bit.  Bytes between frames are never written.  n_frames == 0: HG_OK, nothing happens.
 * HG_ERR_INVALID: n_frames negative or above 65535; NULL pointers with n_frames > 0; an unknown elem; channels outside 1..4; pixel_bytes
 * not 1, 2, 4, 8 or 16; W or H below 1; n_planes below 1; a misaligned pointer, offset or stride.
 * Asynchronous on the ctx stream: geoms and offsets are copied before the call returns, the frame table goes up through page-locked staging,
 * stream-ordered; no GPU wait in the steady state.  Before launching, queued runs whose deferred redo could land on the bytes the call
 * writes in d_out are settled, as the field calls do.  Source planes that are themselves outputs of queued warps are the caller's to settle
 * (hg_sync) -- the contract of the single remaps, which settle nothing.  Like the field calls, none of the remaps touches hg_last_*_kernel,
 * the sampling mode or the layout state. */
/* Host only: offsets[i] = start of frame i's OUTPUT plane (256-byte aligned), *total = bytes needed; px_bytes = bytes per output pixel (>= 1). */
int hg_pack_plane_offsets(const hg_geom *geoms, int n_frames, size_t px_bytes, size_t *offsets, size_t *total);
int hg_remap_index_frames_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                                 const void *d_field, const size_t *field_offsets,
                                 const void *d_planes, size_t n_src_px, int n_planes, size_t plane_stride_bytes,
                                 int pixel_bytes, void *d_out, const size_t *out_offsets);
int hg_remap_bilinear_frames_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                                    const void *d_coords, const size_t *field_offsets,
                                    const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes,
                                    int elem, int channels, void *d_out, const size_t *out_offsets);
/* MINIFICATION on the field seam: the mip pyramid of a plane and a trilinear remap through it.  The remaps above read at most four source
 * pixels per output pixel, so a shrink aliases (a one-pixel checkerboard shrunk 8x comes out 0 / 255); the trilinear remap reads the pyramid
 * level(s) that match the field's own footprint (the same checkerboard: 128 everywhere).  Planes are those of the bilinear remaps: `channels`
 * (1..4) interleaved elements per pixel, elem HG_ELEM_F32 or HG_ELEM_U8, W x H.
 * Level sizes: W_0 = W, H_0 = H, W_k = (W_{k-1} + 1) >> 1, H_k alike; the full pyramid has Lmax = 1 + ceil(log2(max(W, H))) levels, the last
 * one 1 x 1.  Level k >= 1, pixel (x, y), per channel: the taps are the level k-1 pixels at columns min(2x, W_{k-1}-1) and min(2x+1, W_{k-1}-1)
 * and rows alike, a b / c d;  u8: out = ((a + b) + (c + d) + 2) >> 2 in integers;  f32: out = ((a + b) + (c + d)) * 0.25f, in that order,
 * contraction off.
 * hg_pyramid_levels (host only): Lmax, or 0 for W or H < 1.
 * hg_pyramid_layout (host only): offsets[k], k = 1 .. levels-1, is the byte offset of level k inside ONE pyramid buffer: 256-byte aligned,
 * a level tightly packed, ascending; offsets[0] = 0 and is unused (level 0 is never copied: it stays the caller's plane); *total = the bytes
 * of one pyramid (0 for levels == 1).  levels must lie in 1..Lmax.  HG_ERR_INVALID: an unknown elem, channels outside 1..4, levels outside
 * 1..Lmax (W or H < 1 included), NULL offsets or total.
 * hg_pyramid_build_device: builds levels 1 .. levels-1 of every one of the n_planes planes (plane p at d_planes + p * plane_stride_bytes),
 * pyramid p going to d_pyr + p * pyr_stride_bytes in hg_pyramid_layout's layout.  Asynchronous on the ctx stream: one launch per level covers
 * all planes, each launch reading the level before it.  levels == 1: HG_OK, nothing happens.  d_planes, d_pyr and both strides are aligned
 * to the element size (the rules of hg_remap_bilinear_frames_device); pyr_stride_bytes >= *total.  The call settles nothing: source planes
 * that are outputs of queued warps are the caller's to settle (hg_sync), as for every remap.  HG_ERR_INVALID: what the layout refuses, W or H
 * or n_planes < 1, NULL or misaligned pointers, a misaligned or too small stride.
 * hg_remap_trilinear_frames_device: hg_remap_bilinear_frames_device's arguments, then the pyramids hg_pyramid_build_device made of the same
 * planes (d_pyr, pyr_stride_bytes; frame f reads pyramid f % n_planes) and the number of levels to use.  Offset defaults, the f % n_planes
 * rule, refusals, staging through the page-locked ring, "settle queued runs whose redo could land on d_out" and "no effect on hg_last_*, the
 * sampling mode or the layout state" are those of hg_remap_bilinear_frames_device.  Unlike the other remaps it reads a frame as a 2-D
 * obj_w x obj_h array, row-major.  Pixel (i, j) of a frame, (sx, sy) its f32 coordinate:
 *   1. sx or sy NaN or infinite: every channel is 0.
 *   2. Footprint, all in f32, contraction off.  Horizontal neighbour: pixel (i+1, j) if i+1 < obj_w and both its words are finite, otherwise
 *      pixel (i-1, j) under the same conditions, otherwise none; vertical neighbour likewise with j+1, then j-1.  For a neighbour (nx, ny):
 *      dx = nx - sx, dy = ny - sy, q_dir = dx*dx + dy*dy; a missing neighbour gives 0.  q = fmaxf(q_h, q_v); an overflow to +Inf is legal.
 *   3. Level.  !(q > 1.0f): level 0 only.  Otherwise e = the unbiased binary exponent of q (q = m 2^e, m in [1, 2)) and k = e >> 1;
 *      k >= levels-1: level levels-1 only; otherwise levels k and k+1 are blended with t = (ldexpf(q, -2k) - 1.0f) * 0.33333334f -- linear in
 *      the squared scale: 0 at a shrink factor of 2^k, approaching 1 at 2^(k+1).
 *   4. Sampling a level, per channel, unrounded f32: level 0 uses (sx, sy) as they are, level k >= 1 uses u = ((sx + 0.5f) * 2^-k) - 0.5f and
 *      v likewise from sy; then exactly the rule of hg_remap_bilinear_f32_device on W_k x H_k (floorf, fraction, both taps clamped in float
 *      before the integer conversion, (p00*(1-fx) + p01*fx)*(1-fy) + (p10*(1-fx) + p11*fx)*fy, u8 taps widened to float first).
 *   5. One level: r = v_k.  Two levels: r = v_k + (v_{k+1} - v_k) * t.  f32 stores r; u8 stores (uint8)min(255, floor(r + 0.5f)).
 * Hence with levels == 1, or a field that nowhere shrinks, the output IS hg_remap_bilinear_frames_device's, bit for bit (d_pyr may then be
 * NULL); a constant plane comes out constant; coordinates of 1e30 are legal.  HG_ERR_INVALID: levels outside 1..Lmax, d_pyr NULL with
 * levels > 1, a misaligned d_pyr or pyr_stride_bytes, and everything the bilinear frames form refuses.
 * Cost (MI355X, 64 frames out of 8 planes of 3840 x 2160, a 4x shrink and a projective set; EXPERIMENTS.md F.5): the pyramids of 8 such planes build in 0.11-0.16 ms
 * (1.7-2.3 TB/s of plane bytes); the trilinear remap takes 1.27-1.77 x the time of hg_remap_bilinear_frames_device on the same fields and planes. */
int hg_pyramid_levels(int W, int H);
int hg_pyramid_layout(int W, int H, int elem, int channels, int levels, size_t *offsets, size_t *total);
int hg_pyramid_build_device(hg_ctx *ctx, const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                            int levels, void *d_pyr, size_t pyr_stride_bytes);
int hg_remap_trilinear_frames_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                                     const void *d_coords, const size_t *field_offsets,
                                     const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes,
                                     int elem, int channels, void *d_out, const size_t *out_offsets,
                                     const void *d_pyr, size_t pyr_stride_bytes, int levels);
/* ANISOTROPIC remap on the field seam.  The trilinear rule chooses one footprint size, q = max(q_h, q_v), so a field that shrinks one axis
 * much more than the other (a plane seen obliquely) is blurred along the axis that did not need it: one-pixel vertical stripes shrunk 8x
 * vertically and not at all horizontally come out 128 everywhere.  hg_remap_aniso_frames_device takes up to max_aniso probes along the longer
 * of the field's two steps, each from the finer level(s) the shorter step allows, and averages them (the same stripes: the stripes).
 * Its arguments are hg_remap_trilinear_frames_device's, followed by max_aniso, which must lie in 1..16 (else HG_ERR_INVALID).  Offset
 * defaults, the f % n_planes rule, alignment rules and refusals, staging through the page-locked ring, "settle queued runs whose redo could
 * land on d_out" and "no effect on hg_last_*, the sampling mode, the plan or what the policy learned" are those of the trilinear form (one
 * host path serves both).  All of the rule is f32 in the written order, contraction off.  Pixel (i, j) of a frame read as obj_w x obj_h,
 * (sx, sy) its coordinate:
 *   1. sx or sy NaN or infinite: every channel is 0.
 *   2. Steps.  The horizontal neighbour is chosen exactly as trilinear step 2 chooses it: (i+1, j) if it exists and is finite, else (i-1, j)
 *      under the same conditions, else none.  hx = nx - sx, hy = ny - sy, q_h = hx*hx + hy*hy; a missing neighbour gives hx = hy = q_h = 0.
 *      The vertical neighbour likewise gives vx, vy, q_v.
 *   3. Axes.  q_h >= q_v: major (mx, my) = (hx, hy), qM = q_h, qm = q_v.  Otherwise the major is the vertical step, qM = q_v, qm = q_h.
 *   4. Probe count N.  !(qM > 1.0f), or qM not finite: N = 1.  Otherwise qm' = fmaxf(qm, 1.0f) (anisotropy never asks for detail finer than
 *      level 0) and N is the smallest n in 1..max_aniso with (float)(n*n) * qm' >= qM; if there is none, N = max_aniso.
 *   5. Level.  q' = qM / (float)(N*N), an IEEE division.  k, "one level or two" and t are trilinear step 3 applied to q' with `levels`.
 *   6. Probes.  N == 1: the single probe is (sx, sy) itself.  Otherwise, for p = 0..N-1: o = (((float)p + 0.5f) / (float)N) - 0.5f and probe p
 *      is (sx + mx*o, sy + my*o), multiply then add.  Each probe is sampled by trilinear steps 4 and 5: r_p = v_k, or v_k + (v_{k+1} - v_k) * t,
 *      unrounded f32 per channel.
 *   7. Average.  acc = r_0, then acc = acc + r_p in ascending p; r = acc / (float)N.  f32 stores r; u8 stores (uint8)min(255, floor(r + 0.5f)).
 * Hence: with max_aniso == 1 the output IS hg_remap_trilinear_frames_device's, bit for bit (N is 1, q' = qM = max(q_h, q_v), acc / 1 is
 * exact); hence with max_aniso == 1 and levels == 1, or, whatever max_aniso is, where the field nowhere shrinks (every N is 1), it is
 * hg_remap_bilinear_frames_device's (levels == 1 with more probes averages bilinear samples of the plane); a constant u8 plane stays
 * constant; coordinates of 1e30 and steps that overflow are legal, and no tap leaves a level.
 * Cost (MI355X, 64 frames out of 8 planes of 3840 x 2160; EXPERIMENTS.md F.6): where every pixel takes one probe (max_aniso = 1, or an
 * isotropic 4x shrink at any max_aniso) the anisotropic remap takes 1.24-1.31 x the time of hg_remap_trilinear_frames_device on the same
 * fields, planes and pyramids; 1.99-2.30 x on a projective set whose pixels take 2 probes; 2.92-4.16 x on an 8x-by-1x shrink (8 probes from
 * level 0, or 4 from two levels with max_aniso = 4). */
int hg_remap_aniso_frames_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                                 const void *d_coords, const size_t *field_offsets,
                                 const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes,
                                 int elem, int channels, void *d_out, const size_t *out_offsets,
                                 const void *d_pyr, size_t pyr_stride_bytes, int levels, int max_aniso);
/* MAGNIFICATION on the field seam: a bicubic remap.  The bilinear remap enlarges with a tent filter: a plane enlarged 3-4x is blurred and shows
 * a kink at every source pixel.  hg_remap_bicubic_frames_device blends 4 x 4 taps with the weights of the (B, C) family of cubics (Mitchell and
 * Netravali): (0, 0.5) is Catmull-Rom, (1/3, 1/3) Mitchell, (1, 0) the cubic B-spline.  A 64 x 64 f32 plane 100 sin(2 pi x / 8) cos(2 pi y / 10)
 * enlarged 4x (pixel centres aligned, the clamped border left out) differs from the function itself by 4.35 RMS through the bilinear remap, 0.49
 * through Catmull-Rom, 2.89 through Mitchell.
 * Its arguments are hg_remap_bilinear_frames_device's, followed by B and C.  Argument meaning, offset defaults (hg_pack_field_offsets /
 * hg_pack_plane_offsets), the f % n_planes rule, alignment rules and refusals, n_frames == 0 (HG_OK, nothing happens), staging of the frame
 * table through the page-locked ring, "settle queued runs whose redo could land on d_out" and "no effect on hg_last_*, the sampling mode, the
 * plan, what the policy learned or staged frame sets" are those of the bilinear frames form (one host path serves both).  In addition
 * HG_ERR_INVALID: B or C NaN or outside [0, 1]; the error text names the parameter.
 * All of the rule is f32 in the written order, contraction off, except the coefficients.  Pixel i of a frame's flat list, (sx, sy) its coordinate:
 *   1. sx or sy NaN or infinite: every channel is 0.
 *   2. Coefficients, once per call on the host, in double from (double)B and (double)C, each rounded once to f32:
 *        p3 = ((12 - 9B) - 6C)/6    p2 = ((-18 + 12B) + 6C)/6    p0 = (6 - 2B)/6
 *        q3 = (-B - 6C)/6    q2 = (6B + 30C)/6    q1 = (-12B - 48C)/6    q0 = (8B + 24C)/6
 *      Catmull-Rom's seven are exact: 1.5, -2.5, 1, -0.5, 2.5, -4, 2.
 *   3. Fractions: x0 = floorf(sx), fx = sx - x0; y0 and fy likewise (the bilinear remap's).
 *   4. Weights for t = fx (and t = fy):  near(x) = (((p3*x) + p2)*x)*x + p0,  far(x) = ((((q3*x) + q2)*x) + q1)*x + q0;
 *      w0 = far(1.0f + t), w1 = near(t), w2 = near(1.0f - t), w3 = far(2.0f - t).
 *   5. Taps: columns clamp(x0 - 1.0f), clamp(x0), clamp(x0 + 1.0f), clamp(x0 + 2.0f) into 0..W-1, every sum formed in f32 and clamped in float
 *      before the integer conversion; rows likewise with y0 and H.  No read leaves the plane; 1e30 is a legal coordinate; W = 1 or H = 1 is legal.
 *   6. Blend per channel, u8 taps widened to float first.  Row n = 0..3 with its taps p[n][0..3]:
 *        h_n = ((p[n][0]*wx0 + p[n][1]*wx1) + p[n][2]*wx2) + p[n][3]*wx3;   then   r = ((h_0*wy0 + h_1*wy1) + h_2*wy2) + h_3*wy3.
 *   7. f32 stores r; u8 stores (uint8)fminf(255.0f, fmaxf(0.0f, floorf(r + 0.5f))) -- the lower clamp is this remap's own: the cubic has negative
 *      lobes, so r can lie below 0 (and above 255) beside an edge.
 * Hence: with Catmull-Rom, a finite coordinate with integer sx in [0, W-1] and integer sy in [0, H-1] gives the source pixel bit for bit (the
 * weights are exactly 0, 1, 0, 0), which is also hg_remap_bilinear_frames_device's pixel there; a constant u8 plane stays constant for every
 * admissible (B, C) (the weight sums differ from 1 by less than 1.1e-6); f32 planes holding NaN or Inf give unspecified payloads.
 * The filter reads level 0 only: where the field shrinks it aliases as the bilinear remap does -- hg_remap_trilinear_frames_device and
 * hg_remap_aniso_frames_device are the forms for shrinking.
 * Cost (MI355X, 64 frames of 3840 x 2160 enlarged 4x out of 8 planes of 960 x 540, and a projective enlargement; EXPERIMENTS.md F.9):
 * medians of 31 regions, every named cubic alike: u8 x 4 planes take 2.20-2.29 x the time of hg_remap_bilinear_frames_device on the same fields and
 * planes (6.57 ms against 2.86 ms for the 4x set, 323 GB/s of output), f32 x 1 planes 1.25-1.59 x (2.11 ms against 1.69 ms, 1.0 TB/s of output) -- four
 * times the taps; the byte kernel pays for unpacking and blending 64 channel taps per pixel, not for memory. */
int hg_remap_bicubic_frames_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                                   const void *d_coords, const size_t *field_offsets,
                                   const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes,
                                   int elem, int channels, void *d_out, const size_t *out_offsets,
                                   float B, float C);
/* MOSAIC on the field seam: the frames of a set blended into ONE canvas on the device (a panorama, a stack of aligned exposures, a
 * stabilised clip pasted on one picture).  Every warp and remap above leaves F frames, each in its own window of destination space;
 * hg_mosaic_frames_device joins them, so that only the canvas has to come down.
 *   geoms[f]        ALL FOUR words are read: pixel (i, j) of frame f lies at destination position (x_off + i, y_off + j); obj_w <= 0 or
 *                   obj_h <= 0 is an empty frame.
 *   d_coords,       the frames' HG_FIELD_COORDS fields under hg_remap_bilinear_frames_device's rules (NULL offsets: packed as
 *   field_offsets   hg_pack_field_offsets packs; otherwise multiples of 8; d_coords aligned to 8 bytes).  A frame pixel COVERS iff both words
 *                   of its coordinate are finite.  Caller-made fields are legal, 1e30 included.
 *   d_frames,       the frames' pixels: `channels` (1..4) interleaved elements of `elem` (HG_ELEM_F32 / HG_ELEM_U8), row-major obj_w x obj_h.
 *   frame_offsets   NULL: packed as hg_pack_plane_offsets packs with px_bytes = channels * element size -- with u8 x 4 the default layout of
 *                   the RGBA warps, whose output is a legal input as it stands; otherwise multiples of the element size.
 *   W, H            >= 1, the source's size: read only by HG_MOSAIC_FEATHER; no ctx state is consulted.
 *   canvas          a window of the same destination space.  d_canvas receives obj_w x obj_h pixels of the frames' elem / channels, tightly
 *                   packed, and EVERY pixel is written.  d_weight may be NULL; otherwise one float32 per canvas pixel (below).
 * The hg_geom limits apply to canvas and to every frame.  All arithmetic is f32 in the written order, contraction off.  Canvas pixel (i, j):
 *   1. X = canvas.x_off + i, Y = canvas.y_off + j (64-bit integers).
 *   2. Frame f is a CANDIDATE iff it is not empty and 0 <= u < obj_w, 0 <= v < obj_h for u = X - x_off_f, v = Y - y_off_f.
 *   3. A candidate is a CONTRIBUTOR iff the coordinate (sx, sy) at (u, v) of its field covers.  p_c is channel c of its pixel at (u, v),
 *      widened to float for u8.
 *   4. No contributor: every channel is 0, the weight is 0.
 *   5. HG_MOSAIC_LAST: the pixel of the contributor with the largest f, copied bit for bit (painter's order); weight 1.0f.
 *   6. HG_MOSAIC_MEAN: w_f = 1.0f.  HG_MOSAIC_FEATHER: dx = fminf(sx + 1.0f, (float)W - sx), dy = fminf(sy + 1.0f, (float)H - sy),
 *      w_f = fmaxf(fminf(fminf(dx, dy), feather), 0x1p-10f) -- under the geometric coverage test 0 <= sx < W "source pixels to the nearest
 *      border, counting this one", capped at feather (+Inf: uncapped); the floor keeps every contributor's weight positive (piecewise
 *      frames test against the minSrc bounds, and a coordinate may round to W in f32).
 *   7. MEAN / FEATHER: in ascending f, acc_c = acc_c + w_f * p_c (multiply, then add) and wsum = wsum + w_f, both from 0.0f.  EXACTLY ONE
 *      contributor: r_c = p_c of that contributor, bit for bit (no multiply, no divide: a mosaic of frames that do not overlap is a paste).
 *      Otherwise r_c = acc_c / wsum, an IEEE division.  f32 stores r_c; u8 stores (uint8)min(255, floor(r_c + 0.5f)).  Weight = wsum.
 * n_frames == 0 is legal: the canvas is zeroed, and geoms / d_coords / d_frames may be NULL.  An empty canvas: HG_OK, nothing is written.
 * HG_ERR_INVALID: n_frames negative or above 65535; d_canvas NULL; geoms / d_coords / d_frames NULL with n_frames > 0; an unknown elem or
 * mode; channels outside 1..4; W or H < 1; in HG_MOSAIC_FEATHER mode a feather that is NaN or <= 0 (ignored otherwise); misaligned pointers
 * or offsets (8 for the coordinates, the element size for frames and canvas, 4 for d_weight); a canvas or a frame beyond the hg_geom limits.
 * Asynchronous on the ctx stream; the frame table goes up through the page-locked staging ring as the frames remaps' does; queued runs whose
 * deferred redo could land on d_canvas or d_weight are settled first; frames or fields that are outputs of queued warps are the caller's to
 * settle (hg_sync), as for every remap.  No effect on hg_last_*, the sampling mode, the plan, what the policy learned or staged frame sets.
 * Cost (MI355X; EXPERIMENTS.md F.7): u8 x 4 frames with the weight plane, medians of 31 regions.  64 frames with identical 3840 x 2160 windows: MEAN 1.58 ms,
 * FEATHER 1.59 ms -- 0.54-0.55 x the time of hg_remap_bilinear_frames_device over the same frames and fields, 2.0 x the byte floor (coordinates and
 * pixels of every candidate once plus the canvas, at 8 TB/s) --, LAST 0.17 ms (it reads one frame).  A strip of 16 frames of 1920 x 1080, each shifted
 * by 60 % of its width (canvas 19200 x 1080): LAST 0.18, MEAN 0.24, FEATHER 0.24 ms, 0.93-1.24 x that remap, 3.0-4.0 x the floor.  Every block walks the
 * whole frame table: 4096 frames of 128 x 128 over a 4K canvas take 8.3 / 15.8 / 15.8 ms, 4-8 x that remap -- thousands of small frames are not what
 * this kernel is laid out for. */
enum { HG_MOSAIC_LAST = 0, HG_MOSAIC_MEAN = 1, HG_MOSAIC_FEATHER = 2 };
int hg_mosaic_frames_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                            const void *d_coords, const size_t *field_offsets,
                            const void *d_frames, const size_t *frame_offsets,
                            int elem, int channels, int W, int H,
                            int mode, float feather,
                            hg_geom canvas, void *d_canvas, float *d_weight);
/* EXPOSURE of a mosaic: one gain per frame, fitted on the overlaps (Brown & Lowe, "Automatic Panoramic Image Stitching using Invariant
 * Features", section 6).  The frames of a panorama were taken at different moments: auto-exposure, vignetting and white balance leave the same
 * surface 10-25 % brighter in one frame than in its neighbour, which HG_MOSAIC_MEAN shows as a step at every window border and
 * HG_MOSAIC_FEATHER as a ramp between two sides of different brightness.  Three entries, none of which brings a frame down:
 * hg_mosaic_overlap_stats_device measures the overlaps on the device, hg_mosaic_solve_gains solves a small system on the host, and
 * hg_mosaic_frames_gain_device applies one factor per frame while it blends.
 *
 * hg_mosaic_overlap_stats_device: geoms, d_coords, field_offsets, d_frames, frame_offsets, channels and canvas mean exactly what they mean in
 * hg_mosaic_frames_device (packing defaults, alignment rules, hg_geom limits).  Elements are HG_ELEM_U8 only: the sums are integers, so the
 * result is exact and identical from run to run.  d_stats: n_frames x n_frames x 2 64-bit words, aligned to 8 bytes; the call zeroes them itself.
 *   CONTRIBUTOR is steps 1-3 above, unchanged.  The INTENSITY of frame a at a canvas pixel is v_a = sum of p_c over its STAT CHANNELS:
 *   channels 0..2 when channels == 4 (alpha takes no part), all channels otherwise.  For every ordered pair (a, b), diagonal included, over all
 *   canvas pixels where a and b both contribute:
 *     stats[(a * F + b) * 2 + 0] = N_ab, the number of such pixels;
 *     stats[(a * F + b) * 2 + 1] = S_ab, the sum of v_a over them.
 *   N is symmetric, N_aa is the area a covers on the canvas and S_aa is a's own sum.
 * n_frames is 0..256 (1 MiB of statistics).  n_frames == 0 and an empty canvas return HG_OK: the n_frames^2 pairs are zeroed, none are written
 * for F = 0.  HG_ERR_INVALID: the mosaic's list, and n_frames > 256; d_stats NULL with n_frames > 0, or misaligned; channels outside 1..4.
 * Asynchronous on the ctx stream; queued runs whose deferred redo could land on d_stats are settled first; no effect on hg_last_*, the
 * sampling mode, the plan, what the policy learned or staged frame sets -- the mosaic's guarantees.
 *
 * hg_mosaic_solve_gains (host, double precision, no context): k = the number of stat channels, I_ab = S_ab / (k N_ab) on the 0..255 scale where
 * N_ab > 0, alpha = 1 / sigma_n^2, beta = 1 / sigma_g^2.  Over the frames with N_aa > 0 it solves A g = b, the normal equations of the error
 *     1/2 sum_a sum_b N_ab [ (g_a I_ab - g_b I_ba)^2 alpha [a != b] + (1 - g_a)^2 beta ]:
 *     A_aa = beta sum_b N_ab + 2 alpha sum_{b != a} N_ab I_ab^2,   A_ab = -2 alpha N_ab I_ab I_ba (a != b),   b_a = beta sum_b N_ab
 * (the sums over b include b = a), by a Cholesky factorisation in index order, and rounds once to f32.  A frame with N_aa = 0 gets 1.0f.
 * The paper's sigma_n = 10 (intensity error, 0..255 scale) and sigma_g = 0.1 (gain prior) are the usual choice; there are no defaults here.
 * HG_ERR_INVALID: sigma_n or sigma_g not finite or <= 0; n_frames outside 0..256; channels outside 1..4; a NULL pointer with n_frames > 0;
 * statistics that are not symmetric in N; a solution with a gain that is not finite and positive.
 *
 * hg_mosaic_frames_gain_device: every argument of hg_mosaic_frames_device in its order, then gains: n_frames floats on the HOST, or NULL.
 * With gains == NULL the call IS hg_mosaic_frames_device: the same kernel, the same bytes.  With gains every value of p_c on a STAT CHANNEL in
 * steps 5-7 becomes q_c = g_f * p_c, one f32 multiply before anything else; channel 3 of a 4-channel frame passes unscaled.  HG_MOSAIC_LAST and
 * the exactly-one-contributor case store q_c -- u8: (uint8)min(255, floor(q_c + 0.5f)) --, the accumulation is acc_c = acc_c + w_f * q_c;
 * weights and the weight plane do not change.  A gain of exactly 1.0f therefore reproduces the ungained bytes.  f32 planes have no exposure
 * statistics, but may be given gains of the caller's own.  HG_ERR_INVALID: the mosaic's list, and a gain that is not finite and > 0.  The gains
 * go up behind the frame table in the same staged upload, as an array of their own.
 * Cost (MI355X; EXPERIMENTS.md F.10): u8 x 4 frames, medians of 31 regions.  64 frames with identical 3840 x 2160 windows (4096 ordered pairs):
 * statistics 4.15 ms, 2.55 x the HG_MOSAIC_MEAN mosaic of the same frames (1.63 ms) -- per frame and tile it issues three vector loads to the
 * mosaic's two and 1.8 x its instructions, and waits 3.3 x as long on them; not memory.  A strip of 16 frames of 1920 x 1080 shifted by 60 % of
 * their width: 0.27 ms, 1.13 x (0.24 ms).  256 frames of 128 x 128 over a 4K canvas: 0.20 ms, 0.20 x.  The gained MEAN and FEATHER mosaics take
 * 1.01-1.04 x the plain ones.  Statistics, 16 F^2 bytes down, host solve and gained mosaic together: 5.9 / 0.58 / 2.2 ms of wall time, 3.6 / 2.3 /
 * 2.2 x one plain mosaic. */
int hg_mosaic_overlap_stats_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                                   const void *d_coords, const size_t *field_offsets,
                                   const void *d_frames, const size_t *frame_offsets,
                                   int channels, hg_geom canvas, uint64_t *d_stats);
int hg_mosaic_solve_gains(const uint64_t *stats, int n_frames, int channels,
                          double sigma_n, double sigma_g, float *gains);
int hg_mosaic_frames_gain_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                                 const void *d_coords, const size_t *field_offsets,
                                 const void *d_frames, const size_t *frame_offsets,
                                 int elem, int channels, int W, int H,
                                 int mode, float feather,
                                 hg_geom canvas, void *d_canvas, float *d_weight,
                                 const float *gains);
/* ROBUST mosaic: an order statistic per canvas pixel in the place of a weighted mean, for a stack of aligned exposures (a tripod burst, a
 * stabilised clip, the overlaps of a panorama).  A walking person, a car or a waving flag covers a pixel in a minority of the frames, so it
 * is not in the median or the trimmed mean of the contributors: no mask, threshold or tuning.  HG_ROBUST_MIN and HG_ROBUST_MAX are the
 * dark-frame and star-trail variants.
 *
 * hg_mosaic_robust_device: geoms, d_coords, field_offsets, d_frames, frame_offsets, channels, canvas, d_canvas and d_weight mean exactly what
 * they mean in hg_mosaic_frames_device (packing defaults, alignment rules, hg_geom limits, EVERY canvas pixel is written, the empty canvas);
 * gains is n_frames floats on the HOST, or NULL, and means what it means in hg_mosaic_frames_gain_device.  There is no W, H: nothing here
 * feathers.  Elements are HG_ELEM_U8 only, as for hg_mosaic_overlap_stats_device and for the same reason: every rule below is integer
 * arithmetic, so the result is exact and identical from run to run.  f32 planes are out of scope.  n_frames is 0..256.  Canvas pixel (i, j):
 *   1. Candidates and contributors are steps 1-3 of hg_mosaic_frames_device.  n is the number of contributors.
 *   2. The value of contributor f on channel c is x = p_c without gains; with gains the byte min(255, floor(g_f * (float)p_c + 0.5f)) on the
 *      STAT CHANNELS (one f32 multiply, rounded as hg_mosaic_frames_gain_device rounds what it stores), channel 3 of a 4-channel frame
 *      unscaled.  A gained value is a byte again BEFORE it is ranked.
 *   3. Every channel is ranked on its own: its n values in ascending order are s_0 <= ... <= s_{n-1}.  Alpha is a channel like any other.
 *      The result may therefore be a colour that no single frame held.
 *   4. n == 0: every channel 0, weight 0.  HG_ROBUST_MIN: s_0.  HG_ROBUST_MAX: s_{n-1}.  HG_ROBUST_MEDIAN: s_{(n-1)/2} for odd n,
 *      (s_{n/2-1} + s_{n/2} + 1) >> 1 for even n.  HG_ROBUST_TRIMMED: t = min((int)(trim * (float)n), (n - 1) / 2) with the product as one
 *      f32 multiply, truncated; m = n - 2 t; S = s_t + ... + s_{n-1-t} as an integer; the result is (2 S + m) / (2 m) in integer division
 *      (S / m rounded to nearest, halves up).  Weight = (float)n in every mode.
 *   5. Hence: ONE contributor gives that contributor's (gained) bytes in every mode, so frames that do not overlap give a paste, equal to
 *      HG_MOSAIC_LAST.  HG_ROBUST_TRIMMED with trim == 0 and no gains equals HG_MOSAIC_MEAN on u8 byte for byte, weight plane included:
 *      there t = 0, m = n, and the mean's accumulator holds S exactly (integers below 2^24).  The exact quotient S / n is a multiple of 1 / n,
 *      a rounding boundary k + 1/2 a multiple of 1/2, so unless they coincide they lie at least 1 / (2 n) >= 1/512 apart, far beyond the errors
 *      of the f32 division of values below 65536 and of the addition of 0.5f (at most 2^-17 each); where they coincide both are exact.  The mean's
 *      floor(acc / wsum + 0.5f) is therefore this entry's (2 S + n) / (2 n).
 * n_frames == 0 zeroes the canvas (geoms / d_coords / d_frames / gains may be NULL).  An empty canvas: HG_OK, nothing is written.
 * HG_ERR_INVALID, in this order: the mosaic's own list in its order -- n_frames negative (or above 65535); d_canvas NULL; channels outside
 * 1..4; geoms / d_coords / d_frames NULL with n_frames > 0; a misaligned d_coords (8) or d_weight (4); a canvas or a frame beyond the hg_geom
 * limits; field offsets that are no multiples of 8 --; n_frames > 256; an unknown mode; in HG_ROBUST_TRIMMED mode a trim that is NaN or
 * outside [0, 0.5) (ignored otherwise); a gain that is not finite and > 0.
 * Asynchronous on the ctx stream; the frame table goes up through the page-locked staging ring as the frames remaps' does, the gains behind
 * it in the same upload; queued runs whose deferred redo could land on d_canvas or d_weight are settled first; frames or fields that are
 * outputs of queued warps are the caller's to settle (hg_sync), as for every remap.  No effect on hg_last_*, the sampling mode, the plan,
 * what the policy learned or staged frame sets.
 * How (hg_k_robust.hip): a selection, not a sort.  A tile of 64 x 4 canvas pixels lists the frames whose window meets it; up to
 * HG_ROBUST_LMAX listed frames have their contributors staged in LDS from ONE walk of global memory (a launch allocates 16, 32 or 64 slots
 * by n_frames: LDS bounds the waves a CU holds), more are walked again per round; the
 * ranks are resolved bit by bit from bit 7 down, 8 rounds of counting for all channels at once; pixels with one or two contributors need none.
 * Cost (MI355X; EXPERIMENTS.md "Robust mosaic"; tools/bench_robust.py): u8 x 4 frames with the weight plane, medians of 25 regions, as ratios to
 * HG_MOSAIC_MEAN on the same frames in the same process and to the byte floor (coordinates and pixels of every candidate once, canvas and weights,
 * at 8 TB/s).  64 frames with identical 3840 x 2160 windows (64 contributors per pixel, staged; mean 1.57 ms): MEDIAN 8.38 ms, 5.3 x the mean, 10.4 x
 * the floor; TRIMMED 8.83 ms, 5.6 x; MIN / MAX 8.34 ms, 5.3 x.  Built with a cap of 32 the same frames are walked in global memory per round and
 * MEDIAN takes 21.8 ms, 13.8 x.  A strip of 16 frames of 1920 x 1080 shifted by 60 % of their width (1-2 contributors, no rounds): every mode 0.28 ms,
 * 1.17 x the mean (0.24 ms), 4.0 x the floor.  256 frames of 128 x 128 over a 4K canvas (at most 3 contributors): 0.36 ms, 0.35 x the mean (1.02 ms),
 * which walks all 256 records in every tile where this kernel walks its list. */
#ifndef HG_ROBUST_LMAX
#define HG_ROBUST_LMAX 64       /* frames hitting one 64 x 4 tile that are staged in LDS; beyond it the tile re-walks them (slower, as correct) */
#endif
enum { HG_ROBUST_MEDIAN = 0, HG_ROBUST_TRIMMED = 1, HG_ROBUST_MIN = 2, HG_ROBUST_MAX = 3 };
int hg_mosaic_robust_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                            const void *d_coords, const size_t *field_offsets,
                            const void *d_frames, const size_t *frame_offsets,
                            int channels, int mode, float trim, const float *gains,
                            hg_geom canvas, void *d_canvas, float *d_weight);
/* MULTI-BAND blending of a mosaic (Brown & Lowe, section 7, after Burt & Adelson): low frequencies are blended over a wide range and high
 * frequencies over a narrow one, so exposure differences fade across a seam while detail comes from one frame only -- no step as with
 * HG_MOSAIC_LAST / HG_MOSAIC_MEAN, no ghosting as with HG_MOSAIC_FEATHER.  As a by-product it yields the SEAM LABEL MAP: which frame owns
 * each canvas pixel.
 *
 * hg_mosaic_multiband_device: the arguments up to canvas, d_canvas and d_weight mean exactly what they mean in hg_mosaic_frames_gain_device
 * (packing defaults, alignment rules, hg_geom limits, gains on the HOST or NULL, a gain of exactly 1.0f == no gain).  feather is the cap of
 * HG_MOSAIC_FEATHER (> 0, +Inf: uncapped) and RANKS the frames here; n_bands is 1..8; d_labels may be NULL, otherwise one int32 per canvas
 * pixel, aligned to 4 bytes; d_work is the caller's scratch, aligned to 256 bytes, of at least the work_bytes hg_mosaic_multiband_layout
 * returns for the same geoms, canvas, channels and n_bands.  The library allocates nothing, as with d_pyr.
 * All arithmetic is f32 in the written order, contraction off.  L = n_bands, A = 2^(L-1).
 *   1. CONTRIBUTORS AND LABELS.  Per canvas pixel, candidates and contributors are steps 1-3 of hg_mosaic_frames_device.  A contributor's
 *      rank is the HG_MOSAIC_FEATHER weight w_f of step 6 (the same expression, cap and 2^-10 floor).  The LABEL is the contributor with the
 *      largest w_f, the lowest f among equals; -1 without a contributor.  d_labels receives it.
 *   2. LEVEL GRIDS.  x = X - canvas.x_off is the level-0 coordinate of a position (y alike); position x of level k stands for x 2^k of
 *      level 0.  Level k of the CANVAS covers [-(A >> k), (A ceil(cw / A) + A) >> k) in x, and likewise in y.  A frame TAKES PART iff its
 *      window meets the canvas window, in [a0, a1) x [b0, b1) of canvas-relative coordinates; frame pixels outside the canvas are not read.
 *      Its level-0 grid is [A (floor(a0 / A) - 1), A (ceil(a1 / A) + 1)) in x, likewise in y: aligned to A with a margin of A, so every
 *      level-k grid is the level-0 grid shifted right by k, and the grids of different frames coincide pixel for pixel.  Every array below is
 *      0.0f outside its grid.
 *   3. LEVEL 0 of frame f: I_f,0,c(x) = q_c if f contributes at x, else 0.0f, with q_c = g_f * p_c on the stat channels (the alpha of 4
 *      channels unscaled; one multiply by 1.0f without gains); M_f,0(x) = 1.0f iff the label at x is f, else 0.0f.  Neither is stored as
 *      floats: "contributes" and "is the label" are two bits of one byte per grid pixel in the work area.
 *   4. REDUCE, k -> k + 1, images and weights alike: for output (x, y) the taps are t[j][i] = in(2x + i - 2, 2y + j - 2), i, j = 0..4;
 *      r_j = ((t0 + t4) + (t1 + t3) * 4.0f) + t2 * 6.0f along row j, out = (((r_0 + r_4) + (r_1 + r_3) * 4.0f) + r_2 * 6.0f) * 0.00390625f.
 *   5. EXPAND of an array T of level k + 1 at position (x, y) of level k.  In one dimension: x even, i = x / 2:
 *      ((T[i-1] + T[i+1]) + T[i] * 6.0f) * 0.125f; x odd, i = (x - 1) / 2: (T[i] + T[i+1]) * 0.5f.  Horizontally on the at most three rows
 *      the vertical rule needs, then the same rule vertically on those results.
 *   6. BLEND AND COLLAPSE, k = L-1 down to 0, per position x of the canvas's level k: over the frames, in ascending f, whose level-k grid
 *      holds x and whose w = M_f,k(x) is not 0.0f: lap_c = I_f,k,c(x) - expand(I_f,k+1,c)(x) (k = L-1: I_f,k,c(x)), num_c = num_c + w * lap_c,
 *      den = den + w, both from 0.0f.  B_c = den > 0 ? num_c / den : 0.0f.  R_k,c = B_c + expand(R_k+1,c)(x) (k = L-1: B_c).
 *   7. STORE, for k = 0 and canvas pixels only.  Label -1: every channel 0, weight 0.0f.  Otherwise f32 stores R_0,c, u8 stores
 *      (uint8)fminf(255.0f, fmaxf(0.0f, floorf(R_0,c + 0.5f))), weight 1.0f.  Every canvas pixel is written.
 * Hence: with n_bands == 1 the canvas is, per pixel, the label frame's q_c -- u8 rounded as the gain mosaic rounds --, a paste along the
 * seam, equal to HG_MOSAIC_LAST where frames do not overlap.  Frames with identical windows, full coverage and the same constant value
 * give that constant.  Non-finite f32 pixels give unspecified payloads.  DECIDED where the rule left a choice: at level 0 the blend runs
 * like every other level (num = 0.0f + 1.0f * lap, B = num / 1.0f), so a Laplacian of -0.0f enters as +0.0f; "label -1" at the store is
 * den == 0 at level 0, the same pixels; expand takes a row outside the grid as a row of 0.0f; the labels' part of the work area is
 * reserved whether d_labels is given or not, since the layout call cannot know.
 * LIMITATION: uncovered pixels enter the image pyramids as 0, as in OpenCV's blender: where a seam runs into a coverage border a faint dark
 * halo is possible (a coverage-normalised pyramid is not offered).  The result depends on the canvas window chosen, through clipping and
 * the grid origin.
 * n_frames == 0 zeroes the canvas, labels are -1 (geoms / d_coords / d_frames may be NULL).  An empty canvas: HG_OK, nothing is written.
 * HG_ERR_INVALID: the gain mosaic's list; n_bands outside 1..8; feather NaN or <= 0; with a non-empty canvas a d_work that is NULL,
 * misaligned or smaller than the layout's work_bytes; a misaligned d_labels; frame grids that need more than 2^31 - 1 blocks in one launch.
 * Asynchronous on the ctx stream; the frame table goes up through the page-locked staging ring; queued runs whose deferred redo could land on
 * d_canvas, d_weight, d_labels or d_work are settled first.  No effect on hg_last_*, the sampling mode, the plan, what the policy learned or
 * staged frame sets.  Launches: k_mb_label, k_mb_seed, L - 1 reduces, L blends -- 2 + (L - 1) + L whatever n_frames is.
 *
 * hg_mosaic_multiband_layout (host only, no context): *work_bytes for these windows.  The work area holds, each part aligned to 256 bytes,
 * in this order: the labels (4 bytes per canvas pixel; used when d_labels is NULL); the flag bytes of every taking-part frame's level-0
 * grid, in frame order; per taking-part frame, for k = 1..L-1, level k of I (channels floats per grid pixel) and then level k of M (one
 * float); levels 1..L-1 of R on the canvas grid (channels floats).  Level 0 of I and R is never stored.  An empty canvas needs 0 bytes.
 * 64 frames of 3840 x 2160, u8 x 4, on their common window at 5 bands: 4 228 678 656 bytes (3.94 GiB) -- 33.2 MB of labels, 64 x 8.5 MB
 * of flags (grids of 3872 x 2192), 64 x 56.4 MB of I and M, 45.1 MB of R.  (Arithmetic, not a measurement.)
 * HG_ERR_INVALID: work_bytes NULL; n_frames outside 0..65535; geoms NULL with n_frames > 0; channels outside 1..4; n_bands outside 1..8; a
 * canvas or a frame beyond the hg_geom limits.
 * Cost (MI355X; EXPERIMENTS.md "Multi-band"; tools/bench_multiband.py): u8 x 4 frames with weight plane and d_labels, medians of 31 regions,
 * as ratios to HG_MOSAIC_FEATHER on the same frames in the same process and to the byte floor of the work-area traffic at 8 TB/s (every used
 * part of the work area written and read once, coordinates twice, pixels once, labels, canvas and weights once).  64 frames with identical
 * 3840 x 2160 windows (feather 1.63 ms): 1 band 3.35 ms, 2.05 x feather, 2.3 x the floor; 3 bands 8.88 ms, 5.4 x, 3.8 x; 5 bands 9.35 ms,
 * 5.7 x, 3.9 x.  A strip of 16 frames of 1920 x 1080 shifted by 60 % of their width, canvas 19200 x 1080 (feather 0.24 ms): 0.58 / 1.51 /
 * 1.60 ms, 2.4 / 6.4 / 6.8 x feather, 4.7 / 7.5 / 7.7 x the floor, with work areas of 116 / 431 / 465 MB.  Level 1 carries three quarters of
 * the pyramid bytes, so bands beyond the third cost little. */
int hg_mosaic_multiband_layout(const hg_geom *geoms, int n_frames, hg_geom canvas,
                               int channels, int n_bands, size_t *work_bytes);
int hg_mosaic_multiband_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames,
                               const void *d_coords, const size_t *field_offsets,
                               const void *d_frames, const size_t *frame_offsets,
                               int elem, int channels, int W, int H, float feather, int n_bands,
                               hg_geom canvas, void *d_canvas, float *d_weight, int32_t *d_labels,
                               const float *gains, void *d_work, size_t work_bytes);
/* The source field of the FORWARD warps (next section): what hg_warp_forward_* would paint, as geometry.  HG_FIELD_INDEX only, hence no
 * format argument: the forward loops copy whole pixels from integer positions, (s % W, s / W) IS the coordinate.  One int32 per output pixel
 * p, row-major obj_w x obj_h: let w be the LAST writer, in the loop's raster order (:919-930 over y < H, x < W; :955-969 over the cells of
 * the source-point bounding box whose forward-map id is > -1), among the source pixels whose flat destination index -- formed as the
 * reference forms it (:924-926 / :962-964: Math.round, `<< 2` on ToInt32, u outside [0, objW) aliasing into the neighbouring rows) -- equals
 * 4p and passes the typed-array bound, and s the flat source pixel index that writer reads (geometric: y W + x; piecewise :960:
 * (cell_y + minSrcY) W + cell_x + minSrcX, which may wrap into a neighbouring source row or leave the array).  field[p] = s if a writer
 * exists and 0 <= s < W H, else -1 (nobody writes, or the last writer reads undefined -> 0, which still overwrites earlier writers).  Hence
 *     out32[p] = field[p] >= 0 ? img32[field[p]] : 0
 * IS the forward warp, byte for byte, holes and overwritten pixels included; hg_remap_index_device sends any other plane the same way.
 * With hg_set_images_device the index of frame f is relative to image f % n_images; only the source's SIZE is read.
 * Layout as above (field_offsets NULL: packed as hg_pack_field_offsets(.., HG_FIELD_INDEX, ..) packs; multiples of 4, HG_ERR_INVALID
 * otherwise; bytes between frames are never written, empty frames write nothing).  Limits and refusals are those of the forward warps
 * (HG_ERR_STATE: no image / no mesh; HG_ERR_INVALID: NULL pointers, unknown kind, a source or source box of 2^31 pixels or more or taller than
 * 65535 rows).  The PATH is chosen exactly as the corresponding forward warp chooses it (option "fwd_tiles", hg_forward_tiles_admissible,
 * the piecewise size / density test) and reported by hg_last_forward_field_kernel: 0 none yet, 1 scatter + winner buffer, 2 the tile-binned
 * kernels.  hg_last_forward_kernel, hg_last_piecewise_*, hg_last_geometric_kernel and the sampling mode stay as they were.  Staged frame sets
 * and the forward triangle map are treated as the corresponding forward warp entry point treats them.
 * Geometric: `m` is the FORWARD matrix (6 / 8 doubles; batch: n x 8).  The host form is synchronous; the batch form is asynchronous on the
 * ctx stream after settling queued runs (nothing of it is ever redone).
 * Piecewise: leaves NO DEFERRED REDO, like hg_field_inverse_piecewise_frames_device: queued warp runs are settled first, as by hg_sync, and
 * keep their own results -- a deferred error of such an earlier run surfaces HERE, as it would from hg_sync, and the field is then not
 * computed; on the tile path the call is settled before it returns, on the scatter path (nothing can be redone) its launches are
 * asynchronous on the ctx stream like a warp's; the tile kernels flag into a status set of the call's own; a frame they flag (a triangle they cannot bound, an overfull tile
 * list) is redone through the scatter path into the field before the call returns and counted in hg_redone_frames.  What such a flag says
 * about the MESH is learned exactly as hg_sync learns it from a warp (capacity 64 -> 128 -> 256 after an overflow; the tile path off for
 * the mesh after an unboundable triangle or an overflow at 256), so warps and field calls find each other's findings. */
int hg_field_forward_geometric(hg_ctx *ctx, int kind, const double *m, hg_geom geom, void *out_host);
int hg_field_forward_geometric_batch_device(hg_ctx *ctx, int kind, const double *m, const hg_geom *geoms, const size_t *field_offsets,
                                            int n_frames, void *d_field);
int hg_field_forward_piecewise(hg_ctx *ctx, const float *dst_points, int max_src_x, int max_src_y, hg_geom geom, void *out_host);
int hg_field_forward_piecewise_batch_device(hg_ctx *ctx, const float *dst_points, int max_src_x, int max_src_y, const hg_geom *geoms,
                                            const size_t *field_offsets, int n_frames, void *d_field);
int hg_last_forward_field_kernel(hg_ctx *ctx);

/* ------------------------------------------------------------------------------------------------ point lists
 * The annotation callers most often hold beside a picture is not a raster but a list of points: landmarks, box corners, contour vertices, a
 * click position.  These calls send such lists through the geometry of a frame set, in either direction, without a field: "which source
 * position lies under this output position" (to source) and "where does this source position land in frame f's output" (to output).  Not
 * part of the reference; geometry only, like the fields: only the source's SIZE is read.
 * Points are interleaved (x, y) float32 in GPU memory, 8-byte aligned.  d_points holds n_sets lists of n_points points each, tightly packed;
 * frame f reads list f % n_sets, the rule hg_set_images_device gives images (n_sets == 1: one list for every frame).  d_out receives
 * n_frames x n_points x 2 float32, tightly packed: frame f starts at f * n_points * 8 bytes.  An UNMAPPED point holds 0x7fc00000 in both
 * words, the exact pattern of HG_FIELD_COORDS.  All arithmetic is f64 in the reference's operation order, contraction off; each result is
 * rounded once to f32.
 * The CELL of a point is (Math.round(x), Math.round(y)), ties toward +Infinity: -0.5 belongs to cell 0, k + 0.5 to cell k + 1.  It is formed
 * and tested in floating point before any integer conversion, so NaN, +-Infinity and 1e30 are legal inputs that simply fall outside.
 * TO SOURCE (output position -> source coordinate; the inverse loops :997-1011 and :1042-1056).  The input (u, v) is in the output WINDOW's
 * pixel coordinates: output pixel (i, j) is the point (i, j).  The point maps iff its cell lies in [0, obj_w) x [0, obj_h) and
 *   geometric  (sx, sy) = transform(inverse matrix, (double)u + x_off, (double)v + y_off) passes the coverage test :1001;
 *   piecewise  the triangle is the id the reference's map holds AT THE POINT'S CELL (the largest id whose fillTriangle spans cover flat index
 *              r * obj_w + c, fill()'s wrap of negative indices included; ids as the coords field treats them), (sx, sy) is that
 *              triangle's inverse matrix applied to the point itself, ((double)u + x_off, (double)v + y_off), and passes :1047 with the
 *              frame's minSrc.  Per-frame source points and minima (hg_piecewise_set_frames_src) are honoured.
 * The result is ((float)sx, (float)sy).  Hence for integer (u, v) inside the window it is the HG_FIELD_COORDS field's value at that pixel,
 * bit for bit, NaN pattern included.
 * TO OUTPUT (source position -> output position; the forward loops :919-926 and :955-964).  The input (px, py) is in source-image pixels.
 *   geometric  the point maps iff its cell lies in [0, W) x [0, H), the loop's domain; (nx, ny) = transform(forward matrix, px, py);
 *   piecewise  mx = cell_x - minSrcX, my = cell_y - minSrcY must lie in the forward map [0, maxSrcX - minSrcX) x [0, maxSrcY - minSrcY) and
 *              the cell must hold an id > -1 (the map of :817-832 the forward warps build and cache); (nx, ny) is that id's forward matrix
 *              (:785-804, f32 entries widened) applied to the point itself.  The mesh-wide source side only, as every forward entry point.
 * The result is ((float)(nx - x_off), (float)(ny - y_off)), the value :924 / :962 hands to Math.round: window-relative, and reported whether
 * or not it falls inside the window -- that is the caller's business.
 * Each entry point follows its field counterpart in what it demands of the context (HG_ERR_STATE: no source image, no mesh, no frame set),
 * in its limits, in what it settles before launching and in how staged frame sets and the forward-map cache are treated; none touches
 * hg_last_*_kernel / _variant / _self, the sampling mode, the plan of the last warp or what the policy learned.  All run on the ctx stream.
 *   hg_points_to_source_geometric_frames_device  the staged set of hg_geometric_set_frames[_points]; asynchronous (as
 *              hg_field_inverse_geometric_frames_device).
 *   hg_points_to_source_piecewise_frames_device  the staged set of hg_piecewise_set_frames / _set_frames_src / hg_piecewise_prepare; SETTLED
 *              INSIDE THE CALL as hg_field_inverse_piecewise_frames_device is: queued warp runs are settled first, and a frame with
 *              irregular triangles (a NaN vertex is legal input) is redone through the materialised map before the call returns and counted
 *              in hg_redone_frames.  The kernel resolves the id of a cell by walking the mesh's triangles, with no map and no span list (hence
 *              no overflow): made for short lists on small meshes.  MEASURED (EXPERIMENTS.md P, 64 4K frames): at 65536 points per frame
 *              and 5000 triangles it is 33x SLOWER than the full-frame hg_field_inverse_piecewise_frames_device(HG_FIELD_COORDS) call it
 *              stands in for (79 ms against 2.4 ms), 3.5x slower at 65536 points and 200 triangles, 1.7x slower at 68 points and 5000
 *              triangles; it wins at 68 points and 200 triangles (0.22 of the field call).  Beyond that, export the field and gather.
 *   hg_points_to_output_geometric_batch_device   m: n_frames x 8 FORWARD matrices (affine in the first 6 of each 8); limits as
 *              hg_field_forward_geometric_batch_device; queued runs are settled, then asynchronous.  No staged set is touched.
 *   hg_points_to_output_piecewise_batch_device   as hg_field_forward_piecewise_batch_device up to the launch: the forward map is built or
 *              reused from the cache, the frames become the staged piecewise set; nothing is ever redone; asynchronous.
 * n_points == 0: HG_OK, nothing happens.  HG_ERR_INVALID: NULL pointers with work to do, n_points negative or above 2^24, n_sets below 1,
 * a pointer not aligned to 8 bytes, and what the counterpart refuses. */
int hg_points_to_source_geometric_frames_device(hg_ctx *ctx, const void *d_points, int n_points, int n_sets, void *d_out);
int hg_points_to_source_piecewise_frames_device(hg_ctx *ctx, const void *d_points, int n_points, int n_sets, void *d_out);
int hg_points_to_output_geometric_batch_device(hg_ctx *ctx, int kind, const double *m, const hg_geom *geoms, int n_frames,
                                               const void *d_points, int n_points, int n_sets, void *d_out);
int hg_points_to_output_piecewise_batch_device(hg_ctx *ctx, const float *dst_points, int max_src_x, int max_src_y, const hg_geom *geoms,
                                               int n_frames, const void *d_points, int n_points, int n_sets, void *d_out);

/* ------------------------------------------------------------------------------------------------ fitting transforms to matches
 * Every geometric entry point above starts from a matrix or from exactly three or four point pairs.  A feature matcher hands over hundreds
 * to thousands of matches per frame, a good part of them wrong: these two calls fit one affine or projective transform per frame that
 * ignores the wrong ones (RANSAC: many minimal hypotheses, each scored by how many matches it explains, the best one refitted by least
 * squares over its inliers).  Not part of the reference.  The result goes straight into hg_geometric_set_frames; hg_transform_limits gives
 * the windows.
 * MATCHES.  d_matches holds n_frames lists of n_points slots, tightly packed; a slot is (x, y, u, v) float32, the buffer is 16-byte
 * aligned.  (x, y) is the FROM position, (u, v) the TO position, and the matrix of frame f maps from -> to: a caller who wants the matrix the
 * inverse warps take passes output positions as from and source positions as to (the convention of hg_geometric_set_frames_points).
 * counts is on the HOST: frame f uses its first counts[f] slots, 0 <= counts[f] <= n_points; NULL = all of them.  NaN, +-Inf and 1e30 are
 * legal coordinates.  A match with a coordinate that is not finite is never an inlier (and never enters a least-squares sum); a match at
 * 1e30 obeys the score rule below like any other, which no sensible threshold lets it pass.
 * K = 3 for HG_AFFINE, 4 for HG_PROJECTIVE.
 * SAMPLES.  Hypothesis h of frame f is K distinct match indices.  d_samples non-NULL: n_frames x n_hyp x 4 int32 in device memory (4-byte
 * aligned), read as they stand; affine ignores the fourth; an index outside [0, counts[f]) or a repeated index makes the hypothesis
 * INVALID.  d_samples NULL: the device draws them by this rule, which hg_fit_sample_indices computes on the host (out = n_frames x n_hyp x 4
 * int32, -1 in all four slots of an invalid hypothesis, -1 in the fourth slot for affine), all in uint32 arithmetic:
 *     mix(a): a ^= a >> 16; a *= 0x7feb352d; a ^= a >> 15; a *= 0x846ca68b; a ^= a >> 16
 *     k = mix(mix(mix(seed + 0x9e3779b9) + f) + h)
 *     draw t = 0, 1, ..., 15:  i_t = (uint32)(((uint64)mix(k + t) * (uint32)counts[f]) >> 32)
 * The draws are walked in order; i_t is accepted when it differs from every index accepted so far; the walk stops at K accepted.  Fewer than
 * K after 16 draws, or counts[f] < K, makes the hypothesis invalid: at counts = 4 about 4 % of the projective hypotheses are, at 5 about
 * 0.2 %, at 65 none in 3840 -- a frame with that few matches has few distinct samples anyway.
 * MINIMAL SOLVE.  Projective: hg_solve_projective on the K sampled (from, to) pairs, h0..h7 with h8 == 1.  Affine: hg_solve_affine widened to
 * double in the first 6 of 8 slots, slots 6 and 7 zero (the layout of every affine matrix here: x' = m0 x + m2 y + m4, y' = m1 x + m3 y + m5).
 * A hypothesis whose matrix has an entry that is not finite is invalid too (collinear or coincident points).
 * SCORE.  For match i < counts[f]: (px, py) = the matrix applied to ((double)x, (double)y) as applyProjectiveTransformToPoint :1401-1404 resp.
 * applyAffineTransformToPoint :1382-1385 do, in f64 with IEEE division and contraction off; e = (px - u)(px - u) + (py - v)(py - v), products
 * and sum rounded separately; the match is an INLIER iff e <= threshold * threshold (a NaN e is none).  The score of a valid hypothesis is
 * its inlier count; the BEST hypothesis has the highest count, the lowest h among equals -- a total order, so the result does not depend on
 * scheduling.  A frame without a valid hypothesis FAILS.
 * OUTPUTS, all in device memory; d_mats (8-byte aligned) and d_counts are required, the others may be NULL.
 *   d_best[f]    the best hypothesis' index, -1 for a failed frame.
 *   d_counts[f]  its inlier count, 0 for a failed frame.
 *   d_mask       n_frames x n_points bytes: 1 for an inlier of the best hypothesis, else 0; slots at and beyond counts[f] are 0; a failed
 *                frame is all 0.
 *   d_min_mats   n_frames x 8 doubles: the best hypothesis' matrix exactly as solved (the bits of hg_solve_projective / hg_solve_affine on
 *                the sampled points); 8 quiet NaNs (0x7ff8000000000000) for a failed frame.
 *   d_mats       n_frames x 8 doubles, the result to use: with refit == 0 a copy of d_min_mats; with refit != 0 the least-squares refit over
 *                the best hypothesis' inliers, and the minimal matrix where the frame has K inliers or fewer or where an entry of the refit
 *                is not finite.
 * The mask and the count always describe the best hypothesis, not the refit (what findHomography-style callers expect, and exact).
 * LEAST SQUARES WITHOUT SAMPLING.  n_hyp == 0 with refit != 0: every match of the frame whose four coordinates are finite is an inlier; the
 * mask and d_counts say so; d_best is -1, d_min_mats holds NaNs, d_mats is the refit -- NaNs when fewer than K such matches remain or an entry
 * is not finite.  n_hyp == 0 with refit == 0 is HG_ERR_INVALID.
 * REFIT, all in f64.  Each side is normalised: c = the mean of the inliers' positions, s = sqrt(2) / the mean of sqrt(ax ax + ay ay) over
 * a = position - c, x' = (x - cx) s (likewise y', and u', v' with the to side's c and s).  Projective: the normal equations A^T A (8 x 8) and
 * A^T b of the rows [x' y' 1 0 0 0 -u'x' -u'y'] -> u' and [0 0 0 x' y' 1 -v'x' -v'y'] -> v', accumulated as the sums of x'x', x'y', y'y', x',
 * y', 1, of the same six weighted by u', by v', and of the first five weighted by w = u'u' + v'v' (w (x'x') and so on); solved by Gaussian
 * elimination with partial pivoting in one lane; denormalised as T_to^-1 H' T_from and divided through by its last entry, so h8 == 1.
 * Affine: the 3 x 3 system of the first six sums with the two right-hand sides (sums of u'[x' y' 1]) and (sums of v'[x' y' 1]), denormalised the
 * same way and written in the affine layout.  Every sum is accumulated in a fixed order (lane-strided partial sums, then a fixed tree) with
 * no floating-point atomics: two runs of one call give the same bits.  The VALUE of the refit is pinned by tolerance, not bit for bit.
 * LIMITS (HG_ERR_INVALID): NULL ctx; unknown kind; NULL or misaligned required pointers when there is work; n_points outside 0..65536; n_hyp
 * outside 0..65536; n_frames outside 0..4096; a counts[f] outside [0, n_points]; threshold not finite or negative (0 is legal).  n_frames == 0
 * is HG_OK and nothing is written.  hg_fit_sample_indices makes the same checks, without a context.
 * CONTEXT.  The call needs no image, mesh or frame set.  It settles what hg_points_to_output_geometric_batch_device settles (queued runs),
 * then is asynchronous on the ctx stream; counts is copied before it returns.  It touches no hg_last_*, no sampling mode, no plan, no policy
 * state and no staged frame set.  Its scratch (n_frames x n_hyp matrices and flags) lives in buffers the context owns, grown on demand and
 * reused.
 * COST.  The hot loop is n_frames x n_hyp x counts reprojections, two IEEE f64 divisions each for projective.  MEASURED (MI355X, whole call,
 * medians of 31; EXPERIMENTS.md, "Fitting"): 64 frames x 2048 matches x 2048 hypotheses 0.46 ms projective (5.9e11 reprojections / s), 0.21 ms
 * affine, the refit 0.02-0.03 ms on top; 64 x 512 x 512 0.10 / 0.07 ms; ONE frame x 4096 x 4096 0.48 / 0.25 ms -- a single frame fills only
 * n_hyp / 256 workgroups, so frames are what the call scales over.  The numpy model takes 94 ms for ONE frame of the first case. */
int hg_fit_sample_indices(int kind, uint32_t seed, int n_frames, const int32_t *counts, int n_points, int n_hyp, int32_t *out);
int hg_fit_matches_frames_device(hg_ctx *ctx, int kind, const void *d_matches, int n_points, const int32_t *counts, int n_frames,
                                 double threshold, int n_hyp, uint32_t seed, const int32_t *d_samples, int refit,
                                 double *d_mats, double *d_min_mats, int32_t *d_counts, int32_t *d_best, uint8_t *d_mask);

/* ------------------------------------------------------------------------------------------------ refining transforms on the pixels
 * The detector's keypoints are integer pixel positions, so a transform fitted to a few dozen matches is good to a fraction of a pixel, not
 * better.  hg_align_refine_frames_device refines such a transform on the PIXELS of the two pictures: direct (photometric) alignment, Gauss-
 * Newton on the intensity difference over a grid of samples (Lucas-Kanade with an affine or projective warp), started from the matrix the fit
 * gave.  Not part of the reference.  It is a LOCAL refinement: it needs a start within a few pixels, or a walk over pyramid levels that
 * brings it there (hg_align_scale_matrix).
 * PLANES.  u8, rows tight, `channels` 1 or 4; of 4 channels the luma (77 R + 150 G + 29 B + 128) >> 8 is used (the detector's), alpha is
 * ignored.  Frame f has its own FROM plane at d_from + f * from_stride_bytes (Wf x Hf) and reads TO plane f % n_to_sets at d_to + (f %
 * n_to_sets) * to_stride_bytes (Wt x Ht), the rule the matcher gives train sets.  The matrix of frame f maps FROM positions to TO positions,
 * in the layouts hg_fit_matches_frames_device writes: projective h0..h7 with h8 == 1, affine m0..m5 in the first six of eight slots (x' =
 * m0 x + m2 y + m4, y' = m1 x + m3 y + m5).  For a chain that matched frames (query) against a keyframe (train), FROM = the frame, TO = the
 * keyframe, and the fit's d_mats is d_mats_in as it stands.
 * SAMPLES.  The FROM pixels (x, y) = (rx + i step, ry + j step), i = 0 .. ceil(rw / step) - 1, j = 0 .. ceil(rh / step) - 1; sample number
 * s = j * ceil(rw / step) + i.  a = the luma there, as a double.
 * NORMALISATION.  Each side uses c = ((W - 1) / 2, (H - 1) / 2) and s = 2 / max(W, H): x' = (x - cx) s, y' = (y - cy) s on the FROM side,
 * likewise u', v' with the TO side's c and s.  With M the input as a 3 x 3 matrix, A = M T_from^-1 (columns 0 and 1 divided by s_from,
 * column 2 = (col0 cx + col1 cy) + col2), B = T_to A (row 0 = (row0 - cx_to row2) s_to, row 1 likewise with cy_to, row 2 as it is), H' = B
 * divided through by its last entry.  Gauss-Newton runs on the entries of H' (affine: its six); the way back is M = T_to^-1 H' T_from as
 * the fit's refit writes it (column 2 = (h2 - h0 (s cx)) - h1 (s cy); row 0 = row0 / s_to + cx_to row2), divided through by its last entry.
 * ONE PASS over the iterate H' (with the photometric terms g, b; they start at 1, 0), all in f64 with IEEE division, contraction off,
 * every product and sum rounded on its own, sums from left to right.  For the sample (x', y'):
 *   1. D = (h6' x' + h7' y') + 1; 1 for affine.
 *   2. u' = ((h0' x' + h1' y') + h2') / D, v' = ((h3' x' + h4' y') + h5') / D; u = u' / s_to + cx_to, v = v' / s_to + cy_to (TO pixels).
 *   3. The sample is VALID iff u and v are finite, D > 0, 1 <= u < Wt - 2 and 1 <= v < Ht - 2: no tap below leaves the plane.
 *   4. x0 = floor(u), fx = u - x0 (likewise y0, fy).  blend(p00, p01, p10, p11) = ((p00 (1 - fx) + p01 fx) (1 - fy)) + ((p10 (1 - fx) + p11 fx)
 *      fy), p = the TO luma (for RGBA the integer luma of each tap first).  I = blend of the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 *      (x0 + 1, y0 + 1).
 *   5. dx = (I(u + 1, v) - I(u - 1, v)) / 2: the same blend, the same fractions, the taps one column to the right resp. left; dy likewise
 *      with rows: 12 distinct taps.  jx = (dx / s_to) / D, jy = (dy / s_to) / D (the derivative with respect to u', v', over D).
 *   6. r = a - I with photometric == 0, r = ((g a) + b) - I with photometric == 1.
 *   7. The Jacobian row.  Projective: [jx x', jx y', jx, jy x', jy y', jy, w x', w y'] with w = -((jx u') + (jy v')).  Affine, in the
 *      affine slot order m0..m5: [jx x', jy x', jx y', jy y', jx, jy].  With photometric [-a, -1] is appended.  P = 6, 8 or 10.
 *   8. Per frame the pass produces n_valid (an integer) and the sums over the valid samples of: J_p J_q for p <= q, row by row of the upper
 *      triangle (P (P + 1) / 2 values), J_p r (P values), r r (one): P (P + 1) / 2 + P + 1 <= HG_ALIGN_SUMS doubles, in that order.
 * UPDATE.  J^T J delta = J^T r is solved by Gaussian elimination with partial pivoting in one lane (the refit's routine); delta_k is added
 * to parameter k (projective h0'..h7'; affine m0'..m5', m0' = h0', m1' = h3', m2' = h1', m3' = h4', m4' = h2', m5' = h5'; then g, b).
 * rms = sqrt(sum r r / n_valid).
 * ITERATION.  Pass 0 evaluates the input.  After update k (k = 1, 2, ...) the DISPLACEMENT is the largest distance, in TO pixels, between
 * the images (steps 1 and 2) of the four corners (rx, ry), (rx + rw - 1, ry), (rx, ry + rh - 1), (rx + rw - 1, ry + rh - 1) of the sample
 * rectangle under the iterate before and after it.  The frame stops iterating when displacement < eps (HG_ALIGN_CONVERGED) or after n_iter
 * updates (HG_ALIGN_MAX_ITER); one more pass then evaluates the final iterate: n_iter + 1 passes at most, n_iter == 0 is an evaluation only
 * (status HG_ALIGN_MAX_ITER, 0 updates).
 * RESULT.  d_mats_out[f] (8 doubles) is the final iterate brought back to pixels, in the input's layout: h8 normalised to 1, affine slots 6
 * and 7 zero.  The INPUT's bits (all 8 slots) are copied instead when
 *   - a pass found n_valid < min_valid (HG_ALIGN_TOO_FEW);
 *   - a solution, an iterate or a photometric term has an entry that is not finite (HG_ALIGN_SINGULAR; a constant TO plane ends here);
 *   - the final rms exceeds pass 0's (HG_ALIGN_WORSE);
 *   - the input matrix has an entry that is not finite (HG_ALIGN_BAD_INPUT; affine: of its first six): a failed frame of the fit, all NaNs,
 *     passes through untouched;
 *   - no update was applied (n_iter == 0): the iterate IS the input.
 * d_mats_out may alias d_mats_in (frame f's slots are read before they are written, by the workgroup that writes them).
 * INFO.  d_info[f] is 48 bytes, 8-byte aligned: { int32 status, updates, n_valid_first, n_valid_last; double rms_first, rms_last, gain, bias }.
 * n_valid_first / rms_first are pass 0's, n_valid_last that of the last pass that ran, rms_last that of the last pass that found min_valid
 * samples; an rms is NaN where no such pass exists; BAD_INPUT has counts 0.  gain, bias = g, b of the returned matrix: 1, 0 without
 * photometric and wherever the input was copied.
 * SUMS.  d_sums is optional (NULL: not written): n_frames x HG_ALIGN_SUMS doubles, the sums of PASS 0 in the order of step 8, the tail zero.
 * DETERMINISM.  A workgroup takes a CHUNK of 8192 consecutive samples; lane t of its 256 adds the samples t, t + 256, ... of the chunk in
 * that order, the workgroup adds the lanes' sums through a fixed tree (lane l += lane l + s for s = 128, 64, .. 1), and the chunks' records
 * are added in ascending chunk order.  No floating-point atomics: two runs of one call give the same bits.  The VALUES are pinned by
 * tolerance, as the refit's are.
 * LIMITS (HG_ERR_INVALID), checked in this order, the shape before the context: unknown kind; Wf, Hf, Wt, Ht outside 1..32768 or W * H >
 * 2^30; channels not 1 or 4; a rectangle that is empty or leaves the FROM plane; step outside 1..64; photometric not 0 or 1; n_iter outside
 * 0..64; eps negative or not finite; min_valid < P; n_frames outside 0..4096; n_to_sets outside 1..max(n_frames, 1); a stride below its
 * plane's bytes; then NULL ctx; NULL d_from, d_to, d_mats_in, d_mats_out or d_info; matrices, sums or info not aligned to 8 bytes.
 * n_frames == 0 is HG_OK and nothing is written.
 * CONTEXT.  As the fit: no image, mesh or frame set is needed; queued runs are settled first, then the call is asynchronous on the ctx
 * stream, with no host synchronisation between the passes (every pass of every frame is launched; the workgroups of a stopped frame read
 * its flag and return, so a stopped frame's outputs are never touched again).  It touches no hg_last_*, no sampling mode, no plan, no policy
 * state and no staged frame set.  Its scratch -- per frame the iterate and flags, per chunk a record of 67 doubles, and for 4-channel planes
 * a one-byte luma copy of every plane, made once per call so that the passes do not redo 12 lumas per sample -- lives in buffers the
 * context owns, grown on demand and reused.
 * hg_align_scale_matrix (host only) converts a matrix between levels of hg_pyramid_build_device, both sides at the same level: a position
 * at level k is x_k = (x_0 + 0.5) 2^-k - 0.5 (the rule hg_remap_trilinear_frames_device states), so with e = 2^(level_in - level_out) and
 * o = (e - 1) / 2 positions move as x_out = e x_in + o and m_out = S m_in S^-1, S = [e 0 o; 0 e o; 0 0 1], divided through by its last
 * entry.  Affine stays affine.  Levels are 0..30; NULL pointers and unknown kinds are HG_ERR_INVALID.  m_out may be m_in.
 * COST.  Every pass reads 12 TO taps and one FROM byte per sample and does about 150 f64 operations on them (P = 10).  MEASURED (MI355X,
 * whole call, medians of 31; EXPERIMENTS.md, "Aligning"): 64 RGBA frames of 1920 x 1080 against one keyframe, projective, photometric, 8
 * updates (9 passes): 30.8 ms at step 1 (3.9e10 samples / s), 8.1 ms at step 2, 2.3 ms at step 4; 8 frames of 3840 x 2160: 17.5 / 4.8 /
 * 1.3 ms; ONE frame of 1920 x 1080: 0.74 / 0.62 / 0.60 ms -- the 20 launches, so frames are what the call scales over.  ONE pass of one
 * 1080p frame takes a plain torch formulation 257 ms at step 1 on the same GPU, the numpy model about 0.2 s at step 2. */
enum { HG_ALIGN_CONVERGED = 0, HG_ALIGN_MAX_ITER = 1, HG_ALIGN_TOO_FEW = 2, HG_ALIGN_SINGULAR = 3, HG_ALIGN_WORSE = 4, HG_ALIGN_BAD_INPUT = 5 };
enum { HG_ALIGN_SUMS = 66 };   /* doubles per frame in d_sums */
int hg_align_scale_matrix(int kind, const double *m_in, int level_in, int level_out, double *m_out);
int hg_align_refine_frames_device(hg_ctx *ctx, int kind,
                                  const void *d_from, int Wf, int Hf, int n_frames, size_t from_stride_bytes,
                                  const void *d_to, int Wt, int Ht, int n_to_sets, size_t to_stride_bytes, int channels,
                                  int rx, int ry, int rw, int rh, int step,
                                  int photometric, int n_iter, double eps, int min_valid,
                                  const double *d_mats_in, double *d_mats_out, void *d_info, double *d_sums);

/* ------------------------------------------------------------------------------------------------ adjusting a frame set over all pairs
 * The fit and the alignment give one matrix per PAIR of pictures.  A panorama is no star around one keyframe: frame 7 overlaps frame 6, not
 * frame 0, so its place in the canvas is a product of pairwise matrices, every factor adds its error, and where a strip closes on itself the
 * product misses by many pixels.  hg_bundle_adjust_frames_device refines the frame -> canvas matrices of ALL frames at once so that the
 * matches of all pairs agree in the canvas: Levenberg-Marquardt on the device, nothing but the info record crossing to the host.  Not part of
 * the reference.  It is the PLANAR-MOSAIC formulation: the residual lives in the canvas, at least one frame is held fixed, the unknowns are
 * the entries of the matrices themselves (h8 == 1 is kept).  There is no rotation / focal-length camera model and there are no lens terms; a
 * set whose true geometry is not a chain of homographies (parallax) is not helped.  It is a LOCAL refinement: start from a chain
 * (hg_bundle_chain_from_pairs).
 * MATRICES.  The layouts of the fit: projective h0..h7 with h8 == 1, affine m0..m5 in the first six of eight slots (x' = m0 x + m2 y + m4,
 * y' = m1 x + m3 y + m5).  d_mats_in[f] (8 doubles) maps positions of frame f to the common canvas.  All frames are W x H; the size is used
 * for the normalisation and the displacement measure only.
 * PAIRS AND MATCHES.  pairs (HOST) holds n_pairs x 2 int32: pair p = (a, b), a != b, both in 0..n_frames-1; repeated and reversed pairs are
 * legal.  List p of d_matches is n_points slots of (x, y, u, v) float32, tightly packed, the buffer 16-byte aligned -- the matcher's and the
 * fit's layout; (x, y) lies in frame a, (u, v) in frame b.  counts (HOST, NULL = n_points each): pair p uses its first counts[p] slots.
 * d_mask (optional) is the fit's d_mask as it stands: n_pairs x n_points bytes, 0 = leave the slot out.  A "pair" here is what the matcher
 * and the fit call a frame, so their outputs are this call's inputs with no repacking.
 * NORMALISATION.  One T for frames and canvas, the alignment's rule with both sides W x H: c = ((W - 1) / 2, (H - 1) / 2), s = 2 / max(W, H),
 * x' = (x - cx) s.  The iterate of frame f is M' = T M T^-1 divided through by its last entry, formed exactly as the alignment forms H'; the
 * way back is the alignment's too.  An input with an entry that is not finite (affine: of its first six), or whose M' has one, becomes an
 * all-NaN iterate.
 * ONE SLOT, all in f64 with IEEE division and square root, contraction off, sums from left to right.  With (x', y'), (u', v') the normalised
 * coordinates widened from f32 and A, B the iterates of frames a and b:
 *   D_a = (A6 x' + A7 y') + 1 (1 for affine), pa = (((A0 x' + A1 y') + A2) / D_a, ((A3 x' + A4 y') + A5) / D_a); D_b, pb alike from B, (u', v').
 *   The slot is VALID iff it lies below counts[p], its mask byte is not 0, each of its four coordinates c has |c| <= 16777216 (2^24: beyond
 *   it f32 holds no pixel positions; NaN fails), pa and pb are finite, D_a > 0 and D_b > 0.  NaN, +-Inf and 1e30 are legal coordinates and
 *   never valid.  r = pa - pb; e = sqrt(rx rx + ry ry) / s, the residual in canvas pixels.
 *   WEIGHT.  huber == 0 or e <= huber: w = 1, rho = e e.  Else w = huber / e, rho = (2 huber) e - huber huber.  The COST is the sum of rho
 *   over the valid slots of all pairs (pixels squared); rms = sqrt(cost / n_valid).
 *   ROWS.  Projective, the x row and the y row of J_a = d pa / d A:  [x'/D_a, y'/D_a, 1/D_a, 0, 0, 0, -((pa_x x') / D_a), -((pa_x y') / D_a)]
 *   and [0, 0, 0, x'/D_a, y'/D_a, 1/D_a, -((pa_y x') / D_a), -((pa_y y') / D_a)]; J_b is the same on (u', v', pb, D_b), negated.  Affine, in the
 *   slot order m0..m5: [x', 0, y', 0, 1, 0] and [0, x', 0, y', 0, 1]; J_b negated.  P = 8 or 6.  v_x = [J_a row x | J_b row x | r_x], v_y
 *   alike: 2 P + 1 values each.
 * PAIR RECORD.  G = the sum over the pair's valid slots of w (v_x^T v_x + v_y^T v_y), entry (i, j) of a slot formed as w * ((v_x[i] v_x[j])
 * + (v_y[i] v_y[j])): a symmetric (2 P + 1) x (2 P + 1) matrix whose blocks are sum w J_a^T J_a, sum w J_a^T J_b, sum w J_b^T J_b, sum w
 * J_a^T r and sum w J_b^T r.  The record is its upper triangle row by row -- entry (i, j), i <= j, at i (2 P + 1) - i (i - 1) / 2 + (j - i)
 * -- with the LAST entry (r, r) replaced by the pair's cost, then n_valid as a double: (2 P + 1)(P + 1) + 1 = 154 resp. 92 doubles.
 * d_pair_sums is optional: n_pairs x HG_BUNDLE_SUMS doubles, PASS 0's records, the tail of an affine record zero.
 * UNKNOWNS.  The P parameters of every FREE frame.  A frame is FIXED where fixed[f] != 0 (HOST, n_frames bytes); at least one must be.  A
 * frame is UNANCHORED where no path of pairs with counts > 0 leads from it to a fixed frame (decided on the host); it is treated as fixed.
 * N = P x (free frames) must be <= 2048.  Free frame number i (ascending frame index) owns unknowns i P .. i P + P - 1.
 * SYSTEM.  H (N x N) and g (N) are sums over the records in ascending pair index: for pair (a, b), sum w J_a^T J_a goes to a's diagonal block,
 * sum w J_b^T J_b to b's, sum w J_a^T J_b to block (a, b) and its transpose to (b, a) where both are free; g_a -= sum w J_a^T r, g_b -= sum
 * w J_b^T r.  Blocks of frames that are not free are dropped.
 * LEVENBERG-MARQUARDT.  Pass 0 evaluates the input: cost c, n_valid n, lambda = lambda0.  Round k = 1 .. n_iter solves (H + lambda I) delta =
 * g; the parameters are normalised to O(1), so additive damping is well scaled, and H + lambda I is positive definite for every lambda > 0,
 * frames without a valid match included.  The CANDIDATE is the iterate + delta (parameter k of a frame is entry k of M' for projective, m_k
 * for affine); a pass evaluates it.  ACCEPT iff every entry of the candidate of every free frame with a finite input is finite, its n_valid
 * is >= n and its cost is < c: the candidate becomes the iterate, lambda = max(lambda / 10, 1e-12).  Otherwise REJECT: lambda = 10 lambda
 * and the same H and g are solved again.  The call stops with
 *   HG_BUNDLE_CONVERGED  when after an accepted round the largest distance, in canvas pixels, between the images of the four frame corners
 *                        (0, 0), (W-1, 0), (0, H-1), (W-1, H-1) of any free frame with a finite input under the iterate before and after is
 *                        < eps (the alignment's measure);
 *   HG_BUNDLE_STALLED    when after a rejected round lambda > 1e12;
 *   HG_BUNDLE_MAX_ITER   after n_iter rounds (n_iter == 0, or N == 0: an evaluation only, 0 rounds);
 *   HG_BUNDLE_SINGULAR   when a pivot of the factorisation is not positive and finite; the round counts, its candidate is not evaluated.
 * SOLVE.  Cholesky of H + lambda I with g as one more row below it: l_jj = sqrt(a_jj), l_ij = a_ij / l_jj, where every a_ij has had l_ik
 * l_jk subtracted for k = 0, 1, .. j - 1, one product at a time in that order; row N then holds y = L^-1 g.  L^T delta = y by back
 * substitution: delta_k = y_k / l_kk, then y_i -= l_ki delta_k for i < k, k descending.  For N <= 128 ONE workgroup per round does everything
 * but the pass -- the pass's reduction, the decision, assembly, damping, factorisation, substitution and the candidate -- with H and g in LDS;
 * above, the factorisation is blocked (panels of 32 columns: the diagonal block, the rows below it, the trailing matrix) in the scratch.  Both
 * follow the order above, so they give the same bits.
 * RESULT.  d_mats_out[f] is the final iterate brought back to pixels, in the input's layout.  The INPUT's bits (all 8 slots) are copied
 * for fixed frames, unanchored frames and frames whose input is not finite -- such a frame makes all its slots invalid, so its neighbours
 * simply do not see it -- and for every frame when no round was accepted.  d_mats_out may alias d_mats_in.
 * INFO.  d_info, 8-byte aligned, 48 + ((4 n_frames + 7) & ~7) + 24 n_pairs bytes: first { int32 status, rounds, accepted, n_valid_first,
 * n_valid_last, 0; double rms_first, rms_last, lambda_last } -- first: pass 0, last: the returned iterate, an rms is NaN where n_valid is 0,
 * lambda_last the damping the next round would have used; then one int32 per frame (HG_BUNDLE_FRAME_ADJUSTED: it was an unknown,
 * _FIXED, _UNANCHORED, _BAD_INPUT: free, but its input is not finite), padded to 8 bytes; then per pair { int32 n_valid_first, n_valid_last;
 * double rms_first, rms_last }, which tells a caller WHICH pair is inconsistent.
 * DETERMINISM.  A workgroup takes a CHUNK of 512 consecutive slots of one pair and adds every entry of the record over the chunk's slots in
 * ascending slot order (one lane per entry); the chunks' records are added in ascending chunk order, the pairs' records in ascending pair
 * index, the cost and the count over pairs p, p + 256, .. per lane and then through the alignment's tree.  The factorisation's order is the
 * one above.  No floating-point atomics: two runs of one call give the same bytes in every output.  VALUES are pinned by tolerance.
 * LIMITS (HG_ERR_INVALID), checked in this order, the shape before the context: unknown kind; W, H outside 1..32768; n_frames outside
 * 0..256; n_pairs outside 0..8192; n_points outside 0..65536; pairs NULL with n_pairs > 0, a pair index out of range, a == b; a count outside
 * [0, n_points]; n_iter outside 0..64; eps, lambda0 or huber negative or not finite, lambda0 == 0; (n_frames == 0 is HG_OK here, nothing
 * is written;) fixed NULL; no fixed frame; more than 2048 unknowns; scratch_bytes below hg_bundle_layout's; NULL d_mats_in, d_mats_out,
 * d_info, d_scratch, or d_matches while a count is > 0; d_matches or d_scratch not aligned to 16 bytes, matrices, info or sums not to 8; NULL
 * ctx.
 * CONTEXT.  As the fit and the alignment: no image, mesh or frame set is needed; queued runs are settled first, then the call is
 * asynchronous on the ctx stream with no host synchronisation between the rounds (every round is queued; the kernels of rounds after the
 * stop read the flag and return).  The host arrays are copied before it returns.  It touches no hg_last_*, no sampling mode, no plan, no
 * policy state and no staged frame set.  hg_bundle_layout gives the scratch for a shape (kind, n_frames, n_pairs, n_points; 0 for no
 * frames): it may be reused once the call has completed.
 * HOST HELPERS, in double.  hg_bundle_chain_from_pairs builds a start: pair_mats[p] (8 doubles) maps frame a to frame b -- what the fit
 * writes with a as FROM.  M_anchor = identity.  Frames are reached breadth-first from the anchor: level 0 is the anchor; for level L = 0, 1,
 * .. the pairs are walked in ascending index, and a pair with one end in level L and the other not yet reached gives that end its matrix,
 * M_a = M_b Q resp. M_b = M_a Q^-1 (3 x 3 products, sums from left to right, divided through by the last entry; Q^-1 as below), and puts it
 * into level L + 1.  Pairs whose matrix has an entry that is not finite are skipped; frames never reached come back as 8 NaNs.  n_frames <=
 * 256, n_pairs <= 8192.  hg_bundle_invert_matrix: the adjugate of the 3 x 3 form divided through by its last entry, written in the layout of
 * `kind` (affine stays affine, slots 6 and 7 zero); m_out may be m_in.  It is what turns a frame -> canvas matrix into the canvas -> frame
 * matrix hg_geometric_set_frames takes.
 * COST.  A pass is about 600 f64 operations per slot at P = 8; a factorisation N^3 / 3 multiply-subtracts; a round of the large path is 3
 * launches per 32 columns.  MEASURED (MI355X, whole call, medians of 31; EXPERIMENTS.md, "Bundle adjustment"; tools/bench_bundle.py), 10
 * rounds each: 64 projective frames x 125 pairs x 2048 matches (504 unknowns) 10.8 ms, of which the pass over all 256 000 matches, its
 * reduction and the decision are under 0.1 ms -- a round is its solve, 1.07 ms; 16 frames x 29 pairs x 2048 (120 unknowns, one workgroup)
 * 3.6 ms, 0.35 ms a round; 256 frames x 1014 pairs x 256 matches (2040 unknowns) 49.1 ms, 4.9 ms a round, 68 MB of scratch.  ONE round of
 * the numpy model of the first case takes 629 ms. */
enum { HG_BUNDLE_MAX_FRAMES = 256, HG_BUNDLE_MAX_PAIRS = 8192 };
enum { HG_BUNDLE_CONVERGED = 0, HG_BUNDLE_MAX_ITER = 1, HG_BUNDLE_STALLED = 2, HG_BUNDLE_SINGULAR = 3 };
enum { HG_BUNDLE_FRAME_ADJUSTED = 0, HG_BUNDLE_FRAME_FIXED = 1, HG_BUNDLE_FRAME_UNANCHORED = 2, HG_BUNDLE_FRAME_BAD_INPUT = 3 };
enum { HG_BUNDLE_SUMS = 154 };   /* doubles per pair in d_pair_sums */
int hg_bundle_layout(int kind, int n_frames, int n_pairs, int n_points, size_t *scratch_bytes);
int hg_bundle_adjust_frames_device(hg_ctx *ctx, int kind, int W, int H, int n_frames, const uint8_t *fixed,
                                   const int32_t *pairs, int n_pairs, const void *d_matches, int n_points, const int32_t *counts,
                                   const uint8_t *d_mask, int n_iter, double eps, double lambda0, double huber,
                                   const double *d_mats_in, double *d_mats_out, void *d_info, double *d_pair_sums,
                                   void *d_scratch, size_t scratch_bytes);
int hg_bundle_chain_from_pairs(int kind, int n_frames, const int32_t *pairs, int n_pairs, const double *pair_mats, int anchor,
                               double *mats_out);
int hg_bundle_invert_matrix(int kind, const double *m_in, double *m_out);

/* ------------------------------------------------------------------------------------------------ thin-plate splines
 * The piecewise transform is C0 only -- every triangle edge is a kink -- and undefined outside the hull of its mesh.  The THIN-PLATE SPLINE
 * is the smooth interpolant through the same landmark pairs, defined everywhere.  Not part of the reference.  These calls fit one spline per
 * frame on the device, and export it as a source field (what every remap, the mosaics and the multi-band blend read) or send point lists
 * through it.  None needs an image, a mesh or a frame set.
 * POINTS.  Frame f has n_points pairs (from_i -> to_i), 3 <= n_points <= HG_TPS_MAX_POINTS, interleaved (x, y) float32, 8-byte aligned.
 * d_from holds n_from_sets lists of n_points points, d_to n_to_sets lists, tightly packed; frame f reads from-list f % n_from_sets and
 * to-list f % n_to_sets.  The spline maps FROM-space positions to TO-space positions.  For a source field FROM holds output-space (destiny)
 * points and TO source-image points, the convention of hg_geometric_set_frames_points; swapping the roles gives the landmark-to-output map
 * (a spline has no closed-form inverse: that map is a second spline, solved on its own).
 * All arithmetic is f64, IEEE division and square root, contraction off.
 * NORMALISATION (the rule of the fit's refit, on the from side).  c = the mean of the from-points, s = sqrt(2) / the mean of
 * sqrt(ax ax + ay ay) over a = from_i - c, d_i = (from_i - c) s; t = the mean of the to-points, b_i = to_i - t.  Sums run in index order.
 * SYSTEM, of size M = n_points + 3: [[K + lambda I, P], [P^T, 0]] [w; a] = [b; 0] with K_ij = U(|d_i - d_j|^2), U(q) = q log q, U(0) = 0
 * (r^2 log r^2, twice the textbook kernel; the factor is absorbed into w), row i of P = [1, dx_i, dy_i], and two right-hand sides, the x and
 * the y parts of b.  lambda >= 0 is finite and lives in the normalised frame; 0 interpolates.
 * SOLVE.  Gaussian elimination with partial pivoting: in column k the pivot is the entry of largest magnitude in rows k.., the lowest row
 * among equals; rows are swapped; row i > k becomes row_i - (a_ik / pivot) row_k, entry by entry, the right-hand sides alike; then back
 * substitution, x_k = b_k / a_kk, b_i -= a_ik x_k for i < k.  The order is fixed: two runs give the same bits.  One workgroup per frame; the
 * matrix lives in LDS for n_points <= 69, else in d_scratch (hg_tps_layout: n_frames x M x M doubles, 0 for n_points <= 69).
 * RECORD of a frame: 16 + 4 n_points doubles.  [0] cx [1] cy [2] s [3] tx [4] ty [8] a0x [9] a0y [10] a1x [11] a1y [12] a2x [13] a2y, the
 * other slots below 16 are 0; then n_points x (dx_i, dy_i, wx_i, wy_i).
 * STATUS of a frame (int32): HG_TPS_BAD_INPUT when any coordinate of the frame is not finite; else HG_TPS_SINGULAR when the mean distance is
 * 0 (all from-points coincide), a pivot is 0 or not finite, or a coefficient is not finite; else HG_TPS_OK.  Two coincident from-points at
 * lambda == 0 are HG_TPS_SINGULAR: their rows stay equal through the elimination, so a pivot is exactly 0; at lambda > 0 they solve.  A set
 * that is NEARLY singular but still gives finite numbers is the caller's business: it is HG_TPS_OK with whatever coefficients came out.
 * Every slot of a failed frame's record is 0x7ff8000000000000; other frames are not affected.
 * EVALUATION at the from-space position (X, Y): x' = (X - cx) s, y' = (Y - cy) s, q_i = (x' - dx_i)^2 + (y' - dy_i)^2,
 *   sx = tx + (((a0x + a1x x') + a2x y') + sum_i wx_i U(q_i)), sy alike, the sum in index order, in f64: the terms are large and cancel (at
 * 200 points and 20 px displacements sum |w U| reaches 5e6 for results of a few thousand), so an f32 sum would be wrong by tenths of a pixel.
 * The logarithm is this library's own (tps_log, csrc/hg_tps_dev.h), good to 2 ulp and not libm's to the bit: values are pinned by tolerance.
 * hg_field_tps_frames_device writes the source field of the frames' splines: pixel (i, j) of frame f is the position (i + x_off, j + y_off);
 * it is covered iff sx >= 0 && sx < W && sy >= 0 && sy < H (NaN fails; W, H >= 1 are arguments, as for the remaps), and its value is stored by
 * the rules of the other field calls: HG_FIELD_INDEX and HG_FIELD_COORDS mean exactly what they mean above, -1 and the NaN pattern
 * included.  field_offsets, packing, alignment, "bytes between frames are never written" and the settling of queued runs are those of
 * hg_field_inverse_geometric_frames_device.  A failed frame is all -1 resp. all NaN.
 * STEP is 1, 2, 4, 8, 16 or 32.  1 evaluates every pixel: the defined result.  Above 1 the spline is evaluated on the LATTICE of window columns
 * and rows k step, k = 0 .. nodes - 1, nodes = max(2, (n + step - 2) / step + 1) for a window of n pixels along the axis: the last node lies
 * at or beyond the last pixel, so nodes may lie outside the window.  Node values go as f64 pairs into d_scratch (hg_tps_field_layout; 16-byte
 * aligned; per frame nodes_x x nodes_y x 16 bytes, frames at the 256-byte grain).  Pixel column c has k = min(c / step, nodes - 2) and fx =
 * (c - k step) / step, rows alike, and blends its four nodes in f64 as (n00 (1 - fx) + n01 fx) (1 - fy) + (n10 (1 - fx) + n11 fx) fy; it is
 * then tested and stored like any other.  A pixel on a node takes the node's value as it stands and equals the step-1 field bit for bit.
 * The mode is an APPROXIMATION whose error sits around the control points, where the spline's second derivative has a log singularity.  On
 * the numpy model, 68 points on a smooth deformation with 0.5 px of landmark noise: step 4 is off by 0.05 px at its worst pixel (mean
 * 0.0006), step 8 by 0.18 px (mean 0.0025); with 8 px of independent noise per landmark step 2 is already 0.5 px off at its worst pixel.
 * Measure on your own landmarks (tools/bench_tps.py reports the error per step).
 * hg_points_tps_frames_device sends point lists through the splines, in the layout of the point-list calls: d_points holds n_sets lists of
 * n_pts (x, y) float32, frame f reads list f % n_sets, d_out receives n_frames x n_pts pairs.  Positions are ABSOLUTE from-space positions
 * and there is no coverage test: the result is ((float)sx, (float)sy).  A position that is not finite, a failed frame and a result with a NaN
 * part hold 0x7fc00000 in both words; 1e30 is a legal input.  An integer position equals the HG_FIELD_COORDS field's value at that pixel where
 * the pixel is covered, bit for bit.
 * LIMITS (HG_ERR_INVALID), the shape before the context: n_points outside 3..1024; n_frames outside 0..4096; set counts below 1; lambda
 * negative or not finite; an unknown format or step; W or H below 1; for HG_FIELD_INDEX a source of 2^31 pixels or more; n_pts outside
 * 0..2^24; what hg_geom refuses; a field offset that is no multiple of the pixel size; then NULL or misaligned pointers when there is work,
 * and a NULL ctx.  n_frames == 0 (and n_pts == 0, and a set of empty windows) is HG_OK and nothing is written.
 * CONTEXT.  hg_tps_solve_frames_device settles what hg_fit_matches_frames_device settles (queued runs), the other two what their
 * counterparts settle; then each is asynchronous on the ctx stream.  None touches hg_last_*, the sampling mode, a plan, policy state or a
 * staged frame set.  Scratch comes from the caller and may be reused once the call that used it has completed.
 * COST.  n_points logarithms in f64 per pixel (the project's own, good to 2 ulp: 46 instructions per term).  MEASURED (MI355X, whole call,
 * medians of 9; EXPERIMENTS.md, "Thin-plate"; tools/bench_tps.py): 64 frames of 3840 x 2160, HG_FIELD_COORDS, 68 points: 45.5 ms at step 1
 * (7.9e11 terms / s, bound by f64 issue whatever n_points is), 5.1 ms at step 4, 2.0 ms at step 8, 1.5 ms at step 16; the solve 0.3 ms.  200
 * points: 132 / 11.3 / 3.5 / 1.9 ms, the solve 1.8 ms.  1024 points: 677 / 50 / 13 / 4.5 ms, the solve 221 ms (one workgroup per frame, the
 * matrix in scratch).  The piecewise coords field of the same 68 landmarks takes 1.9 ms; scipy's RBFInterpolator 5.3 s for ONE frame.  The
 * lattice's error on those frames, which move every landmark 77 px on its own (max / mean px): 68 points 0.30 / 0.005 at step 4, 0.89 / 0.02
 * at step 8; at 200 points, where that is more than the landmarks' spacing and the spline folds, 41 / 0.02 at step 4. */
enum { HG_TPS_MAX_POINTS = 1024 };
enum { HG_TPS_OK = 0, HG_TPS_SINGULAR = 1, HG_TPS_BAD_INPUT = 2 };
int hg_tps_layout(int n_points, int n_frames, size_t *record_bytes_per_frame, size_t *solve_scratch_bytes);
int hg_tps_solve_frames_device(hg_ctx *ctx, const void *d_from, int n_from_sets, const void *d_to, int n_to_sets, int n_points, int n_frames,
                               double lambda, double *d_records, int32_t *d_status, void *d_scratch);
int hg_tps_field_layout(const hg_geom *geoms, int n_frames, int step, size_t *scratch_bytes);
int hg_field_tps_frames_device(hg_ctx *ctx, const double *d_records, int n_points, const hg_geom *geoms, int n_frames, int W, int H,
                               int format, int step, const size_t *field_offsets, void *d_field, void *d_scratch);
int hg_points_tps_frames_device(hg_ctx *ctx, const double *d_records, int n_points, int n_frames, const void *d_points, int n_pts, int n_sets,
                                void *d_out);

/* ------------------------------------------------------------------------------------------------ camera models
 * Every geometry above is a map between two planes.  On a planar canvas the frames at the ends of a strip stretch without bound, and at 180
 * degrees the map is singular: a panorama wider than about 100 degrees needs a CYLINDER or a SPHERE as its canvas.  And real lenses bend
 * straight lines, which no homography follows.  These calls write the source field of a frame set from a CAMERA per frame -- a rotation,
 * focal lengths, a principal point and Brown-Conrady lens terms -- onto a plane, a cylinder or a sphere, and send point lists through the
 * same map in both directions.  Not part of the reference.  A field is what every remap, the pyramids, the mosaics, the multi-band and the
 * robust blend read; none of these calls needs an image, a mesh or a frame set.
 * All arithmetic is f64, IEEE division and square root, contraction off, in the operation order written here; sin, cos, atan2 are the
 * platform's, good to a few ulp, so values are pinned by tolerance.
 * RECORD of a frame: HG_CAMERA_RECORD_DOUBLES = 32 doubles.  [0..8] R, row-major, camera <- world; [9] fx [10] fy [11] cx [12] cy; [13] k1
 * [14] k2 [15] p1 [16] p2 [17] k3 (Brown-Conrady, OpenCV's meaning); [18] r2_max; [19] a_c, the azimuth atan2(w.x, w.z) of the optical axis
 * w = R^T (0, 0, 1); the other slots are 0.  World axes: x to the right, y down, z forward at azimuth 0.
 * SURFACE is HG_SURFACE_PLANE, HG_SURFACE_CYLINDER or HG_SURFACE_SPHERE.  The canvas parameters scale, u0, v0 are per call: pixels per radian
 * (for the plane: the canvas focal length) and the canvas position of azimuth 0, elevation 0.
 * CANVAS -> SOURCE at the canvas position (U, V): a = (U - u0) / scale, b = (V - v0) / scale;
 *   PLANE ray = (a, b, 1); CYLINDER ray = (sin a, b, cos a); SPHERE ray = (sin a cos b, sin b, cos a cos b);
 *   c = R ray, each component as ((r0 x + r1 y) + r2 z); xn = c.x / c.z, yn = c.y / c.z; r2 = xn xn + yn yn;
 *   rad = 1 + r2 (k1 + r2 (k2 + r2 k3));
 *   xd = xn rad + (((2 p1) xn) yn + p2 (r2 + (2 xn) xn));  yd = yn rad + (p1 (r2 + (2 yn) yn) + ((2 p2) xn) yn);
 *   sx = fx xd + cx, sy = fy yd + cy.
 * A pixel is covered iff c.z > 0, r2 <= r2_max, 0 <= sx < W and 0 <= sy < H (NaN fails), and its value is stored by the rules of the other
 * field calls: HG_FIELD_INDEX and HG_FIELD_COORDS mean exactly what they mean above, -1 and the NaN pattern included.  r2_max exists because
 * the radial polynomial folds back at large r: without it, rays far outside the picture land inside it.
 * SOURCE -> CANVAS at the source position (x, y): xd = (x - cx) / fx, yd = (y - cy) / fy; undistortion by the fixed-point rule, starting
 * from (xn, yn) = (xd, yd), exactly HG_CAMERA_UNDISTORT_ITERS = 20 rounds of
 *   r2, rad and the two tangential sums tx, ty (the bracketed terms above) at (xn, yn); xn <- (xd - tx) / rad, yn <- (yd - ty) / rad;
 * then (xn, yn) goes through the distortion once more and the point is valid iff it lands within 1e-9 of (xd, yd) in both parts (<=) and
 * r2 <= r2_max.  w = R^T (xn, yn, 1), each component as ((r0 xn + r3 yn) + r6).
 *   PLANE: valid iff w.z > 0; a = w.x / w.z, b = w.y / w.z.
 *   CYLINDER: a = atan2(w.x, w.z), b = w.y / sqrt(w.x w.x + w.z w.z).  SPHERE: a alike, b = atan2(w.y, sqrt(w.x w.x + w.z w.z)).
 *   On the two curved surfaces a is unwrapped about the frame's own axis: a = a_c + remainder(a - a_c, 2 pi), IEEE remainder, 2 pi =
 *   6.283185307179586: a frame that straddles the +-pi seam keeps a contiguous window.
 *   U = u0 + scale a, V = v0 + scale b.
 * Canvas positions beyond +-pi scale are legal everywhere, because sin and cos are periodic.
 * HOST CALLS (no device, no context; errors in hg_last_error(NULL)).
 *   hg_camera_pack_record fills a record, a_c included.  dist is {k1, k2, p1, p2, k3} or NULL.  Without distortion r2_max = +Infinity; with
 *     it r2_max = 1.05 x the largest undistorted r2 over the four corners and the four edge midpoints of [0, W] x [0, H], and the call
 *     returns HG_ERR_INVALID when one of those eight does not pass the validity rule above (taken with r2_max = +Infinity): the distortion
 *     is too strong for this picture.  It refuses NULL, W or H below 1, anything not finite, fx or fy <= 0 and an R with |R^T R - I| > 1e-6
 *     in any entry.
 *   hg_camera_limits returns the window {x_off, y_off, w, h} (the members of an hg_geom) that holds the frame: hg_transform_limits'
 *     counterpart.  Every border position of the source -- steps of one pixel along the four edges of [0, W] x [0, H] -- goes through
 *     source -> canvas in double; positions that are not valid or not finite are left out; the window reaches from floor(min) - 1 to
 *     ceil(max) + 1 on both axes, ends included.  On the sphere a pole direction (0, +-1, 0) that projects inside the picture (the coverage
 *     rule above) makes the window span a_c +- pi horizontally and reach the pole's row, v0 +- scale pi / 2; on the cylinder, where a pole
 *     lies at infinity, such a picture is refused.  HG_ERR_INVALID also when no border position is valid, for a record with a NaN and for a
 *     window hg_geom cannot hold.
 *   hg_camera_focals_from_matrix: the closed form of Szeliski & Shum for a homography H = K_to R K_from^-1 (row-major h0..h8, x_to ~ H
 *     x_from) between pictures whose coordinates are relative to their principal points, K = diag(f, f, 1).  K_to^-1 H K_from is a multiple
 *     of a rotation: its columns 0 and 1 are orthogonal and of equal length, which gives f_to^2 = -(h0 h1 + h3 h4) / (h6 h7) and
 *     f_to^2 = (h0^2 + h3^2 - h1^2 - h4^2) / ((h7 - h6)(h7 + h6)); its rows 0 and 1 alike, f_from^2 = -(h2 h5) / (h0 h3 + h1 h4) and
 *     f_from^2 = (h5^2 - h2^2) / (h0^2 + h1^2 - h3^2 - h4^2).  Each focal length takes the candidate with the larger denominator magnitude
 *     and is ok (1) iff that value is finite and > 0, else not ok (0) and 0: a rotation about the optical axis says nothing about either.
 *   hg_camera_rotation_from_matrix: K = {fx, fy, cx, cy}; M = K_to^-1 H K_from divided by cbrt(det M), HG_ERR_INVALID when det <= 0 or not
 *     finite; R9 = the nearest rotation by the polar iteration R <- (R + R^-T) / 2, 30 rounds in a fixed order.  R takes directions of
 *     the FROM camera to directions of the TO camera: with the TO camera's record rotation R_to, the FROM camera's is R^T R_to.
 *   Together with the matrices of hg_bundle_adjust_frames_device these take a caller from homographies to cameras.
 * hg_field_camera_frames_device writes the source field of n_frames cameras (d_records: n_frames records on the device, 8-byte aligned):
 * pixel (i, j) of frame f is the canvas position (i + x_off, j + y_off).  field_offsets, packing, alignment, "bytes between frames are never
 * written", the settling of queued runs and the context rules are those of hg_field_tps_frames_device.  A record with a NaN in any slot
 * gives a frame that is all -1 resp. all NaN; other frames are not affected.
 * hg_points_camera_to_source_frames_device sends point lists through canvas -> source, in the layout of the other point-list calls (n_sets
 * lists of n_pts (x, y) float32, frame f reads list f % n_sets, d_out receives n_frames x n_pts pairs): ABSOLUTE canvas positions, no test
 * against W or H, but c.z > 0 and r2 <= r2_max are tested.  An invalid point, a position that is not finite, a frame whose record holds a NaN
 * and a result with a NaN part hold 0x7fc00000 in both words; 1e30 is a legal input.  At an integer position the result equals the
 * HG_FIELD_COORDS value of that pixel, bit for bit, wherever the pixel is covered.  hg_points_camera_to_canvas_frames_device: the same
 * arguments, source -> canvas, with that direction's validity rule.
 * LIMITS (HG_ERR_INVALID), the shape before the context, in this order: an unknown surface or format; scale not finite or <= 0; u0 or v0 not
 * finite; W or H below 1; n_frames outside 0..4096; n_pts outside 0..2^24; set counts below 1; NULL geoms and what hg_geom refuses; for
 * HG_FIELD_INDEX a source of 2^31 pixels or more; a field offset that is no multiple of the pixel size; a widest and a tallest window that
 * together span 2^31 tiles of 256 x 32 pixels or more; then NULL or misaligned pointers where there is work, and a NULL ctx.  n_frames == 0
 * (and n_pts == 0, and a set of empty windows) is HG_OK and nothing is written.
 * COST.  a depends on the column only and b on the row only: a workgroup takes one frame, 256 columns and a band of 32 rows, evaluates the
 * 256 column terms and the 32 row terms once, and the pixel loop is two table reads, the 3 x 3 product, two divisions and the polynomial:
 * 576 sin / cos calls per 8192 pixels on the curved surfaces, none at all on the plane.  MEASURED (MI355X, whole call, medians of 9;
 * EXPERIMENTS.md, "Camera"; tools/bench_camera.py): 64 windows of 3840 x 2160, HG_FIELD_COORDS: plane 1.38 ms, cylinder 1.43 ms, sphere
 * 1.53 ms (1.105 x the plane), the same with lens terms (1.37 / 1.41 / 1.53 ms); the projective field of
 * hg_field_inverse_geometric_frames_device over windows of that size 0.87 ms; the byte floor of 8 bytes per pixel at 8 TB/s 0.53 ms.
 * The call is bound by f64 issue (the 3 x 3 product, two divisions, the polynomial), not by memory.
 * OUT OF SCOPE, each its own addition: a rotation / focal-length bundle adjustment; fisheye lens models (equidistant, stereographic);
 * estimating distortion coefficients; exposing the canvas as anything but a field. */
enum { HG_CAMERA_RECORD_DOUBLES = 32, HG_CAMERA_UNDISTORT_ITERS = 20 };
enum { HG_SURFACE_PLANE = 0, HG_SURFACE_CYLINDER = 1, HG_SURFACE_SPHERE = 2 };
/* host only */
int hg_camera_pack_record(const double *R, double fx, double fy, double cx, double cy, const double *dist, int W, int H, double *record);
int hg_camera_limits(const double *record, int W, int H, int surface, double scale, double u0, double v0, int32_t *out);
int hg_camera_focals_from_matrix(const double *H9, double *f_from, double *f_to, int *ok_from, int *ok_to);
int hg_camera_rotation_from_matrix(const double *H9, const double *K_from, const double *K_to, double *R9);
int hg_field_camera_frames_device(hg_ctx *ctx, const double *d_records, const hg_geom *geoms, int n_frames, int W, int H, int surface,
                                  double scale, double u0, double v0, int format, const size_t *field_offsets, void *d_field);
int hg_points_camera_to_source_frames_device(hg_ctx *ctx, const double *d_records, int n_frames, int surface, double scale, double u0,
                                             double v0, const void *d_points, int n_pts, int n_sets, void *d_out);
int hg_points_camera_to_canvas_frames_device(hg_ctx *ctx, const double *d_records, int n_frames, int surface, double scale, double u0,
                                             double v0, const void *d_points, int n_pts, int n_sets, void *d_out);

/* ------------------------------------------------------------------------------------------------ dense optical flow
 * Every registration above is parametric: six or eight numbers per frame, or landmarks somebody supplies.  Parallax, a rolling shutter and
 * things that move do not fit them.  hg_flow_dense_frames_device registers two pictures PER PIXEL -- pyramidal dense Lucas-Kanade -- and
 * writes the result as a HG_FIELD_COORDS source field, which every remap, the mosaics and the multi-band blend read.  Not part of the
 * reference.  It needs no image, mesh or frame set.
 * PLANES.  n_frames pairs of u8 planes of one size W x H, `channels` 1 or 4, interleaved; FROM plane f lies at d_from + f * from_stride_bytes,
 * TO plane s at d_to + s * to_stride_bytes, and FROM plane f is registered onto TO plane f % n_to_sets (the set rule of the matcher and the
 * aligner).  With 4 channels every pixel is first reduced to the integer luma of the detector and the aligner, (77 R + 150 G + 29 B + 128)
 * >> 8, into scratch; below, T and F are those one-byte planes.  The result of frame f is a field over TO's pixel grid whose values are FROM
 * positions: gathering FROM plane f through it with any remap gives FROM registered to TO.
 * All window sums are INTEGER sums, so their order is free, tiling cannot change a bit, and two runs give the same bytes.  Everything else is
 * f32 or f64 in the written order, IEEE division, ties to even, contraction off: a numpy model of this text matches the device byte for byte.
 * PYRAMIDS.  Levels 0 .. levels-1 of both luma planes are exactly what hg_pyramid_build_device builds of a one-channel u8 plane: level k+1
 * pixel (x, y) = ((a + b) + (c + d) + 2) >> 2 over columns min(2x, Wk-1), min(2x+1, Wk-1) and rows alike of level k, sizes (n + 1) >> 1.  The
 * call builds them itself, in scratch.
 * WALK, from level levels-1 down to level 0.  On a level, T and F are TO's and FROM's level of Wk x Hk pixels, and (u, v) is one f32 pair per
 * pixel.
 *   START.  The coarsest level starts from u = v = 0.  A finer level takes the flow of the level below it -- the (u, v) pairs as a 2-channel
 *     f32 plane of that level's size -- at cx = ((float)x + 0.5f) * 0.5f - 0.5f, cy alike, blended by exactly the rule of
 *     hg_remap_bilinear_f32_device (floorf, fraction, taps clamped in float, that operation order), each part then multiplied by 2.0f.
 *   GRADIENTS.  gx(q) = T(min(x+1, Wk-1), y) - T(max(x-1, 0), y), gy alike: integers in -255..255, TWICE the central difference.
 *     Gxx, Gxy, Gyy = the sums of gx gx, gx gy, gy gy over the window |dx|, |dy| <= radius around the pixel, clipped to the plane; n = the
 *     number of window pixels inside the plane.
 *   GOOD.  A pixel is good iff trace = Gxx + Gyy > 0, det = Gxx Gyy - Gxy Gxy > 0 and (double)det >= ((4.0 * n) * min_eig) * (double)trace.
 *     (det and trace are integers below 2^53, so the doubles are exact; det > 0 follows from the last test unless min_eig is 0, and keeps a
 *     division by zero out of the solve.)  det / trace lies between lmin / 2 and lmin, lmin being the smaller eigenvalue of the window's
 *     tensor of twice-gradients; divided by 4 n it is the per-pixel eigenvalue in true-gradient units that min_eig is compared with.
 *   ONE ITERATION, n_iter of them per level, Jacobi style: every pixel reads the flow of the iteration before.
 *     1. for every pixel q: s = the f32 bilinear blend (that same rule) of F at ((float)x + u(q), (float)y + v(q));
 *     2. e = s - (float)T(q), in f32;
 *     3. e0 = (double)e - (((double)gx * (double)u) + ((double)gy * (double)v)) / 2.0;
 *     4. eq = llrint(16.0 * e0), ties to even;
 *     5. for every pixel p, over its clipped window: bx = sum gx eq, by = sum gy eq, in 64-bit integers;
 *     6. if p is good, in f64: U = -((((double)Gyy * (double)bx) - ((double)Gxy * (double)by)) / (double)det) / 8.0,
 *                               V = -((((double)Gxx * (double)by) - ((double)Gxy * (double)bx)) / (double)det) / 8.0;
 *     7. d = U - (double)u, clamped to [-max_update, max_update]; u_new = (float)((double)u + d); v alike;
 *     8. a pixel that is not good keeps its flow.
 *   Every pixel's equation is linearised around its OWN flow (step 3 takes the pixel's flow back out), and the window solves for ONE common
 *   flow.  The cheaper u += -G^-1 sum g e, with e taken at every pixel's own flow, acts on the flow error as identity - box filter, has gain
 *   above 1 at some frequencies, and diverges (EXPERIMENTS.md, "Dense flow").
 * OUTPUTS, all asynchronous on the ctx stream.
 *   d_field     per frame W x H pairs ((float)x + u, (float)y + v) of level 0, in HG_FIELD_COORDS: a pixel is covered iff 0 <= sx < W and
 *               0 <= sy < H (the f32 values); every other pixel holds 0x7fc00000 in both words.  field_offsets (NULL: packed as
 *               hg_pack_field_offsets does), the multiple-of-8 rule, alignment and "bytes between frames are never written" are those of
 *               hg_field_tps_frames_device.
 *   d_flow      optional (NULL: not wanted): the raw (u, v) pairs with no coverage test, frame f at the same byte offset as in d_field.
 *   d_residual  optional: one byte per pixel, min(255, floor(|e| + 0.5f)) with e = s - (float)T taken once more at the FINAL level-0 flow;
 *               frame f at f * W * H.  A plane to threshold into a moving-object mask.
 *   d_good      optional: one byte per pixel, 1 where the pixel is good on level 0, else 0; frame f at f * W * H.
 * SCRATCH comes from the caller, as for the multi-band blend; the library allocates nothing.  hg_flow_layout (host only) gives the bytes: the
 * luma copies of 4-channel planes, the pyramids of both plane sets, and two flow buffers per level.  d_scratch is aligned to 16 bytes.  Only
 * d_scratch[0, bytes) and the outputs are written.  It may be reused once the call that used it has completed.
 * DEFAULTS the bindings use (from the model runs in EXPERIMENTS.md, "Dense flow"): levels such that the coarsest level is at least 16 pixels
 * on its shorter side, 4 iterations, radius 3, min_eig 1, max_update 1.  More iterations do not make the result worse; one level alone
 * cannot follow a flow of several pixels.
 * LIMITS (HG_ERR_INVALID), the shape before the context, in this order: W, H outside 1..32768 or W * H > 2^30; channels not 1 or 4; levels
 * outside 1..min(hg_pyramid_levels(W, H), 12); n_iter outside 1..32; radius outside 1..7; min_eig negative or not finite; max_update outside
 * (0, 4]; n_frames outside 0..4096; n_to_sets outside 1..max(n_frames, 1); a stride below W * H * channels; then a NULL ctx; then, with
 * n_frames > 0, a field offset that is no multiple of 8, NULL d_from / d_to / d_field / d_scratch, and misaligned d_field / d_flow (8 bytes) or
 * d_scratch (16).  n_frames == 0 is HG_OK and nothing is written.  With these limits |u| stays below 4 * 32 * 2^12, |eq| below 2^33, and every
 * window sum (at most 225 terms of |gx eq| < 2^41) below 2^53.
 * CONTEXT.  The call settles what hg_align_refine_frames_device settles (queued runs), then is asynchronous on the ctx stream: no host wait
 * between levels or iterations.  It touches no hg_last_*, no sampling mode, no plan, no policy state and no staged frame set.
 * COST.  Per pixel and iteration four taps of F, a halo of T and five window sums, formed separably in LDS by one workgroup per 32 x 16
 * tile; G is re-formed there every iteration instead of being stored.  MEASURED (MI355X, whole call, medians of 9; EXPERIMENTS.md, "Dense
 * flow"; tools/bench_flow.py): 64 RGBA pairs of 1920 x 1080 against one keyframe at the defaults (7 levels) 14.2 ms, at radius 7 28.6 ms; 8
 * pairs of 3840 x 2160 (8 levels) 7.2 / 14.4 ms: 5e10 pixel-iterations per second at radius 3, bound by the LDS passes and the 64-bit sums,
 * not by memory (the time doubles with the window's side).  One iteration of one 1080p frame costs 0.042 ms; a plain torch formulation
 * (grid_sample + avg_pool2d) 0.75 ms on the same GPU.  99.4 % of the pixels of those smooth pictures are good at radius 3.
 *
 * hg_field_compose_frames_device CHAINS two fields.  Flow is computed between pictures that were registered roughly before -- FROM warped
 * through a fitted homography's field --, and to feed a mosaic the flow field must be chained with that field: out(p) = inner(outer(p)).
 * Per pixel of frame f, where the outer coordinate is finite and both blended parts are finite, the result is that of
 * hg_remap_bilinear_frames_device with elem = HG_ELEM_F32 and channels = 2 on inner field f % n_inner (Wi x Hi pairs at d_inner +
 * (f % n_inner) * inner_stride_bytes), bit for bit; everywhere else -- a NaN or infinite outer coordinate, which that remap answers with 0, "covered,
 * pixel (0, 0)" to a consumer; an inner tap that is NaN or infinite -- both words hold 0x7fc00000.  Arguments, offsets (out_offsets: multiples
 * of 8, NULL: packed as hg_pack_field_offsets does), refusals and settling are those of hg_remap_bilinear_frames_device; d_out is aligned to 8. */
int hg_flow_layout(int W, int H, int channels, int n_frames, int n_to_sets, int levels, size_t *scratch_bytes);
int hg_flow_dense_frames_device(hg_ctx *ctx, const void *d_from, int n_frames, size_t from_stride_bytes, const void *d_to, int n_to_sets,
                                size_t to_stride_bytes, int W, int H, int channels, int levels, int n_iter, int radius, double min_eig,
                                double max_update, const size_t *field_offsets, void *d_field, void *d_flow, void *d_residual, void *d_good,
                                void *d_scratch);
int hg_field_compose_frames_device(hg_ctx *ctx, const hg_geom *geoms, int n_frames, const void *d_outer, const size_t *outer_offsets,
                                   const void *d_inner, int Wi, int Hi, int n_inner, size_t inner_stride_bytes, void *d_out,
                                   const size_t *out_offsets);

/* ------------------------------------------------------------------------------------------------ matching descriptors
 * The matcher that hands hg_fit_matches_frames_device its matches: for every frame a brute-force search of the nearest and second-nearest
 * train descriptor of every query descriptor, Lowe's ratio test, a distance cap and an optional cross-check, compacted into exactly the slot
 * format the fit reads.  Descriptors -> matches -> transforms -> warps -> mosaic then stay in device memory; only n_frames counts come down
 * to the host.  Not part of the reference.  Every result is an integer or a copied word: the call is exact, it has no tolerance.
 * DESCRIPTORS.  d_query holds n_frames lists of n_query rows of `stride` bytes, d_train holds n_train_sets lists of n_train rows; frame f
 * reads train list f % n_train_sets (the rule hg_set_images_device gives images; one keyframe for all frames is n_train_sets = 1).  Only the
 * first desc_bytes bytes of a row are data; the bytes from desc_bytes to stride are padding, may hold anything and never enter a distance.
 * stride is a multiple of 16 and >= desc_bytes; both buffers are 16-byte aligned.  counts_q (n_frames entries) and counts_t (n_train_sets
 * entries) are on the HOST; NULL = every slot.  Frame f uses its first cq = counts_q[f] query rows and the first ct = counts_t[f %
 * n_train_sets] train rows.
 * DISTANCES, exact non-negative integers.  HG_DESC_BITS (binary descriptors: ORB 32 bytes, BRISK 64, AKAZE 61): d = the number of set bits
 * of q XOR t over desc_bytes bytes (Hamming).  HG_DESC_U8 (byte vectors: SIFT as 128 x u8): d = the sum over k < desc_bytes of
 * (q_k - t_k)(q_k - t_k), bytes read as unsigned; at most 512 * 255 * 255 < 2^25.
 * NEIGHBOURS of query i < cq, with ct >= 1: d1 = the smallest distance over j < ct; j1 = the LOWEST j that attains it; d2 = the second entry
 * of the ascending multiset of the ct distances, so d2 == d1 when two train rows tie for the nearest; with ct == 1 there is no d2.  This is
 * a total order: the result does not depend on tiling or scheduling.
 * ACCEPTANCE.  Query i yields the pair (i, j1) iff all of
 *   1. d1 <= max_distance (uint32 comparison; 0xFFFFFFFF = no cap);
 *   2. the ratio test: ratio == 0 switches it off; otherwise, with ct >= 2, in f64 with the product rounded on its own:
 *        HG_DESC_BITS  (double)d1 < ratio * (double)d2
 *        HG_DESC_U8    (double)d1 < r2 * (double)d2, r2 = ratio * ratio rounded once in double (squared distances, squared ratio)
 *      so a tie d1 == d2 fails every ratio <= 1 (d1 == d2 == 0 included); with ct == 1 there is nothing to compare with and the test PASSES;
 *   3. with cross_check != 0: i is the best query of j1, where the best query of train row j is the query i' < cq with the smallest
 *      distance to j, the lowest i' among equals.
 * OUTPUTS, all in device memory.  d_counts is required; the others may be NULL and are then never written.
 *   d_counts[f]  the number of accepted pairs of frame f.
 *   d_pairs      n_frames x n_query x 2 int32: the accepted pairs (i, j1) of the frame compacted to the front in ascending i, the
 *                remaining slots (-1, -1).
 *   d_matches    n_frames x n_query slots (x, y, u, v) float32, 16-byte aligned: slot k describes pair k; (x, y) is the query row's
 *                position, (u, v) the train row's, copied bit for bit (NaN payloads included) from d_query_pts (n_frames x n_query x 2
 *                float32, 8-byte aligned) and d_train_pts (n_train_sets x n_train x 2, the list of f % n_train_sets); slots at and beyond
 *                d_counts[f] hold 0x7fc00000 in all four words.  Needs both point buffers.  This is d_matches of
 *                hg_fit_matches_frames_device with n_points = n_query and counts = the downloaded d_counts; the fit then gives the matrix
 *                query -> train.  For the matrix the inverse warps take (output -> source) pass the descriptors of the OUTPUT side (the
 *                keyframe, the panorama) as query and those of the frame to be warped as train.
 *   d_nn         n_frames x n_query x 4 int32 {j1, d1, d2, accepted}: the raw two-nearest answer, accepted = 1 or 0; d2 = -1 when
 *                ct == 1; {-1, -1, -1, 0} for i >= cq or ct == 0.
 * LIMITS (HG_ERR_INVALID), checked in this order (the shape first: those checks need no device): unknown kind; desc_bytes outside
 * 1..512; stride not a multiple of 16 or below desc_bytes; n_query outside 0..65536; n_train outside 0..65536; n_frames outside 0..4096;
 * n_train_sets outside 1..max(n_frames, 1); a counts_q[f] outside [0, n_query]; a counts_t[s] outside [0, n_train]; ratio not finite,
 * negative or above 1; NULL ctx; then, with n_frames > 0: d_counts NULL, d_query or d_train NULL while n_query > 0 and n_train > 0; a
 * misaligned pointer (descriptors and d_matches 16, points 8, the int32 outputs 4); d_matches without both point buffers.  n_frames == 0 is HG_OK and nothing is written.  n_query == 0 writes d_counts only, all
 * zeros.  n_train == 0 (or ct == 0) accepts nothing: zero counts, padding everywhere.
 * CONTEXT.  As the fit: no image, mesh or frame set is needed; queued runs are settled first, then the call is asynchronous on the ctx
 * stream; the counts are copied before it returns.  It touches no hg_last_*, no sampling mode, no plan, no policy state and no staged frame
 * set.  Its scratch (one 16-byte record per query row and, with cross_check, per train row of every frame) lives in buffers the context owns,
 * grown on demand and reused.  No floating-point atomics; the only atomics are integer minima on a total order ((d << 32) | i per train
 * row, the cross-check of HG_DESC_U8): two runs of one call give the same bytes.
 * COST.  n_frames x cq x ct distances.  HG_DESC_U8 runs on the i8 matrix cores.  cross_check runs the search a second time with the sides
 * swapped for HG_DESC_BITS (2 x) and folds the best query of a train row into the one search for HG_DESC_U8 (about 1.5 x).  MEASURED
 * (MI355X, whole call, medians of 31; EXPERIMENTS.md, "Matching"): 64 frames x 2048 x 2048 rows take 0.25 ms for 32-byte bits (1.1e12
 * pairs / s; 0.46 ms with cross_check) and 0.18 ms for 128-byte u8 (1.5e12 pairs / s; 0.27 ms); ONE frame x 4096 x 4096 takes 0.34 / 0.14 ms
 * -- a single frame fills only n_query / 64 workgroups, so frames are what the call scales over. */
enum { HG_DESC_BITS = 0, HG_DESC_U8 = 1 };
int hg_match_descriptors_frames_device(hg_ctx *ctx, int desc_kind, int desc_bytes, size_t stride,
                                       const void *d_query, int n_query, const int32_t *counts_q, int n_frames,
                                       const void *d_train, int n_train, const int32_t *counts_t, int n_train_sets,
                                       double ratio, uint32_t max_distance, int cross_check,
                                       const void *d_query_pts, const void *d_train_pts,
                                       int32_t *d_counts, void *d_matches, int32_t *d_pairs, int32_t *d_nn);

/* ------------------------------------------------------------------------------------------------ detecting and describing keypoints
 * The first stage of the chain descriptors -> matches -> transforms -> warps -> mosaic: corner detection, an orientation and a 256-bit binary
 * descriptor per keypoint, for a whole set of planes in one call, written in exactly the layout hg_match_descriptors_frames_device reads
 * (d_desc as d_query / d_train with HG_DESC_BITS and desc_bytes 32, d_points as d_query_pts / d_train_pts, the downloaded d_counts as counts_q
 * / counts_t, n_slots as n_query / n_train).  Not part of the reference.  Every rule is integer arithmetic: the result is exact, it has no
 * tolerance, ties included, and two runs give the same bytes.  It is NOT ORB-compatible: the sampling pattern is this library's own, generated
 * by a rule; both sides of a match come from this call, so it only has to agree with itself.  It is single-scale: for octaves run it on the
 * levels of hg_pyramid_build_device and scale the positions.
 * PLANES.  n_planes planes of u8, W x H, rows tight, `channels` 1 or 4 (interleaved); plane p lies at d_planes + p * plane_stride_bytes.
 * LUMA L.  1 channel: the byte.  4 channels: L = (77 R + 150 G + 29 B + 128) >> 8; alpha is ignored.  Everything below is integers on L.
 * RESPONSE R(x, y), for 4 <= x < W - 4 and 4 <= y < H - 4.  Sobel, y growing downwards: Ix = (L[y-1][x+1] + 2 L[y][x+1] + L[y+1][x+1]) - (the
 * same three at x - 1), Iy = (L[y+1][x-1] + 2 L[y+1][x] + L[y+1][x+1]) - (the same three at y - 1).  A, C, B = the sums of Ix Ix, Iy Iy, Ix Iy
 * over the 7 x 7 window centred on (x, y) (each at most 49 * 1020^2: int32).  R = 16 (A C - B B) - (A + C)^2 in int64: Harris with k = 1/16,
 * |R| < 2^56.
 * CANDIDATES.  A pixel with 16 <= x < W - 16 and 16 <= y < H - 16 is a candidate iff R >= min_response and it beats each of its 8 neighbours
 * under the total order "larger R, among equal R the lower flat index y W + x".  A plane with W < 33 or H < 33 has none.  No read leaves the
 * plane: the deepest reach is the orientation disc, radius 15 (the turned tests reach 13, the 5 x 5 boxes on them 15).
 * SELECTION.  The plane is tiled from (0, 0) by cell x cell cells, cells_x = ceil(W / cell), cells_y alike; a pixel belongs to cell
 * (y / cell) cells_x + x / cell.  Each cell keeps its best per_cell candidates under the same order.  The keypoints of a plane are listed by
 * ascending cell number, within a cell by rank.  n_slots = cells_x cells_y per_cell is the capacity of a plane's list (hg_detect_layout).
 * The bucketing is deliberate: a global top-K clusters on one textured object, a panorama needs matches spread over the overlap.
 * ORIENTATION.  Over the disc dx^2 + dy^2 <= 225: m10 = sum dx L, m01 = sum dy L (int32).  Direction table, 32 bins, Q14: c_0..c_8 = 16384,
 * 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0; c_{16-k} = -c_k; c_{32-k} = c_k; s_k = c_{(k + 24) mod 32}.  The bin is the k that maximises
 * m10 c_k + m01 s_k in int64, the lowest k among equals (a flat patch: 0).
 * PATTERN.  mix(a): a ^= a >> 16; a *= 0x7feb352d; a ^= a >> 15; a *= 0x846ca68b; a ^= a >> 16 in uint32 (the fit's).  Test b = 0..255:
 * key = mix(mix(0x9e3779b9) + b); the words w_t = mix(key + t), t = 0, 1, ..., each propose a point x = (w & 7) + ((w >> 3) & 7) + ((w >> 6) & 7)
 * + ((w >> 9) & 7) - 14, y the same from bits 12, 15, 18, 21; a point with x^2 + y^2 > 144 is skipped; the first kept point is a, the next kept
 * point that differs from a is b.  (Tests 0, 1, 2 are {-1,1,0,0}, {-3,2,10,-3}, {-3,-6,1,4}; test 139 repeats test 79, which is accepted.)
 * Bin k turns every point with arithmetic shifts: x' = (x c_k - y s_k + 8192) >> 14, y' = (x s_k + y c_k + 8192) >> 14; bin 0 is the base
 * pattern; every turned coordinate lies in -12..12.  hg_describe_pattern returns the table.
 * DESCRIPTOR.  S(x, y) = the sum of L over the 5 x 5 box centred on (x, y).  Bit b, stored in byte b >> 3 at bit b & 7, is 1 iff
 * S(p + a'_b) < S(p + b'_b) with the turned table of the keypoint's bin.
 * OUTPUTS, all in device memory; d_counts is required, the others may be NULL and are then never written.
 *   d_counts[p]  int32, 4-byte aligned: the number of keypoints of plane p.
 *   d_points     n_planes x n_slots x 2 float32, 8-byte aligned: (x, y) as floats of the integer pixel position, compacted to the front in
 *                list order; 0x7fc00000 in both words at and beyond the count.  The layout of d_query_pts.
 *   d_desc       n_planes x n_slots rows of desc_stride bytes (a multiple of 16, >= 32), 16-byte aligned: the first 32 bytes of a row are the
 *                descriptor, 32 zero bytes at and beyond the count; bytes 32..desc_stride of every row are never written.
 *   d_info       n_planes x n_slots x {int64 R, int32 bin, int32 flat index}, 8-byte aligned; {0, -1, -1} at and beyond the count.
 * LIMITS (HG_ERR_INVALID), checked in this order (the shape first: those checks need no device; each names itself in hg_last_error): W or H
 * outside 1..32768 or W H > 2^30; channels not 1 or 4; cell outside 8..256; per_cell outside 1..16; n_slots > 65536 (the matcher's row limit);
 * n_planes outside 0..4096; min_response < 1; desc_stride not a multiple of 16 or below 32; plane_stride_bytes < W H channels; NULL ctx; then,
 * with n_planes > 0: d_planes or d_counts NULL, a misaligned pointer.  n_planes == 0 is HG_OK and nothing is written.  hg_detect_layout makes
 * the shape checks that concern it (W, H, cell, per_cell, n_slots) and refuses NULL outputs; hg_describe_pattern refuses NULL.
 * CONTEXT.  As the matcher: no image, mesh or frame set is needed; queued runs are settled first, then the call is asynchronous on the ctx
 * stream.  It touches no hg_last_*, no sampling mode, no plan, no policy state and no staged frame set.  Its scratch (one 16-byte record per
 * slot, one count per cell, one index per slot, and the turned table, uploaded once per context) lives in buffers the context owns, grown
 * on demand and reused.  No floating-point operations and no atomics at all.
 * COST.  Three kernels: the response and the per-cell selection (one workgroup per cell; the halo of 5 makes small cells redundant: about
 * 5x the pixels at cell 8, 1.7x at cell 32), the compaction (one workgroup per plane) and the description (one wavefront per slot).
 * The call is bound by the integer work of the response, not by memory.  MEASURED (MI355X, whole call with all four outputs, medians of 31;
 * EXPERIMENTS.md, "Detecting"; cell 32, per_cell 2, planes of a many-cornered scene): 64 planes of 1920 x 1080 x 4 take 2.36 ms (35 x the
 * 0.066 ms of reading them once at 8 TB/s; 63 % response and selection, 1 % compaction, 36 % description), 8 planes of 3840 x 2160 x 4
 * 1.20 ms, ONE such plane 0.24 ms (the compaction, one workgroup per plane, is a quarter of that); the 1-channel forms 2.20 / 1.17 / 0.23 ms.
 * Against cell 32, at per_cell 1, the 64-plane call costs 5.9 x at cell 8, 2.5 x at cell 16, 0.9 x at cell 64 and 128 (fewer keypoints to
 * describe; the first two kernels alone: 6.1 x, 2.3 x, 1.1 x, 1.2 x) and 1.2 x at cell 256 (1.6 x). */
enum { HG_DETECT_MARGIN = 16, HG_DETECT_DESC_BYTES = 32, HG_DETECT_BINS = 32 };
/* host only: the cell grid and the capacity of a plane's list */
int hg_detect_layout(int W, int H, int cell, int per_cell, int *cells_x, int *cells_y, int *n_slots);
/* host only: HG_DETECT_BINS x 256 x 4 int8 = {ax, ay, bx, by} of test b under bin k */
int hg_describe_pattern(int8_t *out);
int hg_detect_describe_frames_device(hg_ctx *ctx, const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int channels,
                                     int cell, int per_cell, int64_t min_response, size_t desc_stride,
                                     int32_t *d_counts, void *d_points, void *d_desc, void *d_info);

/* ------------------------------------------------------------------------------------------------ forward (scatter) paths
 * What warp() dispatches to when the output is not larger than the input (:421, :426).  `m` is the FORWARD matrix
 * (_transformMatrix).  Sequential "last writer in raster order wins" is reproduced deterministically (atomicMax of the
 * raster rank per output pixel, then a gather).  Synchronous, host output of 4*obj_w*obj_h bytes. */
/* _geometricWarp :911-932.  Limits of the forward paths (HG_ERR_INVALID beyond): source image resp. source-point bounding box
 * below 2^31 pixels and at most 65535 rows; windows as for the inverse paths. */
int hg_warp_forward_geometric(hg_ctx *ctx, int kind, const double *m, hg_geom geom, uint8_t *out_host);
/* Same, asynchronous into GPU memory; batch = n frames (m = n x 8 doubles) back to back, frame f at out_offsets[f]. */
int hg_warp_forward_geometric_device(hg_ctx *ctx, int kind, const double *m, hg_geom geom, void *d_out);
int hg_warp_forward_geometric_batch_device(hg_ctx *ctx, int kind, const double *m, const hg_geom *geoms, const size_t *out_offsets,
                                           int n_frames, void *d_out);
/* _piecewiseAffineWarp :948-972 on the mesh of hg_piecewise_set_mesh (whose min_src_x/y are the loop origin);
 * max_src_x/y = rounded source-point bbox maximum (:758); the forward triangle map :817-832 is rebuilt on the device. */
int hg_warp_forward_piecewise(hg_ctx *ctx, const float *dst_points, int max_src_x, int max_src_y, hg_geom geom, uint8_t *out_host);
/* Same, asynchronous into GPU memory; batch = the caller loop `setDestinyPoints(d_f); warp()` for n destination point sets
 * (dst_points = n_frames x n_points x,y) when warp() takes the forward path (:421).  Like the inverse `_device` entry points
 * the frames are final after hg_sync (or any hg_copy_to_host): a frame the tile-binned kernels flagged is redone there. */
int hg_warp_forward_piecewise_device(hg_ctx *ctx, const float *dst_points, int max_src_x, int max_src_y, hg_geom geom, void *d_out);
int hg_warp_forward_piecewise_batch_device(hg_ctx *ctx, const float *dst_points, int max_src_x, int max_src_y, const hg_geom *geoms,
                                           const size_t *out_offsets, int n_frames, void *d_out);

/* ------------------------------------------------------------------------------------------------ reference-state forms
 * The reference caches two things across calls and its loops read them AS THEY STAND:
 *   - `_piecewiseMatrices` (:769): solved at setDestinyPoints, NOT invalidated by setTriangles (:519) nor -- once a map exists -- by
 *     setSourcePoints (:252-255);
 *   - `_trianglesCorrespondencesMatrix`: ONE field for the forward map (:819-820, source points over the source bounding box) and the
 *     inverse map (:847-848, destiny points over the output window).  After an inverse warp, _piecewiseAffineWarp :957 indexes the
 *     stale inverse map with forward indices ((y - minSrcY) * (maxSrcX - minSrcX) + (x - minSrcX)); cells past its end read
 *     `undefined` and are skipped.
 * A binding that mirrors those caches (js/Homography.mjs does, as value snapshots) uses the entry points above whenever both are
 * current -- the only state a fresh instance can be in -- and these two otherwise.  They take the cached state explicitly: the
 * FORWARD matrices as they were last solved (6 floats per triangle, hg_solve_affine_triangles of the snapshot) and the definition
 * of the map the field holds (the point set + triangles fillTriangle rasterised, matrix_width, height = length / width, yOffset).
 * Exact for any input (materialised map: atomicMax rasteriser + the pixel loop reading it), synchronous, host output of
 * 4 * obj_w * obj_h bytes.  HG_ERR_RANGE when a cell the loop reads holds an id >= n_mats (JS: TypeError at that pixel); the forward
 * form makes that check for a blank window too (the reference's loop runs over the source bounding box whatever the output size).
 * LIMITS of these two forms (HG_ERR_INVALID, a string error in the class, where the reference would still produce pixels or fail
 * differently -- none of them reachable from finite pixel coordinates of images that fit the other entry points): a map coordinate
 * that is infinite or beyond 2^24 in magnitude (NaN is legal: such a triangle rasterises nothing); |map y_off| > 2^26; a map of 2^31
 * cells or more; forward form: a source-point bounding box of 2^31 pixels or more, or taller than 65 535 rows.  Triangle ids are the
 * reference's Int16Array values: with more than 32 767 triangles they wrap (id 32 768 reads back as -32 768 = "no triangle"),
 * reproduced as such. */
typedef struct hg_tri_map_def {
    const float *points; int n_points;              /* interleaved x,y of the point set the map was rasterised from */
    const uint32_t *triangles; int n_triangles;
    int32_t width, height, y_off;                   /* fillTriangle's matrix_width, Int16Array length / width, yOffset (:1111) */
} hg_tri_map_def;
/* affineMatrixFromTriangles for every triangle of a mesh (:785-804; host, no GPU): out = 6 floats per triangle; a vertex id beyond
 * n_points reads `undefined` -> NaN like the reference's Float32Array scratch. */
int hg_solve_affine_triangles(const float *src_points, const float *dst_points, int n_points, const uint32_t *triangles, int n_triangles, float *out);
/* _inversePiecewiseAffineWarp :1029-1058 with stale matrices: the map is always the one of the current destiny points over the
 * current window (:1033), so map->width / height / y_off must equal geom's obj_w / obj_h / y_off. */
int hg_warp_inverse_piecewise_state(hg_ctx *ctx, const float *fwd_mats, int n_mats, const hg_tri_map_def *map, int min_src_x, int min_src_y,
                                    hg_geom geom, uint8_t *out_host);
/* _piecewiseAffineWarp :948-972 over whatever map the shared field holds. */
int hg_warp_forward_piecewise_state(hg_ctx *ctx, const float *fwd_mats, int n_mats, const hg_tri_map_def *map, int min_src_x, int min_src_y,
                                    int max_src_x, int max_src_y, hg_geom geom, uint8_t *out_host);

/* ------------------------------------------------------------------------------------------------ several GPUs, one host thread
 * The caller loop `for (f) { setDestinyPoints(dst_f); warp(); }` (test/benchmark.js:107-110) spread over the devices of one
 * node for hosts that cannot run one process per GPU (the Node binding).  Frames are independent: device i
 * of G warps the contiguous block hg_multi_partition() assigns to it, no data-path collective; the shared source texture is
 * fanned out once per hg_multi_set_image over xGMI peer copies (scatter of 1/G slices from device 0, then an all-gather
 * between the peers, so that every point-to-point link carries 1/G of the image instead of one link carrying all of it).
 * A device id may be listed more than once (several contexts on one GPU). */
typedef struct hg_multi hg_multi;
int hg_multi_create(const int *device_ids, int n_devices, hg_multi **multi);
void hg_multi_destroy(hg_multi *multi);
const char *hg_multi_last_error(const hg_multi *multi);
int hg_multi_device_count(const hg_multi *multi);
hg_ctx *hg_multi_ctx(hg_multi *multi, int index);                       /* the per-device context (options, taps) */
/* hg_set_sampling on every per-device context (HG_ERR_INVALID for an unknown mode, no context changed). */
int hg_multi_set_sampling(hg_multi *multi, int mode);
/* Peer access is checked and enabled pair by pair at hg_multi_create.  hg_multi_peer_note: "" when every pair of distinct devices
 * has it, else a text listing the pairs without ("no peer access: 2->3, 3->2"); hg_multi_peer_access: 1 / 0 for one ordered pair of
 * indices into the device list (-1: bad index).  A pair without access only re-routes ITS copies of the source fan-out. */
const char *hg_multi_peer_note(const hg_multi *multi);
int hg_multi_peer_access(const hg_multi *multi, int from_index, int to_index);
/* Pure function (no GPU): the copy plan of the source fan-out for n_devices devices and the access matrix access[p * n_devices + q]
 * (non-zero: device q copies straight out of device p's memory).  Returns the number of copies and writes up to max_ops of them, 4
 * ints each: {destination index, source index or -1 = the caller's host buffer, slice, phase 0 scatter / 1 all-gather}.  Scatter:
 * slice q goes to device q from device 0; all-gather: q takes slice p from its owner p, else from device 0 (which holds every
 * slice), else from the host.  With full access every ordered pair of devices carries exactly one 1/n slice. */
int hg_multi_plan_fanout(int n_devices, const uint8_t *access, int32_t *ops, int max_ops);
/* Pure function: frames [*first, *first + *count) of n_frames belong to device `index` of n_devices (sizes differ by <= 1). */
int hg_multi_partition(int n_frames, int n_devices, int index, int *first, int *count);
/* Returns once the host buffer has been read (H2D into device 0, plus the slices of devices no other device can serve).  The fan-out
 * between the devices is NOT waited for: every device's warp stream waits for the event "whole image here", so device 0's
 * first frames overlap the scatter + all-gather. */
int hg_multi_set_image(hg_multi *multi, const uint8_t *rgba, int width, int height);
int hg_multi_piecewise_set_mesh(hg_multi *multi, const float *src_points, int n_points, const uint32_t *triangles, int n_triangles,
                                int min_src_x, int min_src_y);
/* dst_points = n_frames x n_points x,y; out_host = NULL (frames stay on their devices: hg_multi_frame) or n_frames host
 * pointers of 4*obj_w*obj_h bytes each (pinned memory from hg_host_alloc lets the devices' copies overlap).  Synchronous. */
int hg_multi_warp_piecewise_batch(hg_multi *multi, const float *dst_points, const hg_geom *geoms, int n_frames, uint8_t *const *out_host);
/* The same for affine / projective frames given as point sets (see hg_geometric_set_frames_points): the matrix of frame f maps
 * from[f] -> to[f] (3 or 4 points each) and is solved on the device that warps the frame. */
int hg_multi_warp_geometric_batch(hg_multi *multi, int kind, const float *from, const float *to, const hg_geom *geoms, int n_frames,
                                  uint8_t *const *out_host);
/* One source per frame -- the video loop `for (f) { warp(frame_f) }` (README.md:121-137), SURVEY.md §8e's "replicas only" branch:
 * images[f] = width x height RGBA8 in host memory for frame f; every device uploads the images of ITS block only, there is no
 * exchange between devices at all.  Afterwards the contexts read those per-frame sources: call hg_multi_set_image again
 * before the next shared-source batch. */
int hg_multi_warp_piecewise_batch_images(hg_multi *multi, const float *dst_points, const hg_geom *geoms, int n_frames,
                                         const uint8_t *const *images, int width, int height, uint8_t *const *out_host);
int hg_multi_warp_geometric_batch_images(hg_multi *multi, int kind, const float *from, const float *to, const hg_geom *geoms, int n_frames,
                                         const uint8_t *const *images, int width, int height, uint8_t *const *out_host);
/* Where frame f of the last batch lives: index into the device list, device pointer, byte size (any of them may be NULL). */
int hg_multi_frame(hg_multi *multi, int frame, int *device_index, void **d_ptr, size_t *bytes);

/* Which kernel produced the last fused piecewise warp of this ctx (tests / profiling): 0 = none yet, 1 = k_pw_rows with
 * 4-row groups, 2 = k_pw_rows one row per workgroup, 3 = k_pw_patch (dense sheared meshes), 4 = k_pw_fused (general),
 * 5 = k_pw_tile (8-row tiles whose gathers follow the source rows: one source per frame, steeply sheared or very dense meshes). */
int hg_last_piecewise_kernel(hg_ctx *ctx);
/* ... and which template instantiation of it (tools/census.py: the census of what the layout policy really picks): kind * 100000 +
 * (512-slot rows) * 10000 + windows / blocks per phase * 1000 + (8-byte row entries) * 100 + (bounds on the high dwords) * 10 + self-span
 * form; kind 1 k_pw_rows, 3 k_pw_rows_s80, 4 k_pw_patch, 5 k_pw_tile, 6 k_pw_fused, 8 k_pw_patch with records in global memory. */
int hg_last_piecewise_variant(hg_ctx *ctx);
/* Which kernel ran the last inverse geometric warp of this ctx (tests / profiling): -1 = none yet; 100 * KIND + 10 * NW + S for
 * k_geo_fast<KIND, NW, S> (KIND 0 affine with f32-valued entries, 2 affine with arbitrary doubles, 1 projective with IEEE divisions,
 * 3 projective in the proven plain division range, 4 projective per frame from the device-side solve; NW windows per wave; S the
 * sampling mode); 1000 + 10 * kind + S for the generic k_geo<kind, S> (kind HG_AFFINE / HG_PROJECTIVE), which takes sources of 2^20
 * pixels or more in width or height, sources of 2 GiB or more, and windows of 2^28 pixels or more in width. */
int hg_last_geometric_kernel(hg_ctx *ctx);
/* 1 if that run's row workgroups evaluated their own spans (k_tri_setup + k_pw_rows<SELF>: no row lists, no slot atomics, option
 * "self_spans"), 0 if they read the per-output-row span lists of k_tri_spans. */
int hg_last_piecewise_self(hg_ctx *ctx);
/* Which kernels ran the last forward warp: 0 = none yet, 1 = scatter (atomicMax on a winner buffer) + gather, 2 = the
 * tile-binned gather (output tiles gather their source pixels, winners resolved in LDS, one or two launches for the whole
 * batch): k_fwd_tiles for affine / projective matrices that pass the admissibility bounds, k_fwd_pw_bins + k_fwd_pw_tiles
 * for piecewise meshes (frames the device cannot bound are flagged and redone through 1 by hg_sync; hg_redone_frames counts
 * them).  Option "fwd_tiles": -1 by size and mesh density (default), 0 never, 1 whenever admissible. */
int hg_last_forward_kernel(hg_ctx *ctx);
/* Host-side admission test of k_fwd_tiles (no GPU needed): 0 = this forward matrix (6 or 8 doubles) / source size / window
 * goes through scatter + gather; 1 = admissible; 2 = admissible and the inverse is trusted for the per-tile source row range.
 * Bounds: DESIGN.md §4.7 / EXPERIMENTS.md (matrix magnitudes, projective denominator >= 1e-2 at the source corners, no source pixel more than
 * 30 columns outside the window, window at least 64 wide). */
int hg_forward_tiles_admissible(int kind, const double *m, int W, int H, hg_geom geom);
/* Status word of the last frame a fused piecewise run flagged (0 = none since hg_create; diagnostics): bit 0 = a triangle with
 * non-finite / absurd vertices, bit 1 = a kernel's limits (more spans in a row than its lists or LDS blocks hold, more candidate triangles
 * than a workgroup's list); with bit 1, bits 4.. say which limit of k_pw_rows<SELF> / k_pw_patch<SELF> / k_pw_tile and the count. */
int hg_last_piecewise_flag(hg_ctx *ctx);
/* Frames the fused kernels only flagged (row lists / kernel limits exceeded, irregular spans) and hg_sync redid through the
 * materialised map, since the ctx was created (tests / profiling: a steady-state workload should show 0). */
long hg_redone_frames(hg_ctx *ctx);
/* Host-side walks over every triangle of a frame set (the layout estimate of hg_piecewise_set_frames) since the ctx was created:
 * a caller that uploads fresh points of one mesh and window shape per step should see this stand still. */
long hg_layout_walks(hg_ctx *ctx);
/* The span cache of k_pw_rows<SELF> in packed 4-row groups (options "span_cache", "span_cache_mb"): while the frame set, the mesh, the source's
 * dimensions and the plan stay the same, warps of the set copy the per-row span slots an earlier warp of it wrote to device memory instead of
 * evaluating the spans again.  out: builds since the ctx was created, warps that ran from the cache, and -- of the build the ctx holds for the
 * current frame set, 0 without one -- 4-row groups with valid records, groups that found no room, bytes held; then the state of the last
 * inverse piecewise warp (0 off, 1 build, 2 use).  Waits for the stream.  Results never depend on the cache. */
int hg_span_cache_stats(hg_ctx *ctx, int64_t out[6]);
/* Layout knobs of the piecewise fast path; they never change results (tests run the parity suite under each setting), only
 * which kernel layout the next hg_piecewise_set_frames picks:
 *   "min_row_groups" (default 1152): frame sets with fewer 4-row groups run one row per workgroup on row lists (k_pw_patch sets keep
 *           the self-span form down to half of it);
 *   "patch" (default -1 = by estimate: rows of more than 56 spans in a frame set that fits the kernel, and every set that fits it when
 *           each frame reads its own source): 0 never use k_pw_patch, 1 use it whenever the frame width allows, 2 the same in its
 *           global-record variant;
 *   "phase" (default -1 = 2 for a shared source -- 4 when the rows carry 3 or more spans per window --, 1 with one source per frame):
 *           windows per gather/store phase of k_pw_rows on ROW LISTS, 1, 2 or 4 (the self-span form always takes 4, k_pw_patch 8 column
 *           blocks: the other depths were never picked by the policy and are gone since round 6);
 *   "geo_windows" (default 8): 256-pixel windows per wave of the affine / projective kernel, 1, 2, 4 or 8;
 *   "self_spans" (default -1 = by policy; 1 = whenever eligible: sparse meshes of up to 8192 triangles; 0 never): no span
 *           producer kernel and no per-output-row span lists -- k_tri_setup writes every triangle's edge equations, inverse matrix
 *           and row reach, and each row workgroup of the warp kernel picks the triangles that reach its rows and evaluates
 *           predictXLimits + the fill() indices for exactly those rows in its prologue.  Bit-identical;
 *   "hi_bounds" (default 1): the source-bounds tests of the pixel loops (:1047, :1001) as 32-bit compares on the high dwords
 *           of the rounded coordinates (exact whenever the source window starts at >= 0 and ends below 2^20; the kernels
 *           fall back to the fp64 compares by themselves otherwise), 0 = always the fp64 compares;
 *   "compact" (default -1 = by estimate: dense rows, or whenever k_pw_patch reads the lists): 1 / 0: 8-byte span-list entries (the
 *           consumer fetches the matrix by triangle id) / 32-byte entries carrying the matrix;
 *   "tri_group" (default -1 = by mesh size: meshes of >= 384 triangles in sets of >= 2048 (frame, triangle) pairs): 16 or 64 (any
 *           other non-zero value = 16): the span producer takes that many triangles per workgroup and solves them one per lane
 *           (k_tri_spans_grouped) instead of one triangle per workgroup whose waves all repeat its solves (k_tri_spans, the
 *           lower-latency choice for a single frame and for sparse meshes); 0: never;
 *   "xcc_rotate" (default -1 = by estimate): 1: XCD x walks row band (x + frame) mod XCCs instead of band x -- even load where
 *           rows differ in cost or the frames share no source; 0: fixed bands (a shared source's band stays in that XCD's L2);
 *   "sub_bands" (default -1 = by the source's size: as many as bring a sub-band's share of the source to ~2.2 MB -- 2 for a 4K source, none for
 *           1080p; 0 / 1 none; 2..64): with ONE source shared by several frames and fixed bands, the rows of a frame are cut into sub-bands that are
 *           dealt to the XCDs round robin, and an XCD takes all frames of one of its sub-bands before the next: the slice of the source a sub-band
 *           reads then stays in that XCD's 4 MiB L2 from frame to frame (k_pw_rows / k_pw_patch / k_pw_tile);
 *   "xcc" (default: hipDeviceAttributeNumberOfXccs of the device, 8 on an unpartitioned MI355X): number of XCCs the
 *           block id -> row band mapping of the warp kernels assumes; a power of two in 1..64;
 *   "upload_kernel" (default -1 = on): frame-set blocks of up to 1 MB go from their page-locked staging slot to the device by a small kernel
 *           that reads host memory instead of a stream-ordered hipMemcpyAsync (whose copy-engine start-up cost 10-15 us per set); 0: always
 *           the copy engine;
 *   "safe_spans" (default -1 = rows of fewer than 3 spans per 256-pixel window; 1 / 0 force / forbid): k_pw_rows flags every span whose two end
 *           pixels pass the source bounds test :1047 (then every pixel between them does: the affine coordinates are monotone along a row) and
 *           runs windows made only of such spans without the per-pixel test, Math.round with one add per coordinate;
 *           k_pw_patch<SELF> does the same per 64-pixel x 4-row block (on unless the option says 0);
 *   "span_cache" (default -1): the span cache of k_pw_rows<SELF> in 4-row groups on a shared source (hg_span_cache_stats): -1 the second warp
 *           of a frame set writes the per-row span slots to device memory and the warps after it copy them instead of evaluating spans, 0 off
 *           (the launches of a library without it), 1 the first warp builds (tests, fuzzers);
 *   "span_cache_mb" (default 256): its budget in MB; a set whose estimated records exceed it is not cached at all.  A negative value is a budget
 *           of that many KB which the estimate does not veto: the groups that find room are cached, the others evaluate their spans as ever;
 *   "tile" (default -1 = wherever k_pw_patch would evaluate its own spans and either every frame reads its own source or, on a shared
 *           source, the mesh is steeply sheared (estimate >= 0.3) or packs more than two spans into a 64-pixel block -- and the host's
 *           estimate says a tile row holds its spans; 1 = whenever k_pw_patch<SELF> would run; 0 never): k_pw_tile instead of k_pw_patch -- 8 x 2048-pixel tiles, gathers in 8-pixel runs along the source
 *           rows; a tile beyond its limits (96 spans per row and tile, 128 triangle pieces) flags its frame, hg_sync
 *           redoes it and the mesh goes back to k_pw_patch;
 *   "fwd_tiles": see hg_last_forward_kernel;
 *   "remap_pack" (default -1 = on): hg_remap_index_frames_device gives a lane 4 consecutive 1-byte pixels and one packed store (the
 *           only pixel size for which that was measured to win); 0: one pixel per lane, for measurements;
 *   "match_cross" (default -1): the cross-check of hg_match_descriptors_frames_device for HG_DESC_U8 finds the best query of a train row
 *           by atomicMin inside the search; 0: by a second search with the sides swapped (what HG_DESC_BITS always does), for measurements.
 *           The results never depend on it.
 * Unknown keys are refused (HG_ERR_INVALID). */
int hg_set_option(hg_ctx *ctx, const char *key, int value);
/* Number of XCCs the ctx maps row bands to (what hg_create read from the device, or the "xcc" option). */
int hg_xcc_count(const hg_ctx *ctx);
/* Host-side proof obligation of that division (no GPU needed): 1 if every pixel of the window `geom` under the inverse
 * projective matrix m[8] keeps numerators and denominator in the plain range (entries 0 or in [2^-100, 2^100], coordinates
 * below 2^28, denominator of one sign and in [2^-100, 2^130] at the four corners), else 0 (-> IEEE divides in the kernel). */
int hg_projective_plain_range(const double *m, hg_geom geom);
/* Host-side proof obligation of the piecewise row kernel's one-fma form (no GPU needed): 1 if, for every integer pixel (x, y) of the window
 * `geom`, (m0*x) + (m2*y) + m4 and (m1*x) + (m3*y) + m5 of applyAffineTransformToPoint :1382-1385 -- inv[6] = an inverse matrix, f32 values --
 * round at most once, so that fma(m0, x, (m2*y) + m4) has the same bits (both partial sums exactly representable; hg_math.h
 * affine_fusable); else 0 (-> the kernel keeps the two roundings).  k_tri_setup evaluates the same predicate per (frame, triangle). */
int hg_affine_one_fma_form(const float inv[6], hg_geom geom);
/* Self-test of the projective kernels' shared-reciprocal division against IEEE division on `samples` pseudo-random
 * operand triples drawn from the range the host admits it for; *mismatches must come back 0. */
int hg_selftest_division(hg_ctx *ctx, uint64_t samples, uint64_t seed, uint64_t *mismatches);
/* ------------------------------------------------------------------------------------------------ measurement aid
 * hipEvent pairs recorded on the ctx stream around each launch of the dominant kernel (the fused piecewise kernel or
 * the geometric kernel; not the tiny per-triangle setup).  hg_set_timing(ctx, 1) enables it and resets the counters;
 * hg_last_kernel_ms = duration of the most recent launch; hg_kernel_ms_stats = sum over (up to the last 256) launches
 * since the reset and how many that is.  Both wait for the stream. */
int hg_set_timing(hg_ctx *ctx, int enabled);
int hg_last_kernel_ms(hg_ctx *ctx, float *ms);
int hg_kernel_ms_stats(hg_ctx *ctx, double *total_ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif /* HGWARP_H */
