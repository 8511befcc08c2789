// hg_ctx.h -- the context behind the C ABI of include/hgwarp.h and the helpers its translation units share
// (hg_api.hip: library / context / buffers / host-side solves / source image; hg_api_geometric.hip; hg_api_piecewise.hip;
// hg_api_forward.hip; hg_api_state.hip; hg_api_field.hip; hg_api_remap.hip; hg_api_mosaic.hip; hg_api_points.hip; hg_api_fit.hip; hg_api_match.hip;
// hg_api_detect.hip; hg_api_multiband.hip; hg_api_align.hip; hg_api_tps.hip; hg_api_flow.hip; hg_api_bundle.hip; hg_api_camera.hip).  Its memory is
// owned through hg_mem.h.  Internal: nothing here is exported.
#pragma once
#include "../../include/hgwarp.h"
#include "hg_kernels.h"
#include "hg_mem.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace hg;

constexpr size_t kFwdStatusRing = 16;   // tile-binned forward piecewise batches that may be queued before their status words are checked
constexpr size_t kStatusRing = 64;      // fused piecewise runs that may be queued before their status words are checked

// ------------------------------------------------------------------------------------------------ errors
extern thread_local std::string g_err;   // (hg_api.hip) message of the last failure on this thread, for calls without a context

// ------------------------------------------------------------------------------------------------ piecewise layout policy (hg_api_piecewise.hip)
// What the host knows about the uploaded frame set: its extents and the layout estimates of hg_piecewise_set_frames (reused for the
// next set of the same shape: LayoutKey).  Estimates only pick kernel layouts; the kernels check the real counts.
struct PwShape {
    int n = 0;                          // frames
    int max_w = 0, max_h = 0;           // largest obj_w; largest obj_h of the frames with obj_w > 0
    int64_t groups = 0;                 // 4-row groups of the frame set
    bool self_geom = true;              // every window suits the self-span prologue's int32 arithmetic (>= 16 columns, < 2^24 rows near the origin)
    int min_row_groups = 1152;          // option "min_row_groups" when the set was staged (what "small set" and the k_pw_patch fit are measured by)
    bool quick = false;                 // estimate guessed from the triangle count, no walk over the triangles
    int cover = 0;                      // estimated longest per-row span list (max_row_cover)
    double tri_rows = 0.0;              // mean rows per triangle
    int group_tris = 0;                 // most triangles with spans in one 4-row group
    double shear = 0.0;                 // mean |d(source row) / d(output x)|
    int tri_rows_max = 0;               // tallest triangle, in rows (0: unknown)
    double fill = 1.0;                  // heaviest XCD row band / mean band (span counts per row), 1 = even rows
    double spans_per_window = 0.0;      // longest row's span count per 256-pixel window
};

// What runs of this mesh taught the policy: a kernel that exceeded its limits once is not taken again until a new mesh (or the option
// that forces it) is set.  Written by hg_set_option, hg_piecewise_set_mesh and learn_from_overflows only.
struct PwLearned {
    bool patch_disabled = false;        // k_pw_patch (row lists or self-spans) -> k_pw_rows
    bool tile_disabled = false;         // k_pw_tile -> k_pw_patch<SELF>
    bool self_disabled = false;         // self-span prologues -> row lists
};

enum class PwKernel { Rows, Patch, PatchGlobal, Tile, Fused };

// plan_piecewise's answer for one inverse piecewise step: the kernel, what run_setup lays out for it, and the launch scalars of PwFrames.
struct PwPlan {
    PwKernel kernel = PwKernel::Fused;  // Fused: the general path (k_tri_setup -> k_pw_fused); any other: k_tri_spans or k_tri_setup in front
    bool self = false;                  // the warp kernel evaluates the spans of its own rows (k_tri_setup in front, no row lists)
    bool bands = false;                 // ... scanning candidate bands of 64 output rows (n_bands of up to band_cap triangles)
    int n_bands = 0, band_cap = 0;
    bool compact = false;               // row lists of 8-byte entries (else 32-byte)
    int row_cap = 64;                   // row-list entries per row the lists were sized for
    int row_group = kRowGroup, tri_threads = 128;
    int tri_group = 0, phase = 2, xcc_rotate = 0, sub_bands = 0, sgpr_cap = 1, lds_pad_kb = 0, no_hi_bounds = 0, safe_spans = 0, safe_spans_patch = 1;
};

// The per-triangle solve arrays of F frames of T triangles (k_tri_setup / k_tri_spans write them): the frame set's, and the one-frame scratch
// of the deferred redo and the reference-state maps.
struct PwSolve {
    DevBuf<TriRange> trir; DevBuf<int2> trix; DevBuf<Seg> segs; DevBuf<float> fwd, inv; DevBuf<int32_t> status;
    int ensure(hg_ctx *c, size_t F, size_t T)
    {
        HG_TRY(::ensure(c, trir, F * T)); HG_TRY(::ensure(c, trix, F * T)); HG_TRY(::ensure(c, segs, F * T * 3));
        HG_TRY(::ensure(c, fwd, F * T * 6)); HG_TRY(::ensure(c, inv, F * T * kInvStride));
        return ::ensure(c, status, F);
    }
    void point(PwFrames &f) const { f.trir = trir; f.trix = trix; f.segs = segs; f.fwd = fwd; f.inv = inv; f.status = status; }
};

struct hg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t copy_stream = nullptr;                         // hg_upload_on_copy_stream: uploads that overlap the warp stream's work
    hipEvent_t copy_event = nullptr;                           // hg_fence_copies
    hipStream_t down_stream = nullptr;                         // hg_download_behind_warps: D2H copies that overlap the warp stream's later work
    hipEvent_t down_event = nullptr;
    std::string err;
    int deferred = HG_OK;

    // source image
    DevBuf<uint8_t> d_img;                                     // owned (hg_set_image) or borrowed from the caller (hg_set_image_device)
    int W = 0, H = 0;
    int n_imgs = 1; size_t img_stride = 0;                     // hg_set_images_device: frame f reads image f % n_imgs

    // mesh (source side)
    DevBuf<float> d_src;
    DevBuf<uint32_t> d_tris;
    std::vector<uint32_t> h_tris;                              // host copies (row-density / shear estimates in hg_piecewise_set_frames)
    std::vector<float> h_src;
    int n_pts = 0, n_tris = 0, min_src_x = 0, min_src_y = 0;
    bool have_mesh = false;

    // piecewise frames
    std::vector<FrameDesc> pw_frames;          // host copy
    DevBuf<uint8_t> d_set;                                     // the frame set in ONE block: F frame records, then F x n_pts x 2 destiny floats (one upload)
    FrameDesc *d_pw_frames = nullptr;                         // = d_set
    float *d_dst = nullptr;                                   // = d_set + F * sizeof(FrameDesc)
    // a frame set with a source side of its own (hg_piecewise_set_frames_src): F x n_pts x 2 source floats and F {minSrcX, minSrcY} pairs behind the
    // destiny points, in the same block; the extremes of the minima over the set (what "fast path" and the bounds form are decided by)
    bool pw_moving = false;
    float *d_srcf = nullptr; int2 *d_min_src = nullptr;
    int ms_lo_x = 0, ms_hi_x = 0, ms_lo_y = 0, ms_hi_y = 0;
    PwSolve solve;                                             // the per-triangle solves of the frame set
    DevBuf<int32_t> d_two_round; int32_t pw_gen = 0;           // PwFrames::two_round / gen
    int32_t *status_ptr = nullptr;                             // where this frame set's status words live (solve.status, or the tail of d_rowcnt)
    PinnedBuf<int32_t> h_status;                               // kStatusRing sets of status words, read back by hg_sync
    PinnedBuf<int32_t> h_flag;                                 // device-visible: set to 1 by any fused kernel that flags a frame (PwFrames::host_flag)
    bool pw_setup_done = false;                                // the per-triangle solves ran for the uploaded frames
    // fast path: per-output-row span lists
    DevBuf<int32_t> d_rowcnt;
    DevBuf<uint8_t> d_rowent;                                  // bytes
    int row_cap = 64;                                          // entries per row; grows (sticky) after an overflow
    bool rows_clean = false;                                   // span counters + the next status set were zeroed by the last k_pw_rows
    int status_slot = 0;                                       // which of the kStatusRing status-word sets the current step uses
    int32_t *status_base = nullptr, *status_next = nullptr;
    PwShape pw_shape;                                          // the uploaded frame set (hg_piecewise_set_frames)
    PwLearned pw_learned;                                      // per-mesh fallbacks (learn_from_overflows)
    PwPlan pw_plan;                                            // the plan of the last set-up (run_setup); frames_of / rows_of hand it to the kernels
    int opt_sub_bands = -1;                                    // option "sub_bands": sub-bands per XCD of the warp kernels on a shared source with fixed bands (0 / 1 off, -1 by the source's size)
    int opt_xcc_rotate = -1;                                   // -1 by estimate, 0 / 1
    int opt_compact = -1;                                      // span-list entry format: 1 = 8-byte entries, 0 = 32-byte entries with the matrix, -1 by estimate
    int pw_last_kernel = 0;                                    // hg_last_piecewise_kernel(): code of the plan the last warp carried out
    int geo_last_kernel = -1;                                  // hg_last_geometric_kernel(): launch_geo's code of the last geometric warp
    int32_t pw_last_flag = 0;                                  // status word of the last frame a fused run flagged (bits 4..: which limit, see k_pw_patch<SELF>)
    long pw_redone = 0;                                        // frames redone through the materialised map (hg_redone_frames())
    int opt_min_row_groups = 1152, opt_patch = -1, opt_phase = -1, opt_geo_nw = 8;   // hg_set_option()
    int sampling = HG_SAMPLE_NEAREST;                          // hg_set_sampling: pixel body of the inverse warps called from now on (queued work keeps its own)
    int xcc_log2 = 3;                                          // log2(XCCs of the device): hipDeviceAttributeNumberOfXccs at hg_create, option "xcc"
    int opt_hi_bounds = 1;                                     // 0: fp64 bounds compares instead of the high-dword form (hg_dev.h)
    // fused runs whose per-frame status words have not been checked yet: up to kStatusRing - 1 calls are queued back to back
    // with nothing but their two kernels in the stream; each flags into its own set of status words, read back by hg_sync
    // stage: which staged frame set (points + windows) the run warped; extent / layout: the bytes it writes from `out` on and a hash of
    // its frames' (offset, size) list -- a later call into the SAME layout supersedes its deferred redos frame by frame, any other
    // overlapping writer settles it first (settle_output_conflicts)
    // kernel / self: what the run's plan carried out (what hg_sync disables when the run exceeded a limit: learn_from_overflows)
    // sampling: the mode the run was queued with (its deferred redos use it, whatever the context's mode is by then)
    struct Pending { uint8_t *out; int slot; int stage; size_t extent; uint64_t layout; PwKernel kernel; bool self; uint8_t sampling; };
    std::vector<Pending> pw_pending_out;
    // Frame sets arrive through a ring of page-locked staging buffers (FrameDesc[F], then the F x n_pts x 2 destination
    // points; `moving` sets: then the F x n_pts x 2 source points and the F source minima): hg_piecewise_set_frames copies the caller's arrays there and queues stream-ordered uploads -- it neither waits
    // for the GPU nor keeps caller memory.  A staged set stays intact until every run that used it has been settled, so frames a
    // fused run flagged can still be redone (through the materialised map) after newer sets were uploaded.
    // (StageRing, hg_mem.h; n / n_pts / moving: what the deferred redo needs to find a frame in the slot)
    struct Stage : StageSlot { int n = 0, n_pts = 0; bool moving = false; };
    StageRing<(int)kStatusRing, Stage> stage;
    // scratch of the deferred redo (one frame): its FrameDesc, points, solves
    DevBuf<FrameDesc> d_redo_frame;
    DevBuf<float> d_redo_dst, d_redo_src;                      // (d_redo_src, d_redo_min: frames of a set with its own source side)
    DevBuf<int2> d_redo_min;
    PwSolve redo;
    // reference-state warps (hg_api_state.hip): the map's own point set and triangles, the cached matrices handed over by the caller
    DevBuf<float> d_st_pts;
    DevBuf<uint32_t> d_st_tris;
    DevBuf<float> d_st_mats;
    // layout of the row counters / status ring as of their last memset (a frame set with the same layout reuses them as they are)
    size_t rows_F = 0; int rows_stride = 0, rows_cap = 0;
    // self-span path (k_tri_setup -> k_pw_rows<SELF>, hg_kernels.h): the row workgroups evaluate their own spans, no row lists
    int pw_last_variant = 0;                                   // variant code of the last piecewise warp kernel launched (launch_pw_rows; hg_last_piecewise_variant)
    int opt_tile = -1;                                         // option "tile": 1 whenever k_pw_patch<SELF> would run, 0 never, -1 by policy
    DevBuf<int4> d_bands;                                      // F x n_bands x band_cap entries of the candidate bands (hg_kernels.h)
    int band_cap = 0;                                          // entries per band; grows (sticky)
    int opt_self = -1;                                         // option "self_spans": 1 whenever eligible, 0 never, -1 by policy (plan_piecewise)
    int rows_parity = 0;                                       // which of the two counter sets the current step counts into (ping-pong, hg_kernels.h)
    int opt_tri_group = -1;                                    // k_tri_spans_grouped: 16 / 64 triangles per workgroup, 0 never, -1 by mesh size
    int opt_upload_kernel = -1;                                // frame-set blocks up to 1 MB go up by k_upload (default) instead of hipMemcpyAsync (0)
    int opt_safe_spans = -1;                                   // option "safe_spans": span flags + bounds-test-free windows in k_pw_rows: 1 / 0, -1 by the spans-per-window estimate
    // span cache of k_pw_rows<SELF> in packed 4-row groups (hg_span_cache.h; span_cache_prepare in hg_api_piecewise.hip)
    DevBuf<uint4> d_span_rec;                                  // records, 16-byte words
    DevBuf<int4> d_span_dir;                                   // entry 0: the cursor (first 8 bytes), then one SpanDirEnt per (frame, 4-row group)
    DevBuf<SpanFrameBlock> d_span_fblk;                        // one block per frame, beside the directory (hg_span_start.h): the use kernel's flat start
    uint32_t span_cap16 = 0; int span_gpf = 0;                 // words the build may hand out; groups per frame of the directory
    uint64_t pw_epoch = 1;                                     // frame-set epoch: bumped by whatever can change an input of k_tri_setup or of the span prologue
    SpanCacheState span_state;
    int opt_span_cache = -1;                                   // option "span_cache": -1 build on the second warp of a set, 0 off, 1 build on the first
    int opt_span_cache_mb = 256;                               // option "span_cache_mb": budget in MB; negative: -KB, and the host's estimate does not veto the build
    long span_builds = 0, span_uses = 0; int span_last = 0;    // hg_span_cache_stats
    // layout estimates of the last frame set, reused for the next set of the same shape (the kernels check the real counts)
    struct LayoutKey { int n = -1, n_tris = -1, max_w = -1, max_h = -1; uint64_t mesh_gen = 0; bool quick = false; } layout_key;
    uint64_t mesh_gen = 0; int layout_age = 0;
    long pw_layout_walks = 0;                                  // host walks over the triangles (hg_layout_walks(): tests / bench)

    // geometric frame sets arrive like the piecewise ones: copied into page-locked staging, uploaded stream-ordered, no GPU wait
    // (nothing refers back to a staged geometric set, so a slot is simply reused once its own upload has completed)
    StageRing<8> geo_stage;
    // geometric frames
    int geo_kind = 0;
    bool geo_f32_exact = false;                                // affine matrices hold float values, |x| < 2^28
    std::vector<FrameDesc> geo_frames;
    DevBuf<FrameDesc> d_geo_frames;
    DevBuf<double> d_mats;
    bool geo_from_points = false;                              // matrices are (re)solved on the device at every warp (hg_geometric_set_frames_points)
    DevBuf<float> d_geo_pts;                                   // F x (from | to) point sets
    DevBuf<int32_t> d_geo_plain;                               // per-frame "plain division range" flags written by k_solve_frames

    // source fields (hg_api_field.hip): the frame records of a set with the FIELD offsets in out_off, staged like a geometric set
    DevBuf<FrameDesc> d_field_frames;
    StageRing<4> field_stage;
    DevBuf<uint8_t> d_field_tmp;                               // the host-output forms' device copy
    DevBuf<RemapFrame> d_remap_frames;                         // the frame table of a frames remap (hg_remap_*_frames_device), staged through field_stage
    DevBuf<uint64_t> d_tri_table;                              // hg_remap_trilinear_frames_device: 32 level offsets, then the TriRemapFrame records; staged through field_stage
    DevBuf<MosaicFrame4> d_mosaic_frames;                      // the frame table of the hg_mosaic_* calls (quads of records) and, behind it, a gained mosaic's gains; staged through field_stage
    DevBuf<uint64_t> d_mb_table;                               // hg_mosaic_multiband_device: the mosaic's quads, then the MbFrame records of the frames that take part; staged through field_stage
    int opt_remap_pack = -1;                                  // k_remap_index_frames: 0 = one pixel per lane even for the pixel sizes that carry the packed form (measurements)

    // fitting transforms to matches (hg_api_fit.hip): the hypotheses' matrices and flags, the per-frame counts and best words; grown on demand
    DevBuf<double> d_fit_mats;
    DevBuf<int32_t> d_fit_valid;
    DevBuf<uint64_t> d_fit_frames;                             // F best words, then the F counts (int32, padded to 8 bytes)
    StageRing<4> fit_stage;                                    // the counts go up through page-locked staging, stream-ordered
    StageRing<4> bundle_stage;                                 // the bundle adjustment's host-built lists (hg_api_bundle.hip), likewise

    // refining transforms on the pixels (hg_api_align.hip): the per-frame iterate and flags, the chunks' partial records and the luma copies of
    // 4-channel planes; grown on demand
    DevBuf<hg::AlignState> d_align_state;
    DevBuf<double> d_align_part;
    DevBuf<uint8_t> d_align_luma;

    // matching descriptors (hg_api_match.hip): the two-nearest records of the queries and, for the cross-check, of the train rows; the counts of
    // both sides; grown on demand
    DevBuf<uint4> d_match_fwd, d_match_rev;
    DevBuf<uint64_t> d_match_keys;                             // the cross-check's atomic form: per train row of every frame the word (d << 32) | i of its best query
    int opt_match_cross = -1;                                  // the cross-check of HG_DESC_U8: 0 = by a second launch with the sides swapped (measurements), else by atomicMin
    DevBuf<int32_t> d_match_counts;                            // F query counts, then n_train_sets train counts (padded to 8 bytes)
    StageRing<4> match_stage;

    // detecting and describing keypoints (hg_api_detect.hip): the per-cell records and counts, the planes' lists of flat indices, and the turned
    // pattern, uploaded once; grown on demand
    DevBuf<uint4> d_detect_rec;
    DevBuf<int32_t> d_detect_cnt, d_detect_list;
    DevBuf<int8_t> d_detect_table;

    // scratch
    DevBuf<int32_t> d_map32;
    DevBuf<int32_t> d_fmap;                                    // forward (source-side) triangle map of the current mesh, kept across warps
    bool fmap_valid = false; int fmap_w = 0, fmap_h = 0;
    DevBuf<int32_t> d_win32;
    DevBuf<uint8_t> d_fwd_par;                                 // k_fwd_tiles: FwdParam[n] then FrameDesc[n]
    DevBuf<int32_t> d_fbbox;                                   // forward piecewise tiles: per-matrix cell bbox of the forward map (valid with it)
    DevBuf<uint32_t> d_frowoff;                                // ... offset of its per-row extents
    DevBuf<int32_t> d_frowext;                                 // ... {min mx, max mx} per (matrix index, map row of its bbox)
    bool fwd_rowext_ok = false;
    DevBuf<int32_t> d_ftile_cnt;                               // F x tiles counters (zero between calls)
    DevBuf<int32_t> d_fwd_status; size_t fwd_status_stride = 0;   // kFwdStatusRing sets of `stride` status words of tile-binned forward piecewise batches (zero between calls)
    DevBuf<int32_t> d_ftile_ent;                               // F x tiles x fwd_pw_cap entries
    int fwd_pw_cap = 64;                                       // entries per tile (doubles after an overflow, up to kFwdPwCapMax)
    bool fwd_pw_tiles_disabled = false;                        // overflowed at the largest capacity once: stay with the scatter path for this mesh
    // queued tile-binned forward piecewise batches: status set `slot` of the forward status ring, frame set in staging slot `stage`
    struct FwdPending { uint8_t *out = nullptr; int n = 0; int slot = 0; int stage = -1; int max_src_x = 0, max_src_y = 0; size_t extent = 0; uint64_t layout = 0; };
    std::vector<FwdPending> fwd_pending;
    int fwd_slot = 0;
    int opt_fwd_tiles = -1;                                    // forward paths: -1 auto, 0 scatter + gather, 1 tiles whenever admissible
    int fwd_last_kernel = 0;                                   // 1 scatter + gather, 2 k_fwd_tiles (hg_last_kernel-style tap for the tests)
    int fwd_field_last_kernel = 0;                             // the same tap of the forward FIELD calls (hg_last_forward_field_kernel): they leave fwd_last_kernel alone
    DevBuf<int32_t> d_ffield_status;                           // status words of ONE forward piecewise field call (read inside the call; not the ring of queued warps)
    DevBuf<int16_t> d_map16;
    DevBuf<uint8_t> d_out_tmp;

    // timing of the dominant kernel: a ring of event pairs recorded around each launch of it
    static constexpr int kEvRing = 256;
    bool timing = false;
    hipEvent_t ev0[kEvRing] = {}, ev1[kEvRing] = {};
    long ev_count = 0;                                         // launches recorded since timing was (re)enabled
};

inline int fail(hg_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    g_err = msg;
    return code;
}

inline hipStream_t stream_of(const hg_ctx *c) { return c->stream; }

// Pixels of a w x h window (none if either is not positive); `bytes` rounded up to the 256-byte grain frames are packed at.
inline size_t frame_px(int64_t w, int64_t h) { return (w > 0 && h > 0) ? (size_t)w * (size_t)h : 0; }
inline size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// n windows of px_bytes per pixel packed back to back at that grain (offsets, total: either may be NULL).
inline void pack_offsets(const hg_geom *g, int n, size_t px_bytes, size_t *offsets, size_t *total)
{
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        if (offsets) offsets[i] = off;
        off += pad256(frame_px(g[i].obj_w, g[i].obj_h) * px_bytes);
    }
    if (total) *total = off;
}
// NaN is a legal (if useless) coordinate -- the reference then simply draws nothing for that triangle -- but magnitudes beyond
// kMaxCoord (Infinity included) are refused: the row loops of the rasterisers are bounded under that assumption (hg_math.h).
inline bool coords_ok(const float *p, size_t n)
{
    for (size_t i = 0; i < n; i++) if (std::fabs((double)p[i]) > kMaxCoord) return false;      // (NaN compares false)
    return true;
}

// A staged block (page-locked, device-visible) to the device, stream-ordered: up to 1 MB by k_upload -- a kernel that reads the host block --,
// beyond that (or with option "upload_kernel" = 0) by the copy engine, whose start-up latency is what a 36-KB frame set paid for (R4.13).
inline int upload_staged(hg_ctx *c, void *d0, const void *s0, size_t b0, void *d1 = nullptr, const void *s1 = nullptr, size_t b1 = 0,
                         void *d2 = nullptr, const void *s2 = nullptr, size_t b2 = 0)
{
    if (b0 + b1 + b2 == 0) return HG_OK;
    if (std::max(b0, std::max(b1, b2)) <= ((size_t)1 << 20) && ((b0 | b1 | b2) & 7) == 0 && c->opt_upload_kernel != 0) {
        UploadSegs sg{{d0, d1, d2}, {s0, s1, s2}, {b0 / 8, b1 / 8, b2 / 8}};
        launch_upload(sg, c->stream);
        HIP_TRY(c, hipGetLastError());
    } else {
        if (b0) HIP_TRY(c, hipMemcpyAsync(d0, s0, b0, hipMemcpyHostToDevice, c->stream));
        if (b1) HIP_TRY(c, hipMemcpyAsync(d1, s1, b1, hipMemcpyHostToDevice, c->stream));
        if (b2) HIP_TRY(c, hipMemcpyAsync(d2, s2, b2, hipMemcpyHostToDevice, c->stream));
    }
    return HG_OK;
}

// What a forward piecewise tile run's flags say about the MESH, whoever ran it (hg_sync for queued warps, a forward field call for itself): an
// overfull tile list doubles the capacity up to kFwdPwCapMax, then switches the tile path off; a triangle the bins kernel could not bound
// switches it off at once (until hg_piecewise_set_mesh or option "fwd_tiles" re-arms it).
inline void learn_forward_tiles(hg_ctx *c, bool overflow, bool unbounded)
{
    if (overflow) {
        if (c->fwd_pw_cap < kFwdPwCapMax) c->fwd_pw_cap = std::min(kFwdPwCapMax, c->fwd_pw_cap * 2);
        else c->fwd_pw_tiles_disabled = true;
    }
    if (unbounded) c->fwd_pw_tiles_disabled = true;          // (a degenerate triangle in this mesh: do not pay for both paths again)
}

inline int bind(hg_ctx *c)
{
    if (!c) return fail(nullptr, HG_ERR_INVALID, "ctx is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ shared between the translation units
int time_begin(hg_ctx *c);                                   // hg_api.hip: event pair around the dominant kernel (hg_set_timing)
int time_end(hg_ctx *c);
int fill_frames(hg_ctx *c, std::vector<FrameDesc> &v, const hg_geom *geoms, const size_t *offs, int n);      // hg_api.hip
// hg_api_remap.hip: the bilinear / bicubic frames remap behind its entry points; compose: the chained field of hg_field_compose_frames_device
int remap_flat_frames(hg_ctx *c, const char *who, const hg_geom *geoms, int n_frames, const void *d_coords, const size_t *field_offsets,
                      const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int elem, int channels,
                      void *d_out, const size_t *out_offsets, const CubicCoef *cubic, bool compose);
// The bytes a frame list writes from its output pointer on, and a hash of its (offset, size) pairs (0 is never returned).
void output_layout(const std::vector<FrameDesc> &frames, size_t *extent, uint64_t *layout);                  // hg_api.hip
// Before a call writes [out, out + extent): queued runs whose deferred redo could land on those bytes later are settled now, unless
// the new call has the same base and layout (then hg_sync skips the older run's redo frame by frame: `superseded`).  layout = 0:
// a writer that keeps no pending record (geometric warps, the scatter paths) -- any overlap settles.
int settle_output_conflicts(hg_ctx *c, const void *out, size_t extent, uint64_t layout);                     // hg_api.hip
// hg_piecewise_set_frames with quick_layout: no host walk over the triangles for the layout estimate (the forward paths, which only
// need the per-triangle solves)
int piecewise_set_frames(hg_ctx *c, const float *dst, const hg_geom *geoms, const size_t *offs, int n, bool quick_layout);   // hg_api_piecewise.hip
PwMesh mesh_of(const hg_ctx *c);                             // hg_api_piecewise.hip: kernel argument blocks of the current mesh / frame set
PwFrames frames_of(const hg_ctx *c);
int check_pw_state(hg_ctx *c);                               // hg_api_piecewise.hip: image, mesh and frame set present?
int redo_forward_frame_staged(hg_ctx *c, int stage, int f, int max_src_x, int max_src_y, uint8_t *d_out);    // hg_api_piecewise.hip, beside its inverse twin
// hg_api_forward.hip: steps (A) and (B) of a forward piecewise call -- checks and limits, the cached forward triangle map, the frame set staged
// and its forward matrices queued (k_tri_setup) -- for the warps, the fields and the point lists
int forward_piecewise_stage(hg_ctx *c, const float *dst_points, int max_src_x, int max_src_y, const hg_geom *geoms, const size_t *offs, int n,
                            bool field, int64_t *map_w, int64_t *map_h);

// ------------------------------------------------------------------------------------------------ what the entry points do alike
// p does not lie at a multiple of a (a power of two).  NULL is aligned: whether a pointer may be NULL is the caller's own check.
inline bool misaligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// A queued run's deferred redo must not land later on what this call writes: queued runs whose output overlaps [ptr, ptr + bytes) are
// settled first.
inline int settle_pending_on(hg_ctx *c, const void *ptr, size_t bytes)
{
    if (c->pw_pending_out.empty() && c->fwd_pending.empty()) return HG_OK;
    return settle_output_conflicts(c, ptr, bytes, 0);
}

// A host-built table (a multiple of 8 bytes) to d_dst through a staging ring, stream-ordered: the next slot is acquired (what: its name in
// the out-of-memory message), fill(h) writes its `bytes`, the upload is queued, and only then is the slot committed -- the event that guards
// its bytes is recorded behind the upload, and a call that failed anywhere has handed nothing over: the next one takes the same slot.
template <int N, typename Slot, typename Fill>
inline int upload_filled(hg_ctx *c, StageRing<N, Slot> &ring, const char *what, void *d_dst, size_t bytes, Fill fill)
{
    Slot *s = nullptr;
    HG_TRY(ring.acquire(c, bytes, what, &s));
    fill(s->h);
    HG_TRY(upload_staged(c, d_dst, s->h, bytes));
    return ring.commit(c, s);
}
// ... a copy of the caller's block a, or of a and b back to back, in ONE upload.
template <int N, typename Slot>
inline int upload_copied(hg_ctx *c, StageRing<N, Slot> &ring, const char *what, void *d_dst, const void *a, size_t a_bytes,
                         const void *b = nullptr, size_t b_bytes = 0)
{
    return upload_filled(c, ring, what, d_dst, a_bytes + b_bytes, [=](uint8_t *h) {
        std::memcpy(h, a, a_bytes);
        if (b_bytes) std::memcpy(h + a_bytes, b, b_bytes);
    });
}
// ... a frame table of the field, remap and mosaic calls, which share a ring (no GPU wait unless the upload that used the slot four calls
// ago is still queued).
inline int upload_frame_table(hg_ctx *c, void *d_dst, const void *a, size_t a_bytes, const void *b = nullptr, size_t b_bytes = 0)
{
    return upload_copied(c, c->field_stage, "field frame staging", d_dst, a, a_bytes, b, b_bytes);
}

// ------------------------------------------------------------------------------------------------ fields
inline bool field_fmt_ok(int fmt) { return fmt == HG_FIELD_INDEX || fmt == HG_FIELD_COORDS; }
inline size_t field_px_bytes(int fmt) { return fmt == HG_FIELD_INDEX ? 4 : 8; }

// What a field call checks of its format: that it is one and, once the call knows the source's size W x H (0 x 0 before that), that the
// index format can address it: below 2^31 pixels.
inline int check_field_fmt(hg_ctx *c, int fmt, int W = 0, int H = 0)
{
    if (!field_fmt_ok(fmt)) return fail(c, HG_ERR_INVALID, "unknown field format (HG_FIELD_INDEX or HG_FIELD_COORDS)");
    if (fmt == HG_FIELD_INDEX && (int64_t)W * H >= ((int64_t)1 << 31))
        return fail(c, HG_ERR_INVALID, "HG_FIELD_INDEX: the source has 2^31 pixels or more (an int32 cannot index it)");
    return HG_OK;
}

// The frame table of a field call over n windows (hg_geom or FrameDesc: x_off, y_off, obj_w, obj_h).  Rec is FrameDesc or a record of its
// size and head (CamFrame, TpsFrame): the window, then the FIELD offset in out_off -- offs[f] as given, a multiple of the field's pixel size,
// or packed as hg_pack_field_offsets does.  A FrameDesc source is copied whole; otherwise the last word is zero and the caller's to fill in.
// extent: the bytes the call writes from d_field on; max_w, max_h: the widest and the tallest non-empty window.
template <typename Rec> struct FieldTable { std::vector<Rec> recs; size_t extent = 0; int max_w = 0, max_h = 0; };

template <typename Rec, typename Win>
inline int field_table(hg_ctx *c, const Win *win, size_t n, int fmt, const size_t *offs, FieldTable<Rec> *t)
{
    static_assert(sizeof(Rec) == sizeof(FrameDesc), "the field calls' frame table carries either record");
    const size_t px = field_px_bytes(fmt);
    t->recs.resize(n);
    t->extent = 0; t->max_w = t->max_h = 0;
    size_t off = 0;
    for (size_t f = 0; f < n; f++) {
        const Win &w = win[f];
        Rec &r = t->recs[f];
        if constexpr (std::is_same<Rec, Win>::value) r = w;
        else r = Rec{w.x_off, w.y_off, w.obj_w, w.obj_h, 0, 0};
        r.out_off = offs ? offs[f] : off;
        if (r.out_off & (px - 1)) return fail(c, HG_ERR_INVALID, "field offsets must be multiples of the field's pixel size (4 or 8 bytes)");
        const size_t n_px = frame_px(w.obj_w, w.obj_h);
        off += pad256(n_px * px);
        if (n_px) { t->extent = std::max(t->extent, (size_t)r.out_off + n_px * px); t->max_w = std::max(t->max_w, w.obj_w); t->max_h = std::max(t->max_h, w.obj_h); }
    }
    return HG_OK;
}
