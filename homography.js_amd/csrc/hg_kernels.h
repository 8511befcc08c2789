// hg_kernels.h -- device-side data layout and kernel launchers (implemented in hg_k_*.hip, one translation unit per kernel family).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hg_math.h"
#include "hg_span_cache.h"
#include "hg_span_runs.h"
#include "hg_span_start.h"
#include "hg_remap_records.h"
#include "hg_align_dev.h"
#include "hg_tps_dev.h"
#include "hg_flow_dev.h"
#include "hg_bundle_dev.h"
#include "hg_camera_dev.h"

namespace hg {

// One output frame (one destination point set / one matrix): the reference's
// (_xOutputOffset, _yOutputOffset, _objectiveWidth, _objectiveHeight) plus where its RGBA goes.
struct FrameDesc {
    int32_t x_off, y_off, obj_w, obj_h;
    uint64_t out_off;        // byte offset of this frame's RGBA8 in the output allocation
    uint64_t map_off;        // cell offset of this frame in the optional int16 debug-map allocation
};

// Per (frame, triangle) raster parameters produced by k_tri_setup.
//   rows y in [y_min, y_end) are the rows fillTriangle visits (:1113-1120);
//   a, b bound which output rows a row-y span can touch:  (y - yOff) in [r - a, r - b]  (see DESIGN.md §4.2).
struct TriRange { int32_t y_min, y_end, a, b; };

// Per-frame status word written by the kernels.
enum : int32_t {
    FRAME_OK = 0,
    FRAME_IRREGULAR = 1,     // a triangle with non-finite / absurd vertices or wider than the whole map: fused path skipped
    FRAME_LDS_OVERFLOW = 2   // some row crossed more spans than the fused kernel's LDS list holds: frame must be redone
};

constexpr int kRowSpanCap = 1024;   // spans per output row held in LDS by the general fused kernel (k_pw_fused)
constexpr int kRowSpanCapFast = 256; // ... by the fast kernel (k_pw_rows), which also keeps a 48-byte matrix per span
constexpr int kRowSpanCapDense = 512; // ... by its dense instantiation (README-scale meshes: ~23 000 triangles, 200-500 spans per row)
constexpr int kRowGroup = 4;            // output rows per k_pw_rows workgroup (64 LDS slots each in packed mode)
constexpr int kInvStride = 8;       // floats per inverse matrix on the device (6 used; 32-byte rows)

struct PwMesh {                     // source side of the mesh + source image (shared by all frames unless the frame set brings its own: PwFrames::src_pts)
    const float *src_pts;           // n_pts x 2
    const uint32_t *tris;           // n_tris x 3
    int32_t n_pts, n_tris;
    int32_t min_src_x, min_src_y;
    const uint8_t *img;             // RGBA8 source, W*H*4 bytes (image 0)
    int32_t W, H;
    int32_t n_imgs;                 // >= 1: frame f reads image f % n_imgs (1 = one source shared by every frame)
    uint64_t img_stride;            // bytes between consecutive source images (hg_set_images_device)
};

// source image of frame f
__host__ __device__ __forceinline__ const uint8_t *frame_img(const PwMesh &m, int f)
{
    return m.n_imgs > 1 ? m.img + (uint64_t)(f % m.n_imgs) * m.img_stride : m.img;
}

struct PwFrames;
// source points / source minima of frame f (frame sets with a source side of their own; f is uniform for the workgroup in every caller)
__device__ __forceinline__ const float *frame_src(const PwMesh &m, const PwFrames &fr, int f);
__device__ __forceinline__ int2 frame_min_src(const PwMesh &m, const PwFrames &fr, int f);

struct PwFrames {                   // per-frame device arrays, frame-major
    const FrameDesc *frames;
    const float *dst_pts;           // F x n_pts x 2
    const float *src_pts;           // F x n_pts x 2: frame f's own source points (hg_piecewise_set_frames_src); nullptr: the mesh's, for every frame
    const int2 *min_src;            // F: frame f's {minSrcX, minSrcY} of the bounds test :1047; nullptr: the mesh's
    int32_t min_src_lo_x, min_src_hi_x, min_src_lo_y, min_src_hi_y;   // host: extremes of min_src over the set (what the launchers decide the bounds form by)
    TriRange *trir;                 // F x n_tris
    int2 *trix;                     // F x n_tris: {floor(min x) - 1, ceil(max x) + 1} of the triangle's destiny vertices (column reach of its spans; k_pw_tile)
    Seg *segs;                      // F x n_tris x 3
    float *fwd;                     // F x n_tris x 6
    float *inv;                     // F x n_tris x kInvStride
    int32_t *status;                // F
    int32_t *two_round;             // F: == gen when k_tri_setup met a triangle (with rows) of the frame whose :1383 sums are not exact (affine_fusable, hg_math.h);
    int32_t gen;                    //    any other value: the row kernel may use one fma per coordinate for the whole frame.  gen: this step's number (never reset: no clearing pass)
    int32_t *host_flag;             // page-locked, device-visible word set to 1 whenever a kernel flags a frame (nullptr: none): lets hg_sync skip reading the status ring
    int32_t n_frames;
    int32_t max_obj_h;              // max over frames (grid size)
    int32_t row_group;              // output rows per k_pw_rows workgroup: kRowGroup (sparse rows) or 1 (dense meshes)
    int32_t tri_threads;            // k_tri_spans workgroup size: 128, or 64 when the triangles are short (one row per thread)
    int32_t tri_group;              // 16 / 64: k_tri_spans_grouped (that many triangles per workgroup, their solves one per lane) instead of k_tri_spans; 0: k_tri_spans
    int32_t phase;                  // k_pw_rows: windows whose gathers are issued before their stores (1, 2 or 4)
    int32_t xcc_rotate;             // 1: XCD x takes band (x + frame) mod XCCs instead of band x (uneven rows, or no source shared between frames)
    int32_t sub_bands;              // host: sub-bands per XCD (0 / 1: none); the launcher derives sub_groups from it for its kernel's row-group height
    int32_t sub_groups;             // shared source, fixed bands: 0, or the row groups of a SUB-band.  The frame's rows are cut into sub-bands of that many groups, dealt to the XCDs round
                                    // robin (sub-band j -> XCD j mod XCCs), and an XCD takes ALL FRAMES of one of its sub-bands before the next (loop interchange): the slice of the source a
                                    // sub-band reads (a few hundred rows) then stays in that XCD's 4 MiB L2 from frame to frame, which a whole band of a 4K source does not (R6.12)
    int32_t xcc_log2;               // log2 of the device's XCC count (8 on an unpartitioned MI355X): block id -> XCD row band
    int32_t lds_pad_kb;             // KB of unused dynamic LDS per k_pw_rows workgroup (caps the workgroups resident per CU: row lists with one source per frame)
    int32_t sgpr_cap;               // k_pw_rows PH = 2: the 80-SGPR instantiation (8 workgroups per CU); host: shared source only
    int32_t no_hi_bounds;           // option "hi_bounds" = 0: keep the fp64 bounds compares (parity suite runs both forms)
    int32_t safe_spans;             // 1: the row kernel flags every span whose two end pixels pass the source bounds test and runs windows made of such spans
                                    // without the per-pixel test (k_pw_rows); 0: no flags (rows of many short spans, where flagging costs more than it saves)
    int32_t safe_spans_patch;       // the same flags in k_pw_patch<SELF> (per 64-pixel x 4-row block)
    int32_t self_spans;             // 1: no row lists -- k_tri_setup ran, the
                                    // warp kernel's workgroups evaluate the spans of their own rows in their prologue
    // Candidate bands of the self-span path for meshes too large to scan per workgroup (k_tri_setup files every triangle under the
    // bands of 1 << band_rows_log2 output rows it can reach; a row workgroup tests only its band's entries).  band_ent == nullptr:
    // workgroups scan trir[frame][0 .. n_tris).  Counters: the row-counter arrays (unused without row lists), index frame * band_stride + band.
    int4 *band_ent;                 // F x n_bands x band_cap entries of TWO int4: {triangle, y_min, y_end, a & 0xffff | b << 16}, {xlo, xhi, 0, 0}
    int32_t *band_cnt;
    int32_t band_stride, n_bands, band_cap, band_rows_log2;
};

__device__ __forceinline__ const float *frame_src(const PwMesh &m, const PwFrames &fr, int f)
{
    return fr.src_pts ? fr.src_pts + (size_t)f * m.n_pts * 2 : m.src_pts;
}
// (scalar registers: the pointer is a kernel argument and f is decoded from the block id -- the readfirstlanes only tell the compiler so)
__device__ __forceinline__ int2 frame_min_src(const PwMesh &m, const PwFrames &fr, int f)
{
    if (!fr.min_src) return make_int2(m.min_src_x, m.min_src_y);
    const int2 v = fr.min_src[__builtin_amdgcn_readfirstlane(f)];
    return make_int2(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y));
}

// Per-output-row span lists of the fast path (k_tri_spans -> k_pw_rows), in global memory.
// Two entry formats, chosen per frame set (RowLists::compact):
//   full    32 bytes: cells [lo,hi) of the row (16 bits each), triangle id, the triangle's inverse matrix.  Sparse rows
//           (<= 56 spans, k_pw_rows' packed 4-row groups): the matrix arrives with the entry, no dependent load in the prologue.
//   compact  8 bytes: cells + id only; consumers fetch the matrix by id from the per-(frame, triangle) tap array fr.inv (L2
//           resident).  Dense rows (k_pw_patch, k_pw_rows one row per workgroup): a quarter of the list traffic -- C5's
//           k_pw_patch 0.508 -> 0.415 ms, k_tri_spans 79 -> 68 us -- at the price of one dependent L2 load per row, which costs
//           sparse C3 3 % and is why both formats exist.
struct RowEnt { uint32_t lo_hi; int32_t id; float m[6]; };
struct RowEnt8 { uint32_t lo_hi; int32_t id; };
static_assert(sizeof(RowEnt) == 32 && sizeof(RowEnt8) == 8, "span entry sizes");
struct RowLists {
    int32_t *cnt;            // F x row_stride: this step's counters (k_tri_spans counts into them, the warp kernel reads them)
    int32_t *cnt_clear;      // the other of the two counter sets, same layout: the warp kernel zeroes it for the NEXT step (ping-pong)
    void *ent;               // F x row_stride x cap entries of 32 (RowEnt) or 8 (RowEnt8) bytes
    int32_t compact;         // 1: RowEnt8
    int32_t row_stride;      // >= max obj_h
    int32_t cap;             // entries per row
};

// k_tri_setup: per (frame, triangle): forward affine (:785-804, :1265-1306), its inverse (:1036-1038, :1345-1365),
// edge equations (:1141-1151) and row range (:1113-1115).
void launch_tri_setup(const PwMesh &mesh, const PwFrames &fr, hipStream_t stream);
struct UploadSegs { void *dst[3]; const void *src[3]; size_t n8[3]; };     // (dst, page-locked device-visible src, count of 8-byte words)
void launch_upload(const UploadSegs &sg, hipStream_t stream);              // small host -> device copies by ONE kernel launch

// k_pw_fused: _inversePiecewiseAffineWarp :1029-1058 for all frames, one workgroup per output row, without a
// materialised triangle map.  map_out (optional, int16 per output pixel) receives the per-pixel triangle id the
// lookup resolved == the reference's _trianglesCorrespondencesMatrix.
// sampling: HG_SAMPLE_NEAREST (0, the reference's pixel body) or HG_SAMPLE_BILINEAR (1), here and in launch_pw_from_map / launch_geo.
void launch_pw_fused(const PwMesh &mesh, const PwFrames &fr, uint8_t *out, int16_t *map_out, int sampling, hipStream_t stream);

// Fast path (see hg_k_piecewise.hip): eligibility, span-list build (includes the per-triangle solves), row warp.
bool pw_fast_ok(const PwMesh &mesh, int max_obj_w);
// ... for a whole frame set: with per-frame source minima, at both extremes of the set
bool pw_fast_ok(const PwMesh &mesh, const PwFrames &fr, int max_obj_w);
void launch_tri_spans(const PwMesh &mesh, const PwFrames &fr, const RowLists &rl, hipStream_t stream);
// The span cache of the packed 4-row self-span form (hg_span_cache.h): mode 0 none, 1 build (the prologue's slots are also written out),
// 2 use (groups whose directory entry is valid copy their slots in instead of evaluating spans).
struct SpanCacheDev {
    int4 *dir = nullptr;                        // n_frames x groups_per_frame SpanDirEnt
    uint4 *rec = nullptr;                       // cap16 16-byte words of records
    unsigned long long *cursor = nullptr;       // words handed out (may run past cap16: those groups are "not cached")
    uint32_t cap16 = 0;
    int32_t groups_per_frame = 0;
    int32_t mode = 0;
};
// The frame blocks of the use form's flat start (hg_span_start.h), n_frames of them: written at build time, handed to launch_pw_rows with mode 2.
void launch_span_frame_blocks(const PwMesh &mesh, const PwFrames &fr, SpanFrameBlock *blk, hipStream_t stream);
int launch_pw_rows(const PwMesh &mesh, const PwFrames &fr, const RowLists &rl, uint8_t *out, int16_t *map_out, int32_t *status_next, hipStream_t stream,
                   const SpanCacheDev &sc = SpanCacheDev(), const SpanFrameBlock *fblk = nullptr);
// Dense meshes (64..199 spans per row, obj_w <= 8192): 4 rows per workgroup, 16 x 4 pixel gather patches, one matrix record
// per triangle of the group.  Same row lists, same status protocol as launch_pw_rows; no map tap.
// (limits on the HOST ESTIMATES, which run ~10 % above the real counts the kernel enforces: 199 spans per row, 208 triangles
// per group; a frame set that does exceed those is redone once through the map path and the context drops back to k_pw_rows)
constexpr int kPatchMaxW = 8192, kPatchMaxRowSpans = 215, kPatchMaxGroupTris = 225;
// global_records: the variant for up to 511 spans per row whose pixels read their matrix from the tap array instead of LDS
constexpr int kPatchMaxRowSpansDense = 480;
int launch_pw_patch(const PwMesh &mesh, const PwFrames &fr, const RowLists &rl, uint8_t *out, int32_t *status_next, bool global_records, hipStream_t stream);
// Sheared meshes (self-span path only): tiles of 8 rows x <= 2048 columns whose gathers follow the source rows (hg_k_tile.hip).
constexpr int kTileRowSpanCap = 96;       // k_pw_tile: spans per row and tile (its LDS span blocks); beyond: the frame is flagged and redone, the mesh goes back to k_pw_patch
int launch_pw_tile(const PwMesh &mesh, const PwFrames &fr, const RowLists &rl, uint8_t *out, int max_obj_w, int32_t *status_next, hipStream_t stream);

// Materialised-map path for ONE frame (index f): map32 := -1; atomicMax rasteriser (:845-861 + :1111-1126); then
// the pixel loop :1042-1056 reading the map.
void launch_map_build(const PwMesh &mesh, const PwFrames &fr, int f, const FrameDesc &fd, int32_t *map32, hipStream_t stream);
void launch_pw_from_map(const PwMesh &mesh, const PwFrames &fr, int f, const FrameDesc &fd, const int32_t *map32,
                        uint8_t *out, int sampling, hipStream_t stream);
void launch_map_to_i16(const int32_t *map32, int16_t *map16, size_t n, hipStream_t stream);
void launch_map_max_i16(const int32_t *map32, size_t n, int32_t *out, hipStream_t stream);      // *out = largest (int16) value of the first n cells, -1 if none
void launch_fill_i32(int32_t *p, size_t n, int32_t v, hipStream_t stream);      // grid-stride fill (map / winner-buffer initialisation)

// Source fields (hg_k_field.hip; include/hgwarp.h HG_FIELD_*).  fmt: 0 = HG_FIELD_INDEX (int32 per pixel), 1 = HG_FIELD_COORDS (2 x f32 per pixel).
// Every frame record handed to these launchers carries the byte offset of the frame's FIELD in out_off (not that of its RGBA).
struct GeoFieldOne { FrameDesc fd; double m[8]; };          // one frame by value (launch_geo_field with frames == nullptr)
// k_geo_field: the field of the loop :997-1011 for all frames in one launch; mats = F x 8 doubles (inverse matrices).
void launch_geo_field(int kind, int fmt, const FrameDesc *frames, const double *mats, const GeoFieldOne &one, int n_frames, int max_h,
                      int W, int H, uint8_t *field, hipStream_t stream);
// k_pw_field: the field of the loop :1042-1056 for all frames, behind k_tri_setup; k_pw_fused's prologue, resolve and flag protocol.
void launch_pw_field(const PwMesh &mesh, const PwFrames &fr, int fmt, uint8_t *field, hipStream_t stream);
// k_field_from_map: the redo of ONE flagged frame (index f) from the map launch_map_build materialised.
void launch_field_from_map(const PwMesh &mesh, const PwFrames &fr, int f, const FrameDesc &fd, const int32_t *map32, int fmt, uint8_t *field,
                           hipStream_t stream);
// The remaps through a field (hg_k_remap.hip).
// k_remap_index<pixel_bytes>: out[i] = 0 <= field[i] < n_src ? src[field[i]] : 0; k_remap_bilinear_f32<channels>: four clamped taps per pixel.
void launch_remap_index(const int32_t *field, size_t n, const void *src, size_t n_src, int pixel_bytes, void *out, hipStream_t stream);
void launch_remap_bilinear_f32(const float *coords, size_t n, const float *src, int W, int H, int channels, float *out, hipStream_t stream);
// The remaps of a whole frame set in one launch (hg_k_remap.hip; the records: hg_remap_records.h).
// k_remap_index_frames<pixel_bytes, packed>: per pixel k_remap_index.  packed: a lane takes 4 consecutive pixels of its frame -- one 16-byte
// field load, four gathers, one store of 4 * pixel_bytes -- in frames whose field and output starts are aligned for it, and one pixel per
// lane elsewhere.  packed is honoured for the pixel sizes remap_index_packs() names; the others always take one pixel per lane.
bool remap_index_packs(int pixel_bytes);                    // does this build carry the packed form for the pixel size? (those measured to win)
void launch_remap_index_frames(const RemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, bool packed, const uint8_t *field,
                               const uint8_t *planes, size_t n_src, size_t plane_stride, int pixel_bytes, uint8_t *out, hipStream_t stream);
// k_remap_bilinear_frames<element, channels>: per pixel k_remap_bilinear_f32; elem 1 (u8) rounds the blend as blend4 does and stores the
// channel bytes of a pixel packed.  frames == nullptr: the one frame `one`, by value (blk0 = 0).
void launch_remap_bilinear_frames(const RemapFrame *frames, const RemapFrame &one, int n_frames, uint32_t n_blocks, uint64_t blk_px,
                                  const uint8_t *coords, const uint8_t *planes, size_t plane_stride, int W, int H, int elem, int channels,
                                  uint8_t *out, hipStream_t stream);

// Mip pyramids and the trilinear remap (hg_k_pyramid.hip; include/hgwarp.h hg_pyramid_* / hg_remap_trilinear_frames_device).
// k_pyr_down<element, channels>: level k (Wd x Hd) of every plane from level k - 1 (Ws x Hs): src / dst are the levels of plane 0, the
// other planes lie src_stride / dst_stride bytes apart.
void launch_pyr_down(const uint8_t *src, size_t src_stride, int Ws, int Hs, uint8_t *dst, size_t dst_stride, int Wd, int Hd, int n_planes,
                     int elem, int channels, hipStream_t stream);
// k_remap_trilinear_frames<element, channels>: lvl_off = `levels` byte offsets on the device (hg_pyramid_layout's; entry 0 unused).
void launch_remap_trilinear_frames(const TriRemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, const uint64_t *lvl_off, int levels,
                                   const uint8_t *coords, const uint8_t *planes, const uint8_t *pyrs, int W, int H, int elem, int channels,
                                   uint8_t *out, hipStream_t stream);
// k_remap_aniso_frames<element, channels> (hg_k_aniso.hip; hg_remap_aniso_frames_device): the trilinear launch plus max_aniso (1..16), the
// cap on the probes a pixel takes along its longer step.
void launch_remap_aniso_frames(const TriRemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, const uint64_t *lvl_off, int levels,
                               int max_aniso, const uint8_t *coords, const uint8_t *planes, const uint8_t *pyrs, int W, int H, int elem, int channels,
                               uint8_t *out, hipStream_t stream);
// k_remap_bicubic_frames<element, channels> (hg_k_bicubic.hip; hg_remap_bicubic_frames_device): the bilinear frames launch plus the cubic's
// coefficients by value; 4 x 4 clamped taps of level 0 per pixel, elem 1 (u8) clamped to 0..255 on both sides.
void launch_remap_bicubic_frames(const RemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, const CubicCoef &k,
                                 const uint8_t *coords, const uint8_t *planes, size_t plane_stride, int W, int H, int elem, int channels,
                                 uint8_t *out, hipStream_t stream);

// The mosaic (hg_k_mosaic.hip; include/hgwarp.h hg_mosaic_frames_device).
// k_mosaic_frames<element, channels>: every pixel of the canvas window (cx, cy, cw, ch), tightly packed at `canvas`, from the frames that
// cover it -- mode 0 the last one's pixel, 1 their mean, 2 their mean weighted by the distance to the W x H source's border capped at
// `feather`; weight (or nullptr): one float per canvas pixel.  n_quads == 0 zeroes the canvas (frames, coords and pixels are not read).
void launch_mosaic_frames(const MosaicFrame4 *frames, int n_quads, const uint8_t *coords, const uint8_t *pixels, int W, int H, int elem, int channels,
                          int mode, float feather, int cx, int cy, int cw, int ch, uint8_t *canvas, float *weight, const float *gains, hipStream_t stream);
// gains (or nullptr: the plain instantiation): one factor per record of the table, applied to every contributor's exposure channels before
// the blend (hg_mosaic_frames_gain_device).
// k_mosaic_stats<channels> (hg_k_mosaic_stats.hip; hg_mosaic_overlap_stats_device): for every ordered pair (a, b) of the n_frames (<= 256)
// u8 frames, the canvas pixels both contribute to and a's summed intensity over them, ADDED to stats[(a * n_frames + b) * 2 + {0, 1}]
// (the caller zeroes them) with 64-bit vector atomics.  The mosaic's tiling and table.
void launch_mosaic_stats(const MosaicFrame4 *frames, int n_frames, const uint8_t *coords, const uint8_t *pixels, int channels, int cx, int cy, int cw,
                         int ch, uint64_t *stats, hipStream_t stream);
// k_mosaic_robust<channels> (hg_k_robust.hip; the rules: hg_robust_dev.h; hg_mosaic_robust_device): every pixel of the canvas window from the
// n_frames (<= 256) u8 frames that cover it -- per channel the median (mode 0), a mean trimmed by `trim` at both ends (1), the minimum (2)
// or the maximum (3) of the contributors' bytes; weight (or nullptr): their number.  gains (or nullptr): one factor per record of the table.
// The mosaic's tiling and table; n_frames == 0 zeroes the canvas.
void launch_mosaic_robust(const MosaicFrame4 *frames, int n_frames, const uint8_t *coords, const uint8_t *pixels, int channels, int mode, float trim,
                          int cx, int cy, int cw, int ch, uint8_t *canvas, float *weight, const float *gains, hipStream_t stream);

// The multi-band mosaic (hg_k_multiband.hip; the rules: hg_multiband_dev.h; include/hgwarp.h hg_mosaic_multiband_device): k_mb_label over the
// quad table of the mosaic, k_mb_seed, one k_mb_reduce<element, channels, FIRST> per level 1..L-1 and one k_mb_blend<element, channels, LAST>
// per level L-1..0 over the table of the n_frames frames that take part.  blocks[0]: the seed's grid, blocks[k]: that of the reduce that
// writes level k (a launch without blocks is skipped); labels = the caller's plane or the one in the work area; weight may be nullptr.
struct MbArgs {
    const MosaicFrame4 *quads; int n_quads; const MbFrame *frames; int n_frames; MbCanvas cv; uint32_t blocks[kMbMaxBands];
    const uint8_t *coords, *pixels; int W, H, elem, channels; float feather; uint8_t *work; int32_t *labels; uint8_t *canvas; float *weight;
};
void launch_multiband(const MbArgs &a, hipStream_t stream);

// Point lists (hg_k_points.hip; include/hgwarp.h hg_points_*): n_sets lists of n_points interleaved (x, y) floats, frame f reads list
// f % n_sets and writes n_points (x, y) pairs at f * n_points of `out`; an unmapped point is the quiet NaN of HG_FIELD_COORDS in both words.
// k_geo_points<kind, dir>: dir 0 = to source (mats: the inverse matrices, W x H the source's size: coverage test :1001), dir 1 = to output
// (mats: the forward matrices, W x H the domain of the loop :919-920).  frames: x_off, y_off, obj_w, obj_h of every frame are read.
void launch_geo_points(int kind, int dir, const FrameDesc *frames, const double *mats, int n_frames, int W, int H, const float *points, int n_points,
                       int n_sets, float *out, hipStream_t stream);
// k_pw_points_src: to source through the staged piecewise set, behind k_tri_setup, no map; frames flagged FRAME_IRREGULAR are left to
// k_points_from_map: ONE frame (index f) from the map launch_map_build materialised.  points / out: the bases of all lists / all results.
void launch_pw_points_src(const PwMesh &mesh, const PwFrames &fr, const float *points, int n_points, int n_sets, float *out, hipStream_t stream);
void launch_points_from_map(const PwMesh &mesh, const PwFrames &fr, int f, const FrameDesc &fd, const int32_t *map32, const float *points,
                            int n_points, int n_sets, float *out, hipStream_t stream);
// k_pw_points_out: to output through the forward triangle map (map_w x map_h cells from (min_src_x, min_src_y)) and the forward matrices
// fwd = F x T x 6 floats of k_tri_setup.
void launch_pw_points_out(const int32_t *fmap, const float *fwd, const FrameDesc *frames, int n_frames, int T, int min_src_x, int min_src_y,
                          int map_w, int map_h, const float *points, int n_points, int n_sets, float *out, hipStream_t stream);

// Fitting transforms to matches (hg_k_fit.hip; the rules: hg_fit_dev.h): k_fit_hypotheses + k_fit_score (n_hyp > 0), then k_fit_finish.
// matches = F x n_points (x, y, u, v) float32, 16-byte aligned; counts = F int32 on the device; samples = F x n_hyp x 4 int32 or nullptr (drawn);
// scratch: hyp_mats = F x n_hyp x 8 doubles, hyp_valid = F x n_hyp flags, best = F words ZEROED by the caller ((count << 32) | (0xffffffff - h)
// of the best valid hypothesis).  out_min / out_best / out_mask may be nullptr.
struct FitArgs {
    int kind; const void *matches; int n_points; const int32_t *counts; int n_frames; double threshold; int n_hyp; uint32_t seed;
    const int32_t *samples; int refit; double *hyp_mats; int32_t *hyp_valid; unsigned long long *best;
    double *out_mats, *out_min; int32_t *out_counts, *out_best; uint8_t *out_mask;
};
void launch_fit(const FitArgs &a, hipStream_t stream);

// Refining transforms on the pixels (hg_k_align.hip; the rules: hg_align_dev.h): n_iter + 1 passes of k_align_accumulate + k_align_update over all
// frames, none of them waited for.  from / to: ONE-byte luma planes (the caller's, or the copies launch_align_luma made of 4-channel planes),
// frame f reads from + f * from_stride and to + (f % n_to_sets) * to_stride.  nx = samples per row of the grid, n_samples = all of them,
// n_chunks = ceil(n_samples / kAlignChunk).  scratch: state = F records, part = F x n_chunks x kAlignRec doubles.  sums may be nullptr.
struct AlignArgs {
    int kind, photometric; const uint8_t *from; int Wf, Hf; size_t from_stride; const uint8_t *to; int Wt, Ht, n_to_sets; size_t to_stride;
    int rx, ry, rw, rh, step, nx, n_samples, n_chunks, n_frames, n_iter; double eps; int min_valid;
    const double *mats_in; double *mats_out; AlignInfo *info; double *sums; AlignState *state; double *part;
};
void launch_align_luma(const uint8_t *src, size_t src_stride, int W, int H, int n_planes, uint8_t *dst, hipStream_t stream);
void launch_align(const AlignArgs &a, hipStream_t stream);

// Thin-plate splines (hg_k_tps.hip; the rules and the argument blocks: hg_tps_dev.h): k_tps_solve, one workgroup per frame; k_tps_field over the
// windows (step 1) or over the lattice and then k_tps_blend (step > 1; fmt = HG_FIELD_*); k_tps_points, frame f reading list f % n_sets.
// Adjusting a frame set over all pairs (hg_k_bundle.hip; the rules and the argument block: hg_bundle_dev.h): pass 0, then per round assembly,
// solve, pass, reduction and decision (up to kBundleLdsCap unknowns all but the pass in ONE workgroup per round, H in LDS; above, the blocked
// factorisation in scratch), none of them waited for.
hipError_t launch_bundle(const BundleArgs &a, hipStream_t stream);   // (the first error of the attribute call or of a launch)

void launch_tps_solve(const TpsSolveArgs &a, hipStream_t stream);
void launch_tps_field(const TpsFieldArgs &a, int fmt, hipStream_t stream);
void launch_tps_points(const double *records, int n_points, int n_frames, const float *points, int n_pts, int n_sets, float *out, hipStream_t stream);

// Camera models (hg_k_camera.hip; the rules and the argument blocks: hg_camera_dev.h): k_camera_field, one workgroup per frame, piece of 256
// columns and band of kCamBandRows rows (fmt = HG_FIELD_*, surface = HG_SURFACE_*); k_camera_points, frame f reading list f % n_sets, canvas ->
// source or source -> canvas.
void launch_camera_field(const CamFieldArgs &a, int fmt, int surface, hipStream_t stream);
void launch_camera_points(const CamPointArgs &a, bool to_source, hipStream_t stream);

// Dense optical flow (hg_k_flow.hip; the rules and the argument blocks: hg_flow_dev.h): k_flow_up, the flow of a level from the level below it;
// k_flow_iter, one Jacobi iteration of a level over tiles of kFlowTileW x kFlowTileH pixels; k_flow_finish, field, flow pairs and residual of
// level 0.  k_field_compose_frames: the bilinear frames remap's launch over an inner field as a 2-channel f32 plane, NaN pattern where not finite.
void launch_flow_up(const FlowUpArgs &a, int n_frames, hipStream_t stream);
void launch_flow_iter(const FlowIterArgs &a, int n_frames, hipStream_t stream);
void launch_flow_finish(const FlowFinishArgs &a, int n_frames, hipStream_t stream);
void launch_field_compose_frames(const RemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, const uint8_t *outer, const uint8_t *inner,
                                 size_t inner_stride, int W, int H, uint8_t *out, hipStream_t stream);

// Matching descriptors (hg_k_match.hip; the rules: hg_match_dev.h): k_match_bits resp. k_match_u8 for the two nearest train rows of every query,
// the same kernel with the sides swapped for the best query of every train row (cross_check), then k_match_finish.  query = F lists of
// n_query rows of `stride` bytes, train = n_train_sets lists of n_train rows (frame f reads list f % n_train_sets), both 16-byte aligned;
// counts_q = F and counts_t = n_train_sets int32 on the device; rr = ratio (bits) resp. ratio * ratio (bytes), ratio_on = 0: no ratio test.
// cross_check: 0 none, 1 the swapped launch (scratch ws_rev), 2 the atomic form (scratch ws_keys = F x n_train words set to all ones by the caller).
// scratch: ws_fwd = F x n_query and ws_rev = F x n_train records {j1, d1, d2, 0}.  out_matches / out_pairs /
// out_nn may be nullptr; out_matches needs both point lists.
struct MatchArgs {
    int kind, desc_bytes; size_t stride; const void *query; int n_query; const void *train; int n_train; int n_frames, n_train_sets;
    const int32_t *counts_q, *counts_t; int ratio_on; double rr; uint32_t max_distance; int cross_check; const void *query_pts, *train_pts;
    uint4 *ws_fwd, *ws_rev; unsigned long long *ws_keys; int32_t *out_counts; void *out_matches; int32_t *out_pairs, *out_nn;
};
void launch_match(const MatchArgs &a, hipStream_t stream);

// Detecting and describing keypoints (hg_k_detect.hip; the rules: hg_detect_dev.h): k_detect_cells, k_detect_compact and, when descriptors or
// info are asked for, k_detect_describe.  planes = n_planes planes of W x H x channels u8 at plane_stride bytes.  scratch: ws_rec = n_planes x
// cells x per_cell 16-byte records, ws_cnt = n_planes x cells counts, ws_list = n_planes x n_slots flat indices in list order (-1: padding),
// ws_table = the turned pattern of hg_describe_pattern (4-byte aligned).  out_points / out_desc / out_info may be nullptr.
struct DetectArgs {
    const uint8_t *planes; int W, H, n_planes; size_t plane_stride; int channels, cell, per_cell, cells_x, cells_y; int64_t min_response; size_t desc_stride;
    void *ws_rec; int32_t *ws_cnt, *ws_list; const int8_t *ws_table; int32_t *out_counts; void *out_points, *out_desc, *out_info;
};
void launch_detect(const DetectArgs &a, hipStream_t stream);

// k_geo: _inverseGeometricWarp pixel loop :997-1011 for all frames.  mats = F x 8 doubles (inverse matrices).
// f32_exact: every affine matrix entry is a float value and |x| < 2^28 (lets the kernel use an exact-product fma).
// n_imgs / img_stride: frame f reads the source at img + (f % n_imgs) * img_stride.
// Returns the code of the kernel it launched (hg_last_geometric_kernel), -1 if it launched none.
int launch_geo(int kind, bool f32_exact, const FrameDesc *frames, const double *mats, int n_frames, int max_w, int max_h,
               const uint8_t *img, int W, int H, int n_imgs, uint64_t img_stride, uint8_t *out, const int32_t *plain, int nw, int xcc_log2, bool rotate_bands,
               int sampling, hipStream_t stream);
// Per-frame matrix solves on the device (one lane per frame): kind 1 = projective 8x8 DLT in numeric.js' LU order, 4 points
// per set; kind 0 = affine closed form, 3 points per set.  mats = F x 8 doubles; plain[f] = 1 where the projective frame's
// window stays in the plain division range (launch_geo then takes the per-frame flag instead of a host proof).
void launch_solve_frames(int kind, const float *from, const float *to, const FrameDesc *frames, double *mats, int32_t *plain, int n, hipStream_t stream);
// (f32_exact doubles as "plain division range proved" for kind 1: see geo_plain_division() in hg_api_geometric.hip)
// div2_plain vs IEEE division on `samples` pseudo-random operand triples; returns the number of mismatching quotients
unsigned long long run_selftest_division(uint64_t seed, uint64_t samples, unsigned long long *d_counter, hipStream_t stream);

// Forward (scatter) paths, SURVEY.md §8f-1: winner buffer `win` = obj_w*obj_h int32 scratch.
// Tile-binned forward warp (k_fwd_tiles): per frame the forward matrix (8 doubles, affine in m[0..5]), the adjugate of its 3x3
// form (any positive multiple of the inverse; use_inv = 0 when it is not trustworthy: tiles then scan every source row).
struct FwdParam { double m[8]; double inv[9]; int32_t use_inv, pad; };
constexpr int kFwdTileW = 64, kFwdTileH = 64, kFwdWrap = 32;
// params == nullptr: one frame, carried by value (p0, f0) in the kernel arguments
struct FwdBatch { const FwdParam *params; const FrameDesc *frames; FwdParam p0; FrameDesc f0; };
// n_imgs / img_stride (all forward launchers that take them): frame f reads the source at img + (f % n_imgs) * img_stride
void launch_fwd_tiles(int kind, const FwdBatch &batch, int n_frames, int max_w, int max_h,
                      const uint8_t *img, int n_imgs, uint64_t img_stride, int W, int H, uint8_t *out, hipStream_t stream);
// Tile-binned forward PIECEWISE warp: k_fmap_bbox (once per mesh: bounding box, in map cells, of the cells the forward
// triangle map assigns to each matrix index), k_fwd_pw_bins (per frame and triangle: which output tiles its pixels can reach,
// per aliasing shift k of the flat index; frames it cannot bound are flagged for the scatter path), k_fwd_pw_tiles (per tile:
// gather the candidates of the filed (triangle, k) entries, winners in LDS).
enum : int32_t { FWD_FALLBACK = 1, FWD_OVERFLOW = 2 };
constexpr int kFwdPwCapMax = 256;
struct FwdPwTiles {
    const int32_t *fmap; const float *fwd; const int32_t *bbox; const FrameDesc *frames;
    const int32_t *rowext;      // per (matrix index t, row of its bbox): {min mx, max mx} of its cells in that map row, at rowoff[t] + (my - bbox.cy0)
    const uint32_t *rowoff;
    int32_t *tile_cnt, *tile_ent, *status;
    int32_t *host_flag;         // page-locked, device-visible word set to 1 by any kernel that flags a frame (nullptr: none); see PwFrames::host_flag
    int32_t T, min_src_x, min_src_y, map_w, map_h, tsx, tsy, cap;
};
void launch_fmap_bbox(const int32_t *fmap, int map_w, int map_h, int32_t *bbox, int T, hipStream_t stream);
void launch_fmap_rowext(const int32_t *fmap, int map_w, int map_h, const int32_t *bbox, const uint32_t *rowoff, int32_t *rowext, size_t total_rows, int T, hipStream_t stream);
void launch_fwd_pw_tiles(const FwdPwTiles &p, int n_frames, int max_w, int max_h, const uint8_t *img, int n_imgs, uint64_t img_stride, int W, int H, uint8_t *out, hipStream_t stream);
void launch_fwd_geo(int kind, const double *d_mat, const uint8_t *img, int W, int H, const FrameDesc &fd, int32_t *win, uint8_t *out, hipStream_t stream);
void launch_fwd_pw(const int32_t *fmap, const float *fwd, const uint8_t *img, int W, int H, int min_src_x, int min_src_y, int map_w, int map_h,
                   const FrameDesc &fd, int32_t *win, uint8_t *out, hipStream_t stream);
// The forward SOURCE FIELD (include/hgwarp.h, hg_field_forward_*): one int32 per output pixel, the flat source index of the pixel the forward loop's
// last writer reads, -1 where nobody writes or that read is outside the source array.  The same launches as above with field tails
// (k_fwd_tiles<.., FIELD>, k_fwd_pw_tiles<FIELD>; scatter path: k_fwd_win_field instead of k_fwd_gather); out_off of every frame record is the
// byte offset of the frame's FIELD.  Only the source's size is read, never its pixels.
void launch_fwd_tiles_field(int kind, const FwdBatch &batch, int n_frames, int max_w, int max_h, int W, int H, uint8_t *field, hipStream_t stream);
void launch_fwd_pw_tiles_field(const FwdPwTiles &p, int n_frames, int max_w, int max_h, int W, int H, uint8_t *field, hipStream_t stream);
void launch_fwd_geo_field(int kind, const double *d_mat, int W, int H, const FrameDesc &fd, int32_t *win, uint8_t *field, hipStream_t stream);
void launch_fwd_pw_field(const int32_t *fmap, const float *fwd, int W, int H, int min_src_x, int min_src_y, int map_w, int map_h,
                         const FrameDesc &fd, int32_t *win, uint8_t *field, hipStream_t stream);

} // namespace hg
