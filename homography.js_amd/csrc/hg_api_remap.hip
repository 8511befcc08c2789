// hg_api_remap.hip -- the C ABI, part 6b: planes of whole frame sets through a source field: the plane offsets (hg_pack_plane_offsets), the
// mip pyramids (hg_pyramid_levels, hg_pyramid_layout, hg_pyramid_build_device) and the index, bilinear, bicubic, trilinear and anisotropic
// frames remaps (hg_remap_*_frames_device, hg_remap_bilinear_u8_device), with remap_flat_frames, which the chained field of hg_api_flow.hip
// shares.  A remap needs no image, mesh or staged frame set: the fields and the planes are the caller's.
#include "hg_ctx.h"

// ------------------------------------------------------------------------------------------------ remaps of whole frame sets
extern "C" int hg_pack_plane_offsets(const hg_geom *g, int n, size_t px_bytes, size_t *offsets, size_t *total)
{
    if (!g || n < 0 || px_bytes < 1 || !offsets || !total) return fail(nullptr, HG_ERR_INVALID, "hg_pack_plane_offsets: bad arguments");
    pack_offsets(g, n, px_bytes, offsets, total);
    return HG_OK;
}

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
    HG_TRY(upload_filled(c, c->field_stage, "field frame staging", c->d_tri_table, words * 8, [&](uint8_t *h) {
        uint64_t *tab = reinterpret_cast<uint64_t *>(h);
        for (int k = 0; k < 32; k++) tab[k] = lvl[k];
        TriRemapFrame *tf = reinterpret_cast<TriRemapFrame *>(tab + 32);
        for (int f = 0; f < n_frames; f++) {
            const RemapFrame &r = recs[(size_t)f];
            tf[f] = TriRemapFrame{r.fld_off, r.out_off, r.n_px, (uint64_t)r.plane * plane_stride_bytes, (uint64_t)r.plane * pyr_stride_bytes, r.blk0,
                                  (uint32_t)std::max(geoms[f].obj_w, 0), (uint32_t)std::max(geoms[f].obj_h, 0), 0};
        }
    }));
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
