// hg_api_mosaic.hip -- the C ABI, part 6c: the frames of a set blended into one canvas through their source fields: the mosaic and the gained
// mosaic (hg_mosaic_frames_device, hg_mosaic_frames_gain_device), the robust mosaic (hg_mosaic_robust_device), the overlap statistics
// (hg_mosaic_overlap_stats_device) and the host-only gain solve (hg_mosaic_solve_gains).  The multi-band mosaic is in hg_api_multiband.hip.
// Like a remap a mosaic needs no image, mesh or staged frame set.
#include "hg_ctx.h"

#include <cmath>

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
