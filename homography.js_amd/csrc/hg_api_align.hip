// hg_api_align.hip -- the C ABI, part 11: refining frame transforms on the pixels (hg_align_scale_matrix, hg_align_refine_frames_device).
// Like a fit, the call is work of its own: it needs no image, mesh or frame set, is independent of the sampling mode, and leaves the warp
// paths' taps (hg_last_*_kernel), the plan of the last warp, what the policy learned and every staged frame set as it found them.
#include "hg_ctx.h"
#include "hg_align_dev.h"

static_assert(HG_ALIGN_SUMS == kAlignSums, "the header's constant is the kernels'");
constexpr int kAlignMaxSide = 32768, kAlignMaxFrames = 4096, kAlignMaxStep = 64, kAlignMaxIter = 64, kAlignMaxLevel = 30;

extern "C" int hg_align_scale_matrix(int kind, const double *m_in, int level_in, int level_out, double *m_out)
{
    if (kind != HG_AFFINE && kind != HG_PROJECTIVE) return fail(nullptr, HG_ERR_INVALID, "align: unknown kind");
    if (level_in < 0 || level_in > kAlignMaxLevel || level_out < 0 || level_out > kAlignMaxLevel)
        return fail(nullptr, HG_ERR_INVALID, "hg_align_scale_matrix: levels must be 0..30");
    if (!m_in || !m_out) return fail(nullptr, HG_ERR_INVALID, "hg_align_scale_matrix: m_in / m_out is NULL");
    double out[8];
    align_scale(kind, m_in, level_in, level_out, out);
    for (int k = 0; k < 8; k++) m_out[k] = out[k];
    return HG_OK;
}

extern "C" int hg_align_refine_frames_device(hg_ctx *c, int kind, const void *d_from, int Wf, int Hf, int n_frames, size_t from_stride_bytes,
                                             const void *d_to, int Wt, int Ht, int n_to_sets, size_t to_stride_bytes, int channels,
                                             int rx, int ry, int rw, int rh, int step, int photometric, int n_iter, double eps, int min_valid,
                                             const double *d_mats_in, double *d_mats_out, void *d_info, double *d_sums)
{
    // (the shape: needs no device)
    if (kind != HG_AFFINE && kind != HG_PROJECTIVE) return fail(c, HG_ERR_INVALID, "align: unknown kind");
    auto bad_plane = [](int W, int H) { return W < 1 || W > kAlignMaxSide || H < 1 || H > kAlignMaxSide || (int64_t)W * H > ((int64_t)1 << 30); };
    if (bad_plane(Wf, Hf) || bad_plane(Wt, Ht)) return fail(c, HG_ERR_INVALID, "align: W and H of both planes must be 1..32768 and W * H <= 2^30");
    if (channels != 1 && channels != 4) return fail(c, HG_ERR_INVALID, "align: channels must be 1 or 4");
    if (rw < 1 || rh < 1 || rx < 0 || ry < 0 || (int64_t)rx + rw > Wf || (int64_t)ry + rh > Hf)
        return fail(c, HG_ERR_INVALID, "align: the rectangle must be non-empty and lie inside the FROM plane");
    if (step < 1 || step > kAlignMaxStep) return fail(c, HG_ERR_INVALID, "align: step must be 1..64");
    if (photometric != 0 && photometric != 1) return fail(c, HG_ERR_INVALID, "align: photometric must be 0 or 1");
    if (n_iter < 0 || n_iter > kAlignMaxIter) return fail(c, HG_ERR_INVALID, "align: n_iter must be 0..64");
    if (!(eps >= 0.0) || !(eps < INFINITY)) return fail(c, HG_ERR_INVALID, "align: eps must be finite and >= 0");
    if (min_valid < align_p(kind, photometric)) return fail(c, HG_ERR_INVALID, "align: min_valid must be >= P (6 affine, 8 projective, plus 2 with gain and bias)");
    if (n_frames < 0 || n_frames > kAlignMaxFrames) return fail(c, HG_ERR_INVALID, "align: n_frames must be 0..4096");
    if (n_to_sets < 1 || n_to_sets > std::max(n_frames, 1)) return fail(c, HG_ERR_INVALID, "align: n_to_sets must be 1..max(n_frames, 1)");
    const size_t from_bytes = (size_t)Wf * (size_t)Hf * (size_t)channels, to_bytes = (size_t)Wt * (size_t)Ht * (size_t)channels;
    if (from_stride_bytes < from_bytes || to_stride_bytes < to_bytes) return fail(c, HG_ERR_INVALID, "align: a plane stride must be >= W * H * channels");
    HG_TRY(bind(c));
    if (n_frames == 0) return HG_OK;
    if (!d_from || !d_to || !d_mats_in || !d_mats_out || !d_info)
        return fail(c, HG_ERR_INVALID, "hg_align_refine_frames_device: d_from / d_to / d_mats_in / d_mats_out / d_info is NULL");
    if (misaligned(d_mats_in, 8) || misaligned(d_mats_out, 8) || misaligned(d_sums, 8))
        return fail(c, HG_ERR_INVALID, "hg_align_refine_frames_device: d_mats_in / d_mats_out / d_sums must be aligned to 8 bytes");
    if (misaligned(d_info, 8)) return fail(c, HG_ERR_INVALID, "hg_align_refine_frames_device: d_info must be aligned to 8 bytes");
    HG_TRY(hg_sync(c));                                      // queued runs: settled first, as the fit does
    const size_t F = (size_t)n_frames;
    const int nx = (rw + step - 1) / step, ny = (rh + step - 1) / step;
    const int n_samples = nx * ny;                           // (<= W * H <= 2^30)
    const int n_chunks = (n_samples + kAlignChunk - 1) / kAlignChunk;
    HG_TRY(ensure(c, c->d_align_state, F));
    HG_TRY(ensure(c, c->d_align_part, F * (size_t)n_chunks * kAlignRec));
    const uint8_t *from = static_cast<const uint8_t *>(d_from), *to = static_cast<const uint8_t *>(d_to);
    size_t from_stride = from_stride_bytes, to_stride = to_stride_bytes;
    if (channels == 4) {                                     // the luma copies: every FROM plane, then the TO planes
        const size_t nf = (size_t)Wf * (size_t)Hf, nt = (size_t)Wt * (size_t)Ht;
        HG_TRY(ensure(c, c->d_align_luma, F * nf + (size_t)n_to_sets * nt));
        launch_align_luma(from, from_stride_bytes, Wf, Hf, n_frames, c->d_align_luma.p, c->stream);
        launch_align_luma(to, to_stride_bytes, Wt, Ht, n_to_sets, c->d_align_luma.p + F * nf, c->stream);
        from = c->d_align_luma.p; from_stride = nf;
        to = c->d_align_luma.p + F * nf; to_stride = nt;
    }
    AlignArgs a{kind, photometric, from, Wf, Hf, from_stride, to, Wt, Ht, n_to_sets, to_stride, rx, ry, rw, rh, step, nx, n_samples, n_chunks, n_frames, n_iter,
                eps, min_valid, d_mats_in, d_mats_out, static_cast<AlignInfo *>(d_info), d_sums, c->d_align_state.p, c->d_align_part.p};
    launch_align(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}
