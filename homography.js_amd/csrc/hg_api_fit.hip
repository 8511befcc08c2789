// hg_api_fit.hip -- the C ABI, part 8: fitting frame transforms to point matches (hg_fit_sample_indices, hg_fit_matches_frames_device).
// A fit is geometry of its own: it needs no image, mesh or frame set, is independent of the sampling mode, and leaves the warp paths' taps
// (hg_last_*_kernel), the plan of the last warp, what the policy learned and every staged frame set as it found them.
#include "hg_ctx.h"
#include "hg_fit_dev.h"

constexpr int kFitMaxPoints = 65536, kFitMaxHyp = 65536, kFitMaxFrames = 4096;

// What both entries check, in the order of the header's list.  c may be NULL (the host entry).
static int check_fit_shape(hg_ctx *c, int kind, int n_frames, const int32_t *counts, int n_points, int n_hyp)
{
    if (kind != HG_AFFINE && kind != HG_PROJECTIVE) return fail(c, HG_ERR_INVALID, "fit: unknown kind");
    if (n_points < 0 || n_points > kFitMaxPoints) return fail(c, HG_ERR_INVALID, "fit: n_points must be 0..65536");
    if (n_hyp < 0 || n_hyp > kFitMaxHyp) return fail(c, HG_ERR_INVALID, "fit: n_hyp must be 0..65536");
    if (n_frames < 0 || n_frames > kFitMaxFrames) return fail(c, HG_ERR_INVALID, "fit: n_frames must be 0..4096");
    if (counts)
        for (int f = 0; f < n_frames; f++)
            if (counts[f] < 0 || counts[f] > n_points) return fail(c, HG_ERR_INVALID, "fit: counts[" + std::to_string(f) + "] must be 0..n_points");
    return HG_OK;
}

extern "C" int hg_fit_sample_indices(int kind, uint32_t seed, int n_frames, const int32_t *counts, int n_points, int n_hyp, int32_t *out)
{
    HG_TRY(check_fit_shape(nullptr, kind, n_frames, counts, n_points, n_hyp));
    if (n_frames == 0 || n_hyp == 0) return HG_OK;
    if (!out) return fail(nullptr, HG_ERR_INVALID, "hg_fit_sample_indices: out is NULL");
    const int K = fit_k(kind);
    for (int f = 0; f < n_frames; f++)
        for (int h = 0; h < n_hyp; h++)
            (void)fit_draw(K, seed, (uint32_t)f, (uint32_t)h, counts ? counts[f] : n_points, out + ((size_t)f * n_hyp + h) * 4);
    return HG_OK;
}

extern "C" int hg_fit_matches_frames_device(hg_ctx *c, int kind, const void *d_matches, int n_points, const int32_t *counts, int n_frames,
                                            double threshold, int n_hyp, uint32_t seed, const int32_t *d_samples, int refit,
                                            double *d_mats, double *d_min_mats, int32_t *d_counts, int32_t *d_best, uint8_t *d_mask)
{
    HG_TRY(bind(c));
    HG_TRY(check_fit_shape(c, kind, n_frames, counts, n_points, n_hyp));
    if (!(threshold >= 0.0) || !(threshold < INFINITY)) return fail(c, HG_ERR_INVALID, "hg_fit_matches_frames_device: threshold must be finite and >= 0");
    if (n_hyp == 0 && !refit) return fail(c, HG_ERR_INVALID, "hg_fit_matches_frames_device: n_hyp == 0 needs refit (the least-squares fit)");
    if (n_frames == 0) return HG_OK;
    if (!d_mats || !d_counts || (n_points > 0 && !d_matches)) return fail(c, HG_ERR_INVALID, "hg_fit_matches_frames_device: d_matches / d_mats / d_counts is NULL");
    if (misaligned(d_matches, 16)) return fail(c, HG_ERR_INVALID, "hg_fit_matches_frames_device: d_matches must be aligned to 16 bytes ((x, y, u, v) float32)");
    if (misaligned(d_mats, 8) || misaligned(d_min_mats, 8)) return fail(c, HG_ERR_INVALID, "hg_fit_matches_frames_device: d_mats / d_min_mats must be aligned to 8 bytes");
    if (misaligned(d_counts, 4) || misaligned(d_best, 4) || misaligned(d_samples, 4))
        return fail(c, HG_ERR_INVALID, "hg_fit_matches_frames_device: d_counts / d_best / d_samples must be aligned to 4 bytes");
    HG_TRY(hg_sync(c));                                      // queued runs: settled first, as the point lists do
    const size_t F = (size_t)n_frames, H = (size_t)n_hyp;
    const size_t cnt_words = (F + 1) / 2;                    // the counts, padded to 8 bytes
    HG_TRY(ensure(c, c->d_fit_mats, std::max<size_t>(F * H * 8, 8)));
    HG_TRY(ensure(c, c->d_fit_valid, std::max<size_t>(F * H, 1)));
    HG_TRY(ensure(c, c->d_fit_frames, F + cnt_words));
    int32_t *d_cnt = reinterpret_cast<int32_t *>(c->d_fit_frames.p + F);
    HG_TRY(upload_filled(c, c->fit_stage, "fit counts staging", d_cnt, cnt_words * 8, [&](uint8_t *h) {
        int32_t *hc = reinterpret_cast<int32_t *>(h);
        for (size_t f = 0; f < 2 * cnt_words; f++) hc[f] = f < F ? (counts ? counts[f] : n_points) : 0;
    }));
    HIP_TRY(c, hipMemsetAsync(c->d_fit_frames.p, 0, F * 8, c->stream));
    FitArgs a{kind, d_matches, n_points, d_cnt, n_frames, threshold, n_hyp, seed, d_samples, refit ? 1 : 0, c->d_fit_mats, c->d_fit_valid,
              reinterpret_cast<unsigned long long *>(c->d_fit_frames.p), d_mats, d_min_mats, d_counts, d_best, d_mask};
    launch_fit(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}
