// hg_api_match.hip -- the C ABI, part 9: matching feature descriptors of frame sets (hg_match_descriptors_frames_device).
// Like a fit, a match is work of its own: it needs no image, mesh or frame set, is independent of the sampling mode, and leaves the warp paths'
// taps (hg_last_*_kernel), the plan of the last warp, what the policy learned and every staged frame set as it found them.
#include "hg_ctx.h"
#include "hg_match_dev.h"

constexpr int kMatchMaxRows = 65536, kMatchMaxFrames = 4096, kMatchMaxBytes = 512;

// The checks that need no pointer, in the order of the header's list.
static int check_match_shape(hg_ctx *c, int kind, int desc_bytes, size_t stride, int n_query, const int32_t *counts_q, int n_frames, int n_train,
                             const int32_t *counts_t, int n_train_sets, double ratio)
{
    if (kind != HG_DESC_BITS && kind != HG_DESC_U8) return fail(c, HG_ERR_INVALID, "match: unknown descriptor kind");
    if (desc_bytes < 1 || desc_bytes > kMatchMaxBytes) return fail(c, HG_ERR_INVALID, "match: desc_bytes must be 1..512");
    if ((stride & 15) != 0 || stride < (size_t)desc_bytes) return fail(c, HG_ERR_INVALID, "match: stride must be a multiple of 16 and >= desc_bytes");
    if (n_query < 0 || n_query > kMatchMaxRows) return fail(c, HG_ERR_INVALID, "match: n_query must be 0..65536");
    if (n_train < 0 || n_train > kMatchMaxRows) return fail(c, HG_ERR_INVALID, "match: n_train must be 0..65536");
    if (n_frames < 0 || n_frames > kMatchMaxFrames) return fail(c, HG_ERR_INVALID, "match: n_frames must be 0..4096");
    if (n_train_sets < 1 || n_train_sets > std::max(n_frames, 1)) return fail(c, HG_ERR_INVALID, "match: n_train_sets must be 1..max(n_frames, 1)");
    if (counts_q)
        for (int f = 0; f < n_frames; f++)
            if (counts_q[f] < 0 || counts_q[f] > n_query) return fail(c, HG_ERR_INVALID, "match: counts_q[" + std::to_string(f) + "] must be 0..n_query");
    if (counts_t)
        for (int s = 0; s < n_train_sets; s++)
            if (counts_t[s] < 0 || counts_t[s] > n_train) return fail(c, HG_ERR_INVALID, "match: counts_t[" + std::to_string(s) + "] must be 0..n_train");
    if (!(ratio >= 0.0) || !(ratio <= 1.0)) return fail(c, HG_ERR_INVALID, "match: ratio must be 0 (no test) .. 1");
    return HG_OK;
}

extern "C" int hg_match_descriptors_frames_device(hg_ctx *c, int desc_kind, int desc_bytes, size_t stride, const void *d_query, int n_query,
                                                  const int32_t *counts_q, int n_frames, const void *d_train, int n_train, const int32_t *counts_t,
                                                  int n_train_sets, double ratio, uint32_t max_distance, int cross_check, const void *d_query_pts,
                                                  const void *d_train_pts, int32_t *d_counts, void *d_matches, int32_t *d_pairs, int32_t *d_nn)
{
    HG_TRY(check_match_shape(c, desc_kind, desc_bytes, stride, n_query, counts_q, n_frames, n_train, counts_t, n_train_sets, ratio));      // (needs no device)
    HG_TRY(bind(c));
    if (n_frames == 0) return HG_OK;
    const bool work = n_query > 0 && n_train > 0;                // (without rows on one side no descriptor is read)
    if (!d_counts || (work && (!d_query || !d_train))) return fail(c, HG_ERR_INVALID, "hg_match_descriptors_frames_device: d_query / d_train / d_counts is NULL");
    if (misaligned(d_query, 16) || misaligned(d_train, 16)) return fail(c, HG_ERR_INVALID, "hg_match_descriptors_frames_device: d_query / d_train must be aligned to 16 bytes");
    if (misaligned(d_counts, 4) || misaligned(d_pairs, 4) || misaligned(d_nn, 4))
        return fail(c, HG_ERR_INVALID, "hg_match_descriptors_frames_device: d_counts / d_pairs / d_nn must be aligned to 4 bytes");
    if (misaligned(d_matches, 16)) return fail(c, HG_ERR_INVALID, "hg_match_descriptors_frames_device: d_matches must be aligned to 16 bytes ((x, y, u, v) float32)");
    if (misaligned(d_query_pts, 8) || misaligned(d_train_pts, 8)) return fail(c, HG_ERR_INVALID, "hg_match_descriptors_frames_device: d_query_pts / d_train_pts must be aligned to 8 bytes");
    if (d_matches && (!d_query_pts || !d_train_pts)) return fail(c, HG_ERR_INVALID, "hg_match_descriptors_frames_device: d_matches needs d_query_pts and d_train_pts");
    HG_TRY(hg_sync(c));                                      // queued runs: settled first, as the fit does
    const size_t F = (size_t)n_frames, S = (size_t)n_train_sets;
    const size_t cnt_words = (F + S + 1) / 2;                // both sides' counts, padded to 8 bytes
    HG_TRY(ensure(c, c->d_match_counts, 2 * cnt_words));
    HG_TRY(ensure(c, c->d_match_fwd, std::max<size_t>(F * (size_t)n_query, 1)));
    const bool bits = desc_kind == HG_DESC_BITS;
    // the cross-check: bits by a second launch with the sides swapped, bytes by atomicMin inside the one launch (what measured faster for each;
    // option "match_cross" 0: the swapped launch for bytes too, for measurements)
    const int cross = !cross_check ? 0 : ((bits || c->opt_match_cross == 0) ? 1 : 2);
    if (cross == 1) HG_TRY(ensure(c, c->d_match_rev, std::max<size_t>(F * (size_t)n_train, 1)));
    if (cross == 2) {
        HG_TRY(ensure(c, c->d_match_keys, std::max<size_t>(F * (size_t)n_train, 1)));
        if (work) HIP_TRY(c, hipMemsetAsync(c->d_match_keys.p, 0xff, F * (size_t)n_train * 8, c->stream));
    }
    HG_TRY(upload_filled(c, c->match_stage, "match counts staging", c->d_match_counts.p, cnt_words * 8, [&](uint8_t *h) {
        int32_t *hc = reinterpret_cast<int32_t *>(h);
        for (size_t f = 0; f < F; f++) hc[f] = counts_q ? counts_q[f] : n_query;
        for (size_t s = 0; s < S; s++) hc[F + s] = counts_t ? counts_t[s] : n_train;
        for (size_t k = F + S; k < 2 * cnt_words; k++) hc[k] = 0;
    }));
    hg::MatchArgs a{bits ? 0 : 1, desc_bytes, stride, d_query, n_query, d_train, n_train, n_frames, n_train_sets, c->d_match_counts.p, c->d_match_counts.p + F,
                    ratio != 0.0 ? 1 : 0, bits ? ratio : ratio * ratio, max_distance, cross, d_query_pts, d_train_pts, c->d_match_fwd.p,
                    cross == 1 ? c->d_match_rev.p : nullptr, cross == 2 ? reinterpret_cast<unsigned long long *>(c->d_match_keys.p) : nullptr, d_counts, d_matches, d_pairs, d_nn};
    hg::launch_match(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}
