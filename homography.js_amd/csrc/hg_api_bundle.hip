// hg_api_bundle.hip -- the C ABI, part 13: adjusting the transforms of a frame set over all pairs (hg_bundle_layout,
// hg_bundle_adjust_frames_device, hg_bundle_chain_from_pairs, hg_bundle_invert_matrix).  Like a fit, the call is work of its own: it needs no
// image, mesh or frame set and leaves the warp paths' taps (hg_last_*_kernel), the sampling mode, the plan of the last warp, what the policy
// learned and every staged frame set as it found them.  Scratch comes from the caller (hg_bundle_layout), as the splines' does.
#include "hg_ctx.h"
#include "hg_bundle_dev.h"

#include <cmath>
#include <cstring>
#include <vector>

static_assert(HG_BUNDLE_SUMS == kBundleRec, "the header's constant is the kernels'");
constexpr int kBundleMaxSide = 32768, kBundleMaxPoints = 65536, kBundleMaxIter = 64;

static int check_bundle_kind(hg_ctx *c, int kind)
{
    if (kind != HG_AFFINE && kind != HG_PROJECTIVE) return fail(c, HG_ERR_INVALID, "bundle: unknown kind");
    return HG_OK;
}

static int check_bundle_shape(hg_ctx *c, int kind, int n_frames, int n_pairs, int n_points)
{
    HG_TRY(check_bundle_kind(c, kind));
    if (n_frames < 0 || n_frames > HG_BUNDLE_MAX_FRAMES) return fail(c, HG_ERR_INVALID, "bundle: n_frames must be 0..256");
    if (n_pairs < 0 || n_pairs > HG_BUNDLE_MAX_PAIRS) return fail(c, HG_ERR_INVALID, "bundle: n_pairs must be 0..8192");
    if (n_points < 0 || n_points > kBundleMaxPoints) return fail(c, HG_ERR_INVALID, "bundle: n_points must be 0..65536");
    return HG_OK;
}

static int check_bundle_pairs(hg_ctx *c, int n_frames, const int32_t *pairs, int n_pairs)
{
    if (n_pairs > 0 && !pairs) return fail(c, HG_ERR_INVALID, "bundle: pairs is NULL");
    for (int p = 0; p < n_pairs; p++) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || a >= n_frames || b < 0 || b >= n_frames || a == b)
            return fail(c, HG_ERR_INVALID, "bundle: pairs[" + std::to_string(p) + "] must name two different frames below n_frames");
    }
    return HG_OK;
}

// Where the parts of the scratch lie (bytes, each at the 256-byte grain), for the worst case of the shape: every frame free, every list full.
struct BundlePlan { size_t state, ints, good, iter, part, recs, Hm, Wm, total; size_t n_ints; };

static BundlePlan bundle_plan(int kind, int n_frames, int n_pairs, int n_points)
{
    const size_t F = (size_t)n_frames, NP = (size_t)n_pairs, P = (size_t)bundle_p(kind);
    const size_t cpp = ((size_t)n_points + kBundleChunk - 1) / kBundleChunk, N = std::min<size_t>(P * F, kBundleMaxUnknowns);
    BundlePlan p;
    size_t off = 0;
    auto part = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    p.n_ints = 4 * NP + 2 * NP * cpp + 2 * F + (F + 1) + 2 * NP;
    p.state = part(sizeof(hg::BundleState));
    p.ints = part(p.n_ints * 4);
    p.good = part(F * 4);
    p.iter = part(2 * F * 8 * 8);
    p.part = part(NP * cpp * kBundleRec * 8);
    p.recs = part(2 * NP * kBundleRec * 8);
    p.Hm = part((N + 1) * N * 8);
    p.Wm = part(N > (size_t)kBundleLdsCap ? (N + 1) * N * 8 : 0);
    p.total = off;
    return p;
}

extern "C" int hg_bundle_layout(int kind, int n_frames, int n_pairs, int n_points, size_t *scratch_bytes)
{
    HG_TRY(check_bundle_shape(nullptr, kind, n_frames, n_pairs, n_points));
    if (!scratch_bytes) return fail(nullptr, HG_ERR_INVALID, "hg_bundle_layout: scratch_bytes is NULL");
    *scratch_bytes = n_frames == 0 ? 0 : bundle_plan(kind, n_frames, n_pairs, n_points).total;
    return HG_OK;
}

extern "C" int hg_bundle_adjust_frames_device(hg_ctx *c, int kind, int W, int H, int n_frames, const uint8_t *fixed, const int32_t *pairs, int n_pairs,
                                              const void *d_matches, int n_points, const int32_t *counts, const uint8_t *d_mask, int n_iter,
                                              double eps, double lambda0, double huber, const double *d_mats_in, double *d_mats_out, void *d_info,
                                              double *d_pair_sums, void *d_scratch, size_t scratch_bytes)
{
    // (the shape: needs no device)
    HG_TRY(check_bundle_kind(c, kind));
    if (W < 1 || W > kBundleMaxSide || H < 1 || H > kBundleMaxSide) return fail(c, HG_ERR_INVALID, "bundle: W and H must be 1..32768");
    HG_TRY(check_bundle_shape(c, kind, n_frames, n_pairs, n_points));
    HG_TRY(check_bundle_pairs(c, n_frames, pairs, n_pairs));
    if (counts)
        for (int p = 0; p < n_pairs; p++)
            if (counts[p] < 0 || counts[p] > n_points) return fail(c, HG_ERR_INVALID, "bundle: counts[" + std::to_string(p) + "] must be 0..n_points");
    if (n_iter < 0 || n_iter > kBundleMaxIter) return fail(c, HG_ERR_INVALID, "bundle: n_iter must be 0..64");
    if (!(eps >= 0.0) || !(eps < INFINITY)) return fail(c, HG_ERR_INVALID, "bundle: eps must be finite and >= 0");
    if (!(lambda0 > 0.0) || !(lambda0 < INFINITY)) return fail(c, HG_ERR_INVALID, "bundle: lambda0 must be finite and > 0");
    if (!(huber >= 0.0) || !(huber < INFINITY)) return fail(c, HG_ERR_INVALID, "bundle: huber must be finite and >= 0");
    if (n_frames == 0) return c ? HG_OK : fail(nullptr, HG_ERR_INVALID, "ctx is NULL");
    if (!fixed) return fail(c, HG_ERR_INVALID, "bundle: fixed is NULL");
    const int F = n_frames, P = bundle_p(kind);
    bool any_fixed = false;
    for (int f = 0; f < F; f++) any_fixed = any_fixed || fixed[f] != 0;
    if (!any_fixed) return fail(c, HG_ERR_INVALID, "bundle: at least one frame must be fixed");
    // which frames a path of pairs with matches ties to a fixed frame, the work list of the pass and the assembly's lists
    const BundlePlan plan = bundle_plan(kind, n_frames, n_pairs, n_points);
    hg::BundleLists lists;
    hg::bundle_build_lists(n_frames, fixed, pairs, n_pairs, counts, n_points, lists);
    const std::vector<int32_t> &ints = lists.ints;
    const size_t n_work = (size_t)lists.n_work, o_work = lists.o_work, o_cls = lists.o_cls, o_fidx = lists.o_fidx, o_rowptr = lists.o_rowptr, o_ent = lists.o_ent;
    const int n_free = lists.n_free, N = P * n_free;
    if (N > kBundleMaxUnknowns) return fail(c, HG_ERR_INVALID, "bundle: more than 2048 unknowns");
    if (scratch_bytes < plan.total) return fail(c, HG_ERR_INVALID, "bundle: scratch_bytes is below hg_bundle_layout's");
    if (!d_mats_in || !d_mats_out || !d_info || !d_scratch || (n_work > 0 && !d_matches))
        return fail(c, HG_ERR_INVALID, "hg_bundle_adjust_frames_device: d_matches / d_mats_in / d_mats_out / d_info / d_scratch is NULL");
    if (misaligned(d_matches, 16) || misaligned(d_scratch, 16)) return fail(c, HG_ERR_INVALID, "hg_bundle_adjust_frames_device: d_matches / d_scratch must be aligned to 16 bytes");
    if (misaligned(d_mats_in, 8) || misaligned(d_mats_out, 8) || misaligned(d_info, 8) || misaligned(d_pair_sums, 8))
        return fail(c, HG_ERR_INVALID, "hg_bundle_adjust_frames_device: d_mats_in / d_mats_out / d_info / d_pair_sums must be aligned to 8 bytes");
    HG_TRY(bind(c));
    HG_TRY(hg_sync(c));                                      // queued runs: settled first, as the fit does
    uint8_t *S = static_cast<uint8_t *>(d_scratch);
    int32_t *d_ints = reinterpret_cast<int32_t *>(S + plan.ints);
    HG_TRY(upload_copied(c, c->bundle_stage, "bundle lists staging", d_ints, ints.data(), ints.size() * 4));
    hg::BundleArgs a{};
    a.kind = kind; a.W = W; a.H = H; a.n_frames = F; a.n_pairs = n_pairs; a.n_points = n_points; a.n_work = (int)n_work; a.n_free = n_free; a.N = N;
    a.n_iter = N == 0 ? 0 : n_iter;
    a.eps = eps; a.lambda0 = lambda0; a.huber = huber;
    a.matches = static_cast<const float *>(d_matches); a.mask = d_mask;
    a.pairs4 = d_ints; a.work = d_ints + o_work; a.cls = d_ints + o_cls; a.fidx = d_ints + o_fidx; a.rowptr = d_ints + o_rowptr; a.ent = d_ints + o_ent;
    a.good = reinterpret_cast<int32_t *>(S + plan.good);
    a.mats_in = d_mats_in; a.mats_out = d_mats_out; a.info = static_cast<uint8_t *>(d_info); a.sums = d_pair_sums;
    a.state = reinterpret_cast<hg::BundleState *>(S + plan.state);
    a.iter = reinterpret_cast<double *>(S + plan.iter); a.part = reinterpret_cast<double *>(S + plan.part);
    a.recs = reinterpret_cast<double *>(S + plan.recs); a.Hm = reinterpret_cast<double *>(S + plan.Hm); a.Wm = reinterpret_cast<double *>(S + plan.Wm);
    HIP_TRY(c, hg::launch_bundle(a, c->stream));
    return HG_OK;
}

extern "C" int hg_bundle_chain_from_pairs(int kind, int n_frames, const int32_t *pairs, int n_pairs, const double *pair_mats, int anchor, double *mats_out)
{
    HG_TRY(check_bundle_shape(nullptr, kind, n_frames, n_pairs, 0));
    HG_TRY(check_bundle_pairs(nullptr, n_frames, pairs, n_pairs));
    if (n_frames == 0) return HG_OK;
    if (anchor < 0 || anchor >= n_frames) return fail(nullptr, HG_ERR_INVALID, "hg_bundle_chain_from_pairs: anchor must be a frame");
    if (!mats_out || (n_pairs > 0 && !pair_mats)) return fail(nullptr, HG_ERR_INVALID, "hg_bundle_chain_from_pairs: pair_mats / mats_out is NULL");
    const int np = bundle_p(kind);
    std::vector<double> M((size_t)n_frames * 9, 0.0);
    std::vector<int> level((size_t)n_frames, -1);
    std::vector<uint8_t> usable((size_t)n_pairs, 1);
    for (int p = 0; p < n_pairs; p++)
        for (int k = 0; k < np; k++) if (!align_finite(pair_mats[(size_t)p * 8 + k])) usable[(size_t)p] = 0;
    M[(size_t)anchor * 9 + 0] = 1.0; M[(size_t)anchor * 9 + 4] = 1.0; M[(size_t)anchor * 9 + 8] = 1.0;
    level[(size_t)anchor] = 0;
    for (int lv = 0;; lv++) {
        bool grew = false;
        for (int p = 0; p < n_pairs; p++) {
            if (!usable[(size_t)p]) continue;
            const int a = pairs[2 * p], b = pairs[2 * p + 1];
            double q[9], qi[9], t[9];
            if (level[(size_t)b] == lv && level[(size_t)a] < 0) {          // M_a = M_b Q
                align_to3x3(kind, pair_mats + (size_t)p * 8, q);
                bundle_mul3(&M[(size_t)b * 9], q, t);
                for (int k = 0; k < 9; k++) M[(size_t)a * 9 + k] = t[k] / t[8];
                level[(size_t)a] = lv + 1; grew = true;
            } else if (level[(size_t)a] == lv && level[(size_t)b] < 0) {   // M_b = M_a Q^-1
                align_to3x3(kind, pair_mats + (size_t)p * 8, q);
                bundle_inv3(q, qi);
                bundle_mul3(&M[(size_t)a * 9], qi, t);
                for (int k = 0; k < 9; k++) M[(size_t)b * 9 + k] = t[k] / t[8];
                level[(size_t)b] = lv + 1; grew = true;
            }
        }
        if (!grew) break;
    }
    for (int f = 0; f < n_frames; f++) {
        if (level[(size_t)f] < 0) { for (int k = 0; k < 8; k++) mats_out[(size_t)f * 8 + k] = NAN; }
        else bundle_from3x3(kind, &M[(size_t)f * 9], mats_out + (size_t)f * 8);
    }
    return HG_OK;
}

extern "C" int hg_bundle_invert_matrix(int kind, const double *m_in, double *m_out)
{
    HG_TRY(check_bundle_kind(nullptr, kind));
    if (!m_in || !m_out) return fail(nullptr, HG_ERR_INVALID, "hg_bundle_invert_matrix: m_in / m_out is NULL");
    double a[9], inv[9], out[8];
    align_to3x3(kind, m_in, a);
    bundle_inv3(a, inv);
    bundle_from3x3(kind, inv, out);
    for (int k = 0; k < 8; k++) m_out[k] = out[k];
    return HG_OK;
}
