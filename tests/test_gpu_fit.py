"""hg_fit_matches_frames_device on the GPU against the numpy model of tests/hgtest/fit.py (written from the header's text): the best
hypothesis, its inlier count, its mask and the bits of its minimal matrix are compared exactly; the least-squares refit by tolerance.
tests/test_fit_cpu.py pins the model and the host entry.  Shapes are the smallest at which the kernels can go wrong: three frames, up to
T + 1 matches (T = the scoring kernel's LDS tile, read from hg_fit_dev.h) and up to 257 hypotheses (its workgroup holds 256).

The refit's tolerance.  Metric: the largest displacement, in pixels, between two matrices' images of the four corners of the inliers'
bounding box.  Base: the float64 model against the np.longdouble model on the same inliers; the device may lie 16 x that from the float64
model (it differs from it in summation order only); a base of 0 is replaced by the smallest non-zero base of the planted cases.  Measured
bases on the planted cases (65 matches in a 640 x 480 picture): 5.1e-14 .. 2.3e-13 px affine, 7.6e-14 .. 2.6e-13 px projective; the largest
device / base ratio over this file's refits on an MI355X: 8.07 (EXPERIMENTS.md, "Fitting")."""
import base64
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import fit as FM                 # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import FILL, INVALID  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = (FM.AFFINE, FM.PROJECTIVE)
T = FM.tile()
TAIL = 256                                   # canary bytes behind every output
planted, check, counts_for = FM.planted, FM.check, FM.counts_for

@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ run and check
def run(ctx, kind, matches, counts, threshold, n_hyp, seed=0, samples=None, refit=True, skip=()):
    """Upload, fill every output with FILL (TAIL canary bytes behind each), call, sync, download.  skip: optional outputs passed as NULL."""
    matches = np.asarray(matches, F32)
    F, N = matches.shape[0], matches.shape[1]
    sizes = {"mats": F * 64, "min": F * 64, "counts": F * 4, "best": F * 4, "mask": F * N}
    bufs = {k: ctx.alloc(v + TAIL) for k, v in sizes.items()}
    d_m = ctx.alloc(max(matches.nbytes, 16))
    d_s = ctx.alloc(samples.nbytes) if samples is not None and samples.size else 0
    try:
        if matches.size:
            ctx.to_device(d_m, matches)
        if d_s:
            ctx.to_device(d_s, np.ascontiguousarray(samples, np.int32))
        for k, v in sizes.items():
            ctx.to_device(bufs[k], np.full(v + TAIL, FILL, np.uint8))
        want = {k: (0 if k in skip else bufs[k]) for k in sizes}
        ctx.fit_matches_frames_device(kind, d_m if matches.size else 0, N, counts, F, threshold, n_hyp, seed, want["mats"], want["counts"], d_samples=d_s,
                                      refit=refit, d_min_mats=want["min"], d_best=want["best"], d_mask=want["mask"])
        ctx.sync()
        raw = {k: ctx.to_host(bufs[k], v + TAIL) for k, v in sizes.items()}
    finally:
        for p in list(bufs.values()) + [d_m] + ([d_s] if d_s else []):
            ctx.free(p)
    for k, v in sizes.items():
        assert (raw[k][v:] == FILL).all(), (k, "the canary behind the buffer")
        if k in skip:
            assert (raw[k] == FILL).all(), (k, "an output that was not asked for")
    return FM.unpack(np.concatenate([raw[k][:v] for k, v in sizes.items()]), F, N)


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_points", (0, 3, 4, 5, 63, 64, 65, T - 1, T, T + 1))
def test_match_counts_around_the_tile(ctx, kind, n_points):
    m, _ = planted(kind, 100 + n_points, 3, n_points)
    counts = counts_for(n_points)
    w = FM.fit(kind, m, counts, 1.0, 65, seed=n_points)
    check(kind, run(ctx, kind, m, counts, 1.0, 65, seed=n_points), w, m, ("n_points", n_points))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_hyp", (1, 63, 64, 65, 255, 256, 257))
def test_hypothesis_counts_around_the_workgroup(ctx, kind, n_hyp):
    m, _ = planted(kind, 200 + n_hyp, 3, 65)
    counts = counts_for(65)
    w = FM.fit(kind, m, counts, 1.0, n_hyp, seed=7)
    check(kind, run(ctx, kind, m, counts, 1.0, n_hyp, seed=7), w, m, ("n_hyp", n_hyp))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("threshold", (0.0, 1.0, 1e30))
def test_thresholds(ctx, kind, threshold):
    m, _ = planted(kind, 31, 3, 65)
    if threshold == 1e30:
        m[0, 62, 1] = 100.0                                       # (no 1e30 coordinate under a 1e30 threshold: NaN and +Inf stay)
    w = FM.fit(kind, m, None, threshold, 65, seed=5)
    if threshold == 1e30:
        assert w.counts.tolist() == [63, 65, 65] and (w.mask[0, 63:] == 0).all()      # every finite match; the NaN and the Inf never
    if threshold == 0.0:
        assert (w.counts <= 65 * 0.6).all()
    check(kind, run(ctx, kind, m, None, threshold, 65, seed=5), w, m, ("threshold", threshold))


# ------------------------------------------------------------------------------------------------ caller-given samples
@pytest.mark.parametrize("kind", KINDS)
def test_given_samples_their_refusals_and_the_tie(ctx, kind):
    K = FM.k_of(kind)
    m, truth, counts, s = FM.given_samples_case(kind)
    w = FM.fit(kind, m, counts, 1.0, 8, samples=s)
    assert w.best.tolist() == [2, -1, -1] and w.counts[0] == truth[0].sum() and w.counts[1:].tolist() == [0, 0]
    assert np.array_equal(w.mask[0] > 0, truth[0]) and not w.mask[1:].any()
    assert np.isnan(w.mats[1:]).all() and np.isnan(w.min_mats[1:]).all()
    g = run(ctx, kind, m, counts, 1.0, 8, samples=s)
    check(kind, g, w, m, "given samples")
    assert (g.min_mats[1:].view(np.uint64) == FM.QNAN_BITS).all() and (g.mats[1:].view(np.uint64) == FM.QNAN_BITS).all()
    if K == 3:                                                    # affine with -1 in the fourth slot is valid
        assert FM.sample_ok(kind, s[0, 4], 65)


# ------------------------------------------------------------------------------------------------ refit off, optional outputs, determinism
@pytest.mark.parametrize("kind", KINDS)
def test_without_refit_the_result_is_the_minimal_matrix(ctx, kind):
    m, _ = planted(kind, 51, 3, 65)
    counts = counts_for(65)
    w = FM.fit(kind, m, counts, 1.0, 65, seed=9, refit_on=False)
    g = run(ctx, kind, m, counts, 1.0, 65, seed=9, refit=False)
    check(kind, g, w, m, "refit == 0")
    assert np.array_equal(g.raw["mats"], g.raw["min"])


@pytest.mark.parametrize("kind", KINDS)
def test_optional_outputs_as_null_and_two_runs_of_one_call(ctx, kind):
    m, _ = planted(kind, 61, 3, 65)
    counts = counts_for(65)
    w = FM.fit(kind, m, counts, 1.0, 65, seed=11)
    full = run(ctx, kind, m, counts, 1.0, 65, seed=11)
    check(kind, full, w, m, "all outputs")
    again = run(ctx, kind, m, counts, 1.0, 65, seed=11)
    for k in full.raw:
        assert np.array_equal(full.raw[k], again.raw[k]), (k, "two runs of one call")
    for skip in ("min", "best", "mask"):
        g = run(ctx, kind, m, counts, 1.0, 65, seed=11, skip=(skip,))
        for k in full.raw:
            if k != skip:
                assert np.array_equal(full.raw[k], g.raw[k]), (skip, k)


# ------------------------------------------------------------------------------------------------ least squares without sampling
@pytest.mark.parametrize("kind", KINDS)
def test_least_squares_of_all_finite_matches(ctx, kind):
    K = FM.k_of(kind)
    m, truth = planted(kind, 71, 4, 65)
    m[0, 62, 1] = 100.0                                           # (the 1e30: gone; NaN and +Inf stay and are left out)
    m[2, K - 1:, 0] = np.nan                                      # K - 1 finite matches: NaNs
    counts = [65, 65, 65, K]
    w = FM.fit(kind, m, counts, 1.0, 0)
    assert w.counts.tolist() == [63, 65, K - 1, K] and (w.best == -1).all() and np.isnan(w.min_mats).all() and np.isnan(w.mats[2]).all()
    g = run(ctx, kind, m, counts, 1.0, 0)
    check(kind, g, w, m, "n_hyp == 0")
    assert np.array_equal(run(ctx, kind, m, counts, 1.0, 0).raw["mats"], g.raw["mats"])


# ------------------------------------------------------------------------------------------------ planted models
@pytest.mark.parametrize("kind", KINDS)
def test_planted_models_are_found(ctx, kind):
    m, truth = planted(kind, 3, 3, 65, specials=False)
    assert (truth.sum(1) == 39).all()
    seed = 3
    w = FM.fit(kind, m, None, 1.0, 256, seed=seed)
    for f in range(3):                                            # first the MODEL: its best hypothesis' mask is the planted set
        assert np.array_equal(w.mask[f] > 0, truth[f]), (f, "choose another seed")
    g = run(ctx, kind, m, None, 1.0, 256, seed=seed)
    check(kind, g, w, m, "planted")
    for f in range(3):
        p = m[f][truth[f]].astype(np.float64)
        px, py = FM.project(kind, g.mats[f].reshape(1, 8), p[:, 0], p[:, 1])
        err = np.sqrt((px[0] - p[:, 2]) ** 2 + (py[0] - p[:, 3]) ** 2).max()
        assert err < 1e-3, (f, err)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    m, _ = planted(1, 81, 2, 8)
    d = ctx.alloc(8192)
    try:
        d_m, d_o, d_c = d, d + 4096, d + 6144
        ctx.to_device(d_m, m)
        fit = ctx.fit_matches_frames_device

        def refused(*a, **k):
            assert GF.refusal_code(fit, *a, **k) == INVALID, (a, k)

        refused(2, d_m, 8, None, 2, 1.0, 8, 0, d_o, d_c)                         # kind
        refused(1, d_m, -1, None, 2, 1.0, 8, 0, d_o, d_c)
        refused(1, d_m, 65537, None, 2, 1.0, 8, 0, d_o, d_c)
        refused(1, d_m, 8, None, 2, 1.0, -1, 0, d_o, d_c)
        refused(1, d_m, 8, None, 2, 1.0, 65537, 0, d_o, d_c)
        refused(1, d_m, 8, None, -1, 1.0, 8, 0, d_o, d_c)
        refused(1, d_m, 8, None, 4097, 1.0, 8, 0, d_o, d_c)
        refused(1, d_m, 8, [8, 9], 2, 1.0, 8, 0, d_o, d_c)
        refused(1, d_m, 8, [-1, 8], 2, 1.0, 8, 0, d_o, d_c)
        for thr in (-1.0, float("nan"), float("inf")):
            refused(1, d_m, 8, None, 2, thr, 8, 0, d_o, d_c)
        refused(1, d_m, 8, None, 2, 1.0, 0, 0, d_o, d_c, refit=False)            # n_hyp == 0 without refit
        refused(1, 0, 8, None, 2, 1.0, 8, 0, d_o, d_c)                           # NULL, misaligned
        refused(1, d_m, 8, None, 2, 1.0, 8, 0, 0, d_c)
        refused(1, d_m, 8, None, 2, 1.0, 8, 0, d_o, 0)
        refused(1, d_m + 8, 8, None, 2, 1.0, 8, 0, d_o, d_c)
        refused(1, d_m, 8, None, 2, 1.0, 8, 0, d_o + 4, d_c)
        refused(1, d_m, 8, None, 2, 1.0, 8, 0, d_o, d_c + 2)
        refused(1, d_m, 8, None, 2, 1.0, 8, 0, d_o, d_c, d_min_mats=d_o + 132)
        refused(1, d_m, 8, None, 2, 1.0, 8, 0, d_o, d_c, d_best=d_c + 65)
        refused(1, d_m, 8, None, 2, 1.0, 8, 0, d_o, d_c, d_samples=d_c + 1)
        ctx.to_device(d_o, np.full(4096, FILL, np.uint8))
        fit(1, 0, 8, None, 0, 1.0, 8, 0, 0, 0)                                   # n_frames == 0: HG_OK, nothing is written
        ctx.sync()
        assert (ctx.to_host(d_o, 4096) == FILL).all()
        fit(1, d_m, 8, None, 2, 0.0, 8, 0, d_o, d_c)                             # threshold 0 is legal; the context still works
        ctx.sync()
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def test_state_is_untouched_and_a_staged_set_warps_the_same_bytes():
    W, H, F = 64, 40, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((0.6, 0.45), (7.0, 3.0))
    m, _ = planted(1, 91, F, 65)
    w = FM.fit(1, m, None, 1.0, 64, seed=2)
    with HG.Context(0) as c:
        d_src, d_w, d_m, d_o = c.alloc(img.nbytes), c.alloc(total), c.alloc(m.nbytes), c.alloc(4096)
        try:
            c.set_sampling(HG.SAMPLE_BILINEAR)
            c.to_device(d_src, img)
            c.to_device(d_m, m)
            c.set_image_device(d_src, W, H)
            c.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, offs)
            c.to_device(d_w, np.zeros(total, np.uint8))                       # (the padding between the frames is nobody's: zero both times)
            c.warp_inverse_geometric_frames_device(d_w)
            c.sync()
            alone = c.to_host(d_w, total)
            before = GF.tap_state(c)
            c.to_device(d_w, np.zeros(total, np.uint8))
            c.fit_matches_frames_device(1, d_m, 65, None, F, 1.0, 64, 2, d_o, d_o + 1024, d_best=d_o + 2048)
            assert GF.tap_state(c) == before
            c.sync()
            assert GF.tap_state(c) == before and c.sampling == HG.SAMPLE_BILINEAR
            assert np.array_equal(c.to_host(d_o + 2048, F * 4).view(np.int32), w.best)
            assert np.array_equal(c.to_host(d_o + 1024, F * 4).view(np.int32), w.counts)
            c.warp_inverse_geometric_frames_device(d_w)                       # the staged set is still the warps'
            c.sync()
            assert alone.any() and np.array_equal(c.to_host(d_w, total), alone)
        finally:
            c.set_image(img)
            for p in (d_src, d_w, d_m, d_o):
                c.free(p)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_fit_matches_equals_the_ctypes_call(ctx, tmp_path):
    """tests/js/fit_gpu.mjs: h.fitMatches of js/Homography.mjs on the real addon for the planted case of both kinds (typed and nested
    lists, the last one shorter: padding and counts) must give the bits of the ctypes call; it also feeds the fitted affine matrices to
    warpForwardGeometricBatch."""
    F, N, short, n_hyp, seed = 3, 65, 50, 256, 3
    sets = {name: planted(kind, 3, F, N, specials=False)[0] for name, kind in (("affine", FM.AFFINE), ("projective", FM.PROJECTIVE))}
    case = tmp_path / "fit_case.json"
    case.write_text(json.dumps({"F": F, "N": N, "short": short, "threshold": 1.0, "hypotheses": n_hyp, "seed": seed,
                                "affine": base64.b64encode(sets["affine"].tobytes()).decode(), "projective": base64.b64encode(sets["projective"].tobytes()).decode()}))
    res = GF.run_node_case("fit_gpu.mjs", str(case))
    for name, kind in (("affine", FM.AFFINE), ("projective", FM.PROJECTIVE)):
        counts = [N, N, short]
        g = run(ctx, kind, sets[name], counts, 1.0, n_hyp, seed=seed)
        check(kind, g, FM.fit(kind, sets[name], counts, 1.0, n_hyp, seed=seed), sets[name], ("js", name))
        js = res["cases"][name]
        assert base64.b64decode(js["matrices"]) == g.raw["mats"].tobytes() and base64.b64decode(js["minimal"]) == g.raw["min"].tobytes(), name
        assert js["counts"] == g.counts.tolist() and js["best"] == g.best.tolist(), name
        for f in range(F):
            assert base64.b64decode(js["inliers"][f]) == g.mask[f, :counts[f]].tobytes(), (name, f)
