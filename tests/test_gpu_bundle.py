"""hg_bundle_adjust_frames_device on the GPU against the numpy model of tests/hgtest/bundle.py (written from the header's text).
tests/test_bundle_cpu.py pins the model, the host entries and -- on the cases of this file that ask for it -- the conditions under which
status, rounds, accepted and n_valid are compared exactly.  Shapes are the smallest at which the kernels can go wrong: frames of 96 x 64,
three to six of them, more only where the size of the system asks for it (free-frame counts around kBundleLdsCap and kBundlePanel, read
from hg_bundle_dev.h, and one call at 256 frames), slot counts around the workgroup's 256 lanes and around kBundleChunk.

The tolerance (the fit's and the alignment's recipe).  Metric for matrices: the largest displacement, in canvas pixels, of the four frame
corners between two matrices.  d_pair_sums and every rms: relative error against the longdouble model.  Base: the float64 model against the
model whose sums and solve run in np.longdouble, on the same case; the device may lie 16 x that from the float64 model (it differs from it
in the order of the sums only); a base of 0 is replaced by the smallest non-zero base of the planted cases, and no relative base is taken
below 2^-53 (a float64 cannot be asked to lie closer to a longdouble value than half its ulp).  The float64 model follows the header's
order of operations in the pass and in the solve, so the device lies at the model: the largest device / base ratio over this file on an
MI355X is 1.0 (EXPERIMENTS.md, "Bundle adjustment")."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import bundle as BM              # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import FILL, INVALID, POISON  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = (BM.AFFINE, BM.PROJECTIVE)
CH, CAP, PANEL = BM.chunk(), BM.lds_cap(), BM.panel()
TAIL = 256                                   # canary bytes behind every output
WORST = [0.0]


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()
    print(f"largest device / base ratio of this file: {WORST[0]:.3g}")


# ------------------------------------------------------------------------------------------------ run and check
def run(ctx, c, sums=True, alias=False, garbage=None):
    """Upload the matches and the mask (inside allocations full of POISON) and the matrices, fill every output with FILL (TAIL canary bytes
    behind each), call, sync, download.  sums=False: d_pair_sums is NULL.  alias: d_mats_out is d_mats_in.  garbage: a float32 value written
    into every slot at or beyond counts[p] before the upload."""
    F, NP, n = c.F, len(c.pairs), c.n_points
    M = c.matches.copy()
    if garbage is not None:
        for p in range(NP):
            M[p, int(c.counts[p]):] = garbage
    info_bytes = HG.bundle_info_bytes(F, NP)
    scratch = HG.bundle_layout(c.kind, F, NP, n)
    sizes = {"mats": F * 64, "info": info_bytes, "sums": NP * BM.SUMS * 8}
    bufs = {k: ctx.alloc(v + TAIL) for k, v in sizes.items()}
    d_m, d_k, d_in, d_s = ctx.alloc(M.nbytes + 256), ctx.alloc(NP * n + 256), ctx.alloc(F * 64 + TAIL), ctx.alloc(scratch + 256)
    try:
        ctx.to_device(d_m, np.concatenate([M.view(np.uint8).ravel(), np.full(256, POISON, np.uint8)]))
        ctx.to_device(d_k, np.concatenate([(c.mask if c.mask is not None else np.zeros(0, np.uint8)).ravel(),
                                           np.full(256 + (0 if c.mask is not None else NP * n), POISON, np.uint8)]))
        ctx.to_device(d_in, np.concatenate([c.mats.view(np.uint8).ravel(), np.full(TAIL, FILL, np.uint8)]))
        for k, v in sizes.items():
            ctx.to_device(bufs[k], np.full(v + TAIL, FILL, np.uint8))
        ctx.bundle_adjust_frames_device(c.kind, c.W, c.H, F, c.fixed, c.pairs, d_m, n, c.counts_arg, d_in, d_in if alias else bufs["mats"], bufs["info"],
                                        d_s, scratch, d_mask=d_k if c.mask is not None else 0, n_iter=c.n_iter, eps=c.eps, lambda0=c.lambda0, huber=c.huber,
                                        d_pair_sums=bufs["sums"] if sums else 0)
        ctx.sync()
        raw = {k: ctx.to_host(bufs[k], v + TAIL) for k, v in sizes.items()}
        raw_in = ctx.to_host(d_in, F * 64 + TAIL)
    finally:
        for p in list(bufs.values()) + [d_m, d_k, d_in, d_s]:
            ctx.free(p)
    for k, v in sizes.items():
        assert (raw[k][v:] == FILL).all(), (k, "the canary behind the buffer")
    assert (raw_in[F * 64:] == FILL).all()
    if not sums:
        assert (raw["sums"] == FILL).all(), "an output that was not asked for"
    if alias:
        assert (raw["mats"] == FILL).all()
        raw["mats"] = raw_in
    else:
        assert np.array_equal(raw_in[:F * 64], c.mats.view(np.uint8).ravel()), "the input matrices must not be written"
    return unpack(raw, sizes, F, NP, sums)


def unpack(raw, sizes, F, NP, sums=True):
    info, frames, pairs = HG.bundle_split_info(raw["info"][:sizes["info"]], F, NP)
    g = types.SimpleNamespace(mats=raw["mats"][:F * 64].view(np.float64).reshape(F, 8).copy(),
                              sums=raw["sums"][:sizes["sums"]].view(np.float64).reshape(NP, BM.SUMS).copy() if sums else None,
                              info={k: info[k] for k in info.dtype.names}, frames=frames, pairs={k: pairs[k] for k in pairs.dtype.names})
    g.raw = {k: raw[k][:v].copy() for k, v in sizes.items()}
    return g


def check(c, g, exact=True):
    """By the tolerance; status, rounds, accepted and every n_valid exactly where no decision of the model lies near a tie (the cases of
    BM.gpu_cases() all do: tests/test_bundle_cpu.py)."""
    m64, mld = BM.adjust(c, BM.F64), BM.adjust(c, BM.LD)
    WORST[0] = max(WORST[0], BM.compare(c, g, m64, mld))
    assert BM.decisions_clear(m64, mld) or not exact, "a case that was to be compared exactly has a decision near a tie"
    if BM.decisions_clear(m64, mld):
        BM.compare_exact(g, m64)
    return m64


def same_bytes(a, b, keys=("mats", "info", "sums")):
    for k in keys:
        assert np.array_equal(a.raw[k], b.raw[k]), k


# ------------------------------------------------------------------------------------------------ pass 0 alone
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", BM.COUNTS + (CH - 1, CH, CH + 1, 2 * CH + 1))
def test_slot_counts_around_the_workgroup_and_the_chunk(ctx, kind, n):
    """n slots in the first pair and n_iter = 0: d_pair_sums, n_valid exactly and rms of one pass; d_mats_out is the input's bits."""
    c = BM.count_case(kind, n)
    g = run(ctx, c)
    check(c, g)
    assert g.pairs["n_valid_first"].tolist() == [n, 8] and g.info["rounds"] == 0 and g.info["status"] == BM.MAX_ITER
    assert np.array_equal(g.mats.view(np.uint64), c.mats.view(np.uint64))
    bare = run(ctx, c, sums=False)
    same_bytes(g, bare, ("mats", "info"))


# ------------------------------------------------------------------------------------------------ the size of the system
@pytest.mark.parametrize("kind,n_free", BM.free_counts())
def test_unknowns_around_the_lds_cap_and_the_panel_width(ctx, kind, n_free):
    """Free-frame counts just below, at and just above kBundleLdsCap for both kinds: the one-workgroup solve and the blocked one, with N no
    multiple of the panel width (136 = 4 x 32 + 8, 132) and a multiple of it (192)."""
    c = BM.free_case(kind, n_free)
    g = run(ctx, c)
    check(c, g)
    assert g.info["accepted"] >= 1 and (g.frames[1:] == BM.ADJUSTED).all()


def test_256_frames(ctx):
    """N = 2040: a chain plus a handful of closing pairs, 8 matches per pair, two rounds."""
    c = BM.big_case()
    g = run(ctx, c)
    check(c, g)
    assert g.info["accepted"] == 2 and g.info["rms_last"] < g.info["rms_first"]


# ------------------------------------------------------------------------------------------------ full runs
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("huber", (0.0, 1.0))
def test_planted_frames_are_found(ctx, kind, huber):
    """Noisy planted frames: the device against the model; a second run, d_mats_out aliasing d_mats_in and d_pair_sums as NULL give the
    same bytes."""
    c = BM.planted_case(kind, sigma=0.3, huber=huber, n=70)
    g = run(ctx, c)
    check(c, g)
    assert BM.rms_over_pairs(c, g.mats) < BM.rms_over_pairs(c, c.mats) and g.info["accepted"] >= 1
    same_bytes(g, run(ctx, c))
    same_bytes(g, run(ctx, c, alias=True))
    same_bytes(g, run(ctx, c, sums=False), ("mats", "info"))


@pytest.mark.parametrize("kind", KINDS)
def test_repeated_pairs_and_a_reversed_pair(ctx, kind):
    """A pair listed twice counts twice; a pair given as (b, a) with its coordinates swapped gives the values of (a, b) within tolerance."""
    c = BM.planted_case(kind, sigma=0.3, seed=3)
    fwd = BM.case(kind, c.W, c.H, c.mats, (0,), list(map(tuple, c.pairs)) + [tuple(c.pairs[1])], np.concatenate([c.matches, c.matches[1:2]]))
    rev = BM.case(kind, c.W, c.H, c.mats, (0,), list(map(tuple, c.pairs)) + [tuple(c.pairs[1][::-1])],
                  np.concatenate([c.matches, c.matches[1:2][:, :, [2, 3, 0, 1]]]))
    gf, gr = run(ctx, fwd), run(ctx, rev)
    mf = check(fwd, gf)
    check(rev, gr)
    mld = BM.adjust(fwd, BM.LD)
    for f in range(c.F):
        base = BM.corner_displacement(kind, mf.mats[f], mld.mats[f], c.W, c.H) or BM.floors()["mats"]
        assert BM.corner_displacement(kind, gf.mats[f], gr.mats[f], c.W, c.H) <= 32 * base
    once = run(ctx, c)
    assert not np.array_equal(once.raw["mats"], gf.raw["mats"])


@pytest.mark.parametrize("kind", KINDS)
def test_fixed_unanchored_and_bad_frames(ctx, kind):
    """Six frames: 0 and 3 fixed, 5 tied to the rest by a pair without matches only (UNANCHORED), the input of 2 NaN (BAD_INPUT: its bits
    come back, its pairs have no valid slot, its neighbours are adjusted without it)."""
    c = BM.planted_case(kind, F=6, sigma=0.2, seed=4, fixed=(0, 3), extra=((0, 2), (1, 3), (1, 4)))
    c.counts[4] = 0                                              # the pair (4, 5)
    c.counts_arg = c.counts
    c.mats[2] = np.nan
    g = run(ctx, c)
    check(c, g)
    assert g.frames.tolist() == [BM.FIXED, BM.ADJUSTED, BM.BAD_INPUT, BM.FIXED, BM.ADJUSTED, BM.UNANCHORED]
    for f in (0, 2, 3, 5):
        assert np.array_equal(g.mats[f].view(np.uint64), c.mats[f].view(np.uint64)), f
    assert g.pairs["n_valid_first"][[1, 2, 4]].tolist() == [0, 0, 0] and g.info["accepted"] >= 1


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_to_adjust(ctx, kind):
    """n_points = 0, n_pairs = 0 and every count 0: n_valid 0, no accepted round, the input's bits."""
    c = BM.planted_case(kind, F=3, extra=())
    for d in (BM.case(kind, c.W, c.H, c.mats, (0,), c.pairs, np.zeros((2, 0, 4), np.float32)),
              BM.case(kind, c.W, c.H, c.mats, (0,), np.zeros((0, 2), np.int32), np.zeros((0, 5, 4), np.float32)),
              BM.case(kind, c.W, c.H, c.mats, (0,), c.pairs, c.matches, counts=[0, 0])):
        g = run(ctx, d)
        check(d, g)
        assert g.info["n_valid_first"] == 0 and g.info["accepted"] == 0 and g.info["rounds"] == 0 and np.isnan(g.info["rms_first"])
        assert np.array_equal(g.mats.view(np.uint64), c.mats.view(np.uint64)) and g.frames.tolist() == [BM.FIXED, BM.UNANCHORED, BM.UNANCHORED]


# ------------------------------------------------------------------------------------------------ garbage
@pytest.mark.parametrize("kind", KINDS)
def test_garbage_in_unused_slots_changes_no_byte(ctx, kind):
    """Slots masked out or beyond counts filled with NaN / Inf / 1e30 / other finite values: the bytes of the same call with zeros there.
    Slots with coordinates that are no positions and mask 1 are never valid."""
    c = BM.planted_case(kind, F=4, n=40, sigma=0.2, seed=6)
    c.counts = np.array([30] * len(c.pairs), np.int32)
    c.counts_arg = c.counts
    c.mask = np.ones(c.matches.shape[:2], np.uint8)
    c.mask[:, 5:9] = 0
    clean = c.matches.copy()
    clean[:, 5:9] = 0
    c.matches = clean
    ref = run(ctx, c, garbage=0.0)
    check(c, ref)
    for junk in (np.nan, np.inf, -np.inf, 1e30, 123.25):
        d = types.SimpleNamespace(**vars(c))
        d.matches = clean.copy()
        d.matches[:, 5:9] = junk
        same_bytes(ref, run(ctx, d, garbage=junk))
    d = types.SimpleNamespace(**vars(c))
    d.matches = clean.copy()
    d.mask = None
    d.matches[:, 5, 0], d.matches[:, 6, 1], d.matches[:, 7, 2], d.matches[:, 8, 3] = np.nan, np.inf, 1e30, -np.inf
    g = run(ctx, d)
    check(d, g)
    assert (g.pairs["n_valid_first"] == 26).all() and same_bytes(ref, g, ("mats",)) is None


# ------------------------------------------------------------------------------------------------ the demonstrations of the CPU file
def test_the_ring_closes(ctx):
    c = BM.ring_case()
    g = run(ctx, c)
    check(c, g)
    before, after = BM.rms_over_pairs(c, c.mats), BM.rms_over_pairs(c, g.mats)
    print(f"ring: rms over all 8 pairs {before:.4g} px chained, {after:.4g} px adjusted")
    assert after < before and g.info["status"] == BM.CONVERGED


@pytest.mark.parametrize("kind", KINDS)
def test_huber_resists_outliers(ctx, kind):
    res = {}
    for huber in (0.0, 1.0):
        c = BM.huber_case(huber, kind)
        g = run(ctx, c)
        check(c, g, exact=False)                                 # (affine without huber is linear: its last accepted round gains an ulp)
        res[huber] = BM.truth_error(c, g.mats)
    assert res[1.0] < res[0.0], res


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_that_need_a_device(ctx):
    c = BM.planted_case(1, F=3, extra=())
    scratch = HG.bundle_layout(1, 3, 2, c.n_points)
    d = ctx.alloc(65536 + scratch)
    try:
        d_m, d_in, d_o, d_i, d_s, d_x = d, d + 16384, d + 20480, d + 24576, d + 32768, d + 65536
        ctx.to_device(d_m, c.matches)
        ctx.to_device(d_in, c.mats)
        ba = ctx.bundle_adjust_frames_device

        def refused(*a, **k):
            assert GF.refusal_code(ba, *a, **k) == INVALID, (a, k)

        args = (1, c.W, c.H, 3, c.fixed, c.pairs, d_m, c.n_points, None)
        refused(*args, 0, d_o, d_i, d_x, scratch)                                      # NULL
        refused(*args, d_in, 0, d_i, d_x, scratch)
        refused(*args, d_in, d_o, 0, d_x, scratch)
        refused(*args, d_in, d_o, d_i, 0, scratch)
        refused(1, c.W, c.H, 3, c.fixed, c.pairs, 0, c.n_points, None, d_in, d_o, d_i, d_x, scratch)
        refused(*args, d_in + 4, d_o, d_i, d_x, scratch)                               # misaligned
        refused(*args, d_in, d_o + 4, d_i, d_x, scratch)
        refused(*args, d_in, d_o, d_i + 4, d_x, scratch)
        refused(*args, d_in, d_o, d_i, d_x + 8, scratch)
        refused(*args, d_in, d_o, d_i, d_x, scratch, d_pair_sums=d_s + 4)
        refused(1, c.W, c.H, 3, c.fixed, c.pairs, d_m + 8, c.n_points, None, d_in, d_o, d_i, d_x, scratch)
        refused(*args, d_in, d_o, d_i, d_x, scratch - 1)                               # the scratch
        refused(*args, d_in, d_o, d_i, d_x, scratch, n_iter=65)                        # the shape, with a context
        refused(1, c.W, c.H, 3, [0, 0, 0], c.pairs, d_m, c.n_points, None, d_in, d_o, d_i, d_x, scratch)
        ctx.to_device(d_o, np.full(8192, FILL, np.uint8))
        ba(1, c.W, c.H, 0, [], np.zeros((0, 2), np.int32), 0, 0, None, 0, 0, 0, 0, 0)  # n_frames == 0: HG_OK, nothing is written
        ctx.sync()
        assert (ctx.to_host(d_o, 8192) == FILL).all()
        ba(*args, d_in, d_o, d_i, d_x, scratch, n_iter=1, eps=0.0)                     # eps 0 is legal; the context still works
        ctx.sync()
        info = HG.bundle_split_info(ctx.to_host(d_i, HG.bundle_info_bytes(3, 2)), 3, 2)[0]
        assert info["status"] == BM.MAX_ITER and info["rounds"] == 1
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ the chain on the device
def test_the_chain_detect_match_fit_chain_adjust_invert_warp(ctx):
    """The project's chain fixture (hgtest/detect.py: three frames of 192 x 160 that look at one scene), with pairs AMONG its frames instead
    of frame-to-keyframe only: keypoints detected, the pairs (0, 1), (0, 2), (1, 2) matched and fitted (projective, refit) on the device,
    the pair matrices chained from frame 0 on the host, all three pairs adjusted with the matcher's lists, the matcher's counts and the fit's
    mask as they stand; the adjusted matrices go through hg_bundle_invert_matrix into hg_geometric_set_frames.  The rms over all pairs does
    not rise, and no frame's status is a failure."""
    from hgtest import align as AM
    from hgtest import detect as DM
    from hgtest import match as MM
    frames = AM.chain_models()[1]
    c = DM.CHAIN
    F, (w, h) = 3, c["frame"]
    pairs = np.array([(0, 1), (0, 2), (1, 2)], np.int32)
    NP = len(pairs)
    nq = HG.detect_layout(w, h, c["cell"], c["per_cell"])[2]
    scratch = HG.bundle_layout(BM.PROJECTIVE, F, NP, nq)
    sz = {"frames": frames.nbytes, "cnt": F * 4, "pts": F * nq * 8, "desc": F * nq * 32, "qpts": NP * nq * 8, "qdesc": NP * nq * 32, "tpts": NP * nq * 8,
          "tdesc": NP * nq * 32, "mcounts": NP * 4, "matches": NP * nq * 16, "pmats": NP * 64, "fcounts": NP * 4, "mask": NP * nq, "in": F * 64, "out": F * 64,
          "info": HG.bundle_info_bytes(F, NP), "scratch": scratch}
    b = {k: ctx.alloc(v) for k, v in sz.items()}
    try:
        ctx.to_device(b["frames"], frames)
        ctx.detect_describe_frames_device(b["frames"], w, h, F, 1, b["cnt"], d_points=b["pts"], d_desc=b["desc"], cell=c["cell"], per_cell=c["per_cell"],
                                          min_response=c["min_response"])
        ctx.sync()
        cnt = ctx.to_host(b["cnt"], F * 4).view(np.int32)
        pts, desc = ctx.to_host(b["pts"], F * nq * 8).reshape(F, nq * 8), ctx.to_host(b["desc"], F * nq * 32).reshape(F, nq * 32)
        for side, col in (("q", 0), ("t", 1)):                   # a pair is what the matcher calls a frame: its query is frame a, its train set frame b
            ctx.to_device(b[side + "pts"], np.ascontiguousarray(pts[pairs[:, col]]))
            ctx.to_device(b[side + "desc"], np.ascontiguousarray(desc[pairs[:, col]]))
        ctx.match_descriptors_frames_device(MM.BITS, 32, 32, b["qdesc"], nq, cnt[pairs[:, 0]], NP, b["tdesc"], nq, cnt[pairs[:, 1]], NP, b["mcounts"], ratio=0.8,
                                            d_query_pts=b["qpts"], d_train_pts=b["tpts"], d_matches=b["matches"])
        ctx.sync()
        mcounts = ctx.to_host(b["mcounts"], NP * 4).view(np.int32).copy()
        ctx.fit_matches_frames_device(BM.PROJECTIVE, b["matches"], nq, mcounts, NP, c["threshold"], c["n_hyp"], c["fit_seed"], b["pmats"], b["fcounts"], refit=True,
                                      d_mask=b["mask"])
        ctx.sync()
        pmats = ctx.to_host(b["pmats"], NP * 64).view(np.float64).reshape(NP, 8)
        assert np.isfinite(pmats).all() and (mcounts >= 16).all(), (mcounts, pmats)
        start = HG.bundle_chain_from_pairs(BM.PROJECTIVE, F, pairs, pmats, anchor=0)
        ctx.to_device(b["in"], start)
        ctx.bundle_adjust_frames_device(BM.PROJECTIVE, w, h, F, [1, 0, 0], pairs, b["matches"], nq, mcounts, b["in"], b["out"], b["info"], b["scratch"], scratch,
                                        d_mask=b["mask"], n_iter=10, eps=0.01)
        ctx.sync()
        got = ctx.to_host(b["out"], F * 64).view(np.float64).reshape(F, 8).copy()
        info, fstat, pinfo = HG.bundle_split_info(ctx.to_host(b["info"], sz["info"]), F, NP)
        matches = ctx.to_host(b["matches"], NP * nq * 16).view(np.float32).reshape(NP, nq, 4)
        mask = ctx.to_host(b["mask"], NP * nq).reshape(NP, nq)
        inv = np.stack([HG.bundle_invert_matrix(BM.PROJECTIVE, m) for m in got])
        geoms = [(0, 0, w, h)] * F
        ctx.geometric_set_frames(BM.PROJECTIVE, inv, geoms)     # canvas -> frame: what the inverse warps take
    finally:
        for p in b.values():
            ctx.free(p)
    case = BM.case(BM.PROJECTIVE, w, h, start, (0,), pairs, matches, counts=mcounts, mask=mask)
    before, after = BM.rms_over_pairs(case, start), BM.rms_over_pairs(case, got)
    print(f"chain fixture: rms over the 3 pairs {before:.4g} px chained, {after:.4g} px adjusted; status {int(info['status'])}, rounds {int(info['rounds'])}, "
          f"valid {pinfo['n_valid_last'].tolist()}, pair rms {np.round(pinfo['rms_first'], 3).tolist()} -> {np.round(pinfo['rms_last'], 3).tolist()}")
    assert after <= before and info["status"] in (BM.CONVERGED, BM.MAX_ITER) and info["accepted"] >= 1
    assert fstat.tolist() == [BM.FIXED, BM.ADJUSTED, BM.ADJUSTED]
    assert abs(float(info["rms_last"]) - after) <= 1e-9 * after and np.array_equal(got[0].view(np.uint64), start[0].view(np.uint64))
    check(case, types.SimpleNamespace(mats=got, sums=None, info={k: info[k] for k in info.dtype.names}, frames=fstat, pairs={k: pinfo[k] for k in pinfo.dtype.names}),
          exact=False)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_bundle_adjust_equals_the_ctypes_call(ctx, tmp_path):
    """tests/js/bundle_gpu.mjs: h.bundleAdjust, h.chainMatrices and h.invertMatrix of js/Homography.mjs on the real addon, for a noisy planted
    case of both kinds with lists of different lengths, a mask, two fixed frames and huber, must give the bits of the ctypes calls:
    matrices, status, rounds, accepted, both rms, the frames' states and every pair's record; the chained and the inverted matrices."""
    import base64
    import json
    enc = lambda a: base64.b64encode(np.ascontiguousarray(a).tobytes()).decode()
    cases, spec = {}, {}
    for name, kind in (("affine", BM.AFFINE), ("projective", BM.PROJECTIVE)):
        c = BM.planted_case(kind, F=5, n=40, sigma=0.3, seed=9, fixed=(0, 3), huber=2.0, extra=((0, 2), (4, 1)))
        c.counts = np.array([40, 33, 40, 1, 40, 17][:len(c.pairs)], np.int32)
        c.counts_arg = c.counts
        rng = np.random.default_rng(1)
        c.mask = (rng.random(c.matches.shape[:2]) < 0.9).astype(np.uint8)
        for p in range(len(c.pairs)):
            c.mask[p, c.counts[p]:] = 0
            c.matches[p, c.counts[p]:] = 0                        # (the class pads its lists with zeros)
        pm = np.stack([BM.from3x3(kind, np.linalg.inv(BM.to3x3(kind, c.truth[b])) @ BM.to3x3(kind, c.truth[a])) for a, b in c.pairs])
        cases[name] = (c, pm)
        spec[name] = {"transform": name, "width": c.W, "height": c.H, "fixed": [0, 3], "iterations": c.n_iter, "eps": c.eps, "lambda": c.lambda0, "huber": c.huber,
                      "matrices": enc(c.mats), "pairs": c.pairs.tolist(), "matches": [enc(c.matches[p, :c.counts[p]]) for p in range(len(c.pairs))],
                      "masks": [enc(c.mask[p, :c.counts[p]]) for p in range(len(c.pairs))], "pairMatrices": enc(pm), "anchor": 2}
    path = tmp_path / "bundle_case.json"
    path.write_text(json.dumps(spec))
    res = GF.run_node_case("bundle_gpu.mjs", str(path))
    for name, (c, pm) in cases.items():
        g = run(ctx, c)
        check(c, g, exact=False)
        js = res["cases"][name]
        assert base64.b64decode(js["matrices"]) == g.raw["mats"].tobytes(), name
        assert (js["status"], js["rounds"], js["accepted"]) == (int(g.info["status"]), int(g.info["rounds"]), int(g.info["accepted"])), name
        assert base64.b64decode(js["rms"]) == np.array([g.info["rms_first"], g.info["rms_last"]]).tobytes(), name
        assert js["frames"] == g.frames.tolist() and js["nValid"] == np.stack([g.pairs["n_valid_first"], g.pairs["n_valid_last"]], 1).tolist(), name
        assert base64.b64decode(js["pairRms"]) == np.stack([g.pairs["rms_first"], g.pairs["rms_last"]], 1).tobytes(), name
        assert base64.b64decode(js["chained"]) == HG.bundle_chain_from_pairs(c.kind, c.F, c.pairs, pm, anchor=2).tobytes(), name
        assert base64.b64decode(js["inverse"]) == np.stack([HG.bundle_invert_matrix(c.kind, m) for m in g.mats]).tobytes(), name
