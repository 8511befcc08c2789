"""hg_match_descriptors_frames_device on the GPU against the numpy model of tests/hgtest/match.py (written from the header's text).  Every
output is an integer or a copied word, so every comparison is exact, byte for byte; there is no tolerance in this file.  Every output
buffer is filled with FILL before the call and carries TAIL canary bytes; outputs that were not asked for must come back untouched.
tests/test_match_cpu.py pins the model and runs the binary kernel's text on the host; the matrix-core kernel of HG_DESC_U8 is pinned here
alone.  Shapes are the smallest at which the kernels can go wrong: three frames, sizes around the kernels' query and train tiles (TQ, TT,
read from hg_match_dev.h), descriptor lengths around the word, the 16-byte chunk, the 64-byte k-step and the kernels' width classes."""
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
from hgtest import match as MM               # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import FILL, INVALID  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = (MM.BITS, MM.U8)
TQ, TT = MM.tiles()
TAIL = 256                                   # canary bytes behind every output
NO_CAP = MM.NO_CAP


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ run and check
def run(ctx, c, ratio=0.8, max_distance=NO_CAP, cross=False, skip=(), points=True):
    """Upload the case, fill every output with FILL (TAIL canary bytes behind each), call, sync, download.  skip: optional outputs passed as
    NULL; points=False: no point buffers (then d_matches is NULL too)."""
    F, nq = c.query.shape[:2]
    S, nt = c.train.shape[:2]
    if not points:
        skip = tuple(skip) + ("matches",)
    sizes = dict(MM.sizes(F, nq))
    bufs = {k: ctx.alloc(v + TAIL) for k, v in sizes.items()}
    ins = [np.ascontiguousarray(a) for a in (c.query, c.train, c.qpts, c.tpts)]
    d_in = [ctx.alloc(max(a.nbytes, 16)) for a in ins]
    try:
        for d, a in zip(d_in, ins):
            if a.size:
                ctx.to_device(d, a)
        for k, v in sizes.items():
            ctx.to_device(bufs[k], np.full(v + TAIL, FILL, np.uint8))
        want = {k: (0 if k in skip else bufs[k]) for k in sizes}
        ctx.match_descriptors_frames_device(c.kind, c.desc_bytes, c.stride, d_in[0], nq, c.counts_q, F, d_in[1], nt, c.counts_t, S, want["counts"],
                                            ratio=ratio, max_distance=max_distance, cross_check=cross, d_query_pts=d_in[2] if points else 0,
                                            d_train_pts=d_in[3] if points else 0, d_matches=want["matches"], d_pairs=want["pairs"], d_nn=want["nn"])
        ctx.sync()
        raw = {k: ctx.to_host(bufs[k], v + TAIL) for k, v in sizes.items()}
    finally:
        for p in list(bufs.values()) + d_in:
            ctx.free(p)
    for k, v in sizes.items():
        assert (raw[k][v:] == FILL).all(), (k, "the canary behind the buffer")
        if k in skip:
            assert (raw[k] == FILL).all(), (k, "an output that was not asked for")
    return MM.unpack(np.concatenate([raw[k][:v] for k, v in sizes.items()]), F, nq)


def both(ctx, c, what, ratio=0.8, max_distance=NO_CAP, cross=False):
    """The device against the model; with the cross-check, both of its forms: the default and the swapped launch (option "match_cross" 0)."""
    w = MM.model(c, ratio, max_distance, cross)
    MM.check(run(ctx, c, ratio, max_distance, cross), w, what)
    if cross:
        ctx.set_option("match_cross", 0)
        try:
            MM.check(run(ctx, c, ratio, max_distance, cross), w, (what, "swapped launch"))
        finally:
            ctx.set_option("match_cross", -1)
    return w


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_query", (0, 1, 15, 16, 17, TQ - 1, TQ, TQ + 1))
def test_row_counts_around_the_tiles(ctx, kind, n_query):
    """Every n_train of the list against this n_query (the two differ in all but at most one pairing, so a row / column swap cannot pass);
    the cross-check runs in both of its forms, and its swapped launch puts the train rows on the query tile, so both sizes meet both tiles."""
    nb = 32 if kind == MM.BITS else 128
    for n_train in (0, 1, 2, 15, 16, 17, TT - 1, TT, TT + 1, 2 * TT + 1):
        c = MM.near_case(1000 + 7 * n_query + n_train, kind, 3, n_query, n_train, nb)
        w = both(ctx, c, ("sizes", kind, n_query, n_train), ratio=0.9, cross=True)
        if n_query >= 15 and n_train >= 15:
            assert 0 < w.counts.sum() < 3 * n_query, "the case must accept some queries and reject others"


BYTES = {MM.BITS: (1, 3, 4, 31, 32, 33, 61, 64, 128, 512), MM.U8: (1, 63, 64, 65, 127, 128, 129, 512)}


@pytest.mark.parametrize("kind,desc_bytes", [(k, b) for k in KINDS for b in BYTES[k]])
def test_descriptor_lengths_and_strides(ctx, kind, desc_bytes):
    """stride = the next multiple of 16 and 32 above it; the padding is random and differs between the sides (and the model never reads it)."""
    base = (desc_bytes + 15) // 16 * 16
    for stride in (base, base + 32):
        c = MM.near_case(2000 + desc_bytes, kind, 3, 21, TT + 3, desc_bytes, stride=stride, S=2)
        if stride > desc_bytes:
            assert not np.array_equal(c.query[0, :, desc_bytes:], c.train[0, :21, desc_bytes:])
        both(ctx, c, ("bytes", kind, desc_bytes, stride), ratio=0.9, cross=True)


def test_u8_extremes_at_512_bytes(ctx):
    """All-0 against all-255 (d = 512 * 255^2 = 33 292 800), all-127 against all-128 (d = 512), 0 / 255 alternating in opposite phase: a wrong
    sign in the shift by 128 or a wrapped accumulator changes these."""
    alt = np.tile(np.array([0, 255], np.uint8), 256)
    rows = np.stack([np.zeros(512, np.uint8), np.full(512, 255, np.uint8), np.full(512, 127, np.uint8), np.full(512, 128, np.uint8), alt, alt[::-1]])
    c = MM.random_case(3, MM.U8, 3, 6, 6, 512)
    c.query[:], c.train[:] = rows, rows[[1, 0, 3, 2, 5, 4]]
    c.train[1] = rows[[5, 4, 1, 0, 3, 2]]
    w = both(ctx, c, "u8 extremes", ratio=0.0)
    assert w.D[0][0, 0] == 33292800 and w.D[0][2, 2] == 512 and w.D[0][4, 4] == 33292800 and w.D[0][0, 1] == 0
    c.counts_t = [1, 1, 1]                                        # one train row: every query's only distance is its d1
    w = both(ctx, c, "u8 extremes, one train row", ratio=0.5)
    assert w.nn[0, :, 1].tolist() == [33292800, 0, 512 * 128 * 128, 512 * 127 * 127, 256 * 255 * 255, 256 * 255 * 255] and (w.nn[..., 2] == -1).all()


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("kind", KINDS)
def test_ties(ctx, kind):
    nb = 32 if kind == MM.BITS else 128
    c = MM.near_case(31, kind, 3, TQ + 6, TT + 9, nb)
    c.query[0, 3, :nb] = c.train[0, TT + 2, :nb]                  # an identical pair: d1 = 0 ...
    c.train[0, 5] = c.train[0, TT + 2]                            # ... and a duplicate train row in an earlier tile: j1 = 5, d2 = d1
    c.query[1, TQ + 1] = c.query[1, 2]                            # duplicate queries (in two workgroups) under the cross-check
    c.train[1, 7, :nb] = c.query[1, 2, :nb]
    for ratio in (0.0, 0.8, 1.0):
        w = both(ctx, c, ("ties", kind, ratio), ratio=ratio, cross=True)
        assert w.nn[0, 3].tolist() == [5, 0, 0, 1 if ratio == 0 else 0]
        assert w.nn[1, 2, :2].tolist() == [7, 0] and w.nn[1, TQ + 1, :2].tolist() == [7, 0] and w.nn[1, TQ + 1, 3] == 0      # the lower i keeps the pair
    assert w.nn[1, 2, 3] == 1
    c.counts_t = [1, 1, 1]
    w = both(ctx, c, ("ct == 1", kind), ratio=0.5)
    assert (w.nn[:, :, 2] == -1).all() and w.counts.tolist() == [TQ + 6] * 3


# ------------------------------------------------------------------------------------------------ parameters
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cross", (False, True))
def test_ratio_cap_and_cross_check(ctx, kind, cross):
    c = MM.near_case(41, kind, 3, TQ + 6, TT + 9, 32 if kind == MM.BITS else 128)
    med = int(np.median(MM.model(c, 0.0).nn[:, :, 1]))
    seen = set()
    for ratio in (0.0, 0.5, 0.8, 1.0):
        for cap in (0, med, NO_CAP):
            seen.add(int(both(ctx, c, ("parameters", kind, ratio, cap, cross), ratio, cap, cross).counts.sum()))
    assert len(seen) >= 5, seen                                   # the parameters bite: they give different answers


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sets", (1, 2))
def test_partial_counts_and_train_sets(ctx, kind, sets):
    nb = 32 if kind == MM.BITS else 128
    for cq, ct in (([TQ + 6, 0, 33], [TT + 9, 9]), ([5, TQ, TQ + 1], [0, TT]), ([TQ + 6] * 3, [TT - 1, TT + 1])):
        c = MM.near_case(51 + sets, kind, 3, TQ + 6, TT + 9, nb, S=sets, counts_q=cq, counts_t=ct[:sets])
        both(ctx, c, ("counts", kind, sets, cq, ct), ratio=0.9, cross=True)


# ------------------------------------------------------------------------------------------------ outputs
@pytest.mark.parametrize("kind", KINDS)
def test_optional_outputs_as_null_two_runs_and_point_bits(ctx, kind):
    c = MM.near_case(61, kind, 3, TQ + 6, TT + 9, 32 if kind == MM.BITS else 128, S=2)
    words = c.qpts.view(np.uint32)
    words[0, 0], words[0, 1], words[1, 2] = (0x7fc00001, 0xffc12345), (0x7f800000, 0xff800000), (0x7f812345, 0x80000000)      # NaN payloads, Infs, -0
    c.tpts.view(np.uint32)[0, :4, 0] = (0x7fffffff, 0xff800001, 0x00000001, 0x80000000)
    w = MM.model(c, 0.0)
    full = run(ctx, c, 0.0)
    MM.check(full, w, "all outputs")
    assert (full.matches[0, :2, :2] == words[0, :2]).all()        # (ratio 0, no cap: every query is accepted, in order)
    again = run(ctx, c, 0.0)
    for k in full.raw:
        assert np.array_equal(full.raw[k], again.raw[k]), (k, "two runs of one call")
    for skip in ("matches", "pairs", "nn"):
        g = run(ctx, c, 0.0, skip=(skip,))
        for k in full.raw:
            if k != skip:
                assert np.array_equal(full.raw[k], g.raw[k]), (skip, k)
    g = run(ctx, c, 0.0, points=False)
    assert np.array_equal(g.raw["pairs"], full.raw["pairs"]) and np.array_equal(g.raw["nn"], full.raw["nn"])
    g = run(ctx, c, 0.0, skip=("matches", "pairs", "nn"))
    assert np.array_equal(g.counts, w.counts)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    c = MM.random_case(71, MM.BITS, 2, 8, 8, 32)
    d = ctx.alloc(16384)
    try:
        d_q, d_t, d_qp, d_tp, d_c, d_m, d_p, d_n = d, d + 1024, d + 2048, d + 3072, d + 4096, d + 5120, d + 8192, d + 10240
        ctx.to_device(d_q, c.query)
        ctx.to_device(d_t, c.train)
        match = ctx.match_descriptors_frames_device

        def refused(*a, **k):
            assert GF.refusal_code(match, *a, **k) == INVALID, (a, k)

        good = (0, 32, 32, d_q, 8, None, 2, d_t, 8, None, 2, d_c)
        arg = lambda **k: tuple(k.get(n, v) for n, v in zip("kind bytes stride q nq cq F t nt ct S counts".split(), good))
        refused(*arg(kind=2))
        refused(*arg(bytes=0))
        refused(*arg(bytes=513, stride=528))
        refused(*arg(stride=40))
        refused(*arg(stride=16))
        refused(*arg(nq=-1))
        refused(*arg(nq=65537))
        refused(*arg(nt=-1))
        refused(*arg(nt=65537))
        refused(*arg(F=-1))
        refused(*arg(F=4097))
        refused(*arg(S=0))
        refused(*arg(S=3))
        refused(*arg(cq=[8, 9]))
        refused(*arg(cq=[-1, 8]))
        refused(*arg(ct=[8, 9]))
        for ratio in (-0.5, 1.01, float("nan"), float("inf")):
            refused(*arg(), ratio=ratio)
        refused(*arg(q=0))                                        # NULL, misaligned
        refused(*arg(t=0))
        refused(*arg(counts=0))
        refused(*arg(q=d_q + 8))
        refused(*arg(t=d_t + 4))
        refused(*arg(counts=d_c + 2))
        refused(*arg(), d_pairs=d_p + 1)
        refused(*arg(), d_nn=d_n + 2)
        refused(*arg(), d_matches=d_m + 8, d_query_pts=d_qp, d_train_pts=d_tp)
        refused(*arg(), d_matches=d_m, d_query_pts=d_qp + 4, d_train_pts=d_tp)
        refused(*arg(), d_matches=d_m, d_query_pts=d_qp)          # d_matches without both point buffers
        refused(*arg(), d_matches=d_m, d_train_pts=d_tp)
        refused(*arg(), d_matches=d_m)
        ctx.to_device(d_c, np.full(4096, FILL, np.uint8))
        match(*arg(F=0, S=1, counts=0))                           # n_frames == 0: HG_OK, nothing is written
        ctx.sync()
        assert (ctx.to_host(d_c, 4096) == FILL).all()
        match(*arg(nq=0, q=0), d_pairs=d_p, d_nn=d_n)             # n_query == 0: the counts only, all zeros
        ctx.sync()
        got = ctx.to_host(d_c, 4096)
        assert (got[:8] == 0).all() and (got[8:] == FILL).all()
        match(*arg(), ratio=1.0, max_distance=0)                  # the limits of the parameters are legal; the context still works
        ctx.sync()
        w = MM.model(c, 1.0, 0)
        assert np.array_equal(ctx.to_host(d_c, 8).view(np.int32), w.counts)
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def test_state_is_untouched_and_a_staged_set_warps_the_same_bytes():
    W, H, F = 64, 40, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((0.6, 0.45), (7.0, 3.0))
    m = MM.near_case(81, MM.U8, F, 40, 50, 128, S=2)
    w = MM.model(m, 0.8, cross_check=True)
    with HG.Context(0) as c:
        d_src, d_w, d_q, d_t, d_o = c.alloc(img.nbytes), c.alloc(total), c.alloc(m.query.nbytes), c.alloc(m.train.nbytes), c.alloc(8192)
        try:
            c.set_sampling(HG.SAMPLE_BILINEAR)
            c.to_device(d_src, img)
            c.to_device(d_q, m.query)
            c.to_device(d_t, m.train)
            c.set_image_device(d_src, W, H)
            c.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, offs)
            c.to_device(d_w, np.zeros(total, np.uint8))               # (the padding between the frames is nobody's: zero both times)
            c.warp_inverse_geometric_frames_device(d_w)
            c.sync()
            alone = c.to_host(d_w, total)
            before = GF.tap_state(c)
            c.to_device(d_w, np.zeros(total, np.uint8))
            c.match_descriptors_frames_device(MM.U8, 128, 128, d_q, 40, None, F, d_t, 50, None, 2, d_o, cross_check=True, d_pairs=d_o + 1024)
            assert GF.tap_state(c) == before
            c.sync()
            assert GF.tap_state(c) == before and c.sampling == HG.SAMPLE_BILINEAR
            assert np.array_equal(c.to_host(d_o, F * 4).view(np.int32), w.counts)
            assert np.array_equal(c.to_host(d_o + 1024, F * 40 * 8).view(np.int32).reshape(F, 40, 2), w.pairs)
            c.warp_inverse_geometric_frames_device(d_w)               # the staged set is still the warps'
            c.sync()
            assert alone.any() and np.array_equal(c.to_host(d_w, total), alone)
        finally:
            c.set_image(img)
            for p in (d_src, d_w, d_q, d_t, d_o):
                c.free(p)


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("ratio", (0.8, 0.0))
def test_planted_scene_through_the_match_and_the_fit(ctx, ratio):
    """3 frames of 130 keypoints under known projective transforms, 256-bit descriptors, a true pair 10 % of its bits apart, 30 % of the
    train rows unrelated.  The device's d_matches goes straight into hg_fit_matches_frames_device with the downloaded counts; the fit's exact
    outputs (best index, count, mask, minimal matrix; refit off, so d_mats is exact too) equal hgtest.fit's model run on the MODEL's match
    list.  ratio 0.8 hands the fit clean matches; ratio 0 hands it every nearest neighbour, 39 of 130 wrong."""
    F, N, n_hyp, seed = 3, 130, 256, 3
    c, truth = MM.planted_scene()
    w = MM.model(c, 0.8)
    for f in range(F):                                            # the precondition, on the MODEL: 90 % of the unreplaced pairs at ratio 0.8
        good = truth[f] >= 0
        right = (w.nn[f, :, 3] == 1) & (w.nn[f, :, 0] == truth[f])
        assert good.sum() == 91 and (right & good).sum() >= 0.9 * good.sum(), (f, "choose another seed")
    w = MM.model(c, ratio)
    wf = FM.fit(FM.PROJECTIVE, w.matches.view(np.float32), w.counts, 1.0, n_hyp, seed=seed, refit_on=False)
    assert (wf.counts >= 80).all() and (ratio != 0.0 or ((w.counts == N).all() and (wf.counts < N).all()))
    sizes = {"counts": F * 4, "matches": F * N * 16, "mats": F * 64, "min": F * 64, "fcounts": F * 4, "best": F * 4, "mask": F * N}
    bufs = {k: ctx.alloc(v) for k, v in sizes.items()}
    ins = [c.query, c.train, c.qpts, c.tpts]
    d_in = [ctx.alloc(a.nbytes) for a in ins]
    try:
        for d, a in zip(d_in, ins):
            ctx.to_device(d, a)
        ctx.match_descriptors_frames_device(MM.BITS, 32, 32, d_in[0], N, None, F, d_in[1], N, None, F, bufs["counts"], ratio=ratio,
                                            d_query_pts=d_in[2], d_train_pts=d_in[3], d_matches=bufs["matches"])
        ctx.sync()
        counts = ctx.to_host(bufs["counts"], F * 4).view(np.int32)
        assert np.array_equal(counts, w.counts)
        ctx.fit_matches_frames_device(FM.PROJECTIVE, bufs["matches"], N, counts, F, 1.0, n_hyp, seed, bufs["mats"], bufs["fcounts"], refit=False,
                                      d_min_mats=bufs["min"], d_best=bufs["best"], d_mask=bufs["mask"])
        ctx.sync()
        assert np.array_equal(ctx.to_host(bufs["matches"], F * N * 16).view(np.uint32).reshape(F, N, 4), w.matches)
        g = FM.unpack(np.concatenate([ctx.to_host(bufs[k], sizes[k]) for k in ("mats", "min", "fcounts", "best", "mask")]), F, N)
    finally:
        for p in list(bufs.values()) + d_in:
            ctx.free(p)
    FM.check(FM.PROJECTIVE, g, wf, w.matches.view(np.float32), ("chain", ratio))
    assert np.array_equal(g.raw["mats"], g.raw["min"])


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_match_descriptors_equals_the_ctypes_call(ctx, tmp_path):
    """tests/js/match_gpu.mjs: h.matchDescriptors of js/Homography.mjs on the real addon, for both kinds, sets of different lengths (padding
    and counts), one train set for all frames, with the cross-check and points, must give the words of the ctypes call."""
    F, nq, nt, short = 3, 70, 67, 50
    case = {"F": F, "nq": nq, "nt": nt, "short": short, "ratio": 0.9}
    cs = {}
    for name, kind, nb in (("bits", MM.BITS, 32), ("u8", MM.U8, 128)):
        c = MM.near_case(91, kind, F, nq, nt, nb, S=1, counts_q=[nq, nq, short])
        cs[name] = c
        case[name] = {"bytes": nb, "query": base64.b64encode(c.query.tobytes()).decode(), "train": base64.b64encode(c.train.tobytes()).decode(),
                      "qpts": base64.b64encode(c.qpts.tobytes()).decode(), "tpts": base64.b64encode(c.tpts.tobytes()).decode()}
    path = tmp_path / "match_case.json"
    path.write_text(json.dumps(case))
    res = GF.run_node_case("match_gpu.mjs", str(path))
    for name, c in cs.items():
        g = run(ctx, c, 0.9, cross=True)
        MM.check(g, MM.model(c, 0.9, cross_check=True), ("js", name))
        js = res["cases"][name]
        assert js["counts"] == g.counts.tolist(), name
        for f in range(F):
            n = int(g.counts[f])
            assert base64.b64decode(js["pairs"][f]) == g.pairs[f, :n].tobytes(), (name, f)
            assert base64.b64decode(js["matches"][f]) == g.matches[f, :n].tobytes(), (name, f)
