"""hg_detect_describe_frames_device on the GPU against the numpy model of tests/hgtest/detect.py (written from the header's text).  Every
rule is integer arithmetic, so every comparison is exact, byte for byte, ties included; there is no tolerance in this file.  Every output
buffer is filled with FILL before the call and carries TAIL canary bytes; outputs that were not asked for, and the bytes 32..desc_stride of
the descriptor rows, must come back untouched.  tests/test_detect_cpu.py pins the model and runs the kernels' text on the host.  Shapes are
the smallest at which the kernels can go wrong: planes with one legal position or none, cells of one column, sizes that are no multiple of
a cell or of the kernel's sub-tile (T, read from hg_detect_dev.h), a cell larger than the sub-tile."""
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
from hgtest import detect as DM              # noqa: E402
from hgtest import fit as FM                 # noqa: E402
from hgtest import match as MM               # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import FILL, INVALID  # noqa: E402

pytestmark = pytest.mark.gpu
TAIL = 256                                   # canary bytes behind every output
T = DM.tile()


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def sizes(P, n_slots, stride):
    return (("counts", P * 4), ("points", P * n_slots * 8), ("desc", P * n_slots * stride), ("info", P * n_slots * 16))


def run(ctx, planes, channels, cell, per_cell, min_response=1, stride=32, slack=0, skip=()):
    """Upload the planes (`slack` bytes of 0xFF behind each), fill every output with FILL (TAIL canary bytes behind each), call, sync,
    download.  skip: optional outputs passed as NULL."""
    planes = np.asarray(planes)
    P, H, W = planes.shape[:3]
    n_slots = HG.detect_layout(W, H, cell, per_cell)[2]
    raw_in, plane_stride = DM.pack_planes(planes, slack)
    sz = dict(sizes(P, n_slots, stride))
    bufs = {k: ctx.alloc(v + TAIL) for k, v in sz.items()}
    d_in = ctx.alloc(len(raw_in))
    try:
        ctx.to_device(d_in, np.frombuffer(raw_in, np.uint8))
        for k, v in sz.items():
            ctx.to_device(bufs[k], np.full(v + TAIL, FILL, np.uint8))
        want = {k: (0 if k in skip else bufs[k]) for k in sz}
        ctx.detect_describe_frames_device(d_in, W, H, P, channels, want["counts"], cell=cell, per_cell=per_cell, min_response=min_response,
                                          desc_stride=stride, plane_stride_bytes=plane_stride, d_points=want["points"], d_desc=want["desc"],
                                          d_info=want["info"])
        ctx.sync()
        raw = {k: ctx.to_host(bufs[k], v + TAIL) for k, v in sz.items()}
    finally:
        for p in list(bufs.values()) + [d_in]:
            ctx.free(p)
    for k, v in sz.items():
        assert (raw[k][v:] == FILL).all(), (k, "the canary behind the buffer")
        if k in skip:
            assert (raw[k] == FILL).all(), (k, "an output that was not asked for")
    g = DM.unpack(np.concatenate([raw[k][:v] for k, v in sz.items()]).tobytes(), P, n_slots, stride)
    if "desc" not in skip:
        assert DM.filled(g.rest, FILL), "the bytes 32..desc_stride of a descriptor row"
    g.raw = {k: raw[k][:v] for k, v in sz.items()}
    return g


def both(ctx, planes, channels, cell, per_cell, what, min_response=1, **k):
    w = DM.model(planes, channels, cell, per_cell, min_response)
    DM.check(run(ctx, planes, channels, cell, per_cell, min_response, **k), w, what)
    return w


def content(seed, W, H, channels):
    p = DM.scene(seed, W, H, rects=max(8, W * H // 60), side=14)
    return DM.to_rgba(p, seed) if channels == 4 else p


# ------------------------------------------------------------------------------------------------ plane sizes
SIZES = ((33, 33), (32, 40), (40, 32), (34, 47), (64, 40), (65, 33), (97, 71))


@pytest.mark.parametrize("channels", (1, 4))
@pytest.mark.parametrize("size", SIZES)
def test_plane_sizes_cells_and_ranks(ctx, size, channels):
    """33 x 33: one legal position; 32 x 40 and 40 x 32: none; 65 x 33: a cell of one column; 97 x 71: no multiple of any cell or tile.  Two
    planes per call, a many-cornered scene and noise (noise fills the cells beyond per_cell, so the rank order is exercised)."""
    W, H = size
    noise = DM.noise(7 + W, W, H)
    planes = np.stack([content(W + H, W, H, channels), DM.to_rgba(noise, 3) if channels == 4 else noise])
    total = 0
    for cell in (8, 16, 32):
        for per_cell in (1, 2, 16):
            w = both(ctx, planes, channels, cell, per_cell, ("sizes", size, channels, cell, per_cell))
            total += int(w.counts.sum())
            legal = max(W - 32, 0) * max(H - 32, 0)
            assert (w.counts <= legal).all() and (legal > 0 or total == 0)
    if W >= 34 and H >= 40:
        assert total > 0, "the case must find keypoints"


@pytest.mark.parametrize("channels", (1, 4))
def test_a_cell_larger_than_the_sub_tile(ctx, channels):
    """130 x 66 with cell 64: the workgroup of a cell walks more than one sub-tile (T = 32) and merges their candidates into one running best;
    noise overflows per_cell in every sub-tile.  Also cell 256: one cell for the whole plane."""
    assert T < 64
    W, H = 130, 66
    noise = DM.noise(11, W, H)
    planes = np.stack([content(12, W, H, channels), DM.to_rgba(noise, 5) if channels == 4 else noise])
    for cell in (64, 256):
        for per_cell in (1, 2, 16):
            w = both(ctx, planes, channels, cell, per_cell, ("big cell", channels, cell, per_cell))
            # of the 3 x 2 cells of 64 only the first two columns of the first row reach the candidate zone; noise fills them to the brim
            assert w.counts[1] == per_cell * (2 if cell == 64 else 1)


# ------------------------------------------------------------------------------------------------ contents
def test_constant_checkerboard_and_margin(ctx):
    """A constant plane: nothing.  A checkerboard of 4 x 4 blocks of two values: R repeats with the period of the board, so every maximum is
    tied with its copies and, inside one neighbourhood, the lower flat index has to win.  Squares whose corner responses peak on the margin and
    one pixel outside it: 16 is legal, 15 is not."""
    w = both(ctx, DM.constant(97, 71)[None], 1, 16, 2, "constant")
    assert w.counts.tolist() == [0]
    for cell, per_cell in ((8, 16), (16, 2), (32, 1)):
        w = both(ctx, np.stack([DM.checker(97, 71), DM.checker(97, 71, 0, 255)]), 1, cell, per_cell, ("checker", cell, per_cell))
        assert (w.counts > 0).all()
        r = w.info["R"][0, :w.counts[0]]
        assert len(np.unique(r)) < len(r), "the board must tie responses"
    m = DM.margin_corners()
    w = both(ctx, np.stack([m, m.T.copy()]), 1, 16, 16, "margin")
    xs, ys = w.info["idx"][0, :w.counts[0]] % 80, w.info["idx"][0, :w.counts[0]] // 80
    assert (16, 16) in set(zip(xs.tolist(), ys.tolist())) and (63, 63) in set(zip(xs.tolist(), ys.tolist()))
    assert xs.min() == 16 and ys.min() == 16 and xs.max() == 63 and ys.max() == 63


def test_thresholds(ctx):
    """min_response at 1, at exactly the model's median R of the keypoints (the >=: the median keypoint stays), one above it, and above the
    maximum (no keypoints: padding everywhere)."""
    planes = np.stack([content(21, 97, 71, 1), DM.noise(22, 97, 71)])
    w = both(ctx, planes, 1, 16, 2, "threshold 1")
    r = np.concatenate([w.info["R"][p, :w.counts[p]] for p in range(2)])
    med, top = int(np.sort(r)[len(r) // 2]), int(r.max())
    at = both(ctx, planes, 1, 16, 2, "threshold at the median", min_response=med)
    above = both(ctx, planes, 1, 16, 2, "threshold above the median", min_response=med + 1)
    assert 0 < above.counts.sum() < at.counts.sum() < w.counts.sum()
    assert med in np.concatenate([at.info["R"][p, :at.counts[p]] for p in range(2)])
    none = both(ctx, planes, 1, 16, 2, "threshold above the maximum", min_response=top + 1)
    assert none.counts.tolist() == [0, 0] and (none.points == DM.PAD_WORD).all() and not none.desc.any()
    both(ctx, planes, 1, 16, 2, "the largest threshold", min_response=2 ** 63 - 1)


# ------------------------------------------------------------------------------------------------ strides and counts
@pytest.mark.parametrize("channels", (1, 4))
def test_strides_slack_and_plane_counts(ctx, channels):
    """desc_stride 32 and 48; plane_stride_bytes with slack (3 bytes: the planes of a 4-channel set then lie at odd addresses) filled with
    0xFF; 1, 3 and 5 planes with different contents in one call."""
    W, H = 97, 71
    kinds = [content(31, W, H, 1), DM.noise(32, W, H), DM.checker(W, H), content(33, W, H, 1), DM.constant(W, H)]
    for P in (1, 3, 5):
        planes = np.stack([DM.to_rgba(p, k) if channels == 4 else p for k, p in enumerate(kinds[:P])])
        for stride, slack in ((32, 0), (48, 3), (32, 64), (48, 0)):
            w = both(ctx, planes, channels, 16, 2, ("strides", channels, P, stride, slack), stride=stride, slack=slack)
        assert w.counts[0] > 0 and (P < 5 or w.counts[4] == 0)


def test_full_capacity_once(ctx):
    """n_slots exactly 65536: a 2048 x 2048 plane of noise under cell 8, per_cell 1 -- 65536 workgroups, a scan over 256 steps, and nearly
    every cell inside the margin holds a keypoint."""
    W = H = 2048
    assert HG.detect_layout(W, H, 8, 1) == (256, 256, 65536)
    w = both(ctx, DM.noise(41, W, H)[None], 1, 8, 1, "65536 slots")
    assert w.counts[0] > 55000


# ------------------------------------------------------------------------------------------------ outputs
def test_optional_outputs_as_null_and_two_runs(ctx):
    planes = np.stack([content(51, 97, 71, 4), DM.to_rgba(DM.noise(52, 97, 71), 1), DM.to_rgba(DM.checker(97, 71), 2)])
    w = DM.model(planes, 4, 16, 2, 1)
    full = run(ctx, planes, 4, 16, 2, stride=48)
    DM.check(full, w, "all outputs")
    again = run(ctx, planes, 4, 16, 2, stride=48)
    for k in full.raw:
        assert np.array_equal(full.raw[k], again.raw[k]), (k, "two runs of one call")
    names = ("points", "desc", "info")
    for mask in range(1, 8):
        skip = tuple(n for b, n in enumerate(names) if mask >> b & 1)
        g = run(ctx, planes, 4, 16, 2, stride=48, skip=skip)
        for k in full.raw:
            if k not in skip:
                assert np.array_equal(full.raw[k], g.raw[k]), (skip, k)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    W, H = 64, 40
    planes = content(61, W, H, 4)
    d = ctx.alloc(65536)
    try:
        d_p, d_c, d_pt, d_d, d_i = d, d + 16384, d + 20480, d + 24576, d + 32768
        ctx.to_device(d_p, planes)
        det = ctx.detect_describe_frames_device

        def refused(**k):
            a = dict(d_planes=d_p, w=W, h=H, n_planes=1, channels=4, d_counts=d_c)
            a.update(k)
            assert GF.refusal_code(det, **a) == INVALID, k

        for k in (dict(w=0), dict(w=32769), dict(h=0), dict(h=32769, w=8), dict(channels=3), dict(channels=0), dict(cell=7),
                  dict(cell=257), dict(per_cell=0), dict(per_cell=17), dict(w=2048, h=2048, cell=8, per_cell=2, channels=1), dict(n_planes=-1),
                  dict(n_planes=4097), dict(min_response=0), dict(min_response=-5), dict(desc_stride=40), dict(desc_stride=16), dict(desc_stride=0),
                  dict(plane_stride_bytes=W * H * 4 - 1), dict(d_planes=0), dict(d_counts=0), dict(d_counts=d_c + 2), dict(d_points=d_pt + 4),
                  dict(d_desc=d_d + 8), dict(d_info=d_i + 4)):
            refused(**k)
        ctx.to_device(d_c, np.full(4096, FILL, np.uint8))
        det(0, W, H, 0, 4, 0)                                       # n_planes == 0: HG_OK, nothing is written, no pointer is looked at
        ctx.sync()
        assert (ctx.to_host(d_c, 4096) == FILL).all()
        det(d_p, W, H, 1, 4, d_c, cell=8, per_cell=16, min_response=1)      # the context still works
        ctx.sync()
        assert ctx.to_host(d_c, 4).view(np.int32)[0] == DM.model(planes[None], 4, 8, 16, 1).counts[0]
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def test_state_is_untouched_and_a_staged_set_warps_the_same_bytes():
    W, H, F = 64, 40, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((0.6, 0.45), (7.0, 3.0))
    planes = np.stack([DM.noise(71, 97, 71), content(72, 97, 71, 1)])
    w = DM.model(planes, 1, 16, 2, 1)
    with HG.Context(0) as c:
        d_src, d_w, d_p, d_o = c.alloc(img.nbytes), c.alloc(total), c.alloc(planes.nbytes), c.alloc(65536)
        try:
            c.set_sampling(HG.SAMPLE_BILINEAR)
            c.to_device(d_src, img)
            c.to_device(d_p, planes)
            c.set_image_device(d_src, W, H)
            c.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, offs)
            c.to_device(d_w, np.zeros(total, np.uint8))               # (the padding between the frames is nobody's: zero both times)
            c.warp_inverse_geometric_frames_device(d_w)
            c.sync()
            alone = c.to_host(d_w, total)
            before = GF.tap_state(c)
            c.to_device(d_w, np.zeros(total, np.uint8))
            c.detect_describe_frames_device(d_p, 97, 71, 2, 1, d_o, cell=16, per_cell=2, min_response=1, d_desc=d_o + 1024)
            assert GF.tap_state(c) == before
            c.sync()
            assert GF.tap_state(c) == before and c.sampling == HG.SAMPLE_BILINEAR
            assert np.array_equal(c.to_host(d_o, 8).view(np.int32), w.counts)
            assert np.array_equal(c.to_host(d_o + 1024, 2 * w.n_slots * 32).reshape(2, w.n_slots, 32), w.desc)
            c.warp_inverse_geometric_frames_device(d_w)               # the staged set is still the warps'
            c.sync()
            assert alone.any() and np.array_equal(c.to_host(d_w, total), alone)
        finally:
            c.set_image(img)
            for p in (d_src, d_w, d_p, d_o):
                c.free(p)


# ------------------------------------------------------------------------------------------------ the chain
def chain_models():
    """The chain of the three numpy models on the pictures of DM.chain_case(4): detect both sides, match the frames (query) against the
    keyframe (train) at ratio 0.8, fit projective transforms without a refit."""
    key, frames, truth = DM.chain_case(DM.CHAIN_SEED)
    c = DM.CHAIN
    wk = DM.model(key[None], 1, c["cell"], c["per_cell"], c["min_response"])
    wf = DM.model(frames, 1, c["cell"], c["per_cell"], c["min_response"])
    wm = MM.match(MM.BITS, 32, wf.desc, wk.desc, counts_q=wf.counts, counts_t=wk.counts, ratio=0.8, qpts=wf.points.view(np.float32),
                  tpts=wk.points.view(np.float32))
    wt = FM.fit(FM.PROJECTIVE, wm.matches.view(np.float32), wm.counts, c["threshold"], c["n_hyp"], seed=c["fit_seed"], refit_on=False)
    return key, frames, truth, wk, wf, wm, wt


def test_pictures_through_detection_the_match_and_the_fit(ctx):
    """A seeded scene, a 220 x 180 keyframe crop, three 192 x 160 frames resampled from it (a shift, 20 degrees, 30 degrees with a mild
    perspective).  Both sides are detected on the device, the frames' lists go in as the query and the keyframe's as the one train set of
    hg_match_descriptors_frames_device (ratio 0.8), its d_matches into hg_fit_matches_frames_device (refit 0): the counts, the pairs, the
    mask and the minimal matrices equal the chain of the three numpy models bit for bit.  That the model's chain is a GOOD one (at least 30
    accepted matches per frame, 70 % of them within 1.5 px of the truth, the fitted corners within 2 px) is a statement about the inputs and
    is checked on the model alone, in tests/test_detect_cpu.py and here."""
    key, frames, truth, wk, wf, wm, wt = chain_models()
    DM.chain_is_good(frames, truth, wm, wt)
    c = DM.CHAIN
    F, (w, h), (kw, kh) = 3, c["frame"], c["key"]
    nq, nt = HG.detect_layout(w, h, c["cell"], c["per_cell"])[2], HG.detect_layout(kw, kh, c["cell"], c["per_cell"])[2]
    sz = {"frames": frames.nbytes, "key": key.nbytes, "cq": F * 4, "ct": 4, "qpts": F * nq * 8, "tpts": nt * 8, "qdesc": F * nq * 32, "tdesc": nt * 32,
          "counts": F * 4, "matches": F * nq * 16, "pairs": F * nq * 8, "mats": F * 64, "min": F * 64, "fcounts": F * 4, "best": F * 4, "mask": F * nq}
    b = {k: ctx.alloc(v) for k, v in sz.items()}
    try:
        ctx.to_device(b["frames"], frames)
        ctx.to_device(b["key"], key)
        det = dict(cell=c["cell"], per_cell=c["per_cell"], min_response=c["min_response"])
        ctx.detect_describe_frames_device(b["frames"], w, h, F, 1, b["cq"], d_points=b["qpts"], d_desc=b["qdesc"], **det)
        ctx.detect_describe_frames_device(b["key"], kw, kh, 1, 1, b["ct"], d_points=b["tpts"], d_desc=b["tdesc"], **det)
        ctx.sync()
        cq, ct = ctx.to_host(b["cq"], F * 4).view(np.int32), ctx.to_host(b["ct"], 4).view(np.int32)
        assert np.array_equal(cq, wf.counts) and np.array_equal(ct, wk.counts)
        ctx.match_descriptors_frames_device(MM.BITS, 32, 32, b["qdesc"], nq, cq, F, b["tdesc"], nt, ct, 1, b["counts"], ratio=0.8, d_query_pts=b["qpts"],
                                            d_train_pts=b["tpts"], d_matches=b["matches"], d_pairs=b["pairs"])
        ctx.sync()
        counts = ctx.to_host(b["counts"], F * 4).view(np.int32)
        assert np.array_equal(counts, wm.counts)
        ctx.fit_matches_frames_device(FM.PROJECTIVE, b["matches"], nq, counts, F, c["threshold"], c["n_hyp"], c["fit_seed"], b["mats"], b["fcounts"], refit=False,
                                      d_min_mats=b["min"], d_best=b["best"], d_mask=b["mask"])
        ctx.sync()
        assert np.array_equal(ctx.to_host(b["pairs"], F * nq * 8).view(np.int32).reshape(F, nq, 2), wm.pairs)
        assert np.array_equal(ctx.to_host(b["matches"], F * nq * 16).view(np.uint32).reshape(F, nq, 4), wm.matches)
        g = FM.unpack(np.concatenate([ctx.to_host(b[k], sz[k]) for k in ("mats", "min", "fcounts", "best", "mask")]), F, nq)
    finally:
        for p in b.values():
            ctx.free(p)
    FM.check(FM.PROJECTIVE, g, wt, wm.matches.view(np.float32), "chain")
    assert np.array_equal(g.raw["mats"], g.raw["min"])


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_detect_match_fit_equals_the_ctypes_calls(ctx, tmp_path):
    """tests/js/detect_gpu.mjs: h.detectAndDescribe -> h.matchDescriptors -> h.fitMatches of js/Homography.mjs on the real addon, on one pair
    (the keyframe and the rotated frame of the chain, as RGBA pictures), must give the words of the ctypes calls, which equal the models'."""
    key, frames, truth, _, _, _, _ = chain_models()
    c = DM.CHAIN
    (w, h), (kw, kh) = c["frame"], c["key"]
    rgba = lambda p: np.ascontiguousarray(np.stack([p, p, p, np.full_like(p, 255)], -1))         # grey RGBA: L = (256 p + 128) >> 8 = p
    frame, keyp = rgba(frames[1]), rgba(key)
    path = tmp_path / "detect_case.json"
    path.write_text(json.dumps({"frame": {"width": w, "height": h, "data": base64.b64encode(frame.tobytes()).decode()},
                                "key": {"width": kw, "height": kh, "data": base64.b64encode(keyp.tobytes()).decode()},
                                "cell": c["cell"], "perCell": c["per_cell"], "minResponse": c["min_response"], "threshold": c["threshold"],
                                "nHyp": c["n_hyp"], "seed": c["fit_seed"]}))
    res = GF.run_node_case("detect_gpu.mjs", str(path))
    gf, gk = run(ctx, frame[None], 4, c["cell"], c["per_cell"], c["min_response"]), run(ctx, keyp[None], 4, c["cell"], c["per_cell"], c["min_response"])
    wf, wk = DM.model(frames[1:2], 1, c["cell"], c["per_cell"], c["min_response"]), DM.model(key[None], 1, c["cell"], c["per_cell"], c["min_response"])
    DM.check(gf, wf, "js frame")
    DM.check(gk, wk, "js key")
    for name, g in (("frame", gf), ("key", gk)):
        n = int(g.counts[0])
        js = res[name]
        assert js["count"] == n and base64.b64decode(js["points"]) == g.points[0, :n].tobytes() and base64.b64decode(js["descriptors"]) == g.desc[0, :n].tobytes(), name
    wm = MM.match(MM.BITS, 32, gf.desc, gk.desc, counts_q=gf.counts, counts_t=gk.counts, ratio=0.8, qpts=gf.points.view(np.float32), tpts=gk.points.view(np.float32))
    n = int(wm.counts[0])
    assert res["match"]["count"] == n and base64.b64decode(res["match"]["pairs"]) == wm.pairs[0, :n].tobytes()
    assert base64.b64decode(res["match"]["matches"]) == wm.matches[0, :n].tobytes()
    wt = FM.fit(FM.PROJECTIVE, wm.matches[:, :n].view(np.float32), wm.counts, c["threshold"], c["n_hyp"], seed=c["fit_seed"], refit_on=False)
    assert res["fit"]["count"] == int(wt.counts[0]) and res["fit"]["best"] == int(wt.best[0])
    assert base64.b64decode(res["fit"]["minMatrix"]) == wt.min_mats[0].tobytes()
