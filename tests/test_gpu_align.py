"""hg_align_refine_frames_device on the GPU against the numpy model of tests/hgtest/align.py (written from the header's text).
tests/test_align_cpu.py pins the model, the host entry and -- on every case of this file -- the conditions under which n_valid, status and
updates are compared exactly.  Shapes are the smallest at which the kernels can go wrong: planes of 64 x 48 to 97 x 71 and three frames,
larger only where a sample count asks for it (counts around the workgroup's 256 lanes and around kAlignChunk, read from hg_align_dev.h).

The tolerance (the fit's recipe).  Metric: the largest displacement, in TO pixels, of the four corners of the sample rectangle between two
matrices.  Base: the float64 model against the model whose sums run in np.longdouble, on the same case; the device may lie 16 x that from
the float64 model (it differs from it in the order of the sums only); a base of 0 is replaced by the smallest non-zero base of the planted
cases.  d_sums and both rms: relative error against the longdouble value <= 16 x the record's base (the largest relative error of the
float64 model's entries).  Measured bases on the planted cases: sums 2.3e-15 .. 2.9e-12 (relative), matrices 1.2e-15 .. 1.2e-14 px; the
largest kernel / base ratio of the kernel text run on the host: 2.6; the largest device / base ratio over this file on an MI355X: 3.57
(EXPERIMENTS.md, "Aligning")."""
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
from hgtest import align as AM               # noqa: E402
from hgtest import detect as DM              # noqa: E402
from hgtest import fit as FM                 # noqa: E402
from hgtest import match as MM               # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import FILL, INVALID, POISON  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = (AM.AFFINE, AM.PROJECTIVE)
MODES = [(k, p) for k in KINDS for p in (0, 1)]
CH = AM.chunk()
TAIL = 256                                   # canary bytes behind every output
WORST = [0.0]


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()
    print(f"largest device / base ratio of this file: {WORST[0]:.3g}")


# ------------------------------------------------------------------------------------------------ run and check
def run(ctx, c, sums=True, alias=False):
    """Upload the planes (inside allocations full of POISON, c.slack bytes apart) and the matrices, fill every output with FILL (TAIL canary
    bytes behind each), call, sync, download.  sums=False: d_sums is NULL.  alias: d_mats_out is d_mats_in."""
    F = len(c.frm)
    fb, fs = AM.planes_bytes(c.frm, c.slack, POISON)
    tb, ts = AM.planes_bytes(c.to, c.slack, POISON)
    Hf, Wf = c.frm[0].shape[:2]
    Ht, Wt = c.to[0].shape[:2]
    sizes = {"mats": F * 64, "info": F * 48, "sums": F * 528}
    bufs = {k: ctx.alloc(v + TAIL) for k, v in sizes.items()}
    d_f, d_t, d_in = ctx.alloc(fb.size + 64), ctx.alloc(tb.size + 64), ctx.alloc(F * 64 + TAIL)
    try:
        ctx.to_device(d_f, np.concatenate([fb, np.full(64, POISON, np.uint8)]))
        ctx.to_device(d_t, np.concatenate([tb, np.full(64, POISON, np.uint8)]))
        ctx.to_device(d_in, np.concatenate([c.mats.view(np.uint8).ravel(), np.full(TAIL, FILL, np.uint8)]))
        for k, v in sizes.items():
            ctx.to_device(bufs[k], np.full(v + TAIL, FILL, np.uint8))
        ctx.align_refine_frames_device(c.kind, d_f, Wf, Hf, F, d_t, Wt, Ht, len(c.to), c.channels, c.rect, d_in, d_in if alias else bufs["mats"], bufs["info"],
                                       step=c.step, photometric=c.photometric, n_iter=c.n_iter, eps=c.eps, min_valid=c.min_valid,
                                       d_sums=bufs["sums"] if sums else 0, from_stride_bytes=fs, to_stride_bytes=ts)
        ctx.sync()
        raw = {k: ctx.to_host(bufs[k], v + TAIL) for k, v in sizes.items()}
        raw_in = ctx.to_host(d_in, F * 64 + TAIL)
    finally:
        for p in list(bufs.values()) + [d_f, d_t, d_in]:
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
    g = AM.unpack(raw["mats"][:F * 64], raw["info"][:F * 48], raw["sums"][:F * 528] if sums else None, F)
    g.raw = {k: raw[k][:v].copy() for k, v in sizes.items()}
    return g


def check(c, g, what):
    WORST[0] = max(WORST[0], AM.check(c, g, what))


# ------------------------------------------------------------------------------------------------ chunk and workgroup edges
@pytest.mark.parametrize("kind,photometric", MODES)
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 1))
def test_sample_counts_around_the_workgroup_and_the_chunk(ctx, kind, photometric, n):
    """n samples and n_iter = 0: d_sums, n_valid and rms of one pass."""
    c = AM.count_case(kind, photometric, n)
    g = run(ctx, c)
    check(c, g, ("count", kind, photometric, n))
    assert (g.info["n_valid_first"] == n).all() and (g.info["updates"] == 0).all()
    assert (g.info["status"] == (AM.MAX_ITER if n >= c.P else AM.TOO_FEW)).all()


# ------------------------------------------------------------------------------------------------ geometry of the grid
@pytest.mark.parametrize("kind,photometric", MODES)
@pytest.mark.parametrize("step", (1, 2, 3, 64))
def test_steps_of_the_grid(ctx, kind, photometric, step):
    c = AM.step_case(kind, photometric, step)
    check(c, run(ctx, c), ("step", kind, photometric, step))


@pytest.mark.parametrize("kind,photometric", MODES)
def test_a_rectangle_not_at_the_origin(ctx, kind, photometric):
    c = AM.offset_rect_case(kind, photometric)
    check(c, run(ctx, c), ("offset", kind, photometric))


@pytest.mark.parametrize("kind,photometric", MODES)
@pytest.mark.parametrize("row", (True, False))
def test_one_row_and_one_column_rectangles(ctx, kind, photometric, row):
    """Through the middle of the plane the line's own coordinate is exactly 0 after the normalisation: SINGULAR; with min_valid above the
    line's samples TOO_FEW -- exactly as in the model.  The input's bits come back."""
    c = AM.line_case(kind, photometric, row)
    g = run(ctx, c)
    check(c, g, ("line", kind, photometric, row))
    assert (g.info["status"] == AM.SINGULAR).all()
    c = AM.line_case(kind, photometric, row, 100)
    g = run(ctx, c)
    check(c, g, ("line, too few", kind, photometric, row))
    assert (g.info["status"] == AM.TOO_FEW).all() and np.isnan(g.info["rms_first"]).all()


# ------------------------------------------------------------------------------------------------ planes
@pytest.mark.parametrize("kind,photometric", MODES)
@pytest.mark.parametrize("args", ((1, 1, 0), (4, 1, 0), (4, 2, 0), (1, 3, 64), (4, 3, 64), (1, 1, 32, True), (4, 1, 0, True)))
def test_channels_to_sets_strides_and_a_smaller_to_plane(ctx, kind, photometric, args):
    c = AM.planes_case(kind, photometric, *args)
    g = run(ctx, c)
    check(c, g, ("planes", kind, photometric) + args)
    if len(args) == 4:
        assert ((0 < g.info["n_valid_first"]) & (g.info["n_valid_first"] < 93 * 67)).all()


# ------------------------------------------------------------------------------------------------ statuses in one call
@pytest.mark.parametrize("kind,photometric", MODES)
def test_five_statuses_in_one_call_and_a_stopped_frame_is_left_alone(ctx, kind, photometric):
    c = AM.status_case(kind, photometric)
    g = run(ctx, c)
    check(c, g, ("statuses", kind, photometric))
    assert g.info["status"].tolist() == [AM.CONVERGED, AM.MAX_ITER, AM.TOO_FEW, AM.BAD_INPUT, AM.SINGULAR]
    assert g.info["updates"].tolist()[:2] == [1, 2]
    assert np.array_equal(g.mats[3].view(np.uint64), c.mats[3].view(np.uint64)) and np.isnan(g.mats[3]).all()
    one = run(ctx, AM.alone(c, 0))                                # the early frame, alone: the later passes must not have touched it
    assert one.raw["mats"].tobytes() == g.raw["mats"][:64].tobytes()
    assert one.raw["info"].tobytes() == g.raw["info"][:48].tobytes()
    assert one.raw["sums"].tobytes() == g.raw["sums"][:528].tobytes()


# ------------------------------------------------------------------------------------------------ iteration
@pytest.mark.parametrize("kind,photometric", MODES)
@pytest.mark.parametrize("px", (1.0, 2.0))
def test_planted_transforms_are_found(ctx, kind, photometric, px):
    """FROM resampled from TO on the CPU through a known matrix, started px pixels off: the device against the model by the tolerance, which
    also bounds it against the truth; d_mats_out aliasing d_mats_in, d_sums as NULL and a second run give the same bytes."""
    c = AM.planted_case(kind, photometric, px)
    g = run(ctx, c)
    check(c, g, ("planted", kind, photometric, px))
    w = AM.refine(c)
    for f in range(3):
        before = AM.corner_displacement(kind, c.mats[f], AM.TRUE[kind], c.rect)
        model = AM.corner_displacement(kind, w[f].mat, AM.TRUE[kind], c.rect)
        after = AM.corner_displacement(kind, g.mats[f], AM.TRUE[kind], c.rect)
        assert before > 0.9 * px and after < before / 4 and abs(after - model) < 1e-9, (f, before, model, after)
    again = run(ctx, c)
    for k in g.raw:
        assert np.array_equal(g.raw[k], again.raw[k]), (k, "two runs of one call")
    aliased = run(ctx, c, alias=True)
    bare = run(ctx, c, sums=False)
    for k in ("mats", "info"):
        assert np.array_equal(g.raw[k], aliased.raw[k]), (k, "d_mats_out == d_mats_in")
        assert np.array_equal(g.raw[k], bare.raw[k]), (k, "d_sums == NULL")
    assert np.array_equal(g.raw["sums"], aliased.raw["sums"])


# ------------------------------------------------------------------------------------------------ the chain on the device
def test_the_chain_detect_match_fit_refine_stays_on_the_device(ctx):
    """DM.chain_case(CHAIN_SEED): both sides detected, the frames matched against the keyframe, projective transforms fitted (no refit) and
    refined (8 updates, step 2, photometric) without a matrix leaving device memory: the fit's d_mats is d_mats_in as it stands.  The
    refined matrices meet the bound of tests/test_align_cpu.py::test_the_chain_on_the_models_alone and are no worse than the fitted ones."""
    key, frames, truth, fitted = AM.chain_models()[:4]
    c = DM.CHAIN
    F, (w, h), (kw, kh) = 3, c["frame"], c["key"]
    nq, nt = HG.detect_layout(w, h, c["cell"], c["per_cell"])[2], HG.detect_layout(kw, kh, c["cell"], c["per_cell"])[2]
    sz = {"frames": frames.nbytes, "key": key.nbytes, "cq": F * 4, "ct": 4, "qpts": F * nq * 8, "tpts": nt * 8, "qdesc": F * nq * 32, "tdesc": nt * 32,
          "counts": F * 4, "matches": F * nq * 16, "mats": F * 64, "fcounts": F * 4, "out": F * 64, "info": F * 48}
    b = {k: ctx.alloc(v) for k, v in sz.items()}
    try:
        ctx.to_device(b["frames"], frames)
        ctx.to_device(b["key"], key)
        det = dict(cell=c["cell"], per_cell=c["per_cell"], min_response=c["min_response"])
        ctx.detect_describe_frames_device(b["frames"], w, h, F, 1, b["cq"], d_points=b["qpts"], d_desc=b["qdesc"], **det)
        ctx.detect_describe_frames_device(b["key"], kw, kh, 1, 1, b["ct"], d_points=b["tpts"], d_desc=b["tdesc"], **det)
        ctx.sync()
        cq, ct = ctx.to_host(b["cq"], F * 4).view(np.int32), ctx.to_host(b["ct"], 4).view(np.int32)
        ctx.match_descriptors_frames_device(MM.BITS, 32, 32, b["qdesc"], nq, cq, F, b["tdesc"], nt, ct, 1, b["counts"], ratio=0.8, d_query_pts=b["qpts"],
                                            d_train_pts=b["tpts"], d_matches=b["matches"])
        ctx.sync()
        counts = ctx.to_host(b["counts"], F * 4).view(np.int32)
        ctx.fit_matches_frames_device(FM.PROJECTIVE, b["matches"], nq, counts, F, c["threshold"], c["n_hyp"], c["fit_seed"], b["mats"], b["fcounts"], refit=False)
        ctx.align_refine_frames_device(AM.PROJECTIVE, b["frames"], w, h, F, b["key"], kw, kh, 1, 1, (0, 0, w, h), b["mats"], b["out"], b["info"], step=2,
                                       photometric=True, n_iter=8, eps=0.01)
        ctx.sync()
        got_fit = ctx.to_host(b["mats"], F * 64).view(np.float64).reshape(F, 8)
        got = ctx.to_host(b["out"], F * 64).view(np.float64).reshape(F, 8)
        info = ctx.to_host(b["info"], F * 48).view(AM.INFO)
    finally:
        for p in b.values():
            ctx.free(p)
    assert np.array_equal(got_fit.view(np.uint64), fitted.view(np.uint64)), "the device's fit is the model's, bit for bit"
    before, after = AM.chain_errors(got_fit), AM.chain_errors(got)
    print("chain on the device: corner errors before", before, "after", after, "status", info["status"].tolist(), "updates", info["updates"].tolist())
    for f in range(F):
        assert after[f] <= before[f] and after[f] < AM.CHAIN_BOUND, (f, before[f], after[f])
    assert (info["status"][1:] <= AM.MAX_ITER).all()


# ------------------------------------------------------------------------------------------------ the coarse-to-fine helper
def test_coarse_to_fine_from_six_pixels_off(ctx):
    """hgwarp.align_refine_coarse_to_fine with levels = 3 on a 192 x 160 frame against its 220 x 180 keyframe, started 6 px off, against the
    model's walk (pyramids by the trilinear model, matrices converted by the model's scale_matrix): level 0's records by the tolerance of
    this file, and the result within the chain's bound of the truth."""
    c, truth = AM.walk_case()
    mats, res, cases = AM.walk(c, 3)
    Hf, Wf = c.frm[0].shape
    Ht, Wt = c.to[0].shape
    d_f, d_t = ctx.alloc(c.frm[0].nbytes), ctx.alloc(c.to[0].nbytes)
    try:
        ctx.to_device(d_f, c.frm[0])
        ctx.to_device(d_t, c.to[0])
        got, info = HG.align_refine_coarse_to_fine(ctx, c.kind, d_f, Wf, Hf, 1, d_t, Wt, Ht, 1, 1, c.mats, 3, rect=c.rect, step=c.step, photometric=bool(c.photometric),
                                                   n_iter=c.n_iter, eps=c.eps)
    finally:
        ctx.free(d_f)
        ctx.free(d_t)
    before = AM.corner_displacement(c.kind, c.mats[0], truth, c.rect)
    after = AM.corner_displacement(c.kind, got[0], truth, c.rect)
    ld = AM.walk(c, 3, AM.LD)[0]
    base = AM.corner_displacement(c.kind, mats[0], ld[0], c.rect) or AM.mat_floor()
    dev = AM.corner_displacement(c.kind, got[0], mats[0], c.rect)
    print(f"coarse to fine: {before:.3g} px -> {after:.3g} px; base {base:.3g} px, device {dev:.3g} px")
    WORST[0] = max(WORST[0], dev / base)
    assert (int(info["status"][0]), int(info["updates"][0]), int(info["n_valid_first"][0]), int(info["n_valid_last"][0])) == \
        (res[0].status, res[0].updates, res[0].n_valid_first, res[0].n_valid_last)
    assert dev <= 16 * base, (dev, base)
    assert before > 5.0 and after < AM.CHAIN_BOUND, (before, after)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_that_need_a_device(ctx):
    c = AM.planted_case(1, 1, 1.0)
    Hf, Wf = c.frm[0].shape
    Ht, Wt = c.to[0].shape
    d = ctx.alloc(65536)
    try:
        d_f, d_t, d_m, d_o, d_i, d_s = d, d + 16384, d + 32768, d + 36864, d + 40960, d + 45056
        ctx.to_device(d_f, np.stack(c.frm))
        ctx.to_device(d_t, c.to[0])
        ctx.to_device(d_m, c.mats)
        al = ctx.align_refine_frames_device

        def refused(*a, **k):
            assert GF.refusal_code(al, *a, **k) == INVALID, (a, k)

        rect = c.rect
        refused(1, 0, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i)               # NULL
        refused(1, d_f, Wf, Hf, 3, 0, Wt, Ht, 1, 1, rect, d_m, d_o, d_i)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, 0, d_o, d_i)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, 0, d_i)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, 0)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m + 4, d_o, d_i)         # misaligned
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o + 4, d_i)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i + 4)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i, d_sums=d_s + 4)
        refused(2, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i)             # the shape, with a context
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 3, rect, d_m, d_o, d_i)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, (0, 0, Wf + 1, Hf), d_m, d_o, d_i)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i, step=0)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i, n_iter=65)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i, eps=float("nan"))
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i, min_valid=9)
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 4, 1, rect, d_m, d_o, d_i)             # n_to_sets > n_frames
        refused(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i, from_stride_bytes=Wf * Hf - 1)
        ctx.to_device(d_o, np.full(65536 - 36864, FILL, np.uint8))
        al(1, 0, Wf, Hf, 0, 0, Wt, Ht, 1, 1, rect, 0, 0, 0)                            # n_frames == 0: HG_OK, nothing is written
        ctx.sync()
        assert (ctx.to_host(d_o, 65536 - 36864) == FILL).all()
        al(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, rect, d_m, d_o, d_i, n_iter=1, eps=0.0)                                # eps 0 is legal; the context still works
        ctx.sync()
        assert (ctx.to_host(d_i, 144).view(AM.INFO)["status"] == AM.MAX_ITER).all()
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def test_state_is_untouched_and_a_staged_set_warps_the_same_bytes():
    W, H, F = 64, 40, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((0.6, 0.45), (7.0, 3.0))
    c = AM.planted_case(1, 1, 1.0)
    w = AM.refine(c)
    Hf, Wf = c.frm[0].shape
    Ht, Wt = c.to[0].shape
    with HG.Context(0) as cx:
        d_src, d_w, d_f, d_t, d_o = cx.alloc(img.nbytes), cx.alloc(total), cx.alloc(3 * Wf * Hf), cx.alloc(Wt * Ht), cx.alloc(4096)
        try:
            cx.set_sampling(HG.SAMPLE_BILINEAR)
            cx.to_device(d_src, img)
            cx.to_device(d_f, np.stack(c.frm))
            cx.to_device(d_t, c.to[0])
            cx.to_device(d_o, c.mats)
            cx.set_image_device(d_src, W, H)
            cx.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, offs)
            cx.to_device(d_w, np.zeros(total, np.uint8))                      # (the padding between the frames is nobody's: zero both times)
            cx.warp_inverse_geometric_frames_device(d_w)
            cx.sync()
            alone = cx.to_host(d_w, total)
            before = GF.tap_state(cx)
            cx.to_device(d_w, np.zeros(total, np.uint8))
            cx.align_refine_frames_device(1, d_f, Wf, Hf, 3, d_t, Wt, Ht, 1, 1, c.rect, d_o, d_o + 1024, d_o + 2048, step=c.step, photometric=True,
                                          n_iter=c.n_iter, eps=c.eps)
            assert GF.tap_state(cx) == before
            cx.sync()
            assert GF.tap_state(cx) == before and cx.sampling == HG.SAMPLE_BILINEAR
            info = cx.to_host(d_o + 2048, 144).view(AM.INFO)
            assert info["status"].tolist() == [r.status for r in w] and info["updates"].tolist() == [r.updates for r in w]
            cx.warp_inverse_geometric_frames_device(d_w)                      # the staged set is still the warps'
            cx.sync()
            assert alone.any() and np.array_equal(cx.to_host(d_w, total), alone)
        finally:
            cx.set_image(img)
            for p in (d_src, d_w, d_f, d_t, d_o):
                cx.free(p)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_refine_alignment_equals_the_ctypes_call(ctx, tmp_path):
    """tests/js/align_gpu.mjs: h.refineAlignment of js/Homography.mjs on the real addon for the planted case of both kinds (RGBA planes,
    levels = 1) must give the bits of the ctypes call: matrices, status, updates, rms and gains."""
    cases = {name: AM.planted_case(kind, 1, 1.0, channels=4) for name, kind in (("affine", AM.AFFINE), ("projective", AM.PROJECTIVE))}
    spec = {}
    for name, c in cases.items():
        Hf, Wf = c.frm[0].shape[:2]
        Ht, Wt = c.to[0].shape[:2]
        spec[name] = {"width": Wf, "height": Hf, "toWidth": Wt, "toHeight": Ht, "rect": list(c.rect), "step": c.step, "iterations": c.n_iter, "eps": c.eps,
                      "from": [base64.b64encode(p.tobytes()).decode() for p in c.frm], "to": [base64.b64encode(p.tobytes()).decode() for p in c.to],
                      "matrices": base64.b64encode(c.mats.tobytes()).decode()}
    case = tmp_path / "align_case.json"
    case.write_text(json.dumps(spec))
    res = GF.run_node_case("align_gpu.mjs", str(case))
    for name, c in cases.items():
        g = run(ctx, c)
        check(c, g, ("js", name))
        js = res["cases"][name]
        assert base64.b64decode(js["matrices"]) == g.raw["mats"].tobytes(), name
        assert js["status"] == g.info["status"].tolist() and js["updates"] == g.info["updates"].tolist(), name
        assert base64.b64decode(js["rms"]) == g.info["rms_last"].tobytes() and base64.b64decode(js["gains"]) == np.stack([g.info["gain"], g.info["bias"]], 1).tobytes(), name
