"""The robust mosaic on the GPU (include/hgwarp.h, hg_mosaic_robust_device) against the numpy model of tests/hgtest/robust.py -- every
comparison byte for byte, canvas and weight plane, between guard bytes --, against hg_mosaic_frames_device where the two must agree, and
the drop-in class on the real addon against the ctypes pipeline.  tests/test_robust_cpu.py pins the model itself.  The library's sets are
those of tests/test_gpu_mosaic.py, made once there; sources are 48 x 40 or smaller, canvases 130 x 40 at most; every buffer is filled with
0xA5 before a call and the bytes outside its extent must keep it (GF.run_mosaic, driven through an adapter that sends its mosaic call to the
robust entry)."""
import base64
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
import test_gpu_mosaic as TM                 # noqa: E402  (its inputs; nothing of it is changed)
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import mosaic as MM              # noqa: E402
from hgtest import robust as RB              # noqa: E402
from hgtest.gpu_frames import CO, F32, FILL, INVALID, U8E      # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402

pytestmark = pytest.mark.gpu
SW, SH = TM.SW, TM.SH
PRO_GEOMS, PRO_CANVAS, PW_CANVAS = TM.PRO_GEOMS, TM.PRO_CANVAS, TM.PW_CANVAS
TRIMS = (0.0, 0.1, 0.25, 0.49)
RUNS = tuple((m, t) for m in RB.MODES for t in (TRIMS if m == RB.TRIMMED else (0.0,)))      # every mode, TRIMMED at every trim
LMAX = HG.ROBUST_LMAX


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


class _Robust:
    """A context whose mosaic_frames_device is the robust entry, so that GF.run_mosaic uploads, guards and checks for it."""
    def __init__(self, ctx, trim):
        self._ctx, self._trim = ctx, trim

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def mosaic_frames_device(self, geoms, d_f, d_p, elem, ch, w, h, mode, feather, canvas, d_c, d_w, foffs, poffs, gains=None):
        assert elem == U8E
        self._ctx.mosaic_robust_device(geoms, d_f, d_p, ch, mode, canvas, d_c, d_w, self._trim, foffs, poffs, gains)


def _run(ctx, geoms, fields, frames, ch, mode, trim, canvas, gains=None, **kw):
    """(canvas bytes, weights or None) of the robust mosaic; GF.run_mosaic checks the bytes outside the canvas and the weight plane."""
    return GF.run_mosaic(_Robust(ctx, trim), geoms, fields, frames, U8E, ch, SW, SH, mode, 1.0, canvas, gains, **kw)


def _check(ctx, geoms, fields, frames, ch, canvas, what, runs=RUNS, gains=None, **kw):
    for mode, trim in runs:
        want = RB.mosaic(geoms, fields, frames, ch, mode, trim, canvas, gains)
        GF.check_canvas(_run(ctx, geoms, fields, frames, ch, mode, trim, canvas, gains, **kw), want, (what, ch, mode, trim))


def _u8(name, ch):
    return TM._frames(name, U8E, ch)


def _holes(rng, n, share=0.12):
    """A caller-made field of n pixels: finite coordinates, `share` of them NaN."""
    co = (rng.random((n, 2)) * [SW, SH]).astype(F32)
    co[rng.random(n) < share] = np.nan
    return co


# ------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_every_mode_on_the_librarys_projective_and_piecewise_sets(ctx, channels):
    for name, canvas in (("projective", PRO_CANVAS), ("piecewise", PW_CANVAS)):
        geoms, fields, _ = TM._library_sets()[name]
        n = RB.mosaic(geoms, fields, _u8(name, channels), channels, RB.MIN, 0.0, canvas)[1]
        assert n.max() >= 3 and (n == 0).any()
        if name == "piecewise":                                   # NaN holes: n differs lane by lane inside a wave
            assert sum(int((~np.isfinite(f).all(-1)).sum()) for f in fields) > 50 and (np.diff(n, axis=1) != 0).sum() > 10
        _check(ctx, geoms, fields, _u8(name, channels), channels, canvas, name)


@pytest.mark.parametrize("width", (1, 63, 64, 65, 130))
def test_canvas_widths_and_heights_partly_and_wholly_beside_the_frames(ctx, width):
    geoms, fields, _ = TM._library_sets()["projective"]
    some = beside = False
    for k, height in enumerate((1, 3, 4, 5)):
        ch = 4 - k
        frames = _u8("projective", ch)
        for canvas in ((34 - width // 2, 12 + k, width, height), (110 - width // 2, -12, width, height), (400, 400, width, height)):
            n = RB.mosaic(geoms, fields, frames, ch, RB.MAX, 0.0, canvas)[1]
            assert canvas[0] < 400 or not n.any()                 # wholly beside every frame
            some, beside = some or bool(n.any()), beside or bool(n.any() and (n == 0).any())
            _check(ctx, geoms, fields, frames, ch, canvas, canvas, runs=((RB.MEDIAN, 0.0), (RB.TRIMMED, 0.25), (RB.MAX, 0.0)), weight=k % 2 == 0)
    assert some and (beside or width == 1)                        # frames were blended, and the wider canvases lay partly beside them


def test_explicit_offsets_with_frame_starts_at_odd_addresses(ctx):
    fields = TM._caller_fields(PRO_GEOMS)
    fo8 = [o + 8 * (2 * f + 1) + 512 * f for f, o in enumerate(RF.pack(PRO_GEOMS, 8)[0])]        # odd multiples of 8: no 16-byte alignment
    assert all(o % 8 == 0 and o % 16 != 0 for o in fo8)
    for ch in (1, 2, 3, 4):
        frames = _u8("projective", ch)
        po = [o + 640 * f + (2 * f + 1) for f, o in enumerate(RF.pack(PRO_GEOMS, ch)[0])]         # odd offsets: no 2- or 4-byte load fits
        assert all(o % 2 == 1 for o in po)
        _check(ctx, PRO_GEOMS, fields, frames, ch, PRO_CANVAS, "explicit offsets", runs=((RB.MEDIAN, 0.0), (RB.TRIMMED, 0.1)), foffs=fo8, poffs=po, front=258, cfront=1)
    frames = _u8("projective", 4)                                 # ... and where only SOME frames start aligned for the wide load, under an odd base
    po = [o + (f % 4) for f, o in enumerate(RF.pack(PRO_GEOMS, 4)[0])]
    _check(ctx, PRO_GEOMS, fields, frames, 4, PRO_CANVAS, "mixed alignment", runs=((RB.MIN, 0.0), (RB.TRIMMED, 0.49)), poffs=po, front=257, cfront=3)


# ------------------------------------------------------------------------------------------------ contributor counts and value patterns
def _pattern(rng, kind, shape):
    if kind == "equal":
        return np.full(shape, 93, np.uint8)
    if kind == "two":
        return rng.choice(np.array([17, 201], np.uint8), shape)
    if kind == "bits":                                            # every bit of the select decides somewhere: 0 / 255 at bit 7, 127 / 128 at every lower bit
        return rng.choice(np.array([0, 127, 128, 255], np.uint8), shape)
    return rng.integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("count", (1, 2, 3, 4, 5, 8))
def test_stacks_of_identical_windows_on_every_value_pattern(ctx, count):
    rng = np.random.default_rng(900 + count)
    geoms = [(3, -2, 70, 6)] * count                              # two tiles wide, two high
    fields = [_holes(rng, 420, 0.1 if count > 1 else 0.0) for _ in geoms]
    canvas = (1, -3, 74, 8)
    for k, kind in enumerate(("equal", "two", "random", "bits")):
        ch = 1 + (k + count) % 4
        frames = [_pattern(rng, kind, (420, ch)) for _ in geoms]
        n = RB.mosaic(geoms, fields, frames, ch, RB.MIN, 0.0, canvas)[1]
        assert n.max() == count and (n == 0).any()
        _check(ctx, geoms, fields, frames, ch, canvas, (count, kind))
        if kind == "equal":                                       # ... and every mode returns the value
            out = RB.mosaic(geoms, fields, frames, ch, RB.TRIMMED, 0.25, canvas)[0]
            assert (out[n > 0] == 93).all()


@pytest.mark.parametrize("count", (16, 17, 32, 33, LMAX - 1, LMAX, LMAX + 1))
def test_both_sides_of_the_staging_cap_over_one_tile(ctx, count):
    """`count` frames hit the canvas' first tile row: up to ROBUST_LMAX the kernel stages their contributors in LDS, one more and the tile
    walks global memory again in every round (16 / 17 and 32 / 33: where a launch allocates more slots).  The second tile row is hit by three frames only, so both paths run in one launch."""
    rng = np.random.default_rng(910 + count)
    geoms = [(int(rng.integers(-3, 4)), int(rng.integers(-2, 1)), 66, 4) for _ in range(count - 3)] + [(0, 0, 66, 8)] * 3
    hits = [sum(1 for x, y, w, h in geoms if x < 66 and x + w > 0 and y < Y0 + 4 and y + h > Y0) for Y0 in (0, 4)]
    assert hits == [count, 3], hits
    fields = [_holes(rng, RF.n_px(g), 0.08) for g in geoms]
    canvas = (0, 0, 66, 8)
    for ch, kind in ((4, "random"), (1, "bits"), (3, "two")):
        frames = [_pattern(rng, kind, (RF.n_px(g), ch)) for g in geoms]
        n = RB.mosaic(geoms, fields, frames, ch, RB.MIN, 0.0, canvas)[1]
        assert n.max() >= count - 8 and n[4:].max() == 3
        gains = rng.uniform(0.6, 1.6, count).astype(F32) if ch == 4 else None
        _check(ctx, geoms, fields, frames, ch, canvas, (count, kind), gains=gains)


def test_256_small_frames_over_one_canvas_and_257_refused(ctx):
    rng = np.random.default_rng(920)
    geoms = [(int(x), int(y), 8, 8) for x, y in zip(rng.integers(0, 9, 256), rng.integers(0, 9, 256))]
    fields = [_holes(rng, 64, 0.05) for _ in geoms]
    canvas = (0, 0, 16, 16)
    for ch, kind in ((3, "random"), (4, "bits"), (1, "random")):
        frames = [_pattern(rng, kind, (64, ch)) for _ in geoms]
        n = RB.mosaic(geoms, fields, frames, ch, RB.MIN, 0.0, canvas)[1]
        assert n.max() > 100 and n.min() < 10, (n.max(), n.min())
        _check(ctx, geoms, fields, frames, ch, canvas, ("256 frames", kind))
    full = [(0, 0, 16, 16)] * 256                                 # every pixel under all 256: the largest n and the largest sums
    frames = [np.full((256, 2), 255 if f % 2 else 254, np.uint8) for f in range(256)]
    flat = [np.zeros((256, 2), F32)] * 256
    _check(ctx, full, flat, frames, 2, canvas, "256 contributors")
    assert GF.refusal_code(ctx.mosaic_robust_device, full + [(0, 0, 1, 1)], 4096, 4096, 1, RB.MEDIAN, canvas, 4096) == INVALID
    assert b"hg_mosaic_robust_device" in HG.lib().hg_last_error(ctx._h) and b"256" in HG.lib().hg_last_error(ctx._h)


# ------------------------------------------------------------------------------------------------ against the mosaic itself, and properties
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_trimmed_at_zero_is_the_mean_mosaic_and_one_contributor_is_a_paste(ctx, channels):
    for name, canvas in (("projective", PRO_CANVAS), ("piecewise", PW_CANVAS)):
        geoms, fields, _ = TM._library_sets()[name]
        frames = _u8(name, channels)
        mean = TM._run(ctx, geoms, fields, frames, U8E, channels, MM.MEAN, 1.0, canvas)           # hg_mosaic_frames_device, on the device, here
        got = _run(ctx, geoms, fields, frames, channels, RB.TRIMMED, 0.0, canvas)
        assert mean[1].max() >= 3 and np.array_equal(got[0], mean[0]) and np.array_equal(got[1].view(np.uint32), mean[1].view(np.uint32)), (name, channels)
    rng = np.random.default_rng(930 + channels)                   # many contributors, the values that make halves: the f32 mean must round as the integers do
    geoms = [(0, 0, 64, 4)] * 31
    fields = [_holes(rng, 256, 0.2) for _ in geoms]
    frames = [_pattern(rng, "bits" if channels % 2 else "random", (256, channels)) for _ in geoms]
    mean = TM._run(ctx, geoms, fields, frames, U8E, channels, MM.MEAN, 1.0, (0, 0, 64, 4))
    got = _run(ctx, geoms, fields, frames, channels, RB.TRIMMED, 0.0, (0, 0, 64, 4))
    assert mean[1].max() > 20 and np.array_equal(got[0], mean[0]) and np.array_equal(got[1].view(np.uint32), mean[1].view(np.uint32))
    # one frame, and disjoint frames: HG_MOSAIC_LAST in every mode
    disjoint = [(0, 0, 9, 5), (9, 0, 4, 5), (2, 5, 6, 3), (-4, -3, 4, 3), (70, 1, 30, 4)]
    fields = [_holes(rng, RF.n_px(g), 0.1) for g in disjoint]
    frames = [_pattern(rng, "random", (RF.n_px(g), channels)) for g in disjoint]
    for gs, fs, ps, canvas in ((disjoint, fields, frames, (-5, -4, 110, 13)), (disjoint[:1], fields[:1], frames[:1], (-1, -1, 12, 7))):
        last = TM._run(ctx, gs, fs, ps, U8E, channels, MM.LAST, 1.0, canvas)
        assert last[1].max() == 1
        for mode, trim in RUNS:
            got = _run(ctx, gs, fs, ps, channels, mode, trim, canvas)
            assert np.array_equal(got[0], last[0]) and np.array_equal(got[1], last[1]), (len(gs), mode, trim)


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_gains_against_the_model_and_unit_gains_are_no_gains(ctx, channels):
    geoms, fields, _ = TM._library_sets()["projective"]
    rng = np.random.default_rng(940 + channels)
    frames = [rng.integers(60, 256, (RF.n_px(g), channels), dtype=np.uint8) for g in geoms]
    gains = rng.uniform(0.5, 2.0, len(geoms)).astype(F32)
    gains[0], gains[1] = 0.5, 2.0
    want = RB.mosaic(geoms, fields, frames, channels, RB.MAX, 0.0, PRO_CANVAS, gains)
    plain = RB.mosaic(geoms, fields, frames, channels, RB.MAX, 0.0, PRO_CANVAS)
    k = RB.stat_channels(channels)
    assert (want[0][..., :k][want[1] > 0] == 255).mean() > 0.2 and not np.array_equal(want[0], plain[0])      # bytes do saturate before they are ranked
    if channels == 4:
        assert np.array_equal(want[0][..., 3], plain[0][..., 3]) and want[0][..., 3].any()                   # alpha unscaled
    _check(ctx, geoms, fields, frames, channels, PRO_CANVAS, "gained", gains=gains)
    for mode, trim in ((RB.MEDIAN, 0.0), (RB.TRIMMED, 0.1)):
        none = _run(ctx, geoms, fields, frames, channels, mode, trim, PRO_CANVAS)
        unit = _run(ctx, geoms, fields, frames, channels, mode, trim, PRO_CANVAS, np.ones(len(geoms), F32))
        assert np.array_equal(none[0], unit[0]) and np.array_equal(none[1], unit[1])


def test_min_median_max_are_ordered_and_two_runs_give_the_same_bytes(ctx):
    geoms, fields, _ = TM._library_sets()["projective"]
    for ch in (3, 4):
        frames = _u8("projective", ch)
        got = {m: _run(ctx, geoms, fields, frames, ch, m, 0.25, PRO_CANVAS) for m in RB.MODES}
        lo, med, tri, hi = (got[m][0].astype(int) for m in (RB.MIN, RB.MEDIAN, RB.TRIMMED, RB.MAX))
        assert (lo <= med).all() and (med <= hi).all() and (lo <= tri).all() and (tri <= hi).all() and (lo < hi).any()
        for m in RB.MODES:
            again = _run(ctx, geoms, fields, frames, ch, m, 0.25, PRO_CANVAS)
            assert np.array_equal(again[0], got[m][0]) and np.array_equal(again[1], got[m][1])


# ------------------------------------------------------------------------------------------------ what it is for, out of real warps
def test_a_mover_drops_out_of_the_median_of_five_warped_frames_left_on_the_device():
    """Five pictures of one background, each with a 3 x 3 square of its own painted over it, go through the library's projective warp (one
    transform for all five, a frame set of five windows) and stay on the device with their coordinate fields in the default layouts; the
    robust mosaic of them is the warp of the BACKGROUND, byte for byte; the mean mosaic is not; MAX holds every square."""
    W, H, F = 48, 40, 5
    rng = np.random.default_rng(950)
    back = np.concatenate([rng.integers(30, 200, (H, W, 3), dtype=np.uint8), np.full((H, W, 1), 255, np.uint8)], -1)
    pics = [back.copy() for _ in range(F)]
    for f, p in enumerate(pics):
        p[6 + 5 * f:9 + 5 * f, 4 + 8 * f:7 + 8 * f, :3] = 255
    mat = [0.9, 0.05, 1.5, -0.04, 0.95, 2.0, 2e-4, -1e-4]
    g = (0, 0, 44, 36)
    geoms = [g] * F
    n = g[2] * g[3]
    fo, ftotal = HG.pack_field_offsets(geoms, CO)
    oo, ototal = HG.pack_offsets(geoms)
    with HG.Context(0) as c:
        d_f, d_o, d_c, d_w = c.alloc(ftotal), c.alloc(ototal), c.alloc(n * 4 + 512), c.alloc(n * 4 + 512)
        try:
            c.set_image(back)
            c.geometric_set_frames(1, np.tile(mat, F), geoms)
            c.warp_inverse_geometric_frames_device(d_o)           # five warps of the background: what the median must give
            c.field_inverse_geometric_frames_device(CO, d_f)
            c.sync()
            plain = c.to_host(d_o, ototal)[:n * 4].copy()
            for f, p in enumerate(pics):                          # ... then frame f from picture f: the library's own warp, left on the device
                c.set_image(p)
                c.geometric_set_frames(1, np.asarray(mat, np.float64), [g])
                c.warp_inverse_geometric_frames_device(d_o + oo[f])
            c.sync()
            fields = GF.split(c.to_host(d_f, ftotal), fo, geoms, 8, F32, 2)
            frames = GF.split(c.to_host(d_o, ototal), oo, geoms, 4, np.uint8, 4)
            cover = np.isfinite(fields[0]).all(-1)
            assert cover.mean() > 0.8 and all(not np.array_equal(fr, frames[0]) for fr in frames[1:])       # the squares are in the warps
            out = {}
            for key, mode, trim in (("median", RB.MEDIAN, 0.0), ("trimmed", RB.TRIMMED, 0.25), ("max", RB.MAX, 0.0)):
                c.to_device(d_c, np.full(n * 4 + 512, FILL, np.uint8))
                c.to_device(d_w, np.full(n * 4 + 512, FILL, np.uint8))
                c.mosaic_robust_device(geoms, d_f, d_o, 4, mode, g, d_c, d_w, trim)
                c.sync()
                raw, wr = c.to_host(d_c, n * 4 + 512), c.to_host(d_w, n * 4 + 512)
                assert (raw[n * 4:] == FILL).all() and (wr[n * 4:] == FILL).all()
                GF.check_canvas((raw[:n * 4], wr[:n * 4].view(F32)), RB.mosaic(geoms, fields, frames, 4, mode, trim, g), key)
                out[key] = raw[:n * 4].reshape(-1, 4)
            clean = np.where(cover[:, None], plain.reshape(-1, 4), 0)
            assert np.array_equal(out["median"], clean) and np.array_equal(out["trimmed"], clean)
            c.mosaic_frames_device(geoms, d_f, d_o, U8E, 4, W, H, MM.MEAN, 1.0, g, d_c, 0)
            c.sync()
            mean = c.to_host(d_c, n * 4).reshape(-1, 4)
            assert (mean.astype(int) - clean).max() > 10           # the ghosts of the mean
            lit = [(fr[:, :3] == 255).all(-1) & cover for fr in frames]
            assert all(m.sum() >= 4 for m in lit) and all((out["max"][m][:, :3] == 255).all() for m in lit)
        finally:
            for p_ in (d_f, d_o, d_c, d_w):
                c.free(p_)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_in_the_headers_order():
    g = [(0, 0, 8, 2), (4, 1, 4, 1)]
    cv = (0, 0, 8, 2)
    name = b"hg_mosaic_robust_device"
    with HG.Context(0) as c:
        d = c.alloc(16384)
        d_f, d_p, d_c, d_w = d, d + 4096, d + 8192, d + 12288
        co = (np.random.default_rng(2).random((20, 2)) * [7, 3]).astype(F32)
        px = np.arange(1, 21, dtype=np.uint8).reshape(20, 1)
        gains = np.array([1.5, 0.75], F32)
        c.to_device(d_f, GF.place([co[:16], co[16:]], [0, 256], 512, 0))
        c.to_device(d_p, GF.place([px[:16], px[16:]], [0, 256], 512, 0))
        want, ww = RB.mosaic(g, [co[:16], co[16:]], [px[:16], px[16:]], 1, RB.TRIMMED, 0.0, cv, gains)
        L, vp = HG.lib(), HG.C.c_void_p

        def still_works():
            c.to_device(d_c, np.full(512, FILL, np.uint8))
            c.to_device(d_w, np.full(512, FILL, np.uint8))
            c.mosaic_robust_device(g, d_f, d_p, 1, RB.TRIMMED, cv, d_c, d_w, 0.0, gains=gains)
            c.sync()
            raw, wr = c.to_host(d_c, 512), c.to_host(d_w, 512)
            assert np.array_equal(raw[:16], want.ravel()) and np.array_equal(wr[:64].view(F32), ww.ravel()) and (raw[16:] == FILL).all() and (wr[64:] == FILL).all()

        def refused(*a, **k):
            assert GF.refusal_code(c.mosaic_robust_device, *a, **k) == INVALID, (a, k)
            assert name in L.hg_last_error(c._h), L.hg_last_error(c._h)
            still_works()

        def raw_call(geoms, n, d_coords, d_frames, ch, mode, trim, gn, canvas, d_canvas, d_weight):
            return L.hg_mosaic_robust_device(c._h, geoms, n, vp(d_coords), None, vp(d_frames), None, ch, mode, trim, gn, HG.Geom(*canvas), vp(d_canvas), vp(d_weight))

        try:
            still_works()
            # (geoms, d_coords, d_frames, channels, mode, canvas, d_canvas, d_weight, trim, field_offsets, frame_offsets, gains)
            gg = HG._geoms(g)
            bad_gain = (HG.C.c_float * 2)(1.0, -1.0)
            # each refusal wins over everything the header lists behind it: the later faults are all present in the same call
            assert raw_call(gg, -1, d_f, d_p, 9, 9, 0.7, bad_gain, cv, 0, d_w + 2) == INVALID and b"n_frames" in L.hg_last_error(c._h)
            assert raw_call(gg, 65536, d_f, d_p, 9, 9, 0.7, bad_gain, cv, 0, d_w + 2) == INVALID and b"n_frames" in L.hg_last_error(c._h)
            assert raw_call(gg, 2, d_f, d_p, 9, 9, 0.7, bad_gain, cv, 0, d_w + 2) == INVALID and b"d_canvas" in L.hg_last_error(c._h)
            assert raw_call(gg, 2, 0, d_p, 9, 9, 0.7, bad_gain, cv, d_c, d_w + 2) == INVALID and b"channels" in L.hg_last_error(c._h)
            assert raw_call(gg, 2, 0, d_p, 1, 9, 0.7, bad_gain, cv, d_c, d_w + 2) == INVALID and b"NULL pointer" in L.hg_last_error(c._h)
            assert raw_call(gg, 2, d_f, d_p, 1, 9, 0.7, bad_gain, ((1 << 26) + 1, 0, 8, 2), d_c, d_w + 2) == INVALID and b"aligned" in L.hg_last_error(c._h)
            many = HG._geoms([(0, 0, 1, 1)] * 256 + [(0, 0, 1 << 16, (1 << 15) + 1)])
            assert raw_call(many, 257, d_f, d_p, 1, 9, 0.7, bad_gain, cv, d_c, d_w) == INVALID and b"0..256" not in L.hg_last_error(c._h)      # the hg_geom limits, before the count
            assert name in L.hg_last_error(c._h)
            many = HG._geoms([(0, 0, 1, 1)] * 257)
            assert raw_call(many, 257, d_f, d_p, 1, 9, 0.7, bad_gain, cv, d_c, d_w) == INVALID and b"0..256" in L.hg_last_error(c._h)
            assert raw_call(gg, 2, d_f, d_p, 1, 9, 0.7, bad_gain, cv, d_c, d_w) == INVALID and b"unknown mode" in L.hg_last_error(c._h)
            assert raw_call(gg, 2, d_f, d_p, 1, RB.TRIMMED, 0.7, bad_gain, cv, d_c, d_w) == INVALID and b"trim" in L.hg_last_error(c._h)
            assert raw_call(gg, 2, d_f, d_p, 1, RB.TRIMMED, 0.2, bad_gain, cv, d_c, d_w) == INVALID and b"gain" in L.hg_last_error(c._h)
            still_works()
            # ... and one by one through the binding
            for mode in (-1, 4):
                refused(g, d_f, d_p, 1, mode, cv, d_c, d_w)
            for ch in (0, 5):
                refused(g, d_f, d_p, ch, RB.MEDIAN, cv, d_c, d_w)
            for trim in (0.5, -0.01, float("nan"), float("inf")):
                refused(g, d_f, d_p, 1, RB.TRIMMED, cv, d_c, d_w, trim)
                c.mosaic_robust_device(g, d_f, d_p, 1, RB.MEDIAN, cv, d_c, d_w, trim)          # ... and ignored by the other modes
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                refused(g, d_f, d_p, 1, RB.MIN, cv, d_c, d_w, gains=[1.0, bad])
            refused(g, 0, d_p, 1, RB.MEDIAN, cv, d_c, d_w)                                    # NULL pointers
            refused(g, d_f, 0, 1, RB.MEDIAN, cv, d_c, d_w)
            refused(g, d_f, d_p, 1, RB.MEDIAN, cv, 0, d_w)
            refused(g, d_f, d_p, 1, RB.MEDIAN, (0, 0, 0, 0), 0, d_w)                          # d_canvas NULL even for an empty canvas
            refused(g, d_f + 4, d_p, 1, RB.MEDIAN, cv, d_c, d_w)                              # misaligned coordinates, weights, field offsets
            refused(g, d_f, d_p, 1, RB.MEDIAN, cv, d_c, d_w + 2)
            refused(g, d_f, d_p, 1, RB.MEDIAN, cv, d_c, d_w, 0.0, [0, 260])
            refused(g, d_f, d_p, 1, RB.MEDIAN, ((1 << 26) + 1, 0, 8, 2), d_c, d_w)            # beyond the hg_geom limits
            refused([g[0], (0, 0, 1 << 16, (1 << 15) + 1)], d_f, d_p, 1, RB.MEDIAN, cv, d_c, d_w)
            c.mosaic_robust_device(g, d_f, d_p + 1, 1, RB.MEDIAN, cv, d_c + 1, d_w)           # bytes may start anywhere
            c.sync()
        finally:
            c.free(d)


def test_no_frames_zero_the_canvas_and_an_empty_canvas_writes_nothing(ctx):
    for ch, (mode, trim) in zip((1, 2, 3, 4), ((RB.MEDIAN, 0.0), (RB.TRIMMED, 0.25), (RB.MIN, 0.0), (RB.MAX, 0.0))):
        canvas, weight = _run(ctx, [], [], [], ch, mode, trim, (5, -5, 67, 5))
        assert canvas.size == 67 * 5 * ch and not canvas.any() and not weight.view(np.uint8).any()
    geoms, fields, _ = TM._library_sets()["projective"]
    for canvas in ((0, 0, 0, 9), (0, 0, 9, -1)):
        got, weight = _run(ctx, geoms, fields, _u8("projective", 4), 4, RB.MEDIAN, 0.0, canvas)      # (_run checks that every byte kept FILL)
        assert got.size == 0 and weight.size == 0
    L, vp = HG.lib(), HG.C.c_void_p
    d = ctx.alloc(1024)
    try:
        ctx.to_device(d, np.full(1024, FILL, np.uint8))
        assert L.hg_mosaic_robust_device(ctx._h, None, 0, None, None, None, None, 4, RB.TRIMMED, 0.25, None, HG.Geom(0, 0, 8, 8), vp(d), None) == 0
        ctx.sync()
        raw = ctx.to_host(d, 1024)
        assert not raw[:256].any() and (raw[256:] == FILL).all()
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def test_state_is_untouched_by_a_robust_mosaic_of_warps_left_on_the_device():
    W, H, F = 64, 40, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((0.6, 0.45), (7.0, 3.0))
    x0, y0 = min(g[0] for g in gg), min(g[1] for g in gg)
    canvas = (x0 - 2, y0 - 1, max(g[0] + g[2] for g in gg) - x0 + 3, max(g[1] + g[3] for g in gg) - y0 + 3)
    assert canvas[2] <= 130 and canvas[3] <= 40, canvas
    n = canvas[2] * canvas[3]
    fo, ftotal = HG.pack_field_offsets(gg, CO)
    with HG.Context(0) as c:
        d_src, d_f, d_w, d_k, d_c, d_wt = c.alloc(img.nbytes), c.alloc(ftotal), c.alloc(total), c.alloc(total), c.alloc(n * 4), c.alloc(n * 4)
        try:
            c.set_sampling(HG.SAMPLE_BILINEAR)
            c.set_sampling(HG.SAMPLE_NEAREST)
            c.to_device(d_src, img)
            c.set_image_device(d_src, W, H)
            c.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, offs)
            c.warp_inverse_geometric_frames_device(d_w)
            c.field_inverse_geometric_frames_device(CO, d_f)
            c.sync()
            alone = c.to_host(d_w, total)
            fields = GF.split(c.to_host(d_f, ftotal), fo, gg, 8, F32, 2)
            frames = GF.split(alone, offs, gg, 4, np.uint8, 4)
            c.to_device(d_k, np.zeros(total, np.uint8))
            c.warp_inverse_geometric_frames_device(d_k)                   # queued ...
            mid = GF.tap_state(c)
            c.mosaic_robust_device(gg, d_f, d_w, 4, RB.MEDIAN, canvas, d_c, d_wt)      # ... in front of the robust mosaic of the first warp's frames
            assert GF.tap_state(c) == mid
            c.sync()
            assert GF.tap_state(c) == mid and c.sampling == HG.SAMPLE_NEAREST
            again = c.to_host(d_k, total)
            for f, g in enumerate(gg):
                assert np.array_equal(again[offs[f]:offs[f] + RF.n_px(g) * 4], alone[offs[f]:offs[f] + RF.n_px(g) * 4]), f
            assert np.array_equal(c.to_host(d_w, total), alone)           # the inputs are only read
            want, ww = RB.mosaic(gg, fields, frames, 4, RB.MEDIAN, 0.0, canvas)
            assert ww.max() == 3 and np.array_equal(c.to_host(d_c, n * 4), want.ravel()) and np.array_equal(c.to_host(d_wt, n * 4).view(F32), ww.ravel())
            c.warp_inverse_geometric_frames_device(d_k)                   # the staged frame set is still the warps'
            c.sync()
            assert np.array_equal(c.to_host(d_k, total), again)
        finally:
            c.set_image(img)
            for p in (d_src, d_f, d_w, d_k, d_c, d_wt):
                c.free(p)


def test_a_queued_redo_never_lands_on_a_later_robust_mosaic():
    """The construction of test_gpu_mosaic.py's test of this name: a piecewise warp whose rows carry 1100 spans is queued into buffer B (its
    frame is flagged, to be redone through the map at hg_sync); a robust mosaic then writes its canvas at the start of B and its weight
    plane further into B.  After hg_sync both hold the mosaic's."""
    s = GF.strip_mesh_overflow()
    img, W2, H2, g = s.img, s.W, s.H, s.g
    npx = g[2] * g[3]
    geoms, fields, warped = TM._library_sets()["projective"]
    canvas = PRO_CANVAS
    cpx = canvas[2] * canvas[3]
    w_at = (cpx * 4 + 4095) // 4096 * 4096
    assert w_at + cpx * 4 <= npx * 4 and g[2] * 4 * 2 < cpx * 4      # canvas and weights lie inside B, over several of the warp's rows
    want, ww = RB.mosaic(geoms, fields, warped, 4, RB.TRIMMED, 0.25, canvas)
    fo, ftotal = HG.pack_field_offsets(geoms, CO)
    po, ptotal = HG.pack_plane_offsets(geoms, 4)
    with HG.Context(0) as c:
        d_src, d_b, d_f, d_p = c.alloc(img.nbytes), c.alloc(npx * 4), c.alloc(ftotal), c.alloc(ptotal)
        try:
            c.to_device(d_src, img)
            c.to_device(d_f, GF.place(fields, fo, ftotal, 0))
            c.to_device(d_p, GF.place(warped, po, ptotal, 0))
            c.set_image_device(d_src, W2, H2)
            c.piecewise_set_mesh(s.sp, s.tris, *s.min_src)
            c.piecewise_set_frames(s.dp, [g], [0])
            r0 = c.redone_frames()
            c.warp_inverse_piecewise_frames_device(d_b)
            c.mosaic_robust_device(geoms, d_f, d_p, 4, RB.TRIMMED, canvas, d_b, d_b + w_at, 0.25)
            c.sync()
            assert c.redone_frames() > r0                      # the warp's frame WAS flagged and redone ...
            got = c.to_host(d_b, npx * 4)
            assert np.array_equal(got[:cpx * 4], want.ravel())   # ... and the mosaic stands, canvas and weights
            assert np.array_equal(got[w_at:w_at + cpx * 4].view(F32), ww.ravel())
        finally:
            c.set_image(img)
            for p in (d_src, d_b, d_f, d_p):
                c.free(p)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_robust_blends_match_the_ctypes_pipeline():
    """tests/js/robust_gpu.mjs: h.mosaic(sets, {blend: 'median' | 'trimmed' | 'min' | 'max'}) of js/Homography.mjs on the real addon for a
    projective and a piecewise stack; it prints its windows and the SHA-256 of every canvas and weight plane, and the same loop through
    ctypes -- stage the set, warp, export the coordinate fields, robust mosaic -- must hash alike."""
    res = GF.run_node_case("robust_gpu.mjs")
    W, H = res["W"], res["H"]
    img = GF.js_pattern_planes(W, H)[0]
    assert set(res["cases"]) == {"projective", "piecewise"}
    with HG.Context(0) as c:
        c.set_image(img)
        for name, case in res["cases"].items():
            geoms = [tuple(g) for g in case["geoms"]]
            canvas = tuple(case["canvas"])
            n = canvas[2] * canvas[3]
            assert len(geoms) == 4 and canvas[2] <= 130 and canvas[3] <= 40, (name, canvas)
            c.set_sampling(case["sampling"])
            if name == "piecewise":
                sp = np.frombuffer(base64.b64decode(case["src"]), F32)
                tris = np.frombuffer(base64.b64decode(case["tris"]), np.uint32)
                c.piecewise_set_mesh(sp, tris, *case["minSrc"])
                c.piecewise_set_frames(np.frombuffer(base64.b64decode(case["dst"]), F32), geoms)
            else:
                c.geometric_set_frames_points(1, np.frombuffer(base64.b64decode(case["from"]), F32), np.frombuffer(base64.b64decode(case["to"]), F32), geoms)
            fo, ftotal = HG.pack_field_offsets(geoms, CO)
            oo, ototal = HG.pack_offsets(geoms)
            d_f, d_o, d_c, d_w = c.alloc(ftotal), c.alloc(ototal), c.alloc(n * 4), c.alloc(n * 4)
            try:
                if name == "piecewise":
                    c.warp_inverse_piecewise_frames_device(d_o)
                    c.field_inverse_piecewise_frames_device(CO, d_f)
                else:
                    c.warp_inverse_geometric_frames_device(d_o)
                    c.field_inverse_geometric_frames_device(CO, d_f)
                c.sync()
                for key, (mode, trim, gains) in case["runs"].items():
                    c.mosaic_robust_device(geoms, d_f, d_o, 4, mode, canvas, d_c, d_w, trim, gains=gains)
                    c.sync()
                    got = c.to_host(d_c, n * 4)
                    assert got.any() and hashlib.sha256(got.tobytes()).hexdigest() == case["hashes"][key]["data"], (name, key)
                    assert hashlib.sha256(c.to_host(d_w, n * 4).tobytes()).hexdigest() == case["hashes"][key]["weight"], (name, key)
            finally:
                for p_ in (d_f, d_o, d_c, d_w):
                    c.free(p_)
