"""The mosaic's exposure entries on the GPU (include/hgwarp.h: hg_mosaic_overlap_stats_device, hg_mosaic_frames_gain_device, and
hg_mosaic_solve_gains between them) against the numpy models of tests/hgtest/mosaic_gain.py -- every comparison exact: the statistics are
integers, the gained mosaic is compared bit for bit, canvas and weight plane --, and the drop-in class on the real addon against the ctypes
pipeline.  tests/test_mosaic_gain_cpu.py pins the models themselves.  The inputs are those of tests/test_gpu_mosaic.py, made once there:
canvases of 130 x 40 at most, frames of 48 x 32 at most, except the one case that needs 64-bit sums; every buffer is filled with 0xA5
before a call and the bytes outside its extent must keep it."""
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
import test_gpu_mosaic as TM                 # noqa: E402  (its inputs and its _run; nothing of it is changed)
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import mosaic as MM              # noqa: E402
from hgtest import mosaic_gain as MG         # noqa: E402
from hgtest.gpu_frames import CO, F32, F32E, FILL, INVALID, POISON, U8E      # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402

pytestmark = pytest.mark.gpu
INF = float("inf")
SW, SH = TM.SW, TM.SH
MODES = TM.MODES
PRO_GEOMS, PRO_CANVAS, PW_GEOMS, PW_CANVAS = TM.PRO_GEOMS, TM.PRO_CANVAS, TM.PW_GEOMS, TM.PW_CANVAS


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def _upload(ctx, geoms, fields, frames, px, foffs, poffs, front):
    fo = list(foffs) if foffs is not None else RF.pack(geoms, 8)[0]
    po = list(poffs) if poffs is not None else RF.pack(geoms, px)[0]
    f_total = max([o + RF.n_px(g) * 8 for o, g in zip(fo, geoms)] + [0]) + 256
    p_total = front + max([o + RF.n_px(g) * px for o, g in zip(po, geoms)] + [0]) + 256
    d_f, d_p = ctx.alloc(f_total), ctx.alloc(p_total)
    ctx.to_device(d_f, GF.place(fields, fo, f_total, 0x11))
    ctx.to_device(d_p, GF.place(frames, [front + o for o in po], p_total, POISON))
    return d_f, d_p


def _stats(ctx, geoms, fields, frames, ch, canvas, foffs=None, poffs=None, front=0, sfront=0):
    """Upload the fields and the frames as TM._run does, fill the statistics' allocation with FILL, run hg_mosaic_overlap_stats_device (its
    words start sfront bytes in, a multiple of 8), check that no byte outside them changed, and return the (F, F, 2) uint64 words."""
    F = len(geoms)
    n = F * F * 16
    d_f, d_p = _upload(ctx, geoms, fields, frames, ch, foffs, poffs, front)
    d_s = ctx.alloc(sfront + n + 512)
    try:
        ctx.to_device(d_s, np.full(sfront + n + 512, FILL, np.uint8))
        ctx.mosaic_overlap_stats_device(geoms, d_f, d_p + front, ch, canvas, d_s + sfront, foffs, poffs)
        ctx.sync()
        raw = ctx.to_host(d_s, sfront + n + 512)
    finally:
        for p in (d_f, d_p, d_s):
            ctx.free(p)
    assert (raw[:sfront] == FILL).all() and (raw[sfront + n:] == FILL).all(), "bytes outside the statistics must not be written"
    return raw[sfront:sfront + n].copy().view(np.uint64).reshape(F, F, 2)


def _run(ctx, geoms, fields, frames, elem, ch, mode, feather, canvas, gains, **kw):
    """TM._run with gains: (canvas bytes, weights or None); bytes outside the canvas and the weight plane must keep FILL."""
    return GF.run_mosaic(ctx, geoms, fields, frames, elem, ch, SW, SH, mode, feather, canvas, gains, **kw)


def _same_stats(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} words differ, first at (a, b, word) = {bad[0].tolist()}: got {int(got[tuple(bad[0])])}, want {int(want[tuple(bad[0])])}")


def _u8(name, ch):
    return TM._frames(name, U8E, ch)


# ------------------------------------------------------------------------------------------------ the statistics against the model
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_statistics_of_the_librarys_projective_and_piecewise_sets(ctx, channels):
    geoms, fields, _ = TM._library_sets()["projective"]
    frames = _u8("projective", channels)
    want = MG.overlap_stats(geoms, fields, frames, channels, PRO_CANVAS)
    N = want[..., 0]
    off = N[np.triu_indices(len(geoms), 1)]
    assert (off == 0).any() and (off > 0).any()                    # the premises, on the CPU, before anything is compared
    assert PRO_GEOMS[1] == PRO_GEOMS[5] and N[1, 5] > 0           # the two identical windows; the frame off the canvas and the empty one: zero rows
    assert not want[7].any() and not want[:, 7].any() and not want[4].any() and not want[:, 4].any()
    _same_stats(_stats(ctx, geoms, fields, frames, channels, PRO_CANVAS), want, ("projective", channels))
    twin = list(fields)                                           # ... and with one field behind both of them: N_ab = N_aa = N_bb, S_ab = S_aa
    twin[5] = fields[1]
    want = MG.overlap_stats(geoms, twin, frames, channels, PRO_CANVAS)
    assert want[1, 5, 0] == want[1, 1, 0] == want[5, 5, 0] == want[5, 1, 0] > 0 and want[1, 5, 1] == want[1, 1, 1] != want[5, 1, 1] == want[5, 5, 1]
    _same_stats(_stats(ctx, geoms, twin, frames, channels, PRO_CANVAS), want, ("projective, one field for the twins", channels))
    geoms, fields, _ = TM._library_sets()["piecewise"]
    frames = _u8("piecewise", channels)
    want = MG.overlap_stats(geoms, fields, frames, channels, PW_CANVAS)
    assert sum(int((~np.isfinite(f).all(-1)).sum()) for f in fields) > 50 and (want[..., 0] > 0).all()
    assert want[0, 1, 0] < min(want[0, 0, 0], want[1, 1, 0])
    _same_stats(_stats(ctx, geoms, fields, frames, channels, PW_CANVAS), want, ("piecewise", channels))


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_statistics_of_caller_made_fields_and_explicit_offsets(ctx, channels):
    fields = TM._caller_fields(PRO_GEOMS)
    f0 = fields[0]
    assert np.isnan(f0).any() and np.isinf(f0).any() and (np.abs(f0[np.isfinite(f0)]) >= 1e30).any()
    frames = _u8("projective", channels)
    want = MG.overlap_stats(PRO_GEOMS, fields, frames, channels, PRO_CANVAS)
    assert 0 < want[1, 5, 0] < want[1, 1, 0]                       # the identical windows now have holes of their own
    _same_stats(_stats(ctx, PRO_GEOMS, fields, frames, channels, PRO_CANVAS), want, ("caller-made", channels))
    fo8 = [o + 8 * (2 * f + 1) + 512 * f for f, o in enumerate(RF.pack(PRO_GEOMS, 8)[0])]        # odd multiples of 8: no 16-byte alignment
    po = [o + 640 * f + (2 * f + 1) for f, o in enumerate(RF.pack(PRO_GEOMS, channels)[0])]      # odd offsets: no 2- or 4-byte load fits
    assert all(o % 8 == 0 and o % 16 != 0 for o in fo8) and all(o % 2 == 1 for o in po)
    _same_stats(_stats(ctx, PRO_GEOMS, fields, frames, channels, PRO_CANVAS, foffs=fo8, poffs=po, front=258, sfront=8), want, ("explicit offsets", channels))
    po = [o + (f % 4) for f, o in enumerate(RF.pack(PRO_GEOMS, channels)[0])]                     # ... and where only SOME frames start aligned
    _same_stats(_stats(ctx, PRO_GEOMS, fields, frames, channels, PRO_CANVAS, poffs=po, front=257, sfront=24), want, ("mixed alignment", channels))


@pytest.mark.parametrize("canvas", ((3, 2, 1, 7), (-6, 4, 67, 5), (-10, 11, 130, 3), (29, 9, 2, 2), (400, 400, 5, 3)))
def test_statistics_on_the_small_canvas_shapes(ctx, canvas):
    geoms, fields, _ = TM._library_sets()["projective"]
    for ch in (4, 3, 2, 1):
        frames = _u8("projective", ch)
        want = MG.overlap_stats(geoms, fields, frames, ch, canvas)
        assert canvas[0] < 400 or not want.any()                 # wholly beside every frame
        _same_stats(_stats(ctx, geoms, fields, frames, ch, canvas), want, (canvas, ch))


def test_statistics_of_200_small_frames_thrown_over_the_canvas(ctx):
    """More frames meet one 64 x 4 tile than the block's table holds per side (64), in two tiles and with a partial last chunk, so that the
    pairs are walked chunk by chunk over a table that is zeroed and flushed in between; and many frames contribute to one pixel."""
    rng = np.random.default_rng(45)
    canvas = (-5, 3, 40, 24)
    geoms = [(int(x), int(y), 2, 2) for x, y in zip(rng.integers(-9, 37, 200), rng.integers(0, 29, 200))]
    for k in range(40, 115):                                      # 75 frames into the canvas' first tile row (Y 3..6) ...
        geoms[k] = (int(rng.integers(-6, 35)), int(rng.integers(2, 7)), 2, 2)
    for k in range(115, 185):                                     # ... and 70 into its fourth (Y 15..18)
        geoms[k] = (int(rng.integers(-6, 35)), int(rng.integers(14, 19)), 2, 2)
    for k in range(0, 200, 37):
        geoms[k] = (geoms[k][0], geoms[k][1], 0, 2)
    hot = [k for k in range(200) if k % 37][:16]                  # sixteen of them on one spot
    for k in hot:
        geoms[k] = (11 + k % 2, 9 + (k // 2) % 2, 2, 2)
    fields = [(rng.random((RF.n_px(g), 2)) * [SW + 2, SH + 2] - 1).astype(F32) for g in geoms]
    for co in fields[::5]:
        co[:1] = np.nan
    n = MM.mosaic(geoms, fields, [np.zeros((RF.n_px(g), 1), np.uint8) for g in geoms], SW, SH, MM.MEAN, 1.0, canvas)[1]
    assert n.max() >= 12 and (n == 0).any(), (n.max(), n.min())
    hits = [sum(1 for x, y, w, h in geoms if w > 0 and h > 0 and x < canvas[0] + canvas[2] and x + w > canvas[0] and y < min(Y0 + 4, canvas[1] + canvas[3]) and y + h > Y0)
            for Y0 in range(canvas[1], canvas[1] + canvas[3], 4)]     # frames whose window meets each tile (the canvas is one tile wide)
    assert len(hits) == 6 and sorted(hits)[-2] > 64 and max(hits) < 128 and min(hits) <= 64, hits      # two tiles beyond the table's side, chunks of 64 + a rest; others inside it
    for ch in (3, 4, 1):
        frames = [rng.integers(0, 256, (RF.n_px(g), ch), dtype=np.uint8) for g in geoms]
        want = MG.overlap_stats(geoms, fields, frames, ch, canvas)
        _same_stats(_stats(ctx, geoms, fields, frames, ch, canvas), want, ("200 frames", ch))


def test_sums_beyond_32_bits_accumulate_in_64(ctx):
    """Two frames with the same 2400 x 2400 window, both pointing at the SAME field and the SAME pixels, three channels of 255: every N is
    5 760 000 and every S is 5 760 000 x 765 = 4 406 400 000 > 2^32 -- expected from arithmetic, not from the model."""
    n = 2400 * 2400
    geoms = [(7, -3, 2400, 2400)] * 2
    d_f, d_p, d_s = ctx.alloc(n * 8), ctx.alloc(n * 3), ctx.alloc(64 + 512)
    try:
        ctx.to_device(d_f, np.zeros(n * 8, np.uint8))
        ctx.to_device(d_p, np.full(n * 3, 255, np.uint8))
        ctx.to_device(d_s, np.full(64 + 512, FILL, np.uint8))
        ctx.mosaic_overlap_stats_device(geoms, d_f, d_p, 3, geoms[0], d_s, [0, 0], [0, 0])
        ctx.sync()
        raw = ctx.to_host(d_s, 64 + 512)
    finally:
        for p in (d_f, d_p, d_s):
            ctx.free(p)
    assert n * 765 == 4406400000 > 2 ** 32
    assert raw[:64].view(np.uint64).tolist() == [n, n * 765] * 4 and (raw[64:] == FILL).all()


def test_statistics_of_no_frames_and_of_empty_canvases(ctx):
    geoms, fields, _ = TM._library_sets()["projective"]
    frames = _u8("projective", 4)
    for canvas in ((0, 0, 0, 9), (0, 0, 9, -1)):
        got = _stats(ctx, geoms, fields, frames, 4, canvas)       # the F * F pairs are zeroed, nothing else is written
        assert got.shape == (9, 9, 2) and not got.any()
    assert _stats(ctx, [], [], [], 3, (0, 0, 8, 8)).size == 0     # F = 0: no word is written (_stats checks the fill)
    L, vp = HG.lib(), HG.C.c_void_p
    assert L.hg_mosaic_overlap_stats_device(ctx._h, None, 0, None, None, None, None, 3, HG.Geom(0, 0, 8, 8), None) == 0


# ------------------------------------------------------------------------------------------------ the gained mosaic against the model
def _gains(n, seed):
    g = np.random.default_rng(seed).uniform(0.5, 2.0, n).astype(F32)
    g[0], g[-1] = 0.5, 2.0
    return g


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_gained_mosaic_equals_the_model(ctx, elem, channels):
    for name, canvas in (("projective", PRO_CANVAS), ("piecewise", PW_CANVAS)):
        geoms, fields, _ = TM._library_sets()[name]
        frames = TM._frames(name, elem, channels)
        gains = _gains(len(geoms), 60 + channels)
        for mode, feather in MODES:
            want = MG.mosaic_gain(geoms, fields, frames, SW, SH, mode, feather, canvas, gains)
            plain = MM.mosaic(geoms, fields, frames, SW, SH, mode, feather, canvas)
            assert not np.array_equal(want[0], plain[0]) and np.array_equal(want[1], plain[1])      # the weights do not change
            if channels == 4 and mode == MM.LAST:                 # alpha stays unscaled
                assert np.array_equal(np.ascontiguousarray(want[0][..., 3]).view(np.uint8), np.ascontiguousarray(plain[0][..., 3]).view(np.uint8)) and want[0][..., 3].any()
            GF.check_canvas(_run(ctx, geoms, fields, frames, elem, channels, mode, feather, canvas, gains, weight=name == "projective" or mode != MM.MEAN),
                      want, (name, elem, channels, mode, feather))


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_no_gains_and_unit_gains_are_the_plain_mosaic(ctx, elem, channels):
    geoms, fields, _ = TM._library_sets()["projective"]
    frames = TM._frames("projective", elem, channels)
    for mode, feather in MODES:
        plain = TM._run(ctx, geoms, fields, frames, elem, channels, mode, feather, PRO_CANVAS)
        want = MM.mosaic(geoms, fields, frames, SW, SH, mode, feather, PRO_CANVAS)
        GF.check_canvas(plain, want, "plain")
        for gains in (None, np.ones(len(geoms), F32)):
            got = _run(ctx, geoms, fields, frames, elem, channels, mode, feather, PRO_CANVAS, gains)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1].view(np.uint32), plain[1].view(np.uint32)), (elem, channels, mode, gains is None)
    L, vp = HG.lib(), HG.C.c_void_p                             # gains NULL through the C entry itself: it IS hg_mosaic_frames_device
    px = channels * GF.es(elem)
    n = PRO_CANVAS[2] * PRO_CANVAS[3]
    d_f, d_p = _upload(ctx, geoms, fields, frames, px, None, None, 0)
    d_c, d_w = ctx.alloc(n * px + 512), ctx.alloc(n * 4 + 512)
    try:
        for mode, feather in MODES[1:3]:
            ctx.to_device(d_c, np.full(n * px + 512, FILL, np.uint8))
            ctx.to_device(d_w, np.full(n * 4 + 512, FILL, np.uint8))
            assert L.hg_mosaic_frames_gain_device(ctx._h, HG._geoms(geoms), len(geoms), vp(d_f), None, vp(d_p), None, elem, channels, SW, SH, mode, feather,
                                                  HG.Geom(*PRO_CANVAS), vp(d_c), vp(d_w), None) == 0
            ctx.sync()
            raw, wraw = ctx.to_host(d_c, n * px + 512), ctx.to_host(d_w, n * 4 + 512)
            assert (raw[n * px:] == FILL).all() and (wraw[n * 4:] == FILL).all()
            GF.check_canvas((raw[:n * px], wraw[:n * 4].view(F32)), MM.mosaic(geoms, fields, frames, SW, SH, mode, feather, PRO_CANVAS), ("gains NULL", elem, channels, mode))
    finally:
        for p in (d_f, d_p, d_c, d_w):
            ctx.free(p)
    d = ctx.alloc(1024)
    try:
        ctx.to_device(d, np.full(1024, FILL, np.uint8))
        assert L.hg_mosaic_frames_gain_device(ctx._h, None, 0, None, None, None, None, U8E, 4, 1, 1, MM.LAST, 0.0, HG.Geom(0, 0, 8, 8), vp(d), None, None) == 0
        ctx.sync()
        raw = ctx.to_host(d, 1024)
        assert not raw[:256].any() and (raw[256:] == FILL).all()
    finally:
        ctx.free(d)


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_a_gain_that_takes_bytes_beyond_255_saturates(ctx, channels):
    fields = TM._caller_fields(PRO_GEOMS)
    rng = np.random.default_rng(70 + channels)
    frames = [rng.integers(100, 256, (RF.n_px(g), channels), dtype=np.uint8) for g in PRO_GEOMS]
    for fr in frames:
        fr[(fr == FILL) | (fr == POISON)] = 254
    gains = np.full(len(PRO_GEOMS), 2.0, F32)
    gains[1::2] = 1.75
    po = [o + (2 * f + 1) for f, o in enumerate(RF.pack(PRO_GEOMS, channels)[0])]
    for mode, feather in MODES:
        want = MG.mosaic_gain(PRO_GEOMS, fields, frames, SW, SH, mode, feather, PRO_CANVAS, gains)
        k = MG.stat_channels(channels)
        lit = want[1] > 0
        assert lit.any() and (want[0][..., :k][lit] == 255).mean() > 0.3 and (F32(1.75) * F32(200) > 255)      # g * p does exceed 255
        if channels == 4:
            assert (want[0][..., 3][lit] < 255).any()
        GF.check_canvas(_run(ctx, PRO_GEOMS, fields, frames, U8E, channels, mode, feather, PRO_CANVAS, gains, poffs=po, front=259, cfront=1), want, ("saturating", channels, mode))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    g = [(0, 0, 8, 2), (4, 1, 4, 1)]
    cv = (0, 0, 8, 2)
    with HG.Context(0) as c:
        d = c.alloc(20480)
        d_f, d_p, d_c, d_w, d_s = d, d + 4096, d + 8192, d + 12288, d + 16384
        co = (np.random.default_rng(2).random((20, 2)) * [7, 3]).astype(F32)
        px = np.arange(1, 21, dtype=np.uint8).reshape(20, 1)
        gains = np.array([1.5, 0.75], F32)
        c.to_device(d_f, GF.place([co[:16], co[16:]], [0, 256], 512, 0))
        c.to_device(d_p, GF.place([px[:16], px[16:]], [0, 256], 512, 0))
        want, ww = MG.mosaic_gain(g, [co[:16], co[16:]], [px[:16], px[16:]], 8, 4, MM.FEATHER, 2.0, cv, gains)
        wst = MG.overlap_stats(g, [co[:16], co[16:]], [px[:16], px[16:]], 1, cv)
        assert wst[0, 1, 0] == 4

        def still_works():
            for p in (d_c, d_w, d_s):
                c.to_device(p, np.full(512, FILL, np.uint8))
            c.mosaic_frames_device(g, d_f, d_p, U8E, 1, 8, 4, MM.FEATHER, 2.0, cv, d_c, d_w, gains=gains)
            c.mosaic_overlap_stats_device(g, d_f, d_p, 1, cv, d_s)
            c.sync()
            raw, wr, sr = c.to_host(d_c, 512), c.to_host(d_w, 512), c.to_host(d_s, 512)
            assert np.array_equal(raw[:16], want.ravel()) and np.array_equal(wr[:64].view(F32), ww.ravel()) and (raw[16:] == FILL).all() and (wr[64:] == FILL).all()
            assert np.array_equal(sr[:64].view(np.uint64), wst.ravel()) and (sr[64:] == FILL).all()

        def refused(fn, *a, **k):
            assert GF.refusal_code(fn, *a, **k) == INVALID, (a, k)
            still_works()

        try:
            still_works()
            for bad in (0.0, -1.0, float("nan"), INF, -INF):
                refused(c.mosaic_frames_device, g, d_f, d_p, U8E, 1, 8, 4, MM.FEATHER, 2.0, cv, d_c, d_w, gains=[1.0, bad])
            assert b"hg_mosaic_frames_gain_device" in HG.lib().hg_last_error(c._h)
            refused(c.mosaic_frames_device, g, d_f, d_p, U8E, 5, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w, gains=gains)          # the mosaic's own list still holds
            refused(c.mosaic_frames_device, g, d_f, d_p, U8E, 1, 8, 4, 3, 1.0, cv, d_c, d_w, gains=gains)
            stats = c.mosaic_overlap_stats_device
            refused(stats, g, d_f, d_p, 1, cv, 0)                 # d_stats NULL, misaligned
            refused(stats, g, d_f, d_p, 1, cv, d_s + 4)
            for ch in (0, 5):
                refused(stats, g, d_f, d_p, ch, cv, d_s)
            refused(stats, g, 0, d_p, 1, cv, d_s)                 # the mosaic's list: NULL pointers, alignment, offsets, limits
            refused(stats, g, d_f, 0, 1, cv, d_s)
            refused(stats, g, d_f + 4, d_p, 1, cv, d_s)
            refused(stats, g, d_f, d_p, 1, cv, d_s, [0, 260])
            refused(stats, g, d_f, d_p, 1, ((1 << 26) + 1, 0, 8, 2), d_s)
            refused(stats, [g[0], (0, 0, 1 << 16, (1 << 15) + 1)], d_f, d_p, 1, cv, d_s)
            L, vp = HG.lib(), HG.C.c_void_p
            many = HG._geoms([(0, 0, 1, 1)] * 257)
            assert L.hg_mosaic_overlap_stats_device(c._h, many, 257, vp(d_f), None, vp(d_p), None, 1, HG.Geom(*cv), vp(d_s)) == INVALID
            assert b"hg_mosaic_overlap_stats_device" in L.hg_last_error(c._h)
            assert L.hg_mosaic_overlap_stats_device(c._h, many, -1, vp(d_f), None, vp(d_p), None, 1, HG.Geom(*cv), vp(d_s)) == INVALID
            still_works()
            # (f32 frames cannot be asked for: the entry has no element argument)  The solve's invalid sigmas:
            for sn, sg in ((0.0, 0.1), (10.0, -1.0), (float("nan"), 0.1), (10.0, INF)):
                assert GF.refusal_code(HG.mosaic_solve_gains, wst, 1, sn, sg) == INVALID
            still_works()
            got = HG.mosaic_solve_gains(wst, 1)
            assert got.shape == (2,) and (got > 0).all()
        finally:
            c.free(d)


# ------------------------------------------------------------------------------------------------ what the calls leave alone
def test_state_is_untouched_and_a_queued_nearest_warp_keeps_its_bytes():
    """As the mosaic's test of this name: the warp outputs and fields stay on the device and go into the statistics and the gained mosaic
    as they stand, each queued behind a warp that must keep its bytes."""
    W, H, F = 64, 40, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((0.6, 0.45), (7.0, 3.0))      # windows of 48 x 32 at most, each 7 x 3 further on
    x0, y0 = min(g[0] for g in gg), min(g[1] for g in gg)
    canvas = (x0 - 2, y0 - 1, max(g[0] + g[2] for g in gg) - x0 + 3, max(g[1] + g[3] for g in gg) - y0 + 3)
    assert canvas[2] <= 130 and canvas[3] <= 40, (gg, canvas)
    n = canvas[2] * canvas[3]
    fo, ftotal = HG.pack_field_offsets(gg, CO)
    with HG.Context(0) as c:
        d_src, d_f, d_w, d_k, d_c, d_wt, d_s = c.alloc(img.nbytes), c.alloc(ftotal), c.alloc(total), c.alloc(total), c.alloc(n * 4), c.alloc(n * 4), c.alloc(F * F * 16)
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
            wst = MG.overlap_stats(gg, fields, frames, 4, canvas)
            assert alone.any() and (wst[..., 0][np.triu_indices(F, 1)] > 0).any()
            gains = HG.mosaic_solve_gains(wst, 4)
            for step in ("statistics", "gained mosaic"):
                c.to_device(d_k, np.zeros(total, np.uint8))
                c.warp_inverse_geometric_frames_device(d_k)               # queued ...
                mid = GF.tap_state(c)
                if step == "statistics":                                  # ... in front of the call under test
                    c.mosaic_overlap_stats_device(gg, d_f, d_w, 4, canvas, d_s)
                else:
                    c.mosaic_frames_device(gg, d_f, d_w, U8E, 4, W, H, MM.FEATHER, 6.0, canvas, d_c, d_wt, gains=gains)
                assert GF.tap_state(c) == mid, step
                c.sync()
                assert GF.tap_state(c) == mid and c.sampling == HG.SAMPLE_NEAREST, step
                again = c.to_host(d_k, total)
                for f, g in enumerate(gg):                                # (the padding between frames is nobody's)
                    assert np.array_equal(again[offs[f]:offs[f] + RF.n_px(g) * 4], alone[offs[f]:offs[f] + RF.n_px(g) * 4]), (step, f)
                assert np.array_equal(c.to_host(d_w, total), alone)       # the inputs are only read
            assert np.array_equal(c.to_host(d_s, F * F * 16).view(np.uint64), wst.ravel())
            want, ww = MG.mosaic_gain(gg, fields, frames, W, H, MM.FEATHER, 6.0, canvas, gains)
            assert np.array_equal(c.to_host(d_c, n * 4), want.ravel()) and np.array_equal(c.to_host(d_wt, n * 4).view(F32), ww.ravel())
            c.warp_inverse_geometric_frames_device(d_k)                   # the staged frame set is still the warps'
            c.sync()
            assert np.array_equal(c.to_host(d_k, total), again)
        finally:
            c.set_image(img)
            for p in (d_src, d_f, d_w, d_k, d_c, d_wt, d_s):
                c.free(p)


def test_a_queued_redo_never_lands_on_later_statistics():
    """As the mosaic's test of this name: a piecewise warp whose rows carry 1100 spans is queued into buffer B (its frame is flagged, to be
    redone through the map at hg_sync); the statistics are then written at the start of B.  After hg_sync they stand."""
    s = GF.strip_mesh_overflow()
    img, W2, H2, g = s.img, s.W, s.H, s.g
    npx = g[2] * g[3]
    geoms, fields, warped = TM._library_sets()["projective"]
    F = len(geoms)
    want = MG.overlap_stats(geoms, fields, warped, 4, PRO_CANVAS)
    assert F * F * 16 <= npx * 4 and want.any()
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
            c.mosaic_overlap_stats_device(geoms, d_f, d_p, 4, PRO_CANVAS, d_b)
            c.sync()
            assert c.redone_frames() > r0                      # the warp's frame WAS flagged and redone ...
            assert np.array_equal(c.to_host(d_b, F * F * 16).view(np.uint64), want.ravel())      # ... and the statistics stand
        finally:
            c.set_image(img)
            for p_ in (d_src, d_b, d_f, d_p):
                c.free(p_)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_exposure_gain_matches_the_ctypes_pipeline():
    """tests/js/mosaic_gain_gpu.mjs: h.mosaic(sets, {exposure: 'gain'}) of js/Homography.mjs on the real addon for a projective and a
    piecewise set; it prints its windows and the SHA-256 of canvas, weight plane and gains, and the same loop through ctypes -- stage the
    set, warp, export the coordinate fields, statistics, 16 F^2 bytes down, solve, gained mosaic -- must hash alike."""
    res = GF.run_node_case("mosaic_gain_gpu.mjs")
    W, H = res["W"], res["H"]
    img = GF.js_pattern_planes(W, H)[0]
    assert set(res["cases"]) == {"projective", "piecewise"}
    with HG.Context(0) as c:
        c.set_image(img)
        for name, case in res["cases"].items():
            geoms = [tuple(g) for g in case["geoms"]]
            canvas = tuple(case["canvas"])
            n = canvas[2] * canvas[3]
            F = len(geoms)
            assert F >= 3 and canvas[2] <= 130 and canvas[3] <= 40, (name, canvas)
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
            d_f, d_o, d_c, d_w, d_s = c.alloc(ftotal), c.alloc(ototal), c.alloc(n * 4), c.alloc(n * 4), c.alloc(F * F * 16)
            try:
                if name == "piecewise":
                    c.warp_inverse_piecewise_frames_device(d_o)
                    c.field_inverse_piecewise_frames_device(CO, d_f)
                else:
                    c.warp_inverse_geometric_frames_device(d_o)
                    c.field_inverse_geometric_frames_device(CO, d_f)
                c.sync()
                for key, (mode, feather, sn, sg) in case["runs"].items():
                    c.mosaic_overlap_stats_device(geoms, d_f, d_o, 4, canvas, d_s)
                    c.sync()
                    st = c.to_host(d_s, F * F * 16).view(np.uint64)
                    assert (st.reshape(F, F, 2)[..., 0][np.triu_indices(F, 1)] > 0).any(), name        # the case does overlap
                    gains = HG.mosaic_solve_gains(st, 4, sn, sg)
                    assert np.abs(gains - 1).max() > 1e-4, (name, gains.tolist())
                    c.mosaic_frames_device(geoms, d_f, d_o, U8E, 4, W, H, mode, INF if feather is None else feather, canvas, d_c, d_w, gains=gains)
                    c.sync()
                    got = c.to_host(d_c, n * 4)
                    assert hashlib.sha256(gains.tobytes()).hexdigest() == case["hashes"][key]["gains"], (name, key, gains.tolist())
                    assert got.any() and hashlib.sha256(got.tobytes()).hexdigest() == case["hashes"][key]["data"], (name, key)
                    assert hashlib.sha256(c.to_host(d_w, n * 4).tobytes()).hexdigest() == case["hashes"][key]["weight"], (name, key)
            finally:
                for p_ in (d_f, d_o, d_c, d_w, d_s):
                    c.free(p_)
