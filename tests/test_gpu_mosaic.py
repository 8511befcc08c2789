"""The mosaic on the GPU (include/hgwarp.h: hg_mosaic_frames_device) against the numpy model of tests/hgtest/mosaic.py, bit for bit --
canvas and weight plane --, and the drop-in class on the real addon against the ctypes pipeline.  tests/test_mosaic_cpu.py pins the model
itself against a scalar model written from the header.  Small shapes throughout: canvases of 130 x 40 at most, frames of 48 x 32 at most;
every buffer is filled with 0xA5 before a call and the bytes outside the canvas extent must keep it."""
import base64
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import mosaic as MM              # noqa: E402
from hgtest.gpu_frames import CO, F32, F32E, FILL, INVALID, U8E      # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
INF = float("inf")
SW, SH = 67, 45                              # the source
MODES = ((MM.LAST, 1.0), (MM.MEAN, 1.0), (MM.FEATHER, INF), (MM.FEATHER, 3.5))
# windows that leave the canvas on each of its four sides, one wholly outside, a frame of width 1, an empty frame between full ones, two
# frames with identical windows, negative offsets
PRO_GEOMS = [(0, 0, 48, 32), (30, 10, 48, 32), (-20, -14, 40, 20), (60, 5, 1, 7), (0, 0, 0, 4), (30, 10, 48, 32), (100, -16, 40, 30), (500, 500, 8, 8), (95, 20, 30, 9)]
PRO_CANVAS = (-10, -8, 130, 40)
PW_GEOMS = [(0, 0, 48, 8), (-2, -1, 40, 9), (1, 1, 20, 4)]
PW_CANVAS = (-4, -2, 56, 13)


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ inputs, made once and never modified
@functools.lru_cache(maxsize=None)
def _library_sets():
    """What the library itself makes over the SW x SH source, downloaded once: name -> (geoms, fields, RGBA warp outputs).  A projective
    set on PRO_GEOMS, every frame looking a little beyond the source's border (uncovered rims), and a piecewise set whose windows reach
    beyond the mesh (uncovered pixels are NaN)."""
    out = {}
    img = WL.lcg_image(SW, SH, 5)
    with HG.Context(0) as c:
        c.set_image(img)
        mats = []
        for f, (x, y, w, h) in enumerate(PRO_GEOMS):
            kx, ky = (SW + 6.0) / max(w, 1), (SH + 5.0) / max(h, 1)
            mats.append([kx, 0.02 * f, kx * (0.5 - x) - 3 - 0.02 * f * y, 0.01, ky, ky * (0.5 - y) - 2.5 - 0.01 * x, 1e-4 * f, -2e-4])
        for name, geoms, stage in (("projective", PRO_GEOMS, lambda: c.geometric_set_frames(1, np.concatenate(mats), PRO_GEOMS)), ("piecewise", PW_GEOMS, None)):
            if stage is None:
                nx, ny = 3, 2
                sp, tris = WL.grid_points(SW, SH, nx, ny), WL.grid_triangles(nx, ny)
                p = sp.reshape(-1, 2).astype(np.float64)
                dps = [np.stack([p[:, 0] * kx + 2, p[:, 1] * ky + 1 + 0.4 * np.sin(p[:, 0] / 20 + f)], 1).astype(F32).ravel()
                       for f, (kx, ky) in enumerate(((0.7, 0.12), (0.5, 0.15), (0.25, 0.06)))]
                c.piecewise_set_mesh(sp, tris, *WL.src_min(sp))
                c.piecewise_set_frames(np.concatenate(dps), PW_GEOMS)
            else:
                stage()
            fo, ftotal = HG.pack_field_offsets(geoms, CO)
            oo, ototal = HG.pack_offsets(geoms)
            assert oo == HG.pack_plane_offsets(geoms, 4)[0]          # the RGBA warps' default layout IS the mosaic's default for u8 x 4
            d_f, d_o = c.alloc(ftotal), c.alloc(ototal)
            try:
                if stage is None:
                    c.field_inverse_piecewise_frames_device(CO, d_f)
                    c.warp_inverse_piecewise_frames_device(d_o)
                else:
                    c.field_inverse_geometric_frames_device(CO, d_f)
                    c.warp_inverse_geometric_frames_device(d_o)
                c.sync()
                out[name] = (geoms, GF.split(c.to_host(d_f, ftotal), fo, geoms, 8, F32, 2), GF.split(c.to_host(d_o, ototal), oo, geoms, 4, np.uint8, 4))
            finally:
                c.free(d_f)
                c.free(d_o)
    return out


@functools.lru_cache(maxsize=None)
def _frames(name, elem, ch):
    """The frames' pixels: the library's own warp outputs for u8 x 4, else values of the asked type (no uint8 equals FILL or POISON)."""
    geoms, _, warped = _library_sets()[name]
    if (elem, ch) == (U8E, 4):
        return tuple(warped)
    rng = np.random.default_rng(500 + 10 * ch + elem)
    out = []
    for g in geoms:
        n = RF.n_px(g)
        out.append(rng.integers(1, 160, (n, ch), dtype=np.uint8) if elem == U8E else (rng.standard_normal((n, ch)) * 40 + 3).astype(F32))
        out[-1].setflags(write=False)
    return tuple(out)


def _run(ctx, geoms, fields, frames, elem, ch, mode, feather, canvas, **kw):
    """GF.run_mosaic over the SW x SH source: (canvas bytes, weights or None); it checks the bytes outside the canvas and the weight plane."""
    return GF.run_mosaic(ctx, geoms, fields, frames, elem, ch, SW, SH, mode, feather, canvas, **kw)


def _contributors(geoms, fields, canvas):
    """Contributors per canvas pixel (MEAN's weight plane in the model)."""
    frames = [np.zeros((RF.n_px(g), 1), np.uint8) for g in geoms]
    return MM.mosaic(geoms, fields, frames, SW, SH, MM.MEAN, 1.0, canvas)[1]


# ------------------------------------------------------------------------------------------------ the mosaic against the model
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_mosaic_of_the_librarys_projective_fields_and_warp_outputs(ctx, elem, channels):
    geoms, fields, _ = _library_sets()["projective"]
    n = _contributors(geoms, fields, PRO_CANVAS)                  # the premises, on the CPU, before anything is compared
    assert (n == 0).any() and (n == 1).any() and (n == 2).any() and (n >= 3).any(), np.bincount(n.astype(int).ravel()).tolist()
    for g, co in zip(geoms, fields):
        cov = np.isfinite(co).all(-1)
        assert RF.n_px(g) == 0 or (cov.any() and (RF.n_px(g) < 100 or not cov.all())), g      # every frame covers; the large ones have uncovered rims
    frames = _frames("projective", elem, channels)
    for mode, feather in MODES:
        want = MM.mosaic(geoms, fields, frames, SW, SH, mode, feather, PRO_CANVAS)
        GF.check_canvas(_run(ctx, geoms, fields, frames, elem, channels, mode, feather, PRO_CANVAS), want, ("projective", elem, channels, mode, feather))


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_mosaic_of_a_piecewise_set_with_uncovered_pixels(ctx, elem, channels):
    geoms, fields, _ = _library_sets()["piecewise"]
    nan = sum(int((~np.isfinite(f).all(-1)).sum()) for f in fields)
    assert nan > 50 and sum(int(np.isfinite(f).all(-1).sum()) for f in fields) > 300
    n = _contributors(geoms, fields, PW_CANVAS)
    assert (n == 0).any() and (n == 1).any() and (n == 2).any() and (n == 3).any()
    frames = _frames("piecewise", elem, channels)
    for mode, feather in MODES:
        want = MM.mosaic(geoms, fields, frames, SW, SH, mode, feather, PW_CANVAS)
        GF.check_canvas(_run(ctx, geoms, fields, frames, elem, channels, mode, feather, PW_CANVAS, weight=mode != MM.MEAN), want, ("piecewise", elem, channels, mode, feather))


@pytest.mark.parametrize("canvas", ((3, 2, 1, 7), (-6, 4, 67, 5), (-10, 11, 130, 3), (29, 9, 2, 2), (400, 400, 5, 3)))
def test_canvas_shapes_and_a_null_weight_plane(ctx, canvas):
    geoms, fields, _ = _library_sets()["projective"]
    for elem, ch in ((U8E, 4), (F32E, 3), (U8E, 2)):
        frames = _frames("projective", elem, ch)
        for k, (mode, feather) in enumerate(MODES):
            want = MM.mosaic(geoms, fields, frames, SW, SH, mode, feather, canvas)
            GF.check_canvas(_run(ctx, geoms, fields, frames, elem, ch, mode, feather, canvas, weight=k % 2 == 0), want, (canvas, elem, ch, mode))
    assert not MM.mosaic(geoms, fields, _frames("projective", U8E, 4), SW, SH, MM.MEAN, 1.0, (400, 400, 5, 3))[1].any()      # wholly beside every frame


def _caller_fields(geoms):
    """Caller-made fields: coordinates over the source and beyond every border, with NaN, +-Inf and 1e30 entries."""
    rng = np.random.default_rng(43)
    out = []
    for f, g in enumerate(geoms):
        w, h = max(g[2], 0), max(g[3], 0)
        i, j = np.meshgrid(np.arange(w), np.arange(h))
        co = np.stack([(SW + 4.0) * i / max(w - 1, 1) - 2 + 0.25 * f, (SH + 3.0) * j / max(h - 1, 1) - 1.5 + 0.125 * f], -1).astype(F32).reshape(-1, 2)
        if w * h >= 20:
            co[rng.random(w * h) < 0.1] = np.nan
            co[1:9] = [[np.nan, 3], [3, np.nan], [np.inf, 2], [2, -np.inf], [1e30, 5], [5, -1e30], [-1e30, 1e30], [3e38, -3e38]]
            co[10:12] = [[SW, 4], [SW - 0.5, SH]]
        co.setflags(write=False)
        out.append(co)
    return out


def test_caller_made_fields_with_nan_infinite_and_huge_coordinates(ctx):
    fields = _caller_fields(PRO_GEOMS)
    f0 = fields[0]
    assert np.isnan(f0).any() and np.isinf(f0).any() and (np.abs(f0[np.isfinite(f0)]) >= 1e30).any()
    for elem, ch in ((U8E, 1), (U8E, 4), (F32E, 2), (F32E, 4)):
        frames = _frames("projective", elem, ch)
        for mode, feather in MODES:
            want = MM.mosaic(PRO_GEOMS, fields, frames, SW, SH, mode, feather, PRO_CANVAS)
            if mode == MM.FEATHER:                                # the 1e30 pixels contribute, at the floor weight
                assert (want[1] > 0).any() and float(MM.feather_weight(f0[5], SW, SH, feather)) == 2.0 ** -10
            GF.check_canvas(_run(ctx, PRO_GEOMS, fields, frames, elem, ch, mode, feather, PRO_CANVAS), want, ("caller-made", elem, ch, mode, feather))


def test_explicit_offsets_that_break_every_wider_alignment(ctx):
    fields = _caller_fields(PRO_GEOMS)
    fo8 = [o + 8 * (2 * f + 1) + 512 * f for f, o in enumerate(RF.pack(PRO_GEOMS, 8)[0])]        # odd multiples of 8: no 16-byte alignment
    assert all(o % 8 == 0 and o % 16 != 0 for o in fo8)
    for elem in (U8E, F32E):
        es = GF.es(elem)
        for ch in (1, 2, 3, 4):
            frames = _frames("projective", elem, ch)
            po = [o + 640 * f + es * (2 * f + 1) for f, o in enumerate(RF.pack(PRO_GEOMS, ch * es)[0])]   # odd element offsets: no 2- or 4-byte load fits (u8)
            assert all(o % es == 0 and (o // es) % 2 == 1 for o in po)
            for mode, feather in MODES[1:3]:
                want = MM.mosaic(PRO_GEOMS, fields, frames, SW, SH, mode, feather, PRO_CANVAS)
                got = _run(ctx, PRO_GEOMS, fields, frames, elem, ch, mode, feather, PRO_CANVAS, foffs=fo8, poffs=po, front=256 + 2 * es, cfront=es)
                GF.check_canvas(got, want, ("explicit offsets", elem, ch, mode))
    # ... and where only SOME frames start aligned for the wide load, under an odd base
    frames = _frames("projective", U8E, 4)
    po = [o + (f % 4) for f, o in enumerate(RF.pack(PRO_GEOMS, 4)[0])]
    want = MM.mosaic(PRO_GEOMS, fields, frames, SW, SH, MM.LAST, 1.0, PRO_CANVAS)
    GF.check_canvas(_run(ctx, PRO_GEOMS, fields, frames, U8E, 4, MM.LAST, 1.0, PRO_CANVAS, poffs=po, front=257, cfront=3), want, "mixed alignment")


def test_2500_small_frames_thrown_over_the_canvas(ctx):
    """Many contributors per pixel and more frames than any list a kernel may keep; frames beside the canvas and across its edges."""
    rng = np.random.default_rng(44)
    canvas = (-5, 3, 40, 24)
    geoms = [(int(x), int(y), 2, 2) for x, y in zip(rng.integers(-9, 37, 2500), rng.integers(0, 29, 2500))]
    for k in range(0, 2500, 97):
        geoms[k] = (geoms[k][0], geoms[k][1], 0, 2)
    fields = [(rng.random((RF.n_px(g), 2)) * [SW + 2, SH + 2] - 1).astype(F32) for g in geoms]
    for co in fields[::5]:
        co[:1] = np.nan
    n = _contributors(geoms, fields, canvas)
    assert n.max() >= 12 and (n == 0).any(), (n.max(), n.min())
    for elem, ch in ((U8E, 3), (F32E, 1)):
        frames = [rng.integers(1, 160, (RF.n_px(g), ch), dtype=np.uint8) if elem == U8E else (rng.standard_normal((RF.n_px(g), ch)) * 40).astype(F32) for g in geoms]
        for mode, feather in MODES[:3]:
            want = MM.mosaic(geoms, fields, frames, SW, SH, mode, feather, canvas)
            GF.check_canvas(_run(ctx, geoms, fields, frames, elem, ch, mode, feather, canvas), want, ("2500 frames", elem, ch, mode))


def test_no_frames_zero_the_canvas_and_an_empty_canvas_writes_nothing(ctx):
    for elem, ch in ((U8E, 3), (F32E, 2)):
        for mode, feather in MODES[:3]:
            canvas, weight = _run(ctx, [], [], [], elem, ch, mode, feather, (5, -5, 67, 5))
            assert not canvas.any() and not weight.view(np.uint8).any()
    geoms, fields, _ = _library_sets()["projective"]
    for canvas in ((0, 0, 0, 9), (0, 0, 9, -1)):
        got, weight = _run(ctx, geoms, fields, _frames("projective", U8E, 4), U8E, 4, MM.MEAN, 1.0, canvas)      # (_run checks that every byte kept FILL)
        assert got.size == 0 and weight.size == 0
    L, vp = HG.lib(), HG.C.c_void_p
    d = ctx.alloc(1024)
    try:
        ctx.to_device(d, np.full(1024, FILL, np.uint8))
        assert L.hg_mosaic_frames_device(ctx._h, None, 0, None, None, None, None, U8E, 4, 1, 1, MM.LAST, 0.0, HG.Geom(0, 0, 8, 8), vp(d), None) == 0
        ctx.sync()
        raw = ctx.to_host(d, 1024)
        assert not raw[:256].any() and (raw[256:] == FILL).all()
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    g = [(0, 0, 8, 2), (4, 1, 4, 1)]
    cv = (0, 0, 8, 2)
    with HG.Context(0) as c:
        d = c.alloc(16384)
        d_f, d_p, d_c, d_w = d, d + 4096, d + 8192, d + 12288
        co = (np.random.default_rng(2).random((20, 2)) * [7, 3]).astype(F32)
        px = np.arange(1, 21, dtype=np.float32).reshape(20, 1)
        c.to_device(d_f, GF.place([co[:16], co[16:]], [0, 256], 512, 0))
        c.to_device(d_p, GF.place([px[:16], px[16:]], [0, 256], 512, 0))
        want, ww = MM.mosaic(g, [co[:16], co[16:]], [px[:16], px[16:]], 8, 4, MM.FEATHER, 2.0, cv)

        def still_works():
            c.to_device(d_c, np.full(512, FILL, np.uint8))
            c.to_device(d_w, np.full(512, FILL, np.uint8))
            c.mosaic_frames_device(g, d_f, d_p, F32E, 1, 8, 4, MM.FEATHER, 2.0, cv, d_c, d_w)
            c.sync()
            raw, wr = c.to_host(d_c, 512), c.to_host(d_w, 512)
            assert np.array_equal(raw[:64].view(F32), want.ravel()) and np.array_equal(wr[:64].view(F32), ww.ravel()) and (raw[64:] == FILL).all() and (wr[64:] == FILL).all()

        def refused(*a, **k):
            assert GF.refusal_code(c.mosaic_frames_device, *a, **k) == INVALID, (a, k)
            still_works()

        try:
            still_works()
            # (geoms, d_coords, d_frames, elem, channels, w, h, mode, feather, canvas, d_canvas, d_weight, field_offsets, frame_offsets)
            refused(g, d_f, d_p, 2, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w)                       # elem
            for mode in (-1, 3):
                refused(g, d_f, d_p, F32E, 1, 8, 4, mode, 1.0, cv, d_c, d_w)
            for ch in (0, 5):
                refused(g, d_f, d_p, F32E, ch, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w)
            refused(g, d_f, d_p, F32E, 1, 0, 4, MM.MEAN, 1.0, cv, d_c, d_w)
            refused(g, d_f, d_p, F32E, 1, 8, 0, MM.MEAN, 1.0, cv, d_c, d_w)
            for feather in (0.0, -1.0, float("nan"), -INF):
                refused(g, d_f, d_p, F32E, 1, 8, 4, MM.FEATHER, feather, cv, d_c, d_w)
            c.mosaic_frames_device(g, d_f, d_p, F32E, 1, 8, 4, MM.MEAN, float("nan"), cv, d_c, d_w)      # ... and ignored by the other modes
            c.mosaic_frames_device(g, d_f, d_p, F32E, 1, 8, 4, MM.LAST, -1.0, cv, d_c, d_w)
            refused(g, 0, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w)                      # NULL pointers
            refused(g, d_f, 0, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w)
            refused(g, d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, 0, d_w)
            refused([], d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, 0, d_w)
            refused(g, d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, (0, 0, 0, 0), 0, d_w)            # d_canvas NULL even for an empty canvas
            refused(g, d_f + 4, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w)                # misaligned coordinates, frames, canvas, weights, offsets
            refused(g, d_f, d_p + 2, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w)
            refused(g, d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c + 1, d_w)
            refused(g, d_f, d_p, U8E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w + 2)
            refused(g, d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w, [0, 260])
            refused(g, d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w, None, [0, 258])
            refused(g, d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, ((1 << 26) + 1, 0, 8, 2), d_c, d_w)      # beyond the hg_geom limits
            refused(g, d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, (0, 0, 1 << 16, (1 << 15) + 1), d_c, d_w)
            refused([g[0], (0, -(1 << 26) - 1, 4, 1)], d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w)
            refused([g[0], (0, 0, 1 << 16, (1 << 15) + 1)], d_f, d_p, F32E, 1, 8, 4, MM.MEAN, 1.0, cv, d_c, d_w)
            L, vp = HG.lib(), HG.C.c_void_p
            geoms = HG._geoms(g)
            assert L.hg_mosaic_frames_device(c._h, geoms, -1, vp(d_f), None, vp(d_p), None, 0, 1, 8, 4, 1, 1.0, HG.Geom(*cv), vp(d_c), None) == INVALID
            assert L.hg_mosaic_frames_device(c._h, geoms, 65536, vp(d_f), None, vp(d_p), None, 0, 1, 8, 4, 1, 1.0, HG.Geom(*cv), vp(d_c), None) == INVALID
            assert L.hg_mosaic_frames_device(c._h, None, 2, vp(d_f), None, vp(d_p), None, 0, 1, 8, 4, 1, 1.0, HG.Geom(*cv), vp(d_c), None) == INVALID
            assert b"hg_mosaic_frames_device" in L.hg_last_error(c._h)
            still_works()
        finally:
            c.free(d)


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def test_state_is_untouched_and_a_queued_nearest_warp_keeps_its_bytes():
    """The fields and the warp outputs stay on the device in the library's own layouts and go into the mosaic as they stand."""
    W, H, F = 64, 40, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((0.6, 0.45), (7.0, 3.0))      # windows of 48 x 32 at most, each 7 x 3 further on
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
            assert alone.any() and _contributors(gg, fields, canvas).max() >= 2
            c.to_device(d_k, np.zeros(total, np.uint8))
            c.warp_inverse_geometric_frames_device(d_k)                   # queued ...
            mid = GF.tap_state(c)
            c.mosaic_frames_device(gg, d_f, d_w, U8E, 4, W, H, MM.FEATHER, 6.0, canvas, d_c, d_wt)      # ... in front of the mosaic of the first warp's frames
            assert GF.tap_state(c) == mid
            c.sync()
            assert GF.tap_state(c) == mid and c.sampling == HG.SAMPLE_NEAREST
            again = c.to_host(d_k, total)
            for f, g in enumerate(gg):                                    # (the padding between frames is nobody's)
                assert np.array_equal(again[offs[f]:offs[f] + RF.n_px(g) * 4], alone[offs[f]:offs[f] + RF.n_px(g) * 4]), f
            assert np.array_equal(c.to_host(d_w, total), alone)           # the inputs are only read
            want, ww = MM.mosaic(gg, fields, frames, W, H, MM.FEATHER, 6.0, canvas)
            assert np.array_equal(c.to_host(d_c, n * 4), want.ravel()) and np.array_equal(c.to_host(d_wt, n * 4).view(F32), ww.ravel())
            c.warp_inverse_geometric_frames_device(d_k)                   # the staged frame set is still the warps'
            c.sync()
            assert np.array_equal(c.to_host(d_k, total), again)
        finally:
            c.set_image(img)
            for p in (d_src, d_f, d_w, d_k, d_c, d_wt):
                c.free(p)


def test_a_queued_redo_never_lands_on_a_later_mosaic():
    """A piecewise warp whose rows carry 1100 spans is queued into buffer B (its frame is flagged, to be redone through the map at hg_sync);
    a mosaic then writes its canvas at the start of B and its weight plane further into B.  After hg_sync both hold the mosaic's.  (The
    redo needs the wide source and window of the anisotropic test of the same name: a row must carry more spans than the row kernel
    holds; the mosaic's own canvas stays 130 x 40.)"""
    s = GF.strip_mesh_overflow()
    img, W2, H2, g = s.img, s.W, s.H, s.g
    npx = g[2] * g[3]
    geoms, fields, warped = _library_sets()["projective"]
    canvas = PRO_CANVAS
    cpx = canvas[2] * canvas[3]
    w_at = (cpx * 4 + 4095) // 4096 * 4096
    assert w_at + cpx * 4 <= npx * 4 and g[2] * 4 * 2 < cpx * 4      # canvas and weights lie inside B, over several of the warp's rows
    want, ww = MM.mosaic(geoms, fields, warped, SW, SH, MM.FEATHER, INF, canvas)
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
            c.mosaic_frames_device(geoms, d_f, d_p, U8E, 4, SW, SH, MM.FEATHER, INF, canvas, d_b, d_b + w_at)
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
def test_js_class_mosaic_matches_the_ctypes_pipeline():
    """tests/js/mosaic_gpu.mjs: h.mosaic of js/Homography.mjs on the real addon for an affine, a projective and a piecewise set; it prints
    its windows and the SHA-256 of every canvas and weight plane, and the same loop through ctypes -- stage the set, warp, export the
    coordinate fields, mosaic -- must hash alike."""
    res = GF.run_node_case("mosaic_gpu.mjs")
    W, H = res["W"], res["H"]
    img = GF.js_pattern_planes(W, H)[0]
    assert set(res["cases"]) == {"affine", "projective", "piecewise"}
    with HG.Context(0) as c:
        c.set_image(img)
        for name, case in res["cases"].items():
            geoms = [tuple(g) for g in case["geoms"]]
            canvas = tuple(case["canvas"])
            n = canvas[2] * canvas[3]
            assert len(geoms) >= 3 and canvas[2] <= 130 and canvas[3] <= 40, (name, canvas)
            c.set_sampling(case["sampling"])
            if name == "piecewise":
                sp = np.frombuffer(base64.b64decode(case["src"]), F32)
                tris = np.frombuffer(base64.b64decode(case["tris"]), np.uint32)
                c.piecewise_set_mesh(sp, tris, *case["minSrc"])
                c.piecewise_set_frames(np.frombuffer(base64.b64decode(case["dst"]), F32), geoms)
            else:
                c.geometric_set_frames_points(0 if name == "affine" else 1, np.frombuffer(base64.b64decode(case["from"]), F32),
                                              np.frombuffer(base64.b64decode(case["to"]), F32), geoms)
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
                fields = GF.split(c.to_host(d_f, ftotal), fo, geoms, 8, F32, 2)
                assert _contributors(geoms, fields, canvas).max() >= 2, name         # the case does overlap
                for key, (mode, feather) in case["runs"].items():
                    c.mosaic_frames_device(geoms, d_f, d_o, U8E, 4, W, H, mode, INF if feather is None else feather, canvas, d_c, d_w)
                    c.sync()
                    got = c.to_host(d_c, n * 4)
                    assert got.any() and hashlib.sha256(got.tobytes()).hexdigest() == case["hashes"][key]["data"], (name, key)
                    assert hashlib.sha256(c.to_host(d_w, n * 4).tobytes()).hexdigest() == case["hashes"][key]["weight"], (name, key)
            finally:
                for p_ in (d_f, d_o, d_c, d_w):
                    c.free(p_)
