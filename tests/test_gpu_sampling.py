"""Bilinear sampling of the inverse warps on the GPU (include/hgwarp.h, HG_SAMPLE_BILINEAR) against the numpy model of
tests/hgtest/bilinear.py.  The model's per-pixel triangle ids and inverse matrices come from the CPU oracle (taps), never from the
library under test."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import bilinear as B             # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
BIL, NEAR = HG.SAMPLE_BILINEAR, HG.SAMPLE_NEAREST


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def _exact(got, want, cov, what, coords=None):
    """Byte-exact RGBA, coverage exact, uncovered all-zero.  On a mismatch: how many, and the first few (row, col, got, want) with the
    source coordinate there (`coords`: (sx, sy) arrays of the window, or a callable returning them)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not got[~cov].any(), (what, "uncovered pixels written")
    assert np.array_equal(got.any(-1), want.any(-1)), (what, "coverage")
    bad = np.argwhere((got != want).any(-1))
    if bad.size:
        sx, sy = (coords() if callable(coords) else coords) if coords is not None else (None, None)
        first = [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist(),
                  None if sx is None else (float(sx[r, c]), float(sy[r, c]))) for r, c in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ; (row, col, got, want, (sx, sy)): {first}")


def _geo_coords(kind, m, g):
    return lambda: B.geometric_coords(kind, m, *g)


def _pw_coords(wmap, inv, g):
    return lambda: B.piecewise_coords(wmap, inv, *g)[:2]


def _pw_case(W, H, nx, ny, A, seed, shift=None):
    img = WL.lcg_image(W, H, seed)
    sp, tris = WL.grid_points(W, H, nx, ny), WL.grid_triangles(nx, ny)
    dp = (sp + np.tile(np.asarray(shift, np.float32), sp.size // 2)) if shift is not None else WL.sin_dst(sp, A, 8)
    geom = WL.piecewise_geom(dp)
    msx, msy = WL.src_min(sp)
    return img, sp, tris, dp.astype(np.float32), geom, msx, msy


def _pw_model(img, sp, dp, tris, msx, msy, geom):
    near, wmap, _, inv = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom, taps=True)
    bil, cov = B.warp_piecewise(wmap, inv, img, msx, msy, *geom)
    return near, bil, cov, wmap, inv


def _pw_warp(ctx, img, sp, tris, msx, msy, dp, geom, mode):
    ctx.set_sampling(mode)
    ctx.set_image(img)
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    ctx.piecewise_prepare(dp, geom)
    return ctx.warp_inverse_piecewise()


def test_mode_roundtrip_and_rejects_unknown(ctx):
    assert ctx.sampling == NEAR
    ctx.set_sampling(BIL)
    assert ctx.sampling == BIL
    for bad in (2, -1, 255):
        with pytest.raises(HG.HgError):
            ctx.set_sampling(bad)
        assert ctx.sampling == BIL
    ctx.set_sampling(NEAR)
    assert ctx.sampling == NEAR


def test_integer_shifts_equal_nearest(ctx):
    W, H = 160, 96
    img = WL.lcg_image(W, H, 3)
    ctx.set_image(img)
    for kind, m in ((0, [1, 0, 0, 1, -7, -4]), (1, [1, 0, -7, 0, 1, -4, 0, 0]), (0, [1, 0, 0, 1, 11, 2])):
        g = (-3, -5, W + 9, H + 6)
        ctx.set_sampling(NEAR)
        near = ctx.warp_inverse_geometric(kind, np.array(m, np.float64), g)
        ctx.set_sampling(BIL)
        bil = ctx.warp_inverse_geometric(kind, np.array(m, np.float64), g)
        assert np.array_equal(near, O.warp_inverse_geometric(kind, np.array(m, np.float64), img, *g))
        assert near.any() and np.array_equal(bil, near), (kind, m)
    img, sp, tris, dp, geom, msx, msy = _pw_case(W, H, 8, 6, 0, 4, shift=(6, 3))
    near, want, cov, wmap, inv = _pw_model(img, sp, dp, tris, msx, msy, geom)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *geom)
    assert (sx[valid] == np.round(sx[valid])).all() and (sy[valid] == np.round(sy[valid])).all()    # (the case's premise)
    got = _pw_warp(ctx, img, sp, tris, msx, msy, dp, geom, BIL)
    assert np.array_equal(got, near) and np.array_equal(got, want)
    ctx.set_sampling(NEAR)


def test_constant_colour_source_gives_the_colour_on_exactly_the_covered_pixels(ctx):
    W, H = 200, 120
    colour = np.array([17, 201, 90, 255], np.uint8)
    img = np.broadcast_to(colour, (H, W, 4)).copy()
    ctx.set_sampling(BIL)
    s4, d4 = WL.corners(W, H), WL.projective_dst(W, H)
    pg = tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W, H))
    for kind, m, g in ((0, np.array([0.93, 0.11, -0.21, 1.07, 13.3, -6.6]), (-10, -10, W + 30, H + 20)), (1, HG.solve_projective(d4, s4), pg)):
        ctx.set_image(img)
        got = ctx.warp_inverse_geometric(kind, m, g)
        _, cov = B.warp_geometric(kind, m, img, *g)
        assert cov.any() and not cov.all()
        assert np.array_equal(got.any(-1), cov) and (got[cov] == colour).all() and not got[~cov].any(), kind
    img_p, sp, tris, dp, geom, msx, msy = _pw_case(W, H, 6, 4, 9.0, 1)
    _, _, cov, _, _ = _pw_model(img, sp, dp, tris, msx, msy, geom)
    got = _pw_warp(ctx, img, sp, tris, msx, msy, dp, geom, BIL)
    assert cov.any() and np.array_equal(got.any(-1), cov) and (got[cov] == colour).all() and not got[~cov].any()
    ctx.set_sampling(NEAR)


def test_random_sources_match_the_model(ctx):
    """Affine, projective (one full C2 frame) and piecewise (one full C3 frame, and a mesh with a negative source minimum)."""
    ctx.set_sampling(BIL)
    W, H = 300, 180
    img = WL.lcg_image(W, H, 12)
    ctx.set_image(img)
    m = np.array([0.8133, 0.2071, -0.3313, 0.9377, 21.71, -13.9])
    g = (-40, -20, 420, 260)
    want, cov = B.warp_geometric(0, m, img, *g)
    _exact(ctx.warp_inverse_geometric(0, m, g), want, cov, "affine", _geo_coords(0, m, g))
    W2, H2 = 1920, 1080                                       # C2
    img2 = WL.lcg_image(W2, H2, 2)
    s4, d4 = WL.corners(W2, H2), WL.projective_dst(W2, H2)
    g2 = tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W2, H2))
    m2 = HG.solve_projective(d4, s4)
    ctx.set_image(img2)
    want, cov = B.warp_geometric(1, m2, img2, *g2)
    _exact(ctx.warp_inverse_geometric(1, m2, g2), want, cov, "projective C2", _geo_coords(1, m2, g2))
    cfg = WL.CONFIGS["C3"]                                    # C3: 4K, 200 triangles
    img3, sp, tris, dp, geom, msx, msy = _pw_case(cfg["W"], cfg["H"], cfg["nx"], cfg["ny"], cfg["A"], 3)
    _, want, cov, wm, iv = _pw_model(img3, sp, dp, tris, msx, msy, geom)
    _exact(_pw_warp(ctx, img3, sp, tris, msx, msy, dp, geom, BIL), want, cov, "piecewise C3", _pw_coords(wm, iv, geom))
    assert ctx.last_piecewise_kernel() == 4
    # source points with a negative minimum: coverage on the minSrc window, taps clamped to the image
    img4 = WL.lcg_image(120, 90, 8)
    sp4 = (WL.grid_points(120, 90, 5, 3) - np.tile(np.float32([17, 9]), 24)).astype(np.float32)
    tris4 = WL.grid_triangles(5, 3)
    dp4 = WL.sin_dst(sp4, 3.0, 9)
    geom4 = WL.piecewise_geom(dp4)
    msx4, msy4 = WL.src_min(sp4)
    assert msx4 < 0 and msy4 < 0
    _, want, cov, wm, iv = _pw_model(img4, sp4, dp4, tris4, msx4, msy4, geom4)
    _exact(_pw_warp(ctx, img4, sp4, tris4, msx4, msy4, dp4, geom4, BIL), want, cov, "piecewise, negative source minimum", _pw_coords(wm, iv, geom4))
    assert ctx.last_piecewise_kernel() == 4
    ctx.set_sampling(NEAR)


def _frames_to_host(ctx, d_out, geoms, offs):
    return [ctx.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4) for f, g in enumerate(geoms)]


def test_frame_sets_equal_single_frames(ctx):
    """Piecewise and geometric frame sets with one source per frame, device-side geometric solves, and Multi over [0] and [0, 0]."""
    W, H, nx, ny, F, NI = 256, 160, 8, 5, 5, 3
    imgs = [WL.lcg_image(W, H, 500 + k) for k in range(NI)]
    sp, tris = WL.grid_points(W, H, nx, ny), WL.grid_triangles(nx, ny)
    frames = [WL.sin_dst(sp, 5.0 + f, 8 + (f % 4)) for f in range(F)]
    geoms = [WL.piecewise_geom(d) for d in frames]
    msx, msy = WL.src_min(sp)
    single = [_pw_warp(ctx, imgs[f % NI], sp, tris, msx, msy, frames[f], geoms[f], BIL) for f in range(F)]
    for f in range(F):
        _, want, cov, wm, iv = _pw_model(imgs[f % NI], sp, frames[f], tris, msx, msy, geoms[f])
        _exact(single[f], want, cov, ("piecewise single", f), _pw_coords(wm, iv, geoms[f]))
    stride = W * H * 4 + 256
    offs, total = HG.pack_offsets(geoms)
    s4 = WL.corners(W, H)
    d4s = [WL.projective_dst(W, H, 0.03 * k) for k in range(F)]
    gg = [tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W, H)) for d4 in d4s]
    goffs, gtotal = HG.pack_offsets(gg)
    a3s = np.array([0, 0, 0, H, W, 0], np.float32)
    a3d = [WL.affine_dst(W, H, 0.01 * k) for k in range(F)]
    ag = [tuple(int(v) for v in O.transform_limits(0, O.affine_from_triangles(a3s, d).astype(np.float64), W, H)) for d in a3d]
    aoffs, atotal = HG.pack_offsets(ag)
    d_src = ctx.alloc(stride * NI)
    d_out = ctx.alloc(max(total, gtotal, atotal))
    try:
        for k in range(NI):
            ctx.to_device(d_src, imgs[k], k * stride)
        ctx.set_images_device(d_src, W, H, NI, stride)
        ctx.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        ctx.warp_inverse_piecewise_frames_device(d_out)
        ctx.sync()
        for f, got in enumerate(_frames_to_host(ctx, d_out, geoms, offs)):
            assert np.array_equal(got, single[f]), ("piecewise set", f)
        # geometric: matrices solved on the device (points) vs host-solved single frames, one source per frame
        ctx.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, goffs)
        ctx.warp_inverse_geometric_frames_device(d_out)
        ctx.sync()
        gset = _frames_to_host(ctx, d_out, gg, goffs)
        ctx.geometric_set_frames_points(0, np.concatenate(a3d), np.tile(a3s, F), ag, aoffs)
        ctx.warp_inverse_geometric_frames_device(d_out)
        ctx.sync()
        aset = _frames_to_host(ctx, d_out, ag, aoffs)
    finally:
        ctx.set_image(imgs[0])
        ctx.free(d_out)
        ctx.free(d_src)
    for f in range(F):
        ctx.set_image(imgs[f % NI])
        m = HG.solve_projective(d4s[f], s4)
        one = ctx.warp_inverse_geometric(1, m, gg[f])
        assert np.array_equal(gset[f], one), ("projective set", f)
        want, cov = B.warp_geometric(1, m, imgs[f % NI], *gg[f])
        _exact(one, want, cov, ("projective", f), _geo_coords(1, m, gg[f]))
        ma = HG.solve_affine(a3d[f], a3s).astype(np.float64)
        assert np.array_equal(aset[f], ctx.warp_inverse_geometric(0, ma, ag[f])), ("affine set", f)
    for devs in ([0], [0, 0]):
        with HG.Multi(devs) as mu:
            mu.set_sampling(BIL)
            mu.set_image(imgs[0])
            mu.piecewise_set_mesh(sp, tris, msx, msy)
            mu.warp_piecewise_batch(np.concatenate(frames), geoms)
            for f in range(F):
                ctx.set_image(imgs[0])
                ctx.piecewise_set_mesh(sp, tris, msx, msy)
                ctx.piecewise_prepare(frames[f], geoms[f])
                assert np.array_equal(mu.frame_to_host(f), ctx.warp_inverse_piecewise()), (devs, "piecewise", f)
            mu.warp_geometric_batch(1, np.concatenate(d4s), np.tile(s4, F), gg)
            for f in range(F):
                assert np.array_equal(mu.frame_to_host(f), ctx.warp_inverse_geometric(1, HG.solve_projective(d4s[f], s4), gg[f])), (devs, "projective", f)
            mu.warp_piecewise_batch_images(np.concatenate(frames), geoms, [imgs[f % NI] for f in range(F)])
            for f in range(F):
                assert np.array_equal(mu.frame_to_host(f), single[f]), (devs, "piecewise, one source per frame", f)
    ctx.set_sampling(NEAR)


def _overflow_mesh():
    n, W2, H2 = 1100, 2400, 8
    img = WL.lcg_image(W2, H2, 10)
    xs = np.linspace(0, W2, n + 1)
    sp = np.stack([np.repeat(xs, 2), np.tile([0.0, H2], n + 1)], 1).astype(np.float32).ravel()
    tr = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(n)], np.uint32).ravel()
    dp = sp.copy()
    dp[1::2] *= 1.5
    mm, md = O.minmax_xy(sp), O.minmax_xy(dp)
    g = (int(md[0]), int(md[1]), int(md[2] - md[0]), int(md[3] - md[1]))
    return img, sp, tr, dp, g, int(mm[0]), int(mm[1])


def test_map_path_redo_and_state_form_match_the_model(ctx):
    img, sp, tr, dp, g, msx, msy = _overflow_mesh()
    _, want, cov, wmap, inv = _pw_model(img, sp, dp, tr, msx, msy, g)
    r0 = ctx.redone_frames()
    _exact(_pw_warp(ctx, img, sp, tr, msx, msy, dp, g, BIL), want, cov, "row span cap overflow", _pw_coords(wmap, inv, g))
    assert ctx.redone_frames() > r0                          # (k_pw_fused flagged the frame: redone through the map)
    _exact(ctx.warp_inverse_piecewise_via_map(), want, cov, "via map", _pw_coords(wmap, inv, g))
    # reference-state form: matrices handed over by the caller, the map of the given points
    W, H = 240, 150
    img2, sp2, tris2, dp2, g2, msx2, msy2 = _pw_case(W, H, 6, 5, 7.0, 21)
    _, want2, cov2, wmap2, inv2 = _pw_model(img2, sp2, dp2, tris2, msx2, msy2, g2)
    fwd = O.piecewise_matrices(sp2, dp2, tris2)
    ctx.set_image(img2)
    got = ctx.warp_inverse_piecewise_state(np.asarray(fwd, np.float32), dp2, tris2, msx2, msy2, g2)
    _exact(got, want2, cov2, "state form", _pw_coords(wmap2, inv2, g2))
    ctx.set_sampling(NEAR)
    assert np.array_equal(ctx.warp_inverse_piecewise_state(np.asarray(fwd, np.float32), dp2, tris2, msx2, msy2, g2),
                          O.warp_inverse_piecewise(sp2, dp2, tris2, img2, msx2, msy2, *g2))


def test_mode_switching_on_one_context(ctx):
    W, H = 224, 140
    img, sp, tris, dp, geom, msx, msy = _pw_case(W, H, 7, 5, 6.0, 33)
    near, bil, cov, _, _ = _pw_model(img, sp, dp, tris, msx, msy, geom)
    m = HG.solve_projective(WL.projective_dst(W, H, 0.05), WL.corners(W, H))
    gg = tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(WL.corners(W, H), WL.projective_dst(W, H, 0.05)), W, H))
    gnear = O.warp_inverse_geometric(1, m, img, *gg)
    gbil, gcov = B.warp_geometric(1, m, img, *gg)
    for mode in (NEAR, BIL, NEAR):
        got = _pw_warp(ctx, img, sp, tris, msx, msy, dp, geom, mode)
        gget = ctx.warp_inverse_geometric(1, m, gg)
        if mode == NEAR:
            assert np.array_equal(got, near) and np.array_equal(gget, gnear)
            assert ctx.last_piecewise_kernel() != 4                  # (the fast path, whatever layout the policy picks)
        else:
            _exact(got, bil, cov, "piecewise bilinear")
            assert ctx.last_piecewise_kernel() == 4                  # (k_pw_fused<bilinear>)
            _exact(gget, gbil, gcov, "projective bilinear", _geo_coords(1, m, gg))
    # a bilinear geometric set queued, the mode switched before hg_sync: still bilinear
    offs, total = HG.pack_offsets([gg, gg])
    d_out = ctx.alloc(total)
    try:
        ctx.set_sampling(BIL)
        ctx.geometric_set_frames(1, np.concatenate([m, m]), [gg, gg], offs)
        ctx.warp_inverse_geometric_frames_device(d_out)
        ctx.set_sampling(NEAR)
        ctx.sync()
        for got in _frames_to_host(ctx, d_out, [gg, gg], offs):
            _exact(got, gbil, gcov, "queued bilinear set", _geo_coords(1, m, gg))
    finally:
        ctx.free(d_out)
    # a nearest piecewise run whose frame the kernel flags, the mode switched to bilinear before hg_sync: redone in nearest
    img2, sp2, tr2, dp2, g2, msx2, msy2 = _overflow_mesh()
    want_near = O.warp_inverse_piecewise(sp2, dp2, tr2, img2, msx2, msy2, *g2)
    offs2, total2 = HG.pack_offsets([g2])
    d2 = ctx.alloc(total2)
    try:
        ctx.set_sampling(NEAR)
        ctx.set_image(img2)
        ctx.piecewise_set_mesh(sp2, tr2, msx2, msy2)
        ctx.piecewise_set_frames(dp2, [g2], offs2)
        r0 = ctx.redone_frames()
        ctx.warp_inverse_piecewise_frames_device(d2)
        ctx.set_sampling(BIL)
        ctx.sync()
        assert ctx.redone_frames() > r0
        assert np.array_equal(ctx.to_host(d2, total2, 0).reshape(g2[3], g2[2], 4), want_near)
    finally:
        ctx.free(d2)
    ctx.set_sampling(NEAR)


def test_js_class_bilinear_equals_ctypes(ctx):
    res = GF.run_node_case("sampling_gpu.mjs", timeout=600, verdict=False)      # (its record carries hashes only)
    img = WL.lcg_image(res["W"], res["H"], res["seed"])
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    ctx.set_sampling(BIL)
    ctx.set_image(img)
    pw = [c for c in res["cases"] if c["kind"] == "piecewise"]
    assert len(pw) == 3 and len(res["batch"]) == 3
    for k, c in enumerate(pw):
        sp, dp = np.array(c["src"], np.float32), np.array(c["dst"], np.float32)
        tris = np.array(c["tris"], np.uint32)
        g = tuple(int(v) for v in c["win"])
        got = _pw_warp(ctx, img, sp, tris, int(c["min"][0]), int(c["min"][1]), dp, g, BIL)
        assert (c["w"], c["h"]) == (g[2], g[3]) and sha(got) == c["sha"], ("warp", k)
        assert res["batch"][k]["sha"] == c["sha"], ("warpBatch", k)
        _, want, cov, _, _ = _pw_model(img, sp, dp, tris, int(c["min"][0]), int(c["min"][1]), g)
        _exact(got, want, cov, ("js piecewise", k))
    for c in [c for c in res["cases"] if c["kind"] != "piecewise"]:
        kind = 0 if c["kind"] == "affine" else 1
        g = tuple(int(v) for v in c["win"])
        got = ctx.warp_inverse_geometric(kind, np.array(c["inv"], np.float64), g)
        assert sha(got) == c["sha"] == c["batchSha"], c["kind"]
    ctx.set_sampling(NEAR)


# ------------------------------------------------------------------------------------------------ routing and shape matrix
# Every bilinear k_geo_fast<KIND, 8, 1> on purpose, at widths around the 2048-pixel chunk of a wave and the 64-lane stores, short
# windows, negative window offsets and rows where the projective denominator crosses zero.  The code hg_last_geometric_kernel
# reports is 100 * KIND + 81 for k_geo_fast<KIND, 8, 1>.

WIDTHS = (1, 3, 63, 64, 65, 255, 257, 2047, 2048, 2049, 4097)
HEIGHTS = (1, 3, 5)


def _geo_case(kind_code, W, H, OW, OH):
    """(kind, matrix, window) whose source coordinates run past every edge of a W x H source."""
    g = (-7 if OW % 2 else 5, -2 if OH != 3 else 4, OW, OH)
    a, b = (W + 14.0) / OW, 0.8 * H / OW
    base = np.array([a, b, 0.013, 0.75, -5.3, -1.1 + 0.1 * H], np.float64)
    if kind_code == 0:
        m = base.astype(np.float32).astype(np.float64)
        assert (m.astype(np.float32) == m).all()
        return 0, m, g
    if kind_code == 2:
        m = base + np.array([1e-9, -3e-10, 7e-11, 1e-9, 1e-7, -3e-8])
        assert (m.astype(np.float32) != m).any()
        return 0, m, g
    if kind_code == 3:                                      # den in [~0.7, ~1.3]: the plain division range
        m = np.array([a, 0.013, -5.3, b, 0.75, -1.1 + 0.1 * H, 0.3 / (OW + 300), 0.01], np.float64)
        assert HG.projective_plain_range(m, g)
        return 1, m, g
    # kind 1: den = 1 - x / 64 is exactly 0 in column x = 64 of every row (inf), and the numerator of sx is 0 there in row 0 (NaN)
    m = np.array([-W / 256.0, 5.0, W / 4.0, b, 0.75, -1.1 + 0.1 * H, -1.0 / 64, 0.0], np.float64)
    assert not HG.projective_plain_range(m, g)
    return 1, m, g


def test_geometric_fast_bilinear_every_kind_and_shape(ctx):
    W, H = 300, 200
    img = WL.lcg_image(W, H, 41)
    ctx.set_image(img)
    ctx.set_sampling(BIL)
    seen = set()
    try:
        for kind_code in (0, 2, 3, 1):
            for OW in WIDTHS:
                for OH in HEIGHTS:
                    kind, m, g = _geo_case(kind_code, W, H, OW, OH)
                    got = ctx.warp_inverse_geometric(kind, m, g)
                    code = ctx.last_geometric_kernel()
                    assert code == 100 * kind_code + 81, (kind_code, OW, OH, code)
                    seen.add(code)
                    want, cov = B.warp_geometric(kind, m, img, *g)
                    if OW >= 65:
                        assert cov.any() and (kind_code == 1 or not cov.all()), (kind_code, OW, OH)
                    _exact(got, want, cov, ("fast", kind_code, OW, OH), _geo_coords(kind, m, g))
        assert seen == {81, 181, 281, 381}
        # (the denominator's zero column: inf and NaN coordinates, uncovered)
        sx, sy = B.geometric_coords(1, _geo_case(1, W, H, 257, 5)[1], -7, -2, 257, 5)
        assert not np.isfinite(sx[:, 71]).any() and np.isnan(sx[2, 71]) and np.isinf(sx[0, 71])
    finally:
        ctx.set_sampling(NEAR)


def test_geometric_fast_bilinear_device_solved_frame_set(ctx):
    """KIND 4: device-solved projective frames on both sides of the plain-range proof, applied to the matrices the device solved,
    one source per frame, uneven frames at out-offsets that are multiples of 4 but not of 16."""
    W, H, NI = 300, 200, 2
    imgs = [WL.lcg_image(W, H, 60 + k) for k in range(NI)]
    s4 = WL.corners(W, H)
    d4s = [WL.projective_dst(W, H, t) for t in (0.1, 0.0, 0.2, 0.05)]
    gg = [tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4s[0]), W, H)),
          (30, -3, 600, 40),                                 # reaches past the horizon x = 570: not plain
          (-9, 60, 2049, 3), (11, 190, 63, 17)]
    F = len(gg)
    offs, off = [], 4
    for g in gg:
        offs.append(off)
        off += g[2] * g[3] * 4 + 20
    assert all(o % 4 == 0 for o in offs) and any(o % 16 for o in offs)
    stride = W * H * 4 + 64
    d_src = ctx.alloc(stride * NI)
    d_out = ctx.alloc(off)
    ctx.set_sampling(BIL)
    try:
        for k in range(NI):
            ctx.to_device(d_src, imgs[k], k * stride)
        ctx.set_images_device(d_src, W, H, NI, stride)
        ctx.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, offs)
        ctx.warp_inverse_geometric_frames_device(d_out)
        ctx.sync()
        assert ctx.last_geometric_kernel() == 481
        mats = ctx.get_geometric_matrices(F)
        plain = [HG.projective_plain_range(mats[f], gg[f]) for f in range(F)]
        assert True in plain and False in plain, plain
        for f, g in enumerate(gg):
            got = ctx.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4)
            want, cov = B.warp_geometric(1, mats[f], imgs[f % NI], *g)
            assert cov.any(), f
            _exact(got, want, cov, ("device-solved set", f, plain[f]), _geo_coords(1, mats[f], g))
    finally:
        ctx.set_image(imgs[0])
        ctx.set_sampling(NEAR)
        ctx.free(d_out)
        ctx.free(d_src)


def test_piecewise_bilinear_beyond_32767_triangles(ctx):
    """36 000 triangles: ids of 32 768 and more wrap in the Int16 map (negative: uncovered), the rest sample."""
    img, sp, tris, dp, geom, msx, msy = _pw_case(400, 180, 200, 90, 3.0, 17)
    assert tris.size // 3 > 32767
    _, want, cov, wmap, inv = _pw_model(img, sp, dp, tris, msx, msy, geom)
    assert (wmap < -1).any() and cov.any()
    got = _pw_warp(ctx, img, sp, tris, msx, msy, dp, geom, BIL)
    assert ctx.last_piecewise_kernel() == 4
    _exact(got, want, cov, "Int16 wrap", _pw_coords(wmap, inv, geom))
    ctx.set_sampling(NEAR)


def test_piecewise_bilinear_flagged_frame_one_source_per_frame(ctx):
    """Frames of the row-span-overflow mesh in a set with one source per frame: k_pw_fused flags them, hg_sync redoes each through
    the map on its own source."""
    img0, sp, tr, dp, g, msx, msy = _overflow_mesh()
    W, H = img0.shape[1], img0.shape[0]
    imgs = [img0, WL.lcg_image(W, H, 11)]
    dp2 = sp.copy()
    dp2[1::2] *= 1.25
    dp3 = dp.copy()
    dp3[0::2] += 3.0
    frames = [dp, dp2, dp3]
    geoms = []
    for d in frames:
        md = O.minmax_xy(d)
        geoms.append((int(md[0]), int(md[1]), int(md[2] - md[0]), int(md[3] - md[1])))
    offs, total = HG.pack_offsets(geoms)
    stride = W * H * 4 + 256
    d_src = ctx.alloc(stride * 2)
    d_out = ctx.alloc(total)
    ctx.set_sampling(BIL)
    try:
        for k in range(2):
            ctx.to_device(d_src, imgs[k], k * stride)
        ctx.set_images_device(d_src, W, H, 2, stride)
        ctx.piecewise_set_mesh(sp, tr, msx, msy)
        ctx.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        r0 = ctx.redone_frames()
        ctx.warp_inverse_piecewise_frames_device(d_out)
        ctx.sync()
        assert ctx.redone_frames() > r0
        for f, gf in enumerate(geoms):
            got = ctx.to_host(d_out, gf[2] * gf[3] * 4, offs[f]).reshape(gf[3], gf[2], 4)
            _, want, cov, wmap, inv = _pw_model(imgs[f % 2], sp, frames[f], tr, msx, msy, gf)
            assert cov.any()
            _exact(got, want, cov, ("flagged frame, own source", f), _pw_coords(wmap, inv, gf))
    finally:
        ctx.set_image(img0)
        ctx.set_sampling(NEAR)
        ctx.free(d_out)
        ctx.free(d_src)


def test_piecewise_bilinear_fraction_one_and_border_clamp(ctx):
    """Reference-state form with chosen matrices: fractions that round to 1.0f (sx = n + 1 - 2^-30), coordinates in [W-1, W) and
    [H-1, H) whose upper taps clamp, negative coordinates under a negative source minimum.  Nearest mode pins the map and matrices."""
    W, H, nx, ny = 40, 30, 4, 3
    img = WL.lcg_image(W, H, 23)
    dp = WL.grid_points(W, H, nx, ny)
    tris = WL.grid_triangles(nx, ny)
    T = tris.size // 3
    e = 2.0 ** -30
    shifts = [(e, e), (-0.5, -0.5), (0.5, 0.25), (e, -0.5), (-e, 0.0), (0.0, e), (-1.0 + e, 0.5), (2.0, -e)]
    fwd = np.array([[1, 0, 0, 1, shifts[t % len(shifts)][0], shifts[t % len(shifts)][1]] for t in range(T)], np.float32)
    inv = np.stack([O.inverse_affine(fwd[t]) for t in range(T)])
    g = (0, 0, W, H)
    wmap = O.build_tri_map(dp, tris, W, 0, W * H)
    for msx, msy in ((0, 0), (-3, -2)):
        ctx.set_image(img)
        ctx.set_sampling(NEAR)
        near = ctx.warp_inverse_piecewise_state(fwd, dp, tris, msx, msy, g)
        assert np.array_equal(near, O.warp_inverse_piecewise_loop(wmap, inv, img, msx, msy, *g)), (msx, msy)
        ctx.set_sampling(BIL)
        got = ctx.warp_inverse_piecewise_state(fwd, dp, tris, msx, msy, g)
        want, cov = B.warp_piecewise(wmap, inv, img, msx, msy, *g)
        sx, sy, _ = B.piecewise_coords(wmap, inv, *g)
        fx = (sx - np.floor(sx)).astype(np.float32)
        assert (fx[cov] == 1.0).any()                                    # (the case's premises)
        if msx == 0:
            assert ((sx[cov] >= W - 1) & (sx[cov] < W)).any() and ((sy[cov] >= H - 1) & (sy[cov] < H)).any()
        else:
            assert (sx[cov] < 0).any() and (sy[cov] < 0).any()
        _exact(got, want, cov, ("state form edges", msx, msy), (sx, sy))
    ctx.set_sampling(NEAR)


# ------------------------------------------------------------------------------------------------ bounded fuzz
def _rand_options(c, rng):
    """The speed-only options: none of them may change a byte."""
    c.set_option("geo_windows", int(rng.choice([1, 2, 4, 8])))
    c.set_option("xcc_rotate", int(rng.choice([-1, 0, 1])))
    c.set_option("xcc", int(rng.choice([1, 2, 4, 8, 16])))
    c.set_option("phase", int(rng.choice([-1, 1, 2, 4])))
    c.set_option("tile", int(rng.choice([-1, 0, 1])))
    c.set_option("patch", int(rng.choice([-1, 0, 1])))
    c.set_option("self_spans", int(rng.choice([-1, 0, 1])))


def _rand_geometric(rng, W, H):
    kind = int(rng.integers(0, 2))
    OW, OH = int(rng.integers(1, 320)), int(rng.integers(1, 200))
    g = (int(rng.integers(-40, 40)), int(rng.integers(-40, 40)), OW, OH)
    th = rng.uniform(-0.6, 0.6)
    s = rng.uniform(0.4, 2.5) * max(W, H) / max(OW, OH)
    m6 = [s * np.cos(th), s * np.sin(th), -s * np.sin(th), s * np.cos(th), rng.uniform(-30, W), rng.uniform(-30, H)]
    if kind == 0:
        m = np.array(m6, np.float64)
        if rng.random() < 0.5:
            m = m.astype(np.float32).astype(np.float64)
        return 0, m, g
    p = rng.uniform(-1, 1, 2) * np.array([1.5 / (OW + 300), 1.5 / (OH + 300)])
    if rng.random() < 0.15:
        p[0] = -1.0 / int(rng.integers(1, max(OW, 2)))        # a denominator that reaches zero inside the window
    return 1, np.array([m6[0], m6[2], m6[4], m6[1], m6[3], m6[5], p[0], p[1]], np.float64), g


def test_bilinear_fuzz_bounded():
    """300 seeded trials, byte-exact: affine (f32-valued or not), projective, piecewise with a negative or positive source minimum,
    sources from 1 x 1 to a few hundred pixels, random speed-only options."""
    rng = np.random.default_rng(20261016)
    n = {"geo": 0, "pw": 0}
    with HG.Context(0) as c:
        c.set_sampling(BIL)
        for trial in range(300):
            _rand_options(c, rng)
            if trial % 3 < 2:
                W, H = int(rng.integers(1, 300)), int(rng.integers(1, 300))
                img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
                kind, m, g = _rand_geometric(rng, W, H)
                c.set_image(img)
                got = c.warp_inverse_geometric(kind, m, g)
                want, cov = B.warp_geometric(kind, m, img, *g)
                _exact(got, want, cov, ("fuzz geometric", trial, kind, (W, H), m.tolist(), g), _geo_coords(kind, m, g))
                n["geo"] += 1
            else:
                W, H = int(rng.integers(8, 300)), int(rng.integers(8, 300))
                nx, ny = int(rng.integers(1, 9)), int(rng.integers(1, 7))
                img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
                sp = WL.grid_points(W, H, nx, ny)
                sp = (sp + np.tile(np.float32(rng.integers(-25, 25, 2)), sp.size // 2)).astype(np.float32)
                tris = WL.grid_triangles(nx, ny)
                dp = WL.sin_dst(sp, float(rng.uniform(0, 12)), int(rng.integers(4, 12)))
                dp = (dp * np.float32(rng.uniform(0.6, 1.6))).astype(np.float32)
                geom = WL.piecewise_geom(dp)
                msx, msy = WL.src_min(sp)
                _, want, cov, wmap, inv = _pw_model(img, sp, dp, tris, msx, msy, geom)
                got = _pw_warp(c, img, sp, tris, msx, msy, dp, geom, BIL)
                _exact(got, want, cov, ("fuzz piecewise", trial, (W, H), (nx, ny), (msx, msy)), _pw_coords(wmap, inv, geom))
                n["pw"] += 1
    assert n["geo"] == 200 and n["pw"] == 100
