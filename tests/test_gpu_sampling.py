"""Bilinear sampling of the inverse warps on the GPU (include/hgwarp.h, HG_SAMPLE_BILINEAR) against the numpy model of
tests/hgtest/bilinear.py.  The model's per-pixel triangle ids and inverse matrices come from the CPU oracle (taps), never from the
library under test."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import bilinear as B             # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
BIL, NEAR = HG.SAMPLE_BILINEAR, HG.SAMPLE_NEAREST


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def _close(got, want, cov, what):
    """<= 1 per channel, >= 99.9 % of covered channels exact, coverage exact, uncovered all-zero."""
    assert got.shape == want.shape, what
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max(initial=0) <= 1, (what, int(d.max()))
    if cov.any():
        assert (d[cov] == 0).mean() >= 0.999, (what, float((d[cov] == 0).mean()))
    assert not got[~cov].any(), what
    assert np.array_equal(got.any(-1), want.any(-1)), what


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
    _close(ctx.warp_inverse_geometric(0, m, g), want, cov, "affine")
    W2, H2 = 1920, 1080                                       # C2
    img2 = WL.lcg_image(W2, H2, 2)
    s4, d4 = WL.corners(W2, H2), WL.projective_dst(W2, H2)
    g2 = tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W2, H2))
    m2 = HG.solve_projective(d4, s4)
    ctx.set_image(img2)
    want, cov = B.warp_geometric(1, m2, img2, *g2)
    _close(ctx.warp_inverse_geometric(1, m2, g2), want, cov, "projective C2")
    cfg = WL.CONFIGS["C3"]                                    # C3: 4K, 200 triangles
    img3, sp, tris, dp, geom, msx, msy = _pw_case(cfg["W"], cfg["H"], cfg["nx"], cfg["ny"], cfg["A"], 3)
    _, want, cov, _, _ = _pw_model(img3, sp, dp, tris, msx, msy, geom)
    _close(_pw_warp(ctx, img3, sp, tris, msx, msy, dp, geom, BIL), want, cov, "piecewise C3")
    assert ctx.last_piecewise_kernel() == 4
    # source points with a negative minimum: coverage on the minSrc window, taps clamped to the image
    img4 = WL.lcg_image(120, 90, 8)
    sp4 = (WL.grid_points(120, 90, 5, 3) - np.tile(np.float32([17, 9]), 24)).astype(np.float32)
    tris4 = WL.grid_triangles(5, 3)
    dp4 = WL.sin_dst(sp4, 3.0, 9)
    geom4 = WL.piecewise_geom(dp4)
    msx4, msy4 = WL.src_min(sp4)
    assert msx4 < 0 and msy4 < 0
    _, want, cov, _, _ = _pw_model(img4, sp4, dp4, tris4, msx4, msy4, geom4)
    _close(_pw_warp(ctx, img4, sp4, tris4, msx4, msy4, dp4, geom4, BIL), want, cov, "piecewise, negative source minimum")
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
        _, want, cov, _, _ = _pw_model(imgs[f % NI], sp, frames[f], tris, msx, msy, geoms[f])
        _close(single[f], want, cov, ("piecewise single", f))
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
        _close(one, want, cov, ("projective", f))
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
    _close(_pw_warp(ctx, img, sp, tr, msx, msy, dp, g, BIL), want, cov, "row span cap overflow")
    assert ctx.redone_frames() > r0                          # (k_pw_fused flagged the frame: redone through the map)
    _close(ctx.warp_inverse_piecewise_via_map(), want, cov, "via map")
    # reference-state form: matrices handed over by the caller, the map of the given points
    W, H = 240, 150
    img2, sp2, tris2, dp2, g2, msx2, msy2 = _pw_case(W, H, 6, 5, 7.0, 21)
    _, want2, cov2, wmap2, inv2 = _pw_model(img2, sp2, dp2, tris2, msx2, msy2, g2)
    fwd = O.piecewise_matrices(sp2, dp2, tris2)
    ctx.set_image(img2)
    got = ctx.warp_inverse_piecewise_state(np.asarray(fwd, np.float32), dp2, tris2, msx2, msy2, g2)
    _close(got, want2, cov2, "state form")
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
            _close(got, bil, cov, "piecewise bilinear")
            assert ctx.last_piecewise_kernel() == 4                  # (k_pw_fused<bilinear>)
            _close(gget, gbil, gcov, "projective bilinear")
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
            _close(got, gbil, gcov, "queued bilinear set")
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
    node = shutil.which("node")
    addon = os.path.join(ROOT, "homography.js_amd", "lib", "hgwarp.node")
    assert node is not None and os.path.exists(addon), "node and the N-API addon are needed on a GPU box"
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "sampling_gpu.mjs")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
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
        _close(got, want, cov, ("js piecewise", k))
    for c in [c for c in res["cases"] if c["kind"] != "piecewise"]:
        kind = 0 if c["kind"] == "affine" else 1
        g = tuple(int(v) for v in c["win"])
        got = ctx.warp_inverse_geometric(kind, np.array(c["inv"], np.float64), g)
        assert sha(got) == c["sha"] == c["batchSha"], c["kind"]
    ctx.set_sampling(NEAR)
