"""The generic kernels of the inverse warps, in both sampling modes: k_geo<kind, S> (sources of 2^20 pixels or more in width or
height, sources of 2 GiB or more) and, on a source of 2 GiB or more, k_pw_fused / k_pw_from_map with 64-bit source indexing.
Nearest mode is compared byte for byte with the CPU oracle, bilinear mode with the numpy model of tests/hgtest/bilinear.py, and
hg_last_geometric_kernel proves which kernel ran (1000 + 10 * kind + S for k_geo<kind, S>)."""
import os
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
BIG = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        first = [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ; (row, col, got, want): {first}")


def _want(kind, m, img, g, mode):
    if mode == NEAR:
        return O.warp_inverse_geometric(kind, m, img, *g)
    return B.warp_geometric(kind, m, img, *g)[0]


def _both_modes(ctx, kind, m, img, g, what):
    """One window in nearest and bilinear mode on the source already set; asserts k_geo<kind, S> ran and the bytes."""
    for mode in (NEAR, BIL):
        ctx.set_sampling(mode)
        got = ctx.warp_inverse_geometric(kind, m, g)
        assert ctx.last_geometric_kernel() == 1000 + 10 * kind + mode, (what, mode, ctx.last_geometric_kernel())
        want = _want(kind, m, img, g, mode)
        _same(got, want, (what, "bilinear" if mode else "nearest"))
        assert want.any(), what
    ctx.set_sampling(NEAR)


# Matrices for a wide (W = 2^20, H = 3) source; the tall source (W = 3, H = 2^20) takes them with x and y exchanged.
_WIDE = {
    "affine f32": (0, np.array([1.0, 2.0 ** -19, 2.0 ** -7, 0.625, -3.5, -1.25])),
    "affine doubles": (0, np.array([1.0000000123, 1.7e-7, 0.0123456789, 0.6180339887, -3.3333333, -1.4142135])),
    "projective": (1, np.array([1.0, 0.01, -3.0, 1e-7, 0.7, -1.2, 1e-9, 0.02])),
}


def _transpose(kind, m):
    if kind == 0:                                           # sx = m0 x + m2 y + m4, sy = m1 x + m3 y + m5
        return np.array([m[3], m[2], m[1], m[0], m[5], m[4]])
    return np.array([m[4], m[3], m[5], m[1], m[0], m[2], m[7], m[6]])


def _windows(W, H, wide):
    """Windows reaching past every edge: the first and the last columns (rows) of the long side, and one in the middle."""
    if wide:
        return [(-20, -2, 300, 8), (W - 280, -2, 300, 8), (W // 2 + 3, -1, 257, 6)]
    return [(-2, -20, 8, 300), (-2, H - 280, 8, 300), (-1, H // 2 + 3, 6, 257)]


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "tall"])
def test_generic_geometric_windows(ctx, wide):
    W, H = (BIG, 3) if wide else (3, BIG)
    img = O.lcg_image(W, H, 5 if wide else 6)
    ctx.set_image(img)
    for name, (kind, m) in _WIDE.items():
        mm = m if wide else _transpose(kind, m)
        if name == "affine f32":
            assert (mm.astype(np.float32) == mm).all()
        for g in _windows(W, H, wide):
            _both_modes(ctx, kind, mm, img, g, (name, g))


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "tall"])
def test_generic_geometric_frame_set_uneven_offsets_two_sources(ctx, wide):
    """Uneven frames at out-offsets that are multiples of 4 but not of 16 (the per-pixel store branch), two per-frame sources."""
    W, H = (BIG, 3) if wide else (3, BIG)
    imgs = [O.lcg_image(W, H, 70 + k) for k in range(2)]
    wins = _windows(W, H, wide)
    for name, (kind, m) in _WIDE.items():
        mm = m if wide else _transpose(kind, m)
        m8 = np.zeros(8)
        m8[:mm.size] = mm
        gg = wins + [wins[0]]
        F = len(gg)
        offs, off = [], 4
        for g in gg:
            offs.append(off)
            off += g[2] * g[3] * 4 + 4
        assert any(o % 16 for o in offs) and all(o % 4 == 0 for o in offs)
        stride = W * H * 4 + 64
        d_src = ctx.alloc(2 * stride)
        d_out = ctx.alloc(off)
        try:
            for k in range(2):
                ctx.to_device(d_src, imgs[k], k * stride)
            ctx.set_images_device(d_src, W, H, 2, stride)
            for mode in (NEAR, BIL):
                ctx.set_sampling(mode)
                ctx.geometric_set_frames(kind, np.tile(m8, F), gg, offs)
                ctx.warp_inverse_geometric_frames_device(d_out)
                ctx.sync()
                assert ctx.last_geometric_kernel() == 1000 + 10 * kind + mode
                for f, g in enumerate(gg):
                    got = ctx.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4)
                    _same(got, _want(kind, mm, imgs[f % 2], g, mode), (name, "set", f, mode))
        finally:
            ctx.set_sampling(NEAR)
            ctx.set_image(imgs[0])
            ctx.free(d_out)
            ctx.free(d_src)


def test_generic_geometric_tall_identity_window(ctx):
    """2^20 output rows on the generic path: (2^20 + 3) / 4 = 262 144 workgroups in grid dimension y."""
    W, H = 3, BIG
    img = O.lcg_image(W, H, 9)
    ctx.set_image(img)
    m = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    for mode in (NEAR, BIL):
        ctx.set_sampling(mode)
        got = ctx.warp_inverse_geometric(0, m, (0, 0, W, H))
        assert ctx.last_geometric_kernel() == 1000 + mode
        _same(got, img, ("identity", mode))
    ctx.set_sampling(NEAR)
    assert np.array_equal(O.warp_inverse_geometric(0, m, img, 0, 0, W, H), img)


# ------------------------------------------------------------------------------------------------ a source of 2^31 bytes or more
HW, HH = 32768, 16448                                      # 2.16 GB: rows from 16384 on start above byte 2^31


@pytest.fixture(scope="module")
def huge():
    """One 2 GiB+ source on its own context, built once, freed at the end of the module."""
    img = O.lcg_image(HW, HH, 3)
    assert img.nbytes >= (1 << 31)
    c = HG.Context(0)
    c.set_image(img)
    yield c, img
    c.close()
    del img


def test_huge_source_geometric(huge):
    c, img = huge
    assert (HH - 40) * HW * 4 > (1 << 31)
    wins = [(-9, HH - 40, 300, 48), (HW - 200, HH - 30, 260, 40), (-7, -3, 270, 20)]      # the last rows (past the bottom and right), the first
    mats = {"affine f32": (0, np.array([1.0, 0.0, 2.0 ** -7, 1.0, -3.5, 0.5])),
            "affine doubles": (0, np.array([1.0000000123, 1.7e-7, 0.0123456789, 0.9999998765, -3.3333333, 0.4142135])),
            "projective": (1, np.array([1.0, 0.01, -3.0, 1e-7, 1.0, 0.3, 1e-9, 1e-8]))}
    for name, (kind, mm) in mats.items():
        for g in wins:
            _both_modes(c, kind, mm, img, g, ("huge", name, g))


def test_huge_source_piecewise(huge):
    """A mesh on the bottom rows of the source (byte offsets above 2^31): pw_fast_ok fails, k_pw_fused runs; the via-map form
    (k_pw_from_map) and the reference-state form too."""
    c, img = huge
    x0, y0 = 1000, HH - 60
    sp = (WL.grid_points(240, 60, 6, 3) + np.tile(np.float32([x0, y0]), 28)).astype(np.float32)
    tris = WL.grid_triangles(6, 3)
    dp = WL.sin_dst((sp - np.tile(np.float32([x0, y0]), 28)).astype(np.float32), 4.0, 8)
    geom = WL.piecewise_geom(dp)
    msx, msy = WL.src_min(sp)
    assert msy * HW * 4 >= (1 << 31)
    near, wmap, fwd, inv = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom, taps=True)
    bil, cov = B.warp_piecewise(wmap, inv, img, msx, msy, *geom)
    assert cov.any() and near.any()
    c.piecewise_set_mesh(sp, tris, msx, msy)
    for mode, want in ((NEAR, near), (BIL, bil)):
        c.set_sampling(mode)
        c.piecewise_prepare(dp, geom)
        _same(c.warp_inverse_piecewise(), want, ("piecewise", mode))
        assert c.last_piecewise_kernel() == 4
        _same(c.warp_inverse_piecewise_via_map(), want, ("via map", mode))
        _same(c.warp_inverse_piecewise_state(np.asarray(fwd, np.float32), dp, tris, msx, msy, geom), want, ("state form", mode))
    c.set_sampling(NEAR)
