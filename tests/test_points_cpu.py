"""CPU-side checks of the point lists (include/hgwarp.h, hg_points_*): the header declares and the library exports the entry points, and --
without any GPU -- the numpy model of tests/hgtest/points.py is pinned from both sides: its to-source half to the field model
(tests/hgtest/field.py, itself pinned to the reference) at every integer pixel, its to-output half to the oracle's forward warps by painting
what it returns, and the cell rule at its ties and non-finite inputs."""
import json
import os
import re
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
from hgtest import field as FM               # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import points as P               # noqa: E402
from hgtest import workloads as WL           # noqa: E402

NEW = ["hg_points_to_source_geometric_frames_device", "hg_points_to_source_piecewise_frames_device",
       "hg_points_to_output_geometric_batch_device", "hg_points_to_output_piecewise_batch_device"]
W, H = 160, 96
WIN = (-3, -5, W + 9, H + 6)                 # the window of test_gpu_sampling
CAP = 0.005                                  # share of the mapped pixels a raster anchor may paint at the f64 position instead


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def grid(x0, y0, w, h):
    """Every integer position of a w x h window from (x0, y0), raster order, (n, 2) float32."""
    x, y = np.meshgrid(np.arange(w) + x0, np.arange(h) + y0)
    return np.stack([x, y], -1).reshape(-1, 2).astype(np.float32)


def test_header_declares_and_library_exports_the_points_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in HG.EXPORTS, name
    assert "hg_points_to_source_geometric_frames_device" in text[text.index("#define HG_VERSION"):text.index("#define HG_VERSION") + 600]
    for name in ("points_to_source_geometric_frames_device", "points_to_source_piecewise_frames_device",
                 "points_to_output_geometric_batch_device", "points_to_output_piecewise_batch_device"):
        assert hasattr(HG.Context, name), name


# ------------------------------------------------------------------------------------------------ to source == the coords field
def _sin_mesh():
    sp, tris = WL.grid_points(W, H, 6, 4), WL.grid_triangles(6, 4)
    dp = WL.sin_dst(sp, 7.0, 8)
    return sp, tris, dp, WL.src_min(sp)


GEO_INV = {
    "affine": (0, [0.9, 0.05, -0.1, 1.1, 3.25, -2.5]),
    "projective": (1, [1.02, 0.03, -4.0, -0.02, 0.97, 2.5, 1e-4, -2e-4]),
}


@pytest.mark.parametrize("name", sorted(GEO_INV))
def test_to_source_geometric_model_is_the_coords_field_at_integer_pixels(name):
    kind, m = GEO_INV[name]
    sx, sy = B.geometric_coords(kind, m, *WIN)
    want = FM.coords_field(sx, sy, np.ones(sx.shape, bool), W, H)
    got = P.to_source_geometric(kind, m, grid(0, 0, WIN[2], WIN[3]), WIN, W, H)
    nan = _u32(want)[..., 0] == FM.NAN_BITS
    assert nan.any() and not nan.all()
    assert np.array_equal(_u32(got), _u32(want).reshape(-1, 2))


def test_to_source_piecewise_model_is_the_coords_field_at_integer_pixels():
    sp, tris, dp, (msx, msy) = _sin_mesh()
    img = WL.lcg_image(W, H, 5)
    for g in (WL.piecewise_geom(dp), WIN):
        _, wmap, _, inv = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *g, taps=True)
        sx, sy, valid = B.piecewise_coords(wmap, inv, *g)
        want = FM.coords_field(sx, sy, valid, W, H, msx, msy)
        pts = grid(0, 0, g[2], g[3])
        assert np.array_equal(_u32(P.to_source_piecewise(wmap, inv, pts, g, W, H, msx, msy)), _u32(want).reshape(-1, 2))
        assert np.array_equal(_u32(P.to_source_piecewise_mesh(sp, dp, tris, pts, g, W, H, msx, msy)), _u32(want).reshape(-1, 2))
        nan = _u32(want)[..., 0] == FM.NAN_BITS
        assert nan.any() and not nan.all()


# ------------------------------------------------------------------------------------------------ raster anchor
GEO_FWD = {
    # name -> (kind, forward matrix, window, rows that may be painted at the f64 position: 0 for the integer translation)
    "translation": (0, [1, 0, 0, 1, 7, -4], (2, -6, W + 3, H + 4), 0),
    "affine": (0, [0.8317, 0.1093, -0.0719, 0.9133, 5.3071, 2.2113], (0, 0, W, H), None),
    "projective": (1, [0.9013, 0.0417, 3.0331, -0.0309, 0.8821, 4.0173, 2.1e-4, 1.3e-4], (0, 0, W, H), None),
}


@pytest.mark.parametrize("name", sorted(GEO_FWD))
def test_raster_anchor_geometric(name):
    kind, m, g, exact_zero = GEO_FWD[name]
    m = np.array(m, np.float64)
    img = WL.lcg_image(W, H, 7)
    pts = grid(0, 0, W, H)
    res = P.to_output_geometric(kind, m, pts, g, W, H)
    x, y, ok = P.to_output_geometric(kind, m, pts, g, W, H, raw=True)
    assert ok.all()
    got, left_out = P.paint(res, img.reshape(-1, 4), g[2], g[3], exact=(x, y))
    print(name, "painted at the f64 position:", left_out, "of", int(ok.sum()))
    assert left_out <= CAP * ok.sum(), (left_out, int(ok.sum()))
    if exact_zero is not None:
        assert left_out == exact_zero
    want = O.warp_forward_geometric(kind, m, img, *g)
    assert want.any() and np.array_equal(got, want), name


def test_raster_anchor_piecewise():
    sp, tris, dp, (msx, msy) = _sin_mesh()
    img = WL.lcg_image(W, H, 9)
    mm = O.minmax_xy(sp)
    maxx, maxy = int(mm[2]), int(mm[3])
    g = WL.piecewise_geom(dp)
    fmap = P.forward_map(sp, tris, msx, msy, maxx, maxy)
    fwd = O.piecewise_matrices(sp, dp, tris)
    pts = grid(msx, msy, maxx - msx, maxy - msy)
    res = P.to_output_piecewise(fmap, fwd, pts, g, msx, msy, maxx, maxy)
    x, y, ok = P.to_output_piecewise(fmap, fwd, pts, g, msx, msy, maxx, maxy, raw=True)
    assert ok.sum() > 0.9 * ok.size
    p64 = pts.astype(np.int64)
    s = p64[:, 1] * W + p64[:, 0]                                        # :960, all inside the W x H array here
    assert (s >= 0).all() and (s < W * H).all()
    got, left_out = P.paint(res, img.reshape(-1, 4)[s], g[2], g[3], exact=(x, y))
    assert left_out <= CAP * ok.sum(), (left_out, int(ok.sum()))
    want = O.warp_forward_piecewise(fmap, fwd, img, msx, msy, maxx, maxy, *g)
    assert want.any() and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ cell rule
def test_cell_rule():
    ident = [1, 0, 0, 1, 0, 0]
    g = (0, 0, 10, 6)
    pts = np.float32([[-0.5, 0], [9.5, 0], [9.49, 0], [3.5, 2], [3.49, 2.5], [0, -0.5], [0, 5.5], [-0.51, 0],
                      [np.nan, 1], [1, np.nan], [np.inf, 1], [-np.inf, 1], [1, np.inf], [1e30, 1], [1, -1e30]])
    cx, cy = P.cells(pts)
    assert cx[0] == 0 and cx[1] == 10 and cx[2] == 9 and cx[3] == 4 and cx[4] == 3 and cy[4] == 3 and cy[5] == 0 and cy[6] == 6 and cx[7] == -1
    got = P.to_source_geometric(0, ident, pts, g, 100, 100)
    nan = (_u32(got) == P.NAN_BITS).all(1)
    # -0.5 belongs to cell 0 but its own coordinate fails :1001 under the identity; shifted by one pixel it maps
    assert nan.tolist() == [True, True, False, False, False, True, True, True] + [True] * 7
    shifted = P.to_source_geometric(0, [1, 0, 0, 1, 1, 1], pts, g, 100, 100)
    snan = (_u32(shifted) == P.NAN_BITS).all(1)
    assert snan.tolist() == [False, True, False, False, False, False, True, True] + [True] * 7
    assert shifted[0].tolist() == [0.5, 1.0] and shifted[5].tolist() == [1.0, 0.5]
    # the same rule in the source domain of the to-output forms
    out = P.to_output_geometric(0, ident, pts, (2, 3, 4, 4), 10, 6)
    onan = (_u32(out) == P.NAN_BITS).all(1)
    assert onan.tolist() == [False, True, False, False, False, False, True, True] + [True] * 7
    assert out[0].tolist() == [-2.5, -3.0]                               # reported wherever it falls


# ------------------------------------------------------------------------------------------------ the drop-in class on a mock addon
def test_js_class_transform_points_on_the_mock():
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed")
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "points_class.mjs")], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_points_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert p.returncode == 0 and res["ok"] and not res["fails"], (res["fails"], p.stderr[-2000:])
