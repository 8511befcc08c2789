"""Bilinear sampling (include/hgwarp.h, HG_SAMPLE_BILINEAR) without a GPU: the C ABI symbols, the numpy model of the semantics on
hand-computed cases, and the JavaScript class's {sampling} option over a mock addon that records the addon calls."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import bilinear as B             # noqa: E402

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "homography.js_amd", "lib", "hgwarp.node")


def test_sampling_symbols_resolve():
    L = C.CDLL(HG.LIB_PATH)
    for n in ("hg_set_sampling", "hg_get_sampling", "hg_multi_set_sampling"):
        assert hasattr(L, n), n
        assert n in HG.EXPORTS
    assert (HG.SAMPLE_NEAREST, HG.SAMPLE_BILINEAR) == (0, 1)
    with open(os.path.join(ROOT, "include", "hgwarp.h")) as f:
        h = f.read()
    assert "HG_SAMPLE_NEAREST = 0" in h and "HG_SAMPLE_BILINEAR = 1" in h


def test_sampling_calls_reject_null_handles():
    L = HG.lib()
    m = C.c_int(7)
    assert L.hg_set_sampling(None, 1) == 1                   # HG_ERR_INVALID
    assert L.hg_get_sampling(None, C.byref(m)) == 1 and m.value == 7
    assert L.hg_multi_set_sampling(None, 0) == 1


def _img(px):
    return np.asarray(px, np.uint8).reshape(2, 2, 4)


def test_model_centre_sample_is_the_mean_of_four_pixels():
    img = _img([[0, 10, 20, 255], [100, 30, 0, 255], [50, 70, 9, 0], [250, 90, 1, 255]])
    out = B.sample(img, np.array([0.5]), np.array([0.5]), np.array([True]))
    mean = np.floor(img.reshape(4, 4).astype(np.float64).mean(0) + 0.5)
    assert np.array_equal(out[0], mean.astype(np.uint8)), (out, mean)
    # a quarter step: weights 9/16, 3/16, 3/16, 1/16 on one channel
    out = B.sample(img, np.array([0.25]), np.array([0.25]), np.array([True]))
    assert out[0, 0] == int(np.floor(0 * 9 / 16 + 100 * 3 / 16 + 50 * 3 / 16 + 250 / 16 + 0.5))


def test_model_integer_coordinates_are_the_nearest_pixel():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    ys, xs = np.mgrid[0:5, 0:7].astype(np.float64)
    out = B.sample(img, xs, ys, np.ones(xs.shape, bool))
    assert np.array_equal(out, img)


def test_model_edges_clamp_and_uncovered_stay_zero():
    img = _img([[10, 20, 30, 40], [200, 100, 50, 255], [0, 0, 0, 0], [255, 255, 255, 255]])
    # right column: x0 = 1, x0 + 1 clamps to 1 -> pure vertical blend of the right column
    out = B.sample(img, np.array([1.75]), np.array([0.5]), np.array([True]))
    assert np.array_equal(out[0], [228, 178, 153, 255])                 # floor((p01 + p11) / 2 + 0.5)
    # bottom row, both clamps: the corner pixel itself
    out = B.sample(img, np.array([1.9]), np.array([1.9]), np.array([True]))
    assert np.array_equal(out[0], [255, 255, 255, 255])
    # negative coordinates (piecewise with a negative source minimum): taps clamp to column / row 0
    out = B.sample(img, np.array([-0.5]), np.array([-3.25]), np.array([True]))
    assert np.array_equal(out[0], [10, 20, 30, 40])
    out = B.sample(img, np.array([0.5, np.nan]), np.array([0.5, 0.0]), np.array([False, False]))
    assert not out.any()


def test_model_geometric_coverage_is_the_nearest_test():
    img = np.full((4, 6, 4), 77, np.uint8)
    out, cov = B.warp_geometric(0, [1, 0, 0, 1, -2.5, -1.0], img, 0, 0, 10, 7)    # sx = x - 2.5, sy = y - 1
    xs = np.arange(10) - 2.5
    ys = np.arange(7) - 1.0
    want = (xs[None, :] >= 0) & (xs[None, :] < 6) & (ys[:, None] >= 0) & (ys[:, None] < 4)
    assert np.array_equal(cov, want)
    assert (out[cov] == 77).all() and not out[~cov].any()


def test_model_piecewise_taps_do_not_subtract_the_source_minimum():
    img = np.zeros((3, 4, 4), np.uint8)
    img[..., 0] = np.arange(12, dtype=np.uint8).reshape(3, 4) * 10
    inv = np.array([[1, 0, 0, 1, 0, 0]], np.float32)                     # identity
    out, cov = B.warp_piecewise(np.zeros(4 * 3, np.int16), inv, img, 2, 1, 0, 0, 4, 3)
    # covered: 2 <= x < 6, 1 <= y < 4 (minSrc bounds); the pixels read are img[y, x] of the unshifted image (clamped)
    assert np.array_equal(cov, np.array([[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]], bool))
    assert out[1, 2, 0] == img[1, 2, 0] and out[2, 3, 0] == img[2, 3, 0] and not out[~cov].any()


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is missing")
def test_js_class_sampling_option_over_the_mock_addon():
    """{sampling: 'bilinear'}: same-size affine and a 1.1x piecewise shrink hit no forward entry point (warp and warpBatch), the mode
    reaches the addon before the first warp (one context, and the {devices} multi-context), switching on a live instance reaches the
    context, the default makes no sampling call at all, and a bad mode throws a bare string."""
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "sampling_class.mjs")], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_sampling_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["failures"] == [] and p.returncode == 0
    assert res["checks"] >= 30


# ------------------------------------------------------------------------------------------------ two references for the model
# The vectorised model (tests/hgtest/bilinear.py) and the kernels came in one change.  Here the model is held against a scalar
# form written from the header's text (include/hgwarp.h, hg_set_sampling), one np.float32 operation per step, and against exact
# rational interpolation.

def _scalar_sample(img, sx, sy):
    """One position, straight from the header: x0 = floor(sx), fx = (float)(sx - x0), clamped taps, the f32 blend in its written
    order, min(255, floor(v + 0.5f))."""
    H, W = img.shape[:2]
    x0, y0 = float(math.floor(sx)), float(math.floor(sy))
    fx, fy = np.float32(sx - x0), np.float32(sy - y0)                    # (the f64 difference is exact)
    ix, iy = int(x0), int(y0)
    c0, c1 = min(max(ix, 0), W - 1), min(max(ix + 1, 0), W - 1)
    r0, r1 = min(max(iy, 0), H - 1), min(max(iy + 1, 0), H - 1)
    one, half = np.float32(1.0), np.float32(0.5)
    gx = one - fx
    gy = one - fy
    out = []
    for ch in range(4):
        a, b = np.float32(img[r0, c0, ch]), np.float32(img[r0, c1, ch])
        c, d = np.float32(img[r1, c0, ch]), np.float32(img[r1, c1, ch])
        top = a * gx
        top = top + b * fx
        top = top * gy
        bot = c * gx
        bot = bot + d * fx
        bot = bot * fy
        v = top + bot
        out.append(int(min(np.float32(255.0), np.floor(v + half))))
    return out


def _exact(img, sx, sy):
    """Exact rational bilinear value of every channel at (sx, sy) (the exact fractions of the f64 coordinate, clamped taps)."""
    H, W = img.shape[:2]
    X, Y = Fraction(sx), Fraction(sy)
    x0, y0 = math.floor(X), math.floor(Y)
    fx, fy = X - x0, Y - y0
    c0, c1 = min(max(x0, 0), W - 1), min(max(x0 + 1, 0), W - 1)
    r0, r1 = min(max(y0, 0), H - 1), min(max(y0 + 1, 0), H - 1)
    return [(int(img[r0, c0, ch]) * (1 - fx) + int(img[r0, c1, ch]) * fx) * (1 - fy) +
            (int(img[r1, c0, ch]) * (1 - fx) + int(img[r1, c1, ch]) * fx) * fy for ch in range(4)]


def _edge_coords(W, H, rng):
    """Hand-picked coordinates: integers, n + 0.5 ties, fractions that round to 1.0f, the clamped right / bottom column and row,
    negative coordinates (a piecewise mesh with a negative source minimum), all combined with each other."""
    def axis(n):
        v = [0.0, float(n - 1), n - 0.5, n - 1e-9, n - 2.0 ** -40, -0.25, -1.0, -2.5, -7.75]
        for k in sorted(set([0, n // 2, max(n - 2, 0), n - 1])):
            v += [float(k), k + 0.5, k + 1 - 2.0 ** -30, k + 1 - 2.0 ** -25, k + 2.0 ** -30, k + 0.25, k + 0.75]
        v += list(n - 1 + rng.random(8))                   # [n-1, n): the upper tap clamps
        return np.array(v)
    xs, ys = axis(W), axis(H)
    return np.repeat(xs, ys.size), np.tile(ys, xs.size)


def _random_coords(W, H, n, rng):
    xs = rng.uniform(-3.0, W, n)
    ys = rng.uniform(-3.0, H, n)
    q = rng.random(n) < 0.3                                # a third on coarse grids: exact ties of the blend (v = k + 0.5)
    xs[q] = np.round(xs[q] * 4) / 4
    ys[q] = np.round(ys[q] * 2) / 2
    return xs, ys


_SOURCES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (64, 3), (3, 64), (250, 130)]


def test_model_equals_the_scalar_form_of_the_header():
    rng = np.random.default_rng(2026)
    n_random = 0
    for k, (W, H) in enumerate(_SOURCES):
        img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        if k % 2:                                          # saturated and near-saturated channels: the min(255, .) clamp
            img[..., 1] = 255
            img[..., 2] = rng.integers(250, 256, (H, W), dtype=np.uint8)
        ex, ey = _edge_coords(W, H, rng)
        rx, ry = _random_coords(W, H, 12500, rng)
        n_random += rx.size
        sx, sy = np.concatenate([ex, rx]), np.concatenate([ey, ry])
        got = B.sample(img, sx, sy, np.ones(sx.shape, bool))
        for i in range(sx.size):
            want = _scalar_sample(img, float(sx[i]), float(sy[i]))
            assert list(got[i]) == want, ((W, H), float(sx[i]), float(sy[i]), list(got[i]), want)
    assert n_random >= 100000


def test_model_against_exact_rational_interpolation():
    """Within 1 everywhere; equal wherever the exact value is at least 2^-8 away from a .5 boundary (round half up)."""
    rng = np.random.default_rng(77)
    margin = Fraction(1, 256)
    checked = 0
    for k, (W, H) in enumerate(_SOURCES):
        img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        ex, ey = _edge_coords(W, H, rng)
        rx, ry = _random_coords(W, H, 2500, rng)
        sx, sy = np.concatenate([ex, rx]), np.concatenate([ey, ry])
        got = B.sample(img, sx, sy, np.ones(sx.shape, bool))
        for i in range(sx.size):
            for ch, v in enumerate(_exact(img, float(sx[i]), float(sy[i]))):
                r = math.floor(v + Fraction(1, 2))
                g = int(got[i, ch])
                assert abs(g - r) <= 1, ((W, H), float(sx[i]), float(sy[i]), ch, g, v)
                if abs(v - math.floor(v) - Fraction(1, 2)) >= margin:
                    assert g == r, ((W, H), float(sx[i]), float(sy[i]), ch, g, float(v))
                checked += 1
    assert checked >= 80000


def test_model_rounds_half_up_and_fraction_to_one_takes_the_right_tap():
    img = np.zeros((2, 3, 4), np.uint8)
    img[0, :, 0] = [0, 1, 2]
    img[1, :, 0] = [4, 6, 200]
    one = np.ones(1, bool)
    # an exact tie v = 0.5: round half up gives 1 (round half even would give 0)
    assert B.sample(img, np.array([0.5]), np.array([0.0]), one)[0, 0] == 1
    assert B.sample(img, np.array([1.5]), np.array([0.0]), one)[0, 0] == 2           # v = 1.5 -> 2 under both
    assert B.sample(img, np.array([0.25]), np.array([0.5]), one)[0, 0] == 2          # v = 0 * .375 + 1 * .125 + 4 * .375 + 6 * .125 = 2.375
    assert B.sample(img, np.array([0.75]), np.array([0.5]), one)[0, 0] == 3          # v = 0 * .125 + 1 * .375 + 4 * .125 + 6 * .375 = 3.125
    # fx = (float)(1 - 2^-30) == 1.0f: the blend is all right tap, though x0 stays 0
    assert B.sample(img, np.array([1 - 2.0 ** -30]), np.array([1.0]), one)[0, 0] == 6
    # the right tap of the last column clamps to that column
    assert B.sample(img, np.array([2.5]), np.array([1.0]), one)[0, 0] == 200
