"""Bilinear sampling (include/hgwarp.h, HG_SAMPLE_BILINEAR) without a GPU: the C ABI symbols, the numpy model of the semantics on
hand-computed cases, and the JavaScript class's {sampling} option over a mock addon that records the addon calls."""
import ctypes as C
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
