"""The model of the forward source field (tests/hgtest/fwd_field.py), judged without a GPU before it judges a kernel: on every geometric
case it equals the classifier's own last-writer resolution, and on every case, geometric and piecewise, gathering the case's own picture
through it reproduces the oracle's forward warp byte for byte -- holes, overwritten pixels, alias columns and winners that read outside the
source included."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from hgtest import fwd_edges as F
from hgtest import fwd_field as M
from hgtest import hip
from hgtest import oracle as O

HG = hip.load()
GEO = F.geometric_cases()
PW = F.piecewise_cases()
FUZZ_SEED, FUZZ_DRAWS = 2025, 420          # (tests/test_gpu_forward_field.py runs the same draws)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(GEO))
def test_geometric_model_is_the_classifier_and_gathers_the_warp(name):
    c = GEO[name]
    field = M.geometric_case(c)
    assert field.shape == (c["geom"][3], c["geom"][2]) and field.dtype == np.int32
    _, win = F.classify_geometric(c)
    assert np.array_equal(field.ravel(), win), name                  # (a geometric winner's rank IS its flat source index, always inside the array)
    img = F.image(c)
    assert np.array_equal(M.gather(field, img), O.warp_forward_geometric(c["kind"], c["m"], img, *c["geom"])), name


@pytest.mark.parametrize("name", list(PW))
def test_piecewise_model_gathers_the_warp(name):
    c = PW[name]
    field = M.piecewise_case(c)
    assert field.shape == (c["geom"][3], c["geom"][2]) and field.dtype == np.int32
    img = F.image(c)
    assert np.array_equal(M.gather(field, img), F.piecewise_oracle(c, img)), name


def test_piecewise_model_names_winners_outside_the_source():
    """off_image: pixels whose last writer reads outside the array are -1 in the model although earlier writers read a pixel; winners whose
    column lies outside 0..W-1 keep their wrapped flat index."""
    c = PW["off_image"]
    counts, win, sidx = F.classify_piecewise(c)
    assert counts["lost_to_zero"] > 0 and counts["zero_over_earlier"] > 0 and counts["src_wrapped"] > 0
    s = sidx[np.where(win >= 0, win, 0)]
    want = np.where((win >= 0) & (s >= 0) & (s < c["W"] * c["H"]), s, -1).astype(np.int32)
    assert np.array_equal(M.piecewise_case(c).ravel(), want)


def test_fuzz_draws_are_enough():
    cases, _, _ = F.fuzz(FUZZ_SEED, FUZZ_DRAWS, HG.forward_tiles_admissible)
    assert len(cases) >= 300


def test_library_exports_the_forward_field_calls():
    import hgwarp
    L = hgwarp.lib()
    for name in ("hg_field_forward_geometric", "hg_field_forward_geometric_batch_device", "hg_field_forward_piecewise",
                 "hg_field_forward_piecewise_batch_device", "hg_last_forward_field_kernel"):
        assert name in hgwarp.EXPORTS and hasattr(L, name), name


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "homography.js_amd", "lib", "hgwarp.node")),
                    reason="node or the N-API addon is missing")
def test_js_class_picks_the_loop_and_refuses_over_the_mock_addon():
    """tests/js/field_forward_gpu.mjs with the device calls answered by the JavaScript oracle (tests/js/mock_field_addon.cjs): the class's
    side of sourceField(format, {loop}) -- 'warp' follows warp()'s dispatch, 'forward' forces the forward loop, the refusals are strings,
    neither a map nor a path is recorded.  (That the native layer computes the field is what tests/test_gpu_forward_field.py proves.)"""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "field_forward_gpu.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_field_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert p.returncode == 0 and res["ok"] and not res["fails"], (res["fails"], p.stderr[-2000:])
    assert set(res["report"]) == {"piecewise", "affine"} and res["report"]["piecewise"]["forward_holes"] > 0
