"""Frame sets whose frames bring their own source points (hg_piecewise_set_frames_src) without a GPU: the premises of the GPU tests on
the CPU oracle (wrong frame indexing changes bytes), the host parts of the C ABI (symbols, refusals reachable without a device, the
min_src == NULL rule), and the JavaScript class's warpBatch(dst, {sourcePoints}) over a mock addon against the reference's own loop."""
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
from hgtest import moving as M               # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import workloads as WL           # noqa: E402

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "homography.js_amd", "lib", "hgwarp.node")
NEW = ("hg_piecewise_set_frames_src", "hg_warp_inverse_piecewise_src_batch_device", "hg_piecewise_frame_min_src")


def _diff(a, b):
    return int((a != b).any(-1).sum())


@pytest.mark.parametrize("s", [4, -12])
def test_wrong_frame_indexing_changes_bytes(s):
    """For every frame f > 0 of Set A the correct output differs from "frame 0's source side", from "own points, frame 0's minima" and from
    "own points, minSrcY + 1"; every frame has covered and uncovered pixels; the two shifts give the two bounds forms."""
    ms = M.set_a(s)
    assert ms.F == 4 and (ms.W, ms.H) == (320, 200) and ms.tris.size == 3 * 48
    for f in range(ms.F):
        near, bil, cov = ms.want(f)[:3]
        assert cov.any() and not cov.all(), f
        assert near.shape == (ms.geoms[f][3], ms.geoms[f][2], 4)
        if f == 0:
            continue
        covered = int(cov.sum())
        assert 40000 < covered < 70000, covered
        assert _diff(near, ms.frame(f, src=ms.srcs[0], mins=ms.mins[0])[0]) > 0.9 * covered, f
        assert _diff(near, ms.frame(f, mins=ms.mins[0])[0]) >= 1000, f
        assert _diff(near, ms.frame(f, mins=(ms.mins[f][0], ms.mins[f][1] + 1))[0]) >= 10, f
        assert _diff(bil, ms.frame(f, mins=ms.mins[0])[1]) >= 1000, f
    flat = [v for m in ms.mins for v in m]
    if s == 4:
        assert min(flat) >= 0
    else:
        assert min(flat) < 0 < max(flat)                     # minima of both signs in ONE set: the fp64 bounds form for all its frames
    assert len(set(ms.mins)) == ms.F                         # every frame has minima of its own


def test_extended_and_wide_sets_keep_the_premises():
    ms = M.set_a(4, 5)
    for f in range(5):                                       # frame f over image f % 3 differs from frame f over its own image (f >= 3)
        cov = ms.want(f, 3)[2]
        assert cov.any() and not cov.all()
    assert _diff(ms.want(3, 3)[0], ms.want(3)[0]) > 1000 and _diff(ms.want(4, 3)[0], ms.want(4)[0]) > 1000
    wide = M.wide_set()
    assert wide.F == 3 and all(g[2] > 2048 and g[2] % 256 != 0 for g in wide.geoms)
    for f in range(1, 3):
        near, _, cov = wide.want(f)[:3]
        assert cov.any() and not cov.all()
        assert _diff(near, wide.frame(f, mins=wide.mins[0])[0]) >= 100, f


def test_new_symbols_resolve_and_are_declared():
    L = C.CDLL(HG.LIB_PATH)
    with open(os.path.join(ROOT, "include", "hgwarp.h")) as f:
        h = f.read()
    for n in NEW:
        assert hasattr(L, n) and n in HG.EXPORTS and n + "(" in h, n
    assert HG.lib().hg_version() == 100                      # callers detect the feature by the symbol


def test_refusals_reachable_without_a_device():
    L = HG.lib()
    g = HG._geoms([(0, 0, 8, 8)])
    pts = (C.c_float * 6)(0, 0, 8, 0, 0, 8)
    ms = (C.c_int32 * 2)(0, 0)
    assert L.hg_piecewise_set_frames_src(None, pts, ms, pts, g, None, 1) == 1                    # HG_ERR_INVALID: no context
    assert L.hg_warp_inverse_piecewise_src_batch_device(None, pts, ms, pts, g, None, 1, None) == 1
    out = (C.c_int32 * 2)(7, 7)
    assert L.hg_piecewise_frame_min_src(None, 3, out) == 1 and L.hg_piecewise_frame_min_src(pts, 0, out) == 1
    assert L.hg_piecewise_frame_min_src(pts, 3, None) == 1 and list(out) == [7, 7]


def test_null_minima_follow_hg_minmax_xy():
    """min_src == NULL: the rounded bounding-box minimum of the frame's own points, by the rule of hg_minmax_xy (Math.round: ties up)."""
    rng = np.random.default_rng(7)
    cases = [M.set_a(4).srcs[2], M.set_a(-12).srcs[1], M.wide_set().srcs[2],
             np.float32([0.5, -0.5, 3, 4, 9, 1]), np.float32([-1.5, 2.5, -1.4999, 2.4999, 7, 7]), np.float32([np.nan, 5.5, 3.25, np.nan, 4, 9]),
             np.float32([-(1 << 22) - 3, 2, 5, 1 << 23, 0, 0])]
    cases += [(rng.uniform(-300, 300, 2 * n) * 2).round() / 4 for n in (1, 2, 17)]
    for p in cases:
        p = np.ascontiguousarray(p, np.float32)
        mm = HG.minmax_xy(p)
        assert HG.frame_min_src(p) == (int(mm[0]), int(mm[1])), p
        assert HG.frame_min_src(p) == (int(O.minmax_xy(p)[0]), int(O.minmax_xy(p)[1]))
        if not np.isnan(p).any():
            assert HG.frame_min_src(p) == WL.src_min(p)
    assert HG.frame_min_src(np.float32([0.5, -0.5, 3, 4])) == (1, 0)                              # ties toward +Infinity
    assert HG.frame_min_src(np.float32([np.nan, np.nan])) == (2147483647, 2147483647)             # no finite point: nothing passes :1047


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is missing")
def test_js_class_warp_batch_with_source_points_equals_the_loops():
    """120 seeded sequences: warpBatch(dst, {sourcePoints}) == the class's own loop == the reference's loop (live where a reference checkout
    exists, else its recording tests/golden/ref_moving.json): 0 differing frames, the same instance state afterwards; frames for the forward
    loop, blank frames and {images} are among them; the refusals are bare strings."""
    live = os.path.exists(os.path.join(os.environ.get("HG_REFERENCE", "/root/reference"), "Homography.js"))
    args = ["120", "5"] if live else ["--transcript", os.path.join(ROOT, "tests", "golden", "ref_moving.json")]
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "moving_class.mjs"), *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["failures"] == [] and p.returncode == 0, res["failures"]
    assert res["sequences"] >= 100 and res["live"] == live and res["differing"] == 0 and res["threw"] == 0
    assert res["frames"] >= 300 and res["forward"] >= 50 and res["blank"] >= 10 and res["withImages"] >= 30 and res["batchedFrames"] >= 150
    assert len(res["refusals"]) == 4


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is missing")
def test_recorded_reference_loop_is_the_live_one():
    """The committed recording replays clean on its own (what a checkout without the reference runs)."""
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "moving_class.mjs"), "--transcript", os.path.join(ROOT, "tests", "golden", "ref_moving.json")],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["failures"] == [] and p.returncode == 0 and res["sequences"] == 120 and res["differing"] == 0
