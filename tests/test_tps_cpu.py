"""CPU-side checks of the thin-plate splines (include/hgwarp.h, "thin-plate splines"): the header declares and the library exports the
entries and enums, the layouts, every refusal that needs no device, the numpy model of tests/hgtest/tps.py pinned by hand-worked cases and
against scipy's thin_plate_spline, and the kernel text itself on the host under sanitizers.  tests/test_gpu_tps.py compares the device with
the model."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import tps as TM                 # noqa: E402

NEW = ["hg_tps_layout", "hg_tps_solve_frames_device", "hg_tps_field_layout", "hg_field_tps_frames_device", "hg_points_tps_frames_device"]
INVALID = 1
SZ = C.c_size_t
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def lds_points():
    """The most control points whose system stays in LDS, from the capacity hg_tps_dev.h names."""
    cap = int(re.search(r"kTpsLdsCap = (\d+);", open(os.path.join(CSRC, "hg_tps_dev.h")).read()).group(1))
    n = 3
    while (n + 4) ** 2 <= cap:
        n += 1
    return n


def smooth_case(n, seed, w=300.0, h=200.0, amp=6.0):
    """n landmark pairs: destiny points spread over a w x h box, source points a smooth deformation of them plus a little noise."""
    rng = np.random.default_rng(seed)
    frm = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    to = frm + amp * np.stack([np.sin(frm[:, 1] / 40.0), np.cos(frm[:, 0] / 55.0)], 1) + rng.normal(0, 0.5, (n, 2)) + [12.0, 7.0]
    return frm.astype(np.float32), to.astype(np.float32)


def test_header_declares_and_library_exports_the_tps_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in HG.EXPORTS, name
    assert "thin-plate splines" in text and "thin-plate splines\n" in text.split("enum {")[0] and "by the presence of hg_tps_solve_frames_device" in text.split("enum {")[0]      # the section; the note beside HG_VERSION
    enums = dict(re.findall(r"\b(HG_TPS_[A-Z_]+) = (\d+)", code))
    assert enums == {"HG_TPS_MAX_POINTS": "1024", "HG_TPS_OK": "0", "HG_TPS_SINGULAR": "1", "HG_TPS_BAD_INPUT": "2"}
    assert (HG.TPS_MAX_POINTS, HG.TPS_OK, HG.TPS_SINGULAR, HG.TPS_BAD_INPUT) == (1024, TM.OK, TM.SINGULAR, TM.BAD_INPUT)
    assert callable(HG.tps_layout) and callable(HG.tps_field_layout)
    for m in ("tps_solve_frames_device", "field_tps_frames_device", "points_tps_frames_device"):
        assert callable(getattr(HG.Context, m)), m
    assert lds_points() >= 68                                # configuration C4, the 68-landmark face mesh, solves in LDS


def test_layouts():
    cap = lds_points()
    for n in (3, 4, 68, cap, cap + 1, 200, 1024):
        for f in (0, 1, 7, 4096):
            rec, scr = HG.tps_layout(n, f)
            assert rec == (16 + 4 * n) * 8 == TM.record_doubles(n) * 8
            assert scr == (0 if n <= cap else f * (n + 3) ** 2 * 8), (n, f)
    geoms = [(0, 0, 1, 1), (-5, 3, 70, 9), (2, 2, 0, 5), (0, 0, 257, 5), (1, 1, 33, 64)]
    assert HG.tps_field_layout(geoms, 1) == 0 and HG.tps_field_layout([], 8) == 0
    for step in (2, 4, 8, 16, 32):
        want = sum((TM.nodes(g[2], step) * TM.nodes(g[3], step) * 16 + 255) // 256 * 256 for g in geoms if g[2] > 0 and g[3] > 0)
        assert HG.tps_field_layout(geoms, step) == want, step
    # the lattice: always two nodes, the last at or beyond the last pixel, the one before it inside
    for step in (2, 4, 8, 16, 32):
        for n in range(1, 100):
            k = TM.nodes(n, step)
            assert k >= 2 and (k - 1) * step >= n - 1 and (k == 2 or (k - 2) * step < n - 1), (n, step)


def test_refusals_without_a_device():
    """Every shape check is made before the pointers and the context are looked at (all NULL throughout) and names itself in hg_last_error."""
    L = HG.lib()
    err = lambda: L.hg_last_error(None).decode()
    rec, scr = SZ(0), SZ(0)
    for n, f in ((2, 1), (1025, 1), (-1, 1), (3, -1), (3, 4097)):
        assert L.hg_tps_layout(n, f, C.byref(rec), C.byref(scr)) == INVALID, (n, f)
    assert L.hg_tps_layout(3, 0, None, None) == 0 and L.hg_tps_layout(1024, 4096, C.byref(rec), C.byref(scr)) == 0

    def solve(n_from=1, n_to=1, n=68, f=2, lam=0.0):
        return L.hg_tps_solve_frames_device(None, None, n_from, None, n_to, n, f, lam, None, None, None), err()

    for bad, word in ((dict(n=2), "n_points must"), (dict(n=1025), "n_points must"), (dict(f=-1), "n_frames must"), (dict(f=4097), "n_frames must"),
                      (dict(n_from=0), "n_to_sets must"), (dict(n_to=0), "n_to_sets must"), (dict(lam=-1e-300), "lambda must"),
                      (dict(lam=float("nan")), "lambda must"), (dict(lam=float("inf")), "lambda must")):
        code, msg = solve(**bad)
        assert code == INVALID and word in msg, (bad, msg)
    assert solve(f=0) == (0, err())                          # no frames: HG_OK before any pointer is looked at
    code, msg = solve()
    assert code == INVALID and "is NULL" in msg, msg        # the shape is legal: only the pointers are missing

    G = (HG.Geom * 2)(HG.Geom(0, 0, 8, 8), HG.Geom(-3, 2, 5, 4))

    def field(n=68, f=2, W=64, H=48, fmt=HG.FIELD_COORDS, step=1, geoms=G):
        return L.hg_field_tps_frames_device(None, None, n, geoms, f, W, H, fmt, step, None, None, None), err()

    for bad, word in ((dict(n=2), "n_points must"), (dict(f=4097), "n_frames must"), (dict(step=0), "step must"), (dict(step=3), "step must"),
                      (dict(step=64), "step must"), (dict(geoms=None), "geoms is NULL"), (dict(fmt=2), "unknown field format"), (dict(fmt=-1), "unknown field format"),
                      (dict(W=0), "W and H"), (dict(H=-1), "W and H"), (dict(fmt=HG.FIELD_INDEX, W=65536, H=32768), "2^31 pixels")):
        code, msg = field(**bad)
        assert code == INVALID and word in msg, (bad, msg)
    assert field(fmt=HG.FIELD_COORDS, W=65536, H=32768)[1].find("is NULL") >= 0      # the coords format has no such limit
    assert field(f=0)[0] == 0
    big = (HG.Geom * 1)(HG.Geom(1 << 27, 0, 4, 4))
    assert field(f=1, geoms=big)[0] == INVALID               # what hg_geom refuses
    offs = (SZ * 2)(0, 260)
    assert L.hg_field_tps_frames_device(None, None, 68, G, 2, 64, 48, HG.FIELD_COORDS, 1, offs, None, None) == INVALID and "multiples" in err()
    empty = (HG.Geom * 2)(HG.Geom(0, 0, 0, 8), HG.Geom(0, 0, 8, -1))
    assert field(geoms=empty)[0] == 0                        # a set of empty windows: nothing to do
    total = SZ(0)
    assert L.hg_tps_field_layout(G, 2, 3, C.byref(total)) == INVALID and L.hg_tps_field_layout(None, 2, 2, C.byref(total)) == INVALID
    assert L.hg_tps_field_layout(G, 2, 2, None) == INVALID

    def points(n=68, f=2, n_pts=10, n_sets=1):
        return L.hg_points_tps_frames_device(None, None, n, f, None, n_pts, n_sets, None), err()

    for bad, word in ((dict(n=1025), "n_points must"), (dict(f=-2), "n_frames must"), (dict(n_pts=-1), "n_pts must"), (dict(n_pts=(1 << 24) + 1), "n_pts must"),
                      (dict(n_sets=0), "n_sets must")):
        code, msg = points(**bad)
        assert code == INVALID and word in msg, (bad, msg)
    assert points(n_pts=0)[0] == 0 and points(f=0)[0] == 0
    assert points()[0] == INVALID and "is NULL" in points()[1]
    with pytest.raises(HG.HgError) as e:
        HG.tps_layout(2, 1)
    assert e.value.code == INVALID


def test_model_three_points_are_the_affine_map():
    """Three pairs: the side conditions force w = 0 and the spline is the affine map through the pairs, everywhere."""
    frm = np.array([[0, 0], [10, 0], [0, 10]], np.float32)
    to = np.array([[5, 7], [25, 7], [5, 37]], np.float32)               # x' = 2x + 5, y' = 3y + 7
    rec, st = TM.solve(frm, to)
    assert st == TM.OK
    pts = rec[TM.HEAD:].reshape(3, 4)
    assert np.abs(pts[:, 2:4]).max() < 1e-12
    c = np.array([10 / 3, 10 / 3])
    md = (np.hypot(*(frm[0] - c)) + np.hypot(*(frm[1] - c)) + np.hypot(*(frm[2] - c))) / 3
    assert np.allclose(rec[0:2], c, rtol=0, atol=1e-15) and np.isclose(rec[2], np.sqrt(2) / md, rtol=1e-15)
    assert np.allclose(rec[3:5], [35 / 3, 17], rtol=1e-15) and (rec[5:8] == 0).all() and (rec[14:16] == 0).all()
    # x' = 2 x + 5 = 2 (x'/s + cx) + 5: a1x = 2 / s, a0x = 2 cx + 5 - tx; likewise y
    s = rec[2]
    assert np.allclose(rec[8:14], [2 * c[0] + 5 - 35 / 3, 3 * c[1] + 7 - 17, 2 / s, 0, 0, 3 / s], rtol=0, atol=1e-12)
    X, Y = np.array([-100.0, 3.5, 40.0]), np.array([50.0, -2.25, -30.0])
    sx, sy = TM.evaluate(rec, X, Y)                          # (w is zero up to rounding, about 1e-16: times U of a few thousand)
    assert np.allclose(sx, 2 * X + 5, rtol=0, atol=1e-10) and np.allclose(sy, 3 * Y + 7, rtol=0, atol=1e-10)


def test_model_square_with_one_corner_displaced():
    """The square (+-1, +-1) -- c = 0, mean distance sqrt(2), so s = 1 and d = from -- with the corner (1, 1) moved by e along x.  On the four
    corners e delta_(1,1) = e (1 + x + y + x y) / 4: the constant goes into t, the x and y parts into the affine slopes, and the x y part, e / 4
    in the pattern (+, -, -, +), is what the kernel carries.  The side conditions leave w = k (1, -1, -1, 1); row (-1, -1) of K w is
    k (U(8) - 2 U(4)) (two neighbours at q = 4 with weight -1, the diagonal at q = 8 with +1), so k = (e / 4) / (U(8) - 2 U(4)), U(q) = q log q."""
    frm = np.array([[-1, -1], [1, -1], [-1, 1], [1, 1]], np.float32)    # c = 0, mean distance sqrt(2): s = 1, d = from
    e = 0.5
    to = frm.copy()
    to[3, 0] += e
    rec, st = TM.solve(frm, to)
    assert st == TM.OK and np.allclose(rec[0:3], [0, 0, 1], rtol=0, atol=1e-15)
    u4, u8 = 4 * np.log(4.0), 8 * np.log(8.0)
    k = (e / 4) / (u8 - 2 * u4)
    pts = rec[TM.HEAD:].reshape(4, 4)
    assert np.array_equal(pts[:, 0:2], frm.astype(np.float64))
    assert np.allclose(pts[:, 2], k * np.array([1, -1, -1, 1]), rtol=0, atol=1e-14) and np.abs(pts[:, 3]).max() < 1e-14
    # the affine part is the least-squares plane through the x targets: mean e / 4 (carried by t), slopes e / 4 each
    assert np.allclose(rec[3:5], [e / 4, 0], rtol=0, atol=1e-15)
    assert np.allclose(rec[8:14], [0, 0, 1 + e / 4, 0, e / 4, 1], rtol=0, atol=1e-14)
    assert TM.residual(rec, frm, to) < 1e-14
    sx, sy = TM.evaluate(rec, np.array([0.0]), np.array([0.0]))         # the centre: every q = 2, the kernel terms cancel
    assert abs(sx[0] - e / 4) < 1e-15 and abs(sy[0]) < 1e-15


def test_model_statuses_follow_the_stated_rule():
    frm, to = smooth_case(12, 3)
    assert TM.solve(frm, to)[1] == TM.OK
    bad = frm.copy(); bad[5, 1] = np.nan
    rec, st = TM.solve(bad, to)
    assert st == TM.BAD_INPUT and (rec.view(np.uint64) == TM.NAN64).all()
    bad = to.copy(); bad[0, 0] = np.inf
    assert TM.solve(frm, bad)[1] == TM.BAD_INPUT
    assert TM.solve(np.tile(frm[:1], (12, 1)), to)[1] == TM.SINGULAR                  # mean distance 0
    dup = frm.copy(); dup[7] = dup[2]
    assert TM.solve(dup, to, 0.0)[1] == TM.SINGULAR                                  # equal rows: a pivot is exactly 0
    rec, st = TM.solve(dup, to, 0.01)
    assert st == TM.OK and np.isfinite(rec).all()
    col = np.stack([np.arange(12.0), np.zeros(12)], 1).astype(np.float32)            # collinear: P has rank 2
    assert TM.solve(col, to, 0.0)[1] == TM.SINGULAR


def test_model_agrees_with_scipy_thin_plate_spline():
    scipy_interp = pytest.importorskip("scipy.interpolate")
    worst = 0.0
    for n, seed in ((3, 1), (4, 2), (17, 3), (68, 4), (200, 5)):
        frm, to = smooth_case(n, seed)
        rec, st = TM.solve(frm, to)
        assert st == TM.OK
        rng = np.random.default_rng(seed + 100)
        q = np.stack([rng.uniform(-30, 330, 500), rng.uniform(-30, 230, 500)], 1)
        ref = scipy_interp.RBFInterpolator(frm.astype(np.float64), to.astype(np.float64), kernel="thin_plate_spline", smoothing=0.0, degree=1)(q)
        sx, sy = TM.evaluate(rec, q[:, 0], q[:, 1])
        worst = max(worst, float(np.max(np.hypot(sx - ref[:, 0], sy - ref[:, 1]))))
    assert worst < 1e-7, worst                               # two f64 solves of a system with condition number near 1e5, results of a few hundred px


def test_model_delta_bounds_the_float64_evaluation():
    """The evaluation tolerance against the longdouble model and against permuted sums: the observed error stays far inside delta."""
    for n, seed in ((3, 1), (5, 2), (64, 3), (200, 4)):
        frm, to = smooth_case(n, seed)
        rec, _ = TM.solve(frm, to)
        rng = np.random.default_rng(seed)
        X, Y = rng.uniform(-50, 350, 300), rng.uniform(-50, 250, 300)
        sx, sy = TM.evaluate(rec, X, Y)
        lx, ly = TM.evaluate(rec, X, Y, TM.LD)
        dx, dy = TM.delta(rec, X, Y)
        assert (np.abs(sx - lx) <= 0.25 * dx).all() and (np.abs(sy - ly) <= 0.25 * dy).all()
        perm = rec.copy()
        perm[TM.HEAD:] = rec[TM.HEAD:].reshape(n, 4)[rng.permutation(n)].ravel()
        px, py = TM.evaluate(perm, X, Y)
        assert (np.abs(px - sx) <= 0.25 * dx).all() and (np.abs(py - sy) <= 0.25 * dy).all()
        assert max(dx.max(), dy.max()) < 3e-7


# ------------------------------------------------------------------------------------------------ the kernel text on the host
def pack_case(frm_sets, to_sets, n_frames, lam, W, H, fmt, step, geoms, pts):
    frm_sets, to_sets = np.asarray(frm_sets, np.float32), np.asarray(to_sets, np.float32)
    pts = np.asarray(pts, np.float32).reshape(np.asarray(pts).shape[0], -1, 2)
    n = frm_sets.shape[1]
    head = struct.pack("<10id", n, n_frames, frm_sets.shape[0], to_sets.shape[0], W, H, fmt, step, pts.shape[1], pts.shape[0], lam)
    return head + frm_sets.tobytes() + to_sets.tobytes() + np.asarray(geoms, np.int32).tobytes() + pts.tobytes()


def check_against_model(out, frm_sets, to_sets, n_frames, lam, W, H, fmt, step, geoms, pts, what):
    """The host program's outputs by the GPU test's rules (tests/hgtest/tps.py): statuses exact, records by the solve tolerance, field and points
    by delta from the program's own records.  Returns the largest metric / base ratio."""
    n = frm_sets.shape[1]
    recd = TM.record_doubles(n)
    recs = np.frombuffer(out, np.float64, n_frames * recd).reshape(n_frames, recd)
    pos = n_frames * recd * 8
    status = np.frombuffer(out, np.int32, n_frames, pos)
    pos += n_frames * 4
    px = 4 if fmt == HG.FIELD_INDEX else 8
    pair = lambda f: (frm_sets[f % frm_sets.shape[0]], to_sets[f % to_sets.shape[0]])
    bases = [TM.solve_base(*pair(f), lam)[2] for f in range(n_frames)]
    floor = min(b for b in bases if b)                       # a base of 0 is replaced by the smallest non-zero base of the case
    worst = max(TM.check_record(recs[f], status[f], *pair(f), lam, floor, (what, f)) for f in range(n_frames))
    offs, total = TM.pack256(geoms, px)
    for f, g in enumerate(geoms):
        if g[2] <= 0 or g[3] <= 0 or step != 1:
            continue                                         # (the lattice is compared on the device; here the sanitizers watch its bounds)
        TM.check_field_frame(out[pos + offs[f]:pos + offs[f] + g[2] * g[3] * px], recs[f], status[f] == TM.OK, g, W, H, fmt == HG.FIELD_INDEX, (what, f))
    pos += total
    n_pts = pts.shape[1]
    got = np.frombuffer(out, np.float32, n_frames * n_pts * 2, pos).reshape(n_frames, n_pts, 2)
    for f in range(n_frames):
        TM.check_points_frame(got[f], recs[f], status[f] == TM.OK, pts[f % pts.shape[0]], (what, f))
    return worst


@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/tps_check.cpp: hg_k_tps.hip itself, compiled for the CPU behind the thread-index shim -- the solve's workgroup as real
    threads, the other kernels lane after lane -- and run under ASan + UBSan on exact-size heap buffers: no byte outside a buffer is touched,
    and what the kernels compute is the model's by the GPU test's rules.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "tps_check")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", os.path.join(cpp, "hip_stub"), "-I", CSRC, os.path.join(cpp, "tps_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    cap = lds_points()
    geoms = [(-4, 3, 70, 9), (2, -2, 0, 5), (10, 20, 33, 6)]
    pts = np.array([[[0, 0], [13.5, 7.25], [np.nan, 1], [np.inf, 2], [1e30, -1e30], [299, 199]]], np.float32)
    cases = []
    for k, (n, lam, fmt, step) in enumerate(((3, 0.0, 1, 1), (5, 0.0, 0, 1), (64, 0.0, 1, 4), (cap, 0.5, 1, 1), (cap + 1, 0.0, 0, 32))):
        a, b = smooth_case(n, 10 + k)
        a2, b2 = smooth_case(n, 20 + k)
        frm_sets, to_sets = np.stack([a, a2]), np.stack([b])
        if k == 1:
            frm_sets = frm_sets.copy(); frm_sets[1, 2, 0] = np.nan           # frame 1 fails, frames 0 and 2 are not affected
        if k == 2:
            frm_sets = frm_sets.copy(); frm_sets[1, 9] = frm_sets[1, 4]      # a duplicated point at lambda == 0
        cases.append((frm_sets, to_sets, 3, lam, 180, 120, fmt, step, geoms, pts))
    for k, c in enumerate(cases):
        fin, fout = tmp_path / f"case{k}.in", tmp_path / f"case{k}.out"
        fin.write_bytes(pack_case(*c))
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (k, p.stdout[-2000:], p.stderr[-3000:])
        worst = check_against_model(fout.read_bytes(), *c, what=f"case {k}")
        assert worst <= 16



# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_warp_thin_plate_over_the_recording_mock_addon():
    """tests/js/tps_class.mjs: h.warpThinPlate(sourcePoints, destinyPointSets, options) over a recording mock addon: the destiny sets as FROM
    lists, the default windows, the option defaults and output codes, the bare strings it throws, the shape of the result."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "tps_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_tps_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ok"] and res["fails"] == [] and p.returncode == 0, (res["fails"], p.stderr[-2000:])
    assert res["checks"] >= 30
