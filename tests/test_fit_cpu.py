"""CPU-side checks of the fitting feature (include/hgwarp.h, "fitting transforms to matches"): the header declares and the library exports
the two entry points, hg_fit_sample_indices equals the numpy model of tests/hgtest/fit.py (invalid rows included), every refusal that needs
no device is made, and the model itself is pinned on a hand-computed case.  tests/test_gpu_fit.py compares the device with the model."""
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
from hgtest import fit as FM                 # noqa: E402

NEW = ["hg_fit_sample_indices", "hg_fit_matches_frames_device"]
INVALID = 1
I32P = C.POINTER(C.c_int32)
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def test_header_declares_and_library_exports_the_fit_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in HG.EXPORTS, name
    assert "fitting transforms to matches" in text and "hg_fit_matches_frames_device)" in text.split("enum {")[0]      # the section; the note beside HG_VERSION
    assert callable(HG.fit_sample_indices) and callable(HG.Context.fit_matches_frames_device)
    assert FM.tile() >= 64                                        # the constant the GPU test sizes its cases by


@pytest.mark.parametrize("kind", (FM.AFFINE, FM.PROJECTIVE))
@pytest.mark.parametrize("seed", (0, 1, 0xffffffff))
def test_sample_indices_equal_the_model(kind, seed):
    counts = [0, 2, 3, 4, 5, 64, 65536]
    got = HG.fit_sample_indices(kind, seed, counts, 65536, 65)
    want = FM.sample_indices(kind, seed, counts, 65)
    assert got.shape == (7, 65, 4) and got.dtype == np.int32
    assert np.array_equal(got, want)
    K = FM.k_of(kind)
    assert (got[:2] == -1).all() and (got[2] == -1).all() == (K == 4)      # counts below K: every hypothesis invalid
    ok = got[..., 0] >= 0
    assert ok[5:].all()                                           # 64 and 65536 matches: none invalid
    for f, c in enumerate(counts):
        rows = got[f][ok[f]]
        assert ((rows[:, :K] >= 0) & (rows[:, :K] < max(c, 1))).all()
        assert all(len(set(r[:K].tolist())) == K for r in rows)
        if K == 3:
            assert (rows[:, 3] == -1).all()


def test_counts_null_means_every_slot():
    L = HG.lib()
    a, b = np.empty((2, 7, 4), np.int32), np.empty((2, 7, 4), np.int32)
    cnt = (C.c_int32 * 2)(33, 33)
    assert L.hg_fit_sample_indices(1, 5, 2, None, 33, 7, a.ctypes.data_as(I32P)) == 0
    assert L.hg_fit_sample_indices(1, 5, 2, cnt, 33, 7, b.ctypes.data_as(I32P)) == 0
    assert np.array_equal(a, b) and np.array_equal(a, FM.sample_indices(1, 5, [33, 33], 7))


def test_few_matches_make_some_hypotheses_invalid_and_leave_others():
    """At counts 4 and 5 sixteen draws sometimes hold fewer than four distinct values: among 64 hypotheses x 50 seeds the model has 135 and
    10 invalid rows (frames 0 and 1); at least one invalid and one valid row must exist, and the library agrees row for row."""
    bad = np.zeros(2, int)
    for seed in range(50):
        got = HG.fit_sample_indices(FM.PROJECTIVE, seed, [4, 5], 5, 64)
        assert np.array_equal(got, FM.sample_indices(FM.PROJECTIVE, seed, [4, 5], 64)), seed
        bad += (got[:, :, 0] < 0).sum(1)
    assert (bad >= 1).all() and (bad < 3200).all(), bad.tolist()
    assert bad[0] > bad[1]


def test_refusals_without_a_device():
    L = HG.lib()
    out = np.empty((2, 4, 4), np.int32)
    po = out.ctypes.data_as(I32P)
    cnt = (C.c_int32 * 2)(3, 4)
    assert L.hg_fit_sample_indices(1, 0, 2, cnt, 4, 4, po) == 0
    for args in ((2, 0, 2, cnt, 4, 4, po), (-1, 0, 2, cnt, 4, 4, po),                     # kind
                 (1, 0, 2, None, -1, 4, po), (1, 0, 2, None, 65537, 4, po),               # n_points
                 (1, 0, 2, cnt, 4, -1, po), (1, 0, 2, cnt, 4, 65537, po),                 # n_hyp
                 (1, 0, -1, cnt, 4, 4, po), (1, 0, 4097, None, 4, 4, po),                 # n_frames
                 (1, 0, 2, (C.c_int32 * 2)(3, 5), 4, 4, po), (1, 0, 2, (C.c_int32 * 2)(-1, 4), 4, 4, po),      # a count outside [0, n_points]
                 (1, 0, 2, cnt, 4, 4, None)):                                             # out NULL with work
        assert L.hg_fit_sample_indices(*args) == INVALID, args
    assert L.hg_fit_sample_indices(1, 0, 0, None, 4, 4, None) == 0                        # no frames, no hypotheses: nothing to write
    assert L.hg_fit_sample_indices(1, 0, 2, cnt, 4, 0, None) == 0
    assert L.hg_fit_sample_indices(0, 0, 1, None, 65536, 65536, None) == INVALID          # the limits themselves are legal (out is what is missing)
    with pytest.raises(HG.HgError) as e:
        HG.fit_sample_indices(3, 0, [4], 4, 4)
    assert e.value.code == INVALID
    # the device entry without a context
    assert L.hg_fit_matches_frames_device(None, 1, None, 0, None, 0, 1.0, 1, 0, None, 1, None, None, None, None, None) == INVALID
    assert b"ctx" in L.hg_last_error(None)


def test_model_on_a_hand_computed_case():
    """x' = 2x + 3, y' = 2y - 1 as a homography: the unit square's corners (scaled by 10) map exactly; a fifth match lies 100 px off.
    Hypothesis 0 holds the outlier, hypothesis 1 the four exact pairs: count 4, that mask, that matrix."""
    m = np.array([[[0, 0, 3, -1], [10, 0, 23, -1], [0, 10, 3, 19], [10, 10, 23, 19], [5, 5, 113, 9]]], np.float32)
    s = np.array([[[0, 1, 2, 4], [0, 1, 2, 3]]], np.int32)
    want_h = np.array([2, 0, 3, 0, 2, -1, 0, 0], np.float64)
    r = FM.fit(FM.PROJECTIVE, m, None, 0.5, 2, samples=s)
    assert r.best.tolist() == [1] and r.counts.tolist() == [4] and r.mask.tolist() == [[1, 1, 1, 1, 0]]
    assert np.allclose(r.min_mats[0], want_h, atol=1e-12) and np.array_equal(r.mats[0], r.min_mats[0])      # K inliers: the minimal matrix stands
    assert np.array_equal(r.min_mats[0], HG.solve_projective(m[0, :4, :2].ravel(), m[0, :4, 2:].ravel()))
    a = FM.fit(FM.AFFINE, m, None, 0.5, 2, samples=s)             # affine: (0, 1, 2) in both rows: a tie, the lower index wins; 4 inliers > K
    assert a.best.tolist() == [0] and a.counts.tolist() == [4] and a.mask.tolist() == [[1, 1, 1, 1, 0]]
    assert np.array_equal(a.min_mats[0], [2, 0, 0, 2, 3, -1, 0, 0])
    assert np.allclose(a.mats[0], [2, 0, 0, 2, 3, -1, 0, 0], atol=1e-12) and a.refit_ld[0] is not None
    ls = FM.fit(FM.AFFINE, m[:, :4], None, 0.5, 0)                # least squares without sampling
    assert ls.best.tolist() == [-1] and ls.counts.tolist() == [4] and np.isnan(ls.min_mats).all()
    assert np.allclose(ls.mats[0], [2, 0, 0, 2, 3, -1, 0, 0], atol=1e-12)
    assert FM.corner_displacement(FM.AFFINE, ls.mats[0], [2, 0, 0, 2, 3, -1, 0, 0], m[0, :4, :2]) < 1e-12
    # the rules at the edges: a repeated index, an index at counts[f], -1, collinear points; a NaN match is never an inlier
    assert not FM.sample_ok(1, [0, 0, 1, 2], 5) and not FM.sample_ok(1, [0, 1, 2, 5], 5) and not FM.sample_ok(0, [-1, 1, 2, 3], 5) and FM.sample_ok(0, [0, 1, 2, -1], 5)
    col = np.array([[k, 2 * k, k, k] for k in range(4)], np.float32)
    assert not FM.minimal(1, col, [0, 1, 2, 3])[1] and not FM.minimal(0, col, [0, 1, 2, 3])[1]
    nanm = m[0].copy()
    nanm[0, 3] = np.nan
    assert FM.score(1, want_h, nanm, 1e30).tolist() == [[False, True, True, True, True]]
    assert FM.best([3, 5, 5, 9], [True, True, True, False]) == 1 and FM.best([0, 0], [False, False]) == -1


# ------------------------------------------------------------------------------------------------ the kernel text on the host
@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/fit_check.cpp: hg_k_fit.hip itself, compiled for the CPU behind the thread-index shim -- a block of k_fit_score and
    k_fit_finish as 256 host threads -- and run under ASan + UBSan on exact-size heap buffers: no byte outside a buffer is touched, and what
    the kernels compute is the model's: mask, counts, best and minimal matrices exactly, the refit within the tolerance of the GPU test.  The
    cases are the GPU test's at their smallest sizes.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "fit_check")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", os.path.join(cpp, "hip_stub"), "-I", CSRC, os.path.join(cpp, "fit_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    n_case = [0]

    def run(kind, m, counts, threshold, n_hyp, seed=0, samples=None, refit=True):
        m = np.asarray(m, np.float32)
        F, N = m.shape[0], m.shape[1]
        cnt = np.asarray([N] * F if counts is None else counts, np.int32)
        fin, fout = tmp_path / f"case{n_case[0]}.in", tmp_path / f"case{n_case[0]}.out"
        n_case[0] += 1
        head = struct.pack("<6iIid", kind, F, N, n_hyp, 1 if refit else 0, 0 if samples is None else 1, seed, 0, threshold)
        fin.write_bytes(head + cnt.tobytes() + m.tobytes() + (b"" if samples is None else np.ascontiguousarray(samples, np.int32).tobytes()))
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (n_case[0], (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (n_case[0], (p.stdout + p.stderr)[-3000:])
        return FM.unpack(fout.read_bytes(), F, N)

    T = FM.tile()
    for kind in (FM.AFFINE, FM.PROJECTIVE):
        for n_points in (0, 3, 4, 5, 63, 64, 65, T - 1, T, T + 1):
            m, _ = FM.planted(kind, 100 + n_points, 3, n_points)
            counts = FM.counts_for(n_points)
            FM.check(kind, run(kind, m, counts, 1.0, 65, seed=n_points), FM.fit(kind, m, counts, 1.0, 65, seed=n_points), m, ("n_points", n_points))
        m, _ = FM.planted(kind, 200, 3, 65)
        for n_hyp in (1, 63, 64, 255, 256, 257):
            FM.check(kind, run(kind, m, FM.counts_for(65), 1.0, n_hyp, seed=7), FM.fit(kind, m, FM.counts_for(65), 1.0, n_hyp, seed=7), m, ("n_hyp", n_hyp))
        m[0, 62, 1] = 100.0
        for thr in (0.0, 1e30):
            FM.check(kind, run(kind, m, None, thr, 65, seed=5), FM.fit(kind, m, None, thr, 65, seed=5), m, ("threshold", thr))
        w = FM.fit(kind, m, None, 1.0, 65, seed=5, refit_on=False)
        g = run(kind, m, None, 1.0, 65, seed=5, refit=False)
        FM.check(kind, g, w, m, "refit == 0")
        assert np.array_equal(g.raw["mats"], g.raw["min"])
        mm, truth, counts, s = FM.given_samples_case(kind)
        w = FM.fit(kind, mm, counts, 1.0, 8, samples=s)
        assert w.best.tolist() == [2, -1, -1]
        g = run(kind, mm, counts, 1.0, 8, samples=s)
        FM.check(kind, g, w, mm, "given samples")
        assert (g.mats[1:].view(np.uint64) == FM.QNAN_BITS).all()
        K = FM.k_of(kind)
        m[2, K - 1:, 0] = np.nan
        FM.check(kind, run(kind, m, [65, 65, 65], 1.0, 0), FM.fit(kind, m, [65, 65, 65], 1.0, 0), m, "n_hyp == 0")


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_fit_matches_over_the_recording_mock_addon():
    """tests/js/fit_class.mjs: h.fitMatches(matchSets, options) pads the lists to the longest and hands their lengths down as counts; the
    option defaults; the bare strings it throws; the shape of the result; no image is needed and the instance's state is unchanged."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "fit_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_fit_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ok"] and res["fails"] == [] and p.returncode == 0, (res["fails"], p.stderr[-2000:])
    assert res["checks"] >= 30
