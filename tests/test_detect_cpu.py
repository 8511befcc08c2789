"""CPU-side checks of the keypoint feature (include/hgwarp.h, "detecting and describing keypoints"): the header declares and the library
exports the entries and their constants, the pattern of the library equals the model's and the header's literals, hg_detect_layout and every
refusal that needs no device are made, the numpy model of tests/hgtest/detect.py is pinned on cases worked by hand, the kernel text of
hg_k_detect.hip runs on the host under sanitizers against the model, the chain's pictures meet their condition on the models alone, and the
JS class is driven over a recording mock addon.  tests/test_gpu_detect.py compares the device with the model."""
import ctypes as C
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
from hgtest import detect as DM              # noqa: E402
from hgtest import fit as FM                 # noqa: E402
from hgtest import match as MM               # noqa: E402

INVALID = 1
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")
NAMES = ("hg_detect_layout", "hg_describe_pattern", "hg_detect_describe_frames_device")


def test_header_declares_and_library_exports_the_detect_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    for name in NAMES:
        assert name in declared and hasattr(HG.lib(), name) and name in HG.EXPORTS, name
    assert re.search(r"enum\s*\{\s*HG_DETECT_MARGIN\s*=\s*16\s*,\s*HG_DETECT_DESC_BYTES\s*=\s*32\s*,\s*HG_DETECT_BINS\s*=\s*32\s*\}", code)
    assert (HG.DETECT_MARGIN, HG.DETECT_DESC_BYTES, HG.DETECT_BINS) == (16, 32, 32) == (DM.MARGIN, DM.DESC_BYTES, DM.BINS)
    head = " ".join(text.split("enum {")[0].split())
    assert "detecting and describing keypoints" in text and "keypoints by the presence of hg_detect_describe_frames_device" in head
    assert callable(HG.Context.detect_describe_frames_device) and callable(HG.detect_layout) and callable(HG.describe_pattern)
    assert DM.tile() >= 8 and DM.tile() % 2 == 0                  # the constant the GPU test sizes its cases by


def test_pattern_of_the_library_equals_the_model_and_the_literals():
    t = HG.describe_pattern()
    assert t.shape == (32, 256, 4) and t.dtype == np.int8
    assert t.tobytes() == DM.pattern().tobytes()
    assert t[0, :3].tolist() == [[-1, 1, 0, 0], [-3, 2, 10, -3], [-3, -6, 1, 4]]
    assert np.array_equal(t[0], DM.base_pattern()) and np.abs(t.astype(int)).max() <= 12
    assert (t[0, 139] == t[0, :139]).all(1).any()                 # test 139 repeats an earlier one: accepted
    assert DM.sha(t[0]).startswith("fb6113ea") and DM.sha(t[0]).endswith("93c18633")
    assert DM.sha(t).startswith("e3c0f978") and DM.sha(t).endswith("6b08e676")
    c, s = DM.cos_table().tolist(), DM.sin_table().tolist()
    assert c[:9] == [16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0]
    for k in range(17):
        assert c[16 - k] == -c[k] and c[(32 - k) % 32] == c[k]
    assert s == [c[(k + 24) % 32] for k in range(32)] and s[8] == 16384 and s[24] == -16384      # y grows downwards: bin 8 points down
    assert HG.lib().hg_describe_pattern(None) == INVALID and b"NULL" in HG.lib().hg_last_error(None)


def test_layout_and_its_refusals():
    assert HG.detect_layout(33, 33, 8, 1) == (5, 5, 25) == DM.layout(33, 33, 8, 1)
    assert HG.detect_layout(64, 40, 32, 2) == (2, 2, 8) == DM.layout(64, 40, 32, 2)
    assert HG.detect_layout(2048, 2048, 8, 1) == (256, 256, 65536)             # the limits themselves are legal
    assert HG.detect_layout(32768, 32768, 256, 4) == (128, 128, 65536) and HG.detect_layout(1, 1, 256, 16) == (1, 1, 16)
    L = HG.lib()
    x, y, n = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    for a, word in (((0, 33, 8, 1), "W and H"), ((33, 0, 8, 1), "W and H"), ((32769, 33, 8, 1), "W and H"), ((33, 32769, 8, 1), "W and H"), ((-1, 33, 8, 1), "W and H"),
                    ((33, 33, 7, 1), "cell"), ((33, 33, 257, 1), "cell"), ((33, 33, 8, 0), "per_cell"), ((33, 33, 8, 17), "per_cell"),
                    ((2048, 2048, 8, 2), "n_slots"), ((2049, 2048, 8, 1), "n_slots")):
        assert L.hg_detect_layout(*a, C.byref(x), C.byref(y), C.byref(n)) == INVALID and word in L.hg_last_error(None).decode(), a
        assert (x.value, y.value, n.value) == (-7, -7, -7)
    assert "cell" in (L.hg_detect_layout(33, 33, 7, 0, C.byref(x), C.byref(y), C.byref(n)), L.hg_last_error(None).decode())[1]      # the order
    for args in ((None, C.byref(y), C.byref(n)), (C.byref(x), None, C.byref(n)), (C.byref(x), C.byref(y), None)):
        assert L.hg_detect_layout(33, 33, 8, 1, *args) == INVALID and "NULL" in L.hg_last_error(None).decode()
    with pytest.raises(HG.HgError):
        HG.detect_layout(33, 33, 8, 17)


def test_refusals_without_a_device():
    """The shape checks come before the context is looked at, in the header's order: each one is reached with a NULL context and names itself
    in hg_last_error; a call that passes them all is refused for the NULL context."""
    L = HG.lib()
    ok = dict(W=64, H=40, n_planes=2, stride=64 * 40 * 4, channels=4, cell=32, per_cell=2, thr=10 ** 10, desc_stride=32)

    def call(**k):
        a = dict(ok, **k)
        code = L.hg_detect_describe_frames_device(None, None, a["W"], a["H"], a["n_planes"], a["stride"], a["channels"], a["cell"], a["per_cell"], a["thr"],
                                                  a["desc_stride"], None, None, None, None)
        return code, L.hg_last_error(None).decode()

    for k, word in ((dict(W=0), "W and H"), (dict(W=32769), "W and H"), (dict(H=0), "W and H"), (dict(H=32769), "W and H"), (dict(W=-3), "W and H"),
                    (dict(channels=0), "channels"), (dict(channels=2), "channels"), (dict(channels=3), "channels"), (dict(channels=5), "channels"),
                    (dict(cell=7), "cell"), (dict(cell=257), "cell"), (dict(per_cell=0), "per_cell"), (dict(per_cell=17), "per_cell"),
                    (dict(W=2048, H=2048, cell=8, per_cell=2, stride=2048 * 2048 * 4), "n_slots"),
                    (dict(n_planes=-1), "n_planes"), (dict(n_planes=4097), "n_planes"),
                    (dict(thr=0), "min_response"), (dict(thr=-1), "min_response"), (dict(thr=-2 ** 63), "min_response"),
                    (dict(desc_stride=0), "desc_stride"), (dict(desc_stride=16), "desc_stride"), (dict(desc_stride=40), "desc_stride"), (dict(desc_stride=33), "desc_stride"),
                    (dict(stride=64 * 40 * 4 - 1), "plane_stride_bytes"), (dict(stride=0), "plane_stride_bytes"), (dict(channels=1, stride=64 * 40 - 1), "plane_stride_bytes")):
        code, msg = call(**k)
        assert code == INVALID and word in msg and "ctx" not in msg, (k, msg)
    # the order: the size before the channels before the cell before per_cell before n_slots before n_planes before the threshold before the strides
    bad = dict(W=0, channels=3, cell=7, per_cell=0, n_planes=-1, thr=0, desc_stride=40, stride=0)
    for key, word in (("W", "W and H"), ("channels", "channels"), ("cell", "cell"), ("per_cell", "per_cell"), ("n_planes", "n_planes"), ("thr", "min_response"),
                      ("desc_stride", "desc_stride"), ("stride", "plane_stride_bytes")):
        assert word in call(**bad)[1], (key, call(**bad)[1])
        del bad[key]
    assert "n_slots" in call(W=2048, H=2048, cell=8, per_cell=2, n_planes=-1)[1] and "per_cell" in call(W=2048, H=2048, cell=8, per_cell=17)[1]
    # the limits themselves are legal: what is missing is the context
    for k in (dict(), dict(W=32768, H=32768, cell=256, per_cell=4, stride=2 ** 32, n_planes=4096, thr=2 ** 63 - 1, desc_stride=1024),
              dict(W=1, H=1, channels=1, stride=1, cell=8, per_cell=1, n_planes=0, thr=1), dict(W=2048, H=2048, cell=8, per_cell=1, stride=2 ** 24, channels=1)):
        code, msg = call(**k)
        assert code == INVALID and "ctx" in msg, (k, msg)


# ------------------------------------------------------------------------------------------------ the model, by hand
def test_model_facts_worked_by_hand():
    """1. A constant plane: every Sobel difference is 0, so A = B = C = 0 and R = 0 < min_response (>= 1) everywhere: no keypoints.
    2. A 32 x 40 plane: 16 <= x < W - 16 = 16 has no solution: none, whatever it shows.
    3. A 33 x 33 plane has ONE legal position, (16, 16).  Black with a white quadrant x >= f, y >= f: Ix is non-zero only in the columns f - 1
    and f (rows >= f - 1), Iy only in the rows f - 1 and f, and their product only in the 2 x 2 block at the corner.  For a window centred on
    the diagonal, A = C.  As the centre moves inwards from the corner, A grows with the rows of the vertical edge inside the window, until at
    (f + 2, f + 2) the window f - 1 .. f + 5 holds both edge columns over all seven rows; one step further it loses column f - 1 and A
    halves.  B is the same for every window that holds the corner block, and R = 12 A A - 16 B B grows with A: R peaks at (f + 2, f + 2), two
    pixels inside the white.  So with the first white pixel AT (16, 16) the peak is (18, 18), the neighbour (17, 17) beats the only legal
    position and the plane has NO keypoint; with f = 14 the peak is (16, 16) and the plane has exactly one keypoint, there.  Its orientation:
    the white part of the disc is mirror-symmetric about the diagonal, so m10 = m01 > 0 and m10 (c_k + s_k) is largest where c_k + s_k is:
    k = 4 (2 * 11585 = 23170, against 13623 + 9102 = 22725 at k = 3 and 5): bin 4, the diagonal down and to the right.
    4. Two pixels of equal R in one neighbourhood: a board of 4 x 4 blocks is mirror-symmetric about the lines BETWEEN two pixel columns (and
    rows) at a block border, so the two pixels on either side of such a line have the same R: equal neighbours, and where such a pair is a
    maximum the lower flat index is the keypoint.
    5. The margin (DM.margin_corners): corner peaks at x = 15 resp. y = 15 are maxima of their neighbourhoods and still no keypoints; those at
    16 and at W - 17 are."""
    assert DM.model(DM.constant(64, 48)[None], 1, 8, 16, 1).counts.tolist() == [0]
    assert (DM.response(DM.luma(DM.constant(64, 48), 1))[4:-4, 4:-4] == 0).all()
    assert DM.model(DM.noise(1, 32, 40)[None], 1, 8, 16, 1).counts.tolist() == [0] and DM.model(DM.noise(1, 40, 32)[None], 1, 8, 16, 1).counts.tolist() == [0]
    w = DM.model(DM.quadrant(16)[None], 1, 8, 1, 1)
    R = w.responses[0]
    assert w.counts.tolist() == [0] and R[18, 18] == R.max() and R[17, 17] > R[16, 16] > 0
    w = DM.model(DM.quadrant(14)[None], 1, 8, 1, 1)
    assert w.counts.tolist() == [1] and w.responses[0][16, 16] == w.responses[0].max()
    # cell 8: the pixel (16, 16) lies in cell (16 / 8) * 5 + 16 / 8 = 12, the only one with a keypoint; the list is compacted
    assert w.points[0, 0].view(np.float32).tolist() == [16.0, 16.0] and w.info[0, 0].tolist() == (int(w.responses[0][16, 16]), 4, 16 * 33 + 16)
    assert (w.points[0, 1:] == DM.PAD_WORD).all() and not w.desc[0, 1:].any() and (w.info["idx"][0, 1:] == -1).all() and (w.info["R"][0, 1:] == 0).all()
    m10, m01 = DM.moments(DM.luma(DM.quadrant(14), 1), np.array([16 * 33 + 16]))
    assert m10[0] == m01[0] > 0 and DM.choose_bin(m10, m01).tolist() == [4] and DM.choose_bin([0], [0]).tolist() == [0]
    assert DM.choose_bin([5, 0, -5, 0, 7], [0, 5, 0, -5, 7]).tolist() == [0, 8, 16, 24, 4]
    # ties inside a neighbourhood
    b = DM.checker(64, 64)
    w = DM.model(b[None], 1, 8, 16, 1)
    R = w.responses[0]
    kp = w.info["idx"][0, :w.counts[0]]
    tied = [(i % 64, i // 64) for i in kp.tolist() if any(R[i // 64 + dy, i % 64 + dx] == R[i // 64, i % 64] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))]
    assert len(tied) > 0, "the board must tie neighbours"
    for x, y in tied:                                             # the equal neighbours all have the higher flat index
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dy, dx) != (0, 0) and R[y + dy, x + dx] == R[y, x]:
                    assert (y + dy) * 64 + x + dx > y * 64 + x
    # the margin: a corner peak at x = 15 is a maximum of its neighbourhood and still no keypoint; at 16 it is one
    m = DM.margin_corners()
    w = DM.model(m[None], 1, 16, 16, 1)
    R = w.responses[0]
    kp = set(w.info["idx"][0, :w.counts[0]].tolist())
    for (x, y), kept in (((16, 16), True), ((15, 42), False), ((42, 15), False), ((63, 63), True), ((64, 30), False)):
        assert R[y, x] == R[y - 1:y + 2, x - 1:x + 2].max() and R[y, x] >= 1, (x, y)
        assert ((y * 80 + x) in kp) == kept, (x, y)


def test_the_chain_on_the_models_alone():
    """The condition on the inputs of the GPU test's chain (tests/test_gpu_detect.py), checked where no device is involved: on the pictures of
    DM.chain_case(DM.CHAIN_SEED) the three numpy models give every frame at least 30 accepted matches, at least 70 % of them within 1.5 px of
    the true transform, and a fitted matrix (no refit) that maps the frame's corners within 2 px of the truth.  Measured when the seed was
    chosen (matches, within 1.5 px, inliers, corner error): shift (114, 108, 108, 0.00), 20 degrees (79, 70, 70, 0.58), 30 degrees with
    perspective (76, 61, 60, 0.84)."""
    key, frames, truth = DM.chain_case(DM.CHAIN_SEED)
    c = DM.CHAIN
    wk = DM.model(key[None], 1, c["cell"], c["per_cell"], c["min_response"])
    wf = DM.model(frames, 1, c["cell"], c["per_cell"], c["min_response"])
    wm = MM.match(MM.BITS, 32, wf.desc, wk.desc, counts_q=wf.counts, counts_t=wk.counts, ratio=0.8, qpts=wf.points.view(np.float32), tpts=wk.points.view(np.float32))
    wt = FM.fit(FM.PROJECTIVE, wm.matches.view(np.float32), wm.counts, c["threshold"], c["n_hyp"], seed=c["fit_seed"], refit_on=False)
    got = DM.chain_is_good(frames, truth, wm, wt)
    assert [g[:3] for g in got] == [(114, 108, 108), (79, 70, 70), (76, 61, 60)], got


# ------------------------------------------------------------------------------------------------ the kernel text on the host
@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/detect_check.cpp: hg_k_detect.hip itself, compiled for the CPU behind the thread-index shim -- a workgroup of k_detect_cells
    and of k_detect_compact as 256 host threads, of k_detect_describe as 64 -- and run under ASan + UBSan on exact-size heap buffers: no byte
    outside a buffer is touched, every output equals the model's byte for byte, outputs passed as NULL and the bytes 32..stride of the
    descriptor rows keep their 0xA5 fill.  The cases are the GPU test's small ones.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "detect_check")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", os.path.join(cpp, "hip_stub"), "-I", CSRC, os.path.join(cpp, "detect_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    n_case = [0]

    def run(planes, channels, cell, per_cell, thr=1, stride=32, want=7, slack=0):
        planes = np.asarray(planes)
        P = planes.shape[0]
        fin, fout = tmp_path / f"case{n_case[0]}.in", tmp_path / f"case{n_case[0]}.out"
        n_case[0] += 1
        fin.write_bytes(DM.host_case(planes, channels, cell, per_cell, thr, stride, want, slack))
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        what = (n_case[0], planes.shape, channels, cell, per_cell, thr, stride, want, slack)
        assert p.returncode == 0 and "host check ran" in p.stdout, (what, (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (what, (p.stdout + p.stderr)[-3000:])
        w = DM.model(planes, channels, cell, per_cell, thr)
        g = DM.unpack(fout.read_bytes(), P, w.n_slots, stride)
        skip = [k for k, bit in (("points", 1), ("desc", 2), ("info", 4)) if not want & bit]
        DM.check(g, w, what, skip=skip)
        for k in skip:
            assert DM.filled(getattr(g, k)), (what, k, "an output that was not asked for")
        assert DM.filled(g.rest), (what, "the bytes 32..stride of a descriptor row")
        return w

    rgba = lambda p, s: DM.to_rgba(p, s)
    scene = lambda s, W, H: DM.scene(s, W, H, rects=max(8, W * H // 60), side=14)
    total = 0
    for W, H in ((33, 33), (32, 40), (40, 32), (34, 47), (64, 40), (65, 33), (97, 71)):
        planes = np.stack([scene(W + H, W, H), DM.noise(7 + W, W, H)])
        for k, (cell, per_cell) in enumerate(((8, 1), (8, 16), (16, 2), (32, 1), (32, 16))):
            ch = 1 + 3 * ((k + W) % 2)
            total += int(run(planes if ch == 1 else np.stack([rgba(p, k) for p in planes]), ch, cell, per_cell).counts.sum())
    assert total > 100                                            # the cases bite: the planes hold keypoints (the model counts them)
    big = np.stack([scene(12, 130, 66), DM.noise(11, 130, 66)])
    for cell, per_cell in ((64, 1), (64, 16), (256, 2)):
        assert run(big, 1, cell, per_cell).counts[1] == per_cell * (2 if cell == 64 else 1)
    assert run(DM.constant(97, 71)[None], 1, 16, 2).counts.tolist() == [0]
    run(np.stack([DM.checker(97, 71), DM.checker(97, 71, 0, 255)]), 1, 8, 16)
    run(DM.margin_corners()[None], 1, 16, 16)
    assert run(DM.quadrant(14)[None], 1, 8, 1).counts.tolist() == [1]
    five = [scene(31, 97, 71), DM.noise(32, 97, 71), DM.checker(97, 71), scene(33, 97, 71), DM.constant(97, 71)]
    w = run(np.stack(five[:2]), 1, 16, 2)
    r = np.concatenate([w.info["R"][p, :w.counts[p]] for p in range(2)])
    med = int(np.sort(r)[len(r) // 2])
    assert 0 < run(np.stack(five[:2]), 1, 16, 2, thr=med + 1).counts.sum() < run(np.stack(five[:2]), 1, 16, 2, thr=med).counts.sum() < w.counts.sum()
    assert run(np.stack(five[:2]), 1, 16, 2, thr=int(r.max()) + 1).counts.tolist() == [0, 0]
    for P in (1, 3, 5):
        for ch, stride, slack in ((1, 48, 3), (4, 32, 3), (4, 48, 0), (1, 32, 64)):
            run(np.stack([rgba(p, k) if ch == 4 else p for k, p in enumerate(five[:P])]), ch, 16, 2, stride=stride, slack=slack)
    for want in range(7):
        run(np.stack([rgba(p, k) for k, p in enumerate(five[:3])]), 4, 16, 2, stride=48, want=want)


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_detect_and_describe_over_the_recording_mock_addon():
    """tests/js/detect_class.mjs: h.detectAndDescribe(images, options) packs the pictures back to back; the option defaults; the bare strings
    it throws; the shape of the result, which matchDescriptors takes as it stands."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "detect_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_detect_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ok"] and res["fails"] == [] and p.returncode == 0, (res["fails"], p.stderr[-2000:])
    assert res["checks"] >= 20
