"""CPU-side checks of the matching feature (include/hgwarp.h, "matching descriptors"): the header declares and the library exports the entry
and its constants, the numpy model of tests/hgtest/match.py is pinned on a case worked by hand, every refusal that needs no device is made,
the kernel text of hg_k_match.hip runs on the host under sanitizers against the model, and the JS class is driven over a recording mock
addon.  tests/test_gpu_match.py compares the device with the model."""
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
from hgtest import match as MM               # noqa: E402

INVALID = 1
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def test_header_declares_and_library_exports_the_match_entry_point():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    name = "hg_match_descriptors_frames_device"
    assert name in declared and hasattr(HG.lib(), name) and name in HG.EXPORTS
    assert re.search(r"enum\s*\{\s*HG_DESC_BITS\s*=\s*0\s*,\s*HG_DESC_U8\s*=\s*1\s*\}", code)
    assert (HG.DESC_BITS, HG.DESC_U8) == (0, 1) == (MM.BITS, MM.U8)
    assert "matching descriptors" in text and "matching descriptors by the presence of " + name in text.split("enum {")[0]
    assert callable(HG.Context.match_descriptors_frames_device)
    TQ, TT = MM.tiles()
    assert TQ >= 16 and TT >= 16                                  # the constants the GPU test sizes its cases by


def test_model_on_a_hand_computed_case():
    """3 queries, 4 train rows, 2 bytes.  q0 = q2 = (0x0F, 0x00), q1 = (0xFF, 0xFF); t0 = t1 = (0x0F, 0x01), t2 = (0xFF, 0xFE), t3 = (0, 0).
    Hamming: q0: t0 1 (the bit of 0x01), t1 1, t2 popc(0xF0) + popc(0xFE) = 4 + 7 = 11, t3 popc(0x0F) = 4; q1: t0 popc(0xF0) + popc(0xFE) = 11,
    t1 11, t2 0 + 1 = 1, t3 16; q2 as q0.  So nn = (0, 1, 1), (2, 1, 11), (0, 1, 1): a tie in the train rows gives the LOWER row and d2 == d1.
    Squared L2: q0: t0 0 + 1 = 1, t1 1, t2 240^2 + 254^2 = 57600 + 64516 = 122116, t3 15^2 = 225; q1: t0 122116, t1 122116, t2 0 + 1 = 1,
    t3 2 * 255^2 = 130050."""
    q = np.array([[[0x0F, 0x00], [0xFF, 0xFF], [0x0F, 0x00]]], np.uint8)
    t = np.array([[[0x0F, 0x01], [0x0F, 0x01], [0xFF, 0xFE], [0x00, 0x00]]], np.uint8)
    qp = np.array([[[1, 2], [3, 4], [5, 6]]], np.float32)
    tp = np.array([[[10, 20], [30, 40], [50, 60], [70, 80]]], np.float32)
    assert MM.distances(MM.BITS, q[0], t[0], 2).tolist() == [[1, 1, 11, 4], [11, 11, 1, 16], [1, 1, 11, 4]]
    assert MM.distances(MM.U8, q[0], t[0], 2).tolist() == [[1, 1, 122116, 225], [122116, 122116, 1, 130050], [1, 1, 122116, 225]]
    assert MM.distances(MM.BITS, q[0], t[0], 1).tolist() == [[0, 0, 4, 4], [4, 4, 0, 8], [0, 0, 4, 4]]           # the second byte is padding
    pad = [-1, -1]
    nan4 = [MM.PAD_WORD] * 4
    w = lambda a: np.asarray(a, np.float32).view(np.uint32).tolist()
    # ratio 0.8: the tied queries fail (1 < 0.8 * 1 is false), q1 passes (1 < 0.8 * 11)
    r = MM.match(MM.BITS, 2, q, t, ratio=0.8, qpts=qp, tpts=tp)
    assert r.nn.tolist() == [[[0, 1, 1, 0], [2, 1, 11, 1], [0, 1, 1, 0]]]
    assert r.counts.tolist() == [1] and r.pairs.tolist() == [[[1, 2], pad, pad]]
    assert r.matches.tolist() == [[w([3, 4, 50, 60]), nan4, nan4]]
    # no ratio test: all three, in ascending i
    r = MM.match(MM.BITS, 2, q, t, ratio=0, qpts=qp, tpts=tp)
    assert r.counts.tolist() == [3] and r.pairs.tolist() == [[[0, 0], [1, 2], [2, 0]]]
    assert r.matches.tolist() == [[w([1, 2, 10, 20]), w([3, 4, 50, 60]), w([5, 6, 10, 20])]]
    # cross-check: t0's nearest queries are q0 and q2 at distance 1: the lower one, q0, keeps the pair
    r = MM.match(MM.BITS, 2, q, t, ratio=0, cross_check=True)
    assert r.counts.tolist() == [2] and r.pairs.tolist() == [[[0, 0], [1, 2], pad]] and r.nn[0, :, 3].tolist() == [1, 1, 0]
    assert (r.matches == MM.PAD_WORD).all()                      # (no points: the model leaves the padding everywhere)
    # ratio 1.0 still rejects a tie; the cap 0 rejects d1 = 1; one train row: no d2, the ratio test passes
    assert MM.match(MM.BITS, 2, q, t, ratio=1.0).counts.tolist() == [1]
    assert MM.match(MM.BITS, 2, q, t, ratio=0, max_distance=0).counts.tolist() == [0]
    r = MM.match(MM.BITS, 2, q, t, counts_t=[1], ratio=0.5)
    assert r.nn.tolist() == [[[0, 1, -1, 1], [0, 11, -1, 1], [0, 1, -1, 1]]] and r.counts.tolist() == [3]
    # counts: two queries, no train row
    r = MM.match(MM.BITS, 2, q, t, counts_q=[2], counts_t=[0], ratio=0)
    assert r.counts.tolist() == [0] and (r.nn == [-1, -1, -1, 0]).all() and (r.pairs == -1).all()
    # bytes: the squared ratio: 1 < 0.64 * 122116
    r = MM.match(MM.U8, 2, q, t, ratio=0.8)
    assert r.nn.tolist() == [[[0, 1, 1, 0], [2, 1, 122116, 1], [0, 1, 1, 0]]]


def test_refusals_without_a_device():
    """The shape checks come before the context is looked at, in the header's order: each one is reached with a NULL context and names itself
    in hg_last_error; a call that passes them all is refused for the NULL context."""
    L = HG.lib()
    ok = dict(kind=0, desc_bytes=32, stride=32, n_query=8, counts_q=None, n_frames=2, n_train=8, counts_t=None, n_train_sets=1, ratio=0.8)

    def call(**k):
        a = dict(ok, **k)
        cq = (C.c_int32 * len(a["counts_q"]))(*a["counts_q"]) if a["counts_q"] is not None else None
        ct = (C.c_int32 * len(a["counts_t"]))(*a["counts_t"]) if a["counts_t"] is not None else None
        code = L.hg_match_descriptors_frames_device(None, a["kind"], a["desc_bytes"], a["stride"], None, a["n_query"], cq, a["n_frames"], None, a["n_train"], ct,
                                                    a["n_train_sets"], a["ratio"], 0xffffffff, 0, None, None, None, None, None, None)
        return code, L.hg_last_error(None).decode()

    for k, word in ((dict(kind=2), "kind"), (dict(kind=-1), "kind"),
                    (dict(desc_bytes=0), "desc_bytes"), (dict(desc_bytes=513, stride=528), "desc_bytes"),
                    (dict(stride=40), "stride"), (dict(stride=16), "stride"), (dict(stride=0), "stride"),
                    (dict(n_query=-1), "n_query"), (dict(n_query=65537), "n_query"),
                    (dict(n_train=-1), "n_train"), (dict(n_train=65537), "n_train"),
                    (dict(n_frames=-1), "n_frames"), (dict(n_frames=4097), "n_frames"),
                    (dict(n_train_sets=0), "n_train_sets"), (dict(n_train_sets=3), "n_train_sets"), (dict(n_frames=0, n_train_sets=2), "n_train_sets"),
                    (dict(counts_q=[8, 9]), "counts_q[1]"), (dict(counts_q=[-1, 8]), "counts_q[0]"),
                    (dict(counts_t=[9]), "counts_t[0]"), (dict(counts_t=[-1]), "counts_t[0]"),
                    (dict(ratio=-0.1), "ratio"), (dict(ratio=1.5), "ratio"), (dict(ratio=float("nan")), "ratio"), (dict(ratio=float("inf")), "ratio")):
        code, msg = call(**k)
        assert code == INVALID and word in msg and "ctx" not in msg, (k, msg)
    # the order: a bad kind is named before a bad stride, a bad stride before a bad count
    assert "kind" in call(kind=5, stride=7, counts_q=[99, 0])[1] and "stride" in call(stride=7, counts_q=[99, 0])[1]
    # the limits themselves are legal: what is missing is the context
    for k in (dict(), dict(desc_bytes=512, stride=512, n_query=65536, n_train=65536, n_frames=4096, n_train_sets=4096, ratio=1.0),
              dict(desc_bytes=1, stride=16, n_query=0, n_train=0, n_frames=0, ratio=0.0)):
        code, msg = call(**k)
        assert code == INVALID and "ctx" in msg, (k, msg)


# ------------------------------------------------------------------------------------------------ the kernel text on the host
@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/match_check.cpp: hg_k_match.hip itself, compiled for the CPU behind the thread-index shim -- a workgroup of k_match_bits as
    64 and of k_match_finish as 256 host threads -- and run under ASan + UBSan on exact-size heap buffers: no byte outside a buffer is
    touched, and every output equals the model's byte for byte.  The cases are the GPU test's for HG_DESC_BITS at their smallest sizes; the
    matrix-core kernel of HG_DESC_U8 cannot run on a host and is pinned by the GPU test alone.  A stand-alone program; nothing is loaded
    into Python."""
    exe = str(tmp_path / "match_check")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", os.path.join(cpp, "hip_stub"), "-I", CSRC, os.path.join(cpp, "match_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    n_case = [0]

    def run(c, ratio=0.8, max_distance=MM.NO_CAP, cross=False, want=7, points=True):
        F, nq = c.query.shape[:2]
        S, nt = c.train.shape[:2]
        cq = np.asarray([nq] * F if c.counts_q is None else c.counts_q, np.int32)
        ct = np.asarray([nt] * S if c.counts_t is None else c.counts_t, np.int32)
        fin, fout = tmp_path / f"case{n_case[0]}.in", tmp_path / f"case{n_case[0]}.out"
        n_case[0] += 1
        head = struct.pack("<10iIid", c.desc_bytes, c.stride, F, nq, nt, S, int(cross), 1 if ratio != 0 else 0, 1 if points else 0, want,
                           max_distance, 0, float(ratio))
        fin.write_bytes(head + cq.tobytes() + ct.tobytes() + c.query.tobytes() + c.train.tobytes() + (c.qpts.tobytes() + c.tpts.tobytes() if points else b""))
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (n_case[0], (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (n_case[0], (p.stdout + p.stderr)[-3000:])
        g = MM.unpack(fout.read_bytes(), F, nq)
        w = MM.model(c, ratio, max_distance, bool(cross), points=points and bool(want & 1))
        skip = [k for k, bit in (("matches", 1), ("pairs", 2), ("nn", 4)) if not (want & bit) or (k == "matches" and not points)]
        MM.check(g, w, (c.desc_bytes, c.stride, nq, nt, ratio, max_distance, cross, want), skip=skip)
        for k in skip:
            assert (g.raw[k] == 0xA5).all(), (k, "an output that was not asked for")
        return g, w

    TQ, TT = MM.tiles()
    for nq, nt in ((0, 5), (1, 2), (17, 0), (16, 1), (15, 17), (TQ - 1, TT + 1), (TQ, TT - 1), (TQ + 1, TT), (3, 2 * TT + 1)):
        run(MM.near_case(300 + nq + nt, MM.BITS, 3, nq, nt, 32, counts_q=[nq, min(5, nq), 0] if nq > 5 else None), cross=(nq + nt) % 2 == 0)
    for nb in (1, 3, 4, 31, 32, 33, 61, 64, 128, 512):
        base = (nb + 15) // 16 * 16
        for stride in (base, base + 32):
            run(MM.near_case(400 + nb, MM.BITS, 2, 21, 19, nb, stride=stride, S=1), ratio=0.9, cross=True)
    c = MM.near_case(500, MM.BITS, 3, 70, 67, 32, S=2, counts_q=[70, 0, 33], counts_t=[67, 9])
    g, w = run(c, ratio=0.0)
    med = int(np.median(w.nn[0, :70, 1]))
    for ratio in (0.0, 0.5, 0.8, 1.0):
        for cap in (0, med, MM.NO_CAP):
            for cross in (False, True):
                run(c, ratio, cap, cross)
    assert 0 < run(c, 0.8, med, True)[1].counts.sum() < run(c, 0.0)[1].counts.sum()      # the tests bite: some pass, some do not
    for want in (0, 1, 2, 4, 6):
        run(c, want=want)
    run(c, points=False)
    c.train[0, 1] = c.train[0, 0]                                 # a tie in the train rows; duplicate queries under the cross-check
    c.query[0, 1, :32] = c.train[0, 0, :32]
    c.query[0, 5] = c.query[0, 1]
    g, w = run(c, ratio=0.0, cross=True)
    assert w.nn[0, 1].tolist() == [0, 0, 0, 1] and w.nn[0, 5].tolist() == [0, 0, 0, 0]
    assert run(c, ratio=1.0)[1].nn[0, 1, 3] == 0


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_match_descriptors_over_the_recording_mock_addon():
    """tests/js/match_class.mjs: h.matchDescriptors(querySets, trainSets, options) pads the sets to the longest and a stride of 16, hands
    their lengths down as counts; the option defaults; the bare strings it throws; the shape of the result."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "match_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_match_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ok"] and res["fails"] == [] and p.returncode == 0, (res["fails"], p.stderr[-2000:])
    assert res["checks"] >= 20
