"""CPU-side checks of the mosaic (include/hgwarp.h, hg_mosaic_frames_device): declaration, export and refusals that need no device, the
vectorised numpy model of tests/hgtest/mosaic.py against a scalar model written from the header text, hand-computed cases, the model's own
properties (disjoint frames are pasted, one frame gives itself, LAST is painting in order, a constant stays constant, MEAN's weight plane
counts the contributors), the kernel's source text on the host under sanitizers, and the class's mosaic() over a recording mock."""
import ctypes as C
import functools
import json
import math
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
from hgtest import mosaic as MM              # noqa: E402

INVALID = 1
F32 = np.float32
INF = float("inf")
SW, SH = 37, 23                               # the source whose border the feather weights measure
MODES = (MM.LAST, MM.MEAN, MM.FEATHER)


# ------------------------------------------------------------------------------------------------ symbols and host-only refusals
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    name = "hg_mosaic_frames_device"
    assert name in declared and hasattr(L, name) and name in HG.EXPORTS
    assert name in text[text.index("#define HG_VERSION"):text.index("enum {")]       # how the feature is detected
    assert re.search(r"int hg_mosaic_frames_device\([^;]*int mode, float feather,\s*hg_geom canvas, void \*d_canvas, float \*d_weight\);", code)
    assert re.search(r"enum \{ HG_MOSAIC_LAST = 0, HG_MOSAIC_MEAN = 1, HG_MOSAIC_FEATHER = 2 \};", code)
    assert (HG.MOSAIC_LAST, HG.MOSAIC_MEAN, HG.MOSAIC_FEATHER) == (0, 1, 2) == MODES
    assert callable(HG.Context.mosaic_frames_device)


def test_a_null_context_is_refused_whatever_else_is_passed():
    L = HG.lib()
    g = (HG.Geom * 1)(HG.Geom(0, 0, 4, 4))
    p = C.c_void_p(4096)
    for mode, feather in ((0, 1.0), (2, INF), (3, 1.0), (2, -1.0)):
        assert L.hg_mosaic_frames_device(None, g, 1, p, None, p, None, HG.ELEM_U8, 4, 4, 4, mode, feather, HG.Geom(0, 0, 4, 4), p, None) == INVALID
    assert b"ctx" in L.hg_last_error(None)


# ------------------------------------------------------------------------------------------------ the scalar model, from the header text
def _scalar_mosaic(geoms, fields, frames, W, H, mode, feather, canvas, is_u8, ch, seen):
    cx, cy, cw, chh = canvas
    out = np.zeros((chh, cw, ch), np.uint8 if is_u8 else F32)
    weight = np.zeros((chh, cw), F32)
    for j in range(chh):
        for i in range(cw):
            X, Y = cx + i, cy + j                                                              # 1
            con = []
            for f, (x, y, w, h) in enumerate(geoms):
                if w <= 0 or h <= 0:
                    continue
                u, v = X - x, Y - y                                                            # 2
                if not (0 <= u < w and 0 <= v < h):
                    continue
                sx, sy = fields[f][v * w + u]                                                  # 3
                if not (math.isfinite(sx) and math.isfinite(sy)):
                    continue
                con.append((F32(sx), F32(sy), frames[f].reshape(-1, ch)[v * w + u]))
            seen.add(min(len(con), 3))
            if not con:                                                                        # 4
                continue
            if mode == MM.LAST:                                                                # 5
                out[j, i] = con[-1][2]
                weight[j, i] = 1
                continue
            acc, wsum = [F32(0)] * ch, F32(0)
            with np.errstate(all="ignore"):
                for sx, sy, p in con:                                                          # 6, 7
                    if mode == MM.MEAN:
                        wf = F32(1)
                    else:
                        dx = min(F32(sx + F32(1)), F32(F32(W) - sx))
                        dy = min(F32(sy + F32(1)), F32(F32(H) - sy))
                        wf = max(min(min(dx, dy), F32(feather)), F32(2.0 ** -10))
                    acc = [F32(a + F32(wf * F32(pc))) for a, pc in zip(acc, p)]
                    wsum = F32(wsum + wf)
                weight[j, i] = wsum
                if len(con) == 1:
                    out[j, i] = con[0][2]
                    continue
                r = [F32(a / wsum) for a in acc]
            out[j, i] = [int(min(F32(255), F32(math.floor(F32(v + F32(0.5)))))) for v in r] if is_u8 else r
    return out, weight


MODEL_GEOMS = [(0, 0, 20, 14), (7, 3, 18, 12), (-5, -4, 12, 9), (0, 0, 0, 5), (7, 3, 18, 12), (22, 10, 1, 9), (30, -2, 16, 6), (100, 100, 4, 4), (3, 12, 25, 1)]
MODEL_CANVAS = (-3, -2, 41, 22)


def _field(rng, w, h, f):
    """Coordinates over the source and a little beyond every border, with the entries a caller-made field may carry."""
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    co = np.stack([(SW + 4.0) * i / max(w - 1, 1) - 2 + 0.25 * f, (SH + 3.0) * j / max(h - 1, 1) - 1.5 + 0.125 * f], -1).astype(F32)
    if w * h >= 20:
        co[rng.random((h, w)) < 0.15] = np.nan
        flat = co.reshape(-1, 2)
        flat[1:9] = [[np.nan, 3], [3, np.nan], [np.inf, 2], [2, -np.inf], [1e30, 5], [5, -1e30], [0, SH - 1], [SW - 1, 0]]
        flat[10:13] = [[SW, 4], [SW - 0.5, SH - 0.25], [-1e30, 1e30]]
    return co.reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _model_set(elem, ch):
    """(fields, frames) over MODEL_GEOMS; no uint8 value equals the canvas fill of the host check."""
    rng = np.random.default_rng(100 + 10 * ch + elem)
    fields, frames = [], []
    for f, (_, _, w, h) in enumerate(MODEL_GEOMS):
        n = max(w, 0) * max(h, 0)
        fields.append(_field(rng, w, h, f) if n else np.zeros((0, 2), F32))
        frames.append(rng.integers(1, 160, (n, ch), dtype=np.uint8) if elem == HG.ELEM_U8 else (rng.standard_normal((n, ch)) * 40 + 3).astype(F32))
        fields[-1].setflags(write=False)
        frames[-1].setflags(write=False)
    return fields, frames


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_the_vectorised_model_matches_the_scalar_model():
    seen = set()
    for elem, ch in ((HG.ELEM_U8, 3), (HG.ELEM_F32, 2), (HG.ELEM_U8, 1)):
        fields, frames = _model_set(elem, ch)
        for mode in MODES:
            for feather in ((INF, 2.5) if mode == MM.FEATHER else (1.0,)):
                for canvas in (MODEL_CANVAS, (9, 5, 7, 3)):
                    got, gw = MM.mosaic(MODEL_GEOMS, fields, frames, SW, SH, mode, feather, canvas)
                    want, ww = _scalar_mosaic(MODEL_GEOMS, fields, frames, SW, SH, mode, feather, canvas, elem == HG.ELEM_U8, ch, seen)
                    assert got.dtype == want.dtype and got.shape == want.shape
                    assert np.array_equal(_bits(got), _bits(want)), (elem, ch, mode, feather, canvas, np.argwhere(_bits(got) != _bits(want))[:4].tolist())
                    assert gw.dtype == F32 and np.array_equal(_bits(gw), _bits(ww)), (elem, ch, mode, feather, canvas)
    assert seen == {0, 1, 2, 3}                                   # pixels with no, one, two and more contributors
    co = np.concatenate([f for f in _model_set(HG.ELEM_U8, 3)[0]])
    fin = np.isfinite(co).all(-1)
    assert np.isnan(co).any() and np.isinf(co).any() and (np.abs(co[fin]) >= 1e30).any() and (co[fin][:, 0] >= SW).any() and (co[fin][:, 0] < 0).any()


def test_hand_computed_cases():
    g = [(0, 0, 2, 1), (0, 0, 2, 1)]
    co = [np.array([[3, 3], [4, 3]], F32)] * 2
    px = [np.full((2, 1), 200, np.uint8), np.full((2, 1), 100, np.uint8)]
    out, w = MM.mosaic(g, co, px, 9, 7, MM.MEAN, 1.0, (0, 0, 2, 1))
    assert out.tolist() == [[[150], [150]]] and w.tolist() == [[2, 2]]
    # the feather weight: at sx = 0 and sx = W - 1 one pixel to the border, in the middle of W = 9 five, of H = 7 four
    W, H = 9, 7
    fw = lambda sx, sy, feather=INF: float(MM.feather_weight(np.array([sx, sy], F32), W, H, feather))
    assert fw(0, 3) == 1 and fw(8, 3) == 1 and fw(4, 3) == 4 and fw(4, 0) == 1 and fw(4, 6) == 1 and fw(4, 3.5) == 3.5 and fw(3, 3) == 4
    assert fw(4, 3, 2.0) == 2 and fw(4, 3, 0.5) == 0.5 and fw(0, 3, 2.0) == 1          # the cap
    assert fw(-3, 3) == 2.0 ** -10 and fw(9, 3) == 2.0 ** -10 and fw(1e30, 3) == 2.0 ** -10 and fw(4, -1e30) == 2.0 ** -10 and fw(4, 3, 1e-9) == 2.0 ** -10      # the floor
    # feathered: 200 at the border (w = 1) and 100 in the middle (w = 4): (200 + 400) / 5 = 120; capped at 1: the mean
    co = [np.array([[0, 3]], F32), np.array([[4, 3]], F32)]
    g = [(5, 5, 1, 1), (5, 5, 1, 1)]
    px = [np.full((1, 1), 200, np.uint8), np.full((1, 1), 100, np.uint8)]
    out, w = MM.mosaic(g, co, px, W, H, MM.FEATHER, INF, (5, 5, 1, 1))
    assert out.ravel().tolist() == [120] and w.ravel().tolist() == [5]
    out, w = MM.mosaic(g, co, px, W, H, MM.FEATHER, 1.0, (5, 5, 1, 1))
    assert out.ravel().tolist() == [150] and w.ravel().tolist() == [2]
    out, w = MM.mosaic(g, co, px, W, H, MM.LAST, 1.0, (4, 5, 3, 1))
    assert out.ravel().tolist() == [0, 100, 0] and w.ravel().tolist() == [0, 1, 0]
    # a coordinate outside [0, W) still contributes, at the floor weight: (200 * 2^-10 + 100 * 4) / (4 + 2^-10) rounds to 100
    co = [np.array([[-2, 3]], F32), np.array([[4, 3]], F32)]
    out, w = MM.mosaic(g, co, px, W, H, MM.FEATHER, INF, (5, 5, 1, 1))
    assert out.ravel().tolist() == [100] and w.ravel().tolist() == [4 + 2.0 ** -10]


# ------------------------------------------------------------------------------------------------ properties of the model
def test_disjoint_frames_are_pasted_byte_for_byte_and_one_frame_gives_itself():
    rng = np.random.default_rng(7)
    geoms = [(0, 0, 9, 5), (9, 0, 4, 5), (2, 5, 6, 3), (-4, -3, 4, 3)]
    for dtype, ch in ((np.uint8, 3), (F32, 2)):
        frames = [rng.integers(0, 256, (g[2] * g[3], ch)).astype(dtype) for g in geoms]
        if dtype == F32:
            frames[0][:4, 0] = [np.nan, -0.0, np.inf, 1e-42]       # bit for bit: a NaN, a negative zero, a denormal
        fields = [np.full((g[2] * g[3], 2), 5, F32) for g in geoms]
        fields[1][3] = np.nan
        canvas = (-4, -3, 17, 11)
        paste = np.zeros((11, 17, ch), dtype)
        count = np.zeros((11, 17), F32)
        for g, fr, co in zip(geoms, frames, fields):
            cover = np.isfinite(co).all(-1).reshape(g[3], g[2])
            view = paste[g[1] + 3:g[1] + 3 + g[3], g[0] + 4:g[0] + 4 + g[2]]
            view[cover] = fr.reshape(g[3], g[2], ch)[cover]
            count[g[1] + 3:g[1] + 3 + g[3], g[0] + 4:g[0] + 4 + g[2]] += cover
        assert count.max() == 1
        for mode in MODES:
            out, w = MM.mosaic(geoms, fields, frames, SW, SH, mode, 3.0, canvas)
            assert np.array_equal(_bits(out), _bits(paste)), (dtype, mode)
            assert np.array_equal(w > 0, count > 0)
            for g, fr, co in zip(geoms, frames, fields):          # one frame on its own window: itself where it covers
                one, _ = MM.mosaic([g], [co], [fr], SW, SH, mode, 3.0, g)
                cover = np.isfinite(co).all(-1)
                assert np.array_equal(_bits(one.reshape(-1, ch)[cover]), _bits(fr[cover])) and not _bits(one.reshape(-1, ch)[~cover]).any()


def test_last_is_painting_in_order_and_mean_counts_the_contributors():
    for elem, ch in ((HG.ELEM_U8, 3), (HG.ELEM_F32, 2)):
        fields, frames = _model_set(elem, ch)
        cx, cy, cw, chh = MODEL_CANVAS
        paint = np.zeros((chh, cw, ch), frames[0].dtype)
        count = np.zeros((chh, cw), F32)
        for (x, y, w, h), co, fr in zip(MODEL_GEOMS, fields, frames):
            for v in range(max(h, 0)):
                for u in range(max(w, 0)):
                    i, j = x + u - cx, y + v - cy
                    if 0 <= i < cw and 0 <= j < chh and np.isfinite(co[v * w + u]).all():
                        paint[j, i] = fr[v * w + u]
                        count[j, i] += 1
        out, w1 = MM.mosaic(MODEL_GEOMS, fields, frames, SW, SH, MM.LAST, 1.0, MODEL_CANVAS)
        assert np.array_equal(_bits(out), _bits(paint)) and np.array_equal(w1, (count > 0).astype(F32))
        _, wm = MM.mosaic(MODEL_GEOMS, fields, frames, SW, SH, MM.MEAN, 1.0, MODEL_CANVAS)
        assert np.array_equal(wm, count) and count.max() >= 3


def test_a_constant_u8_value_stays_constant_over_any_overlap():
    fields, _ = _model_set(HG.ELEM_U8, 3)
    for value in (1, 127, 128, 255):
        frames = [np.full((f.shape[0], 3), value, np.uint8) for f in fields]
        for mode, feather in ((MM.LAST, 1.0), (MM.MEAN, 1.0), (MM.FEATHER, INF), (MM.FEATHER, 0.3)):
            out, w = MM.mosaic(MODEL_GEOMS, fields, frames, SW, SH, mode, feather, MODEL_CANVAS)
            assert (out[w > 0] == value).all() and not out[w == 0].any() and (w > 0).any() and (w == 0).any(), (value, mode, feather)


# ------------------------------------------------------------------------------------------------ the kernel's text on the host
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/mosaic_check.cpp: k_mosaic_frames -- hg_k_mosaic.hip itself --, compiled for the CPU behind a thread-index shim and run under ASan + UBSan on exact-size buffers -- no byte outside a buffer is
    touched, whatever the alignment -- and what it computes is the model's, bit for bit: every element type, channel count and mode,
    misaligned frames and canvases, no frames at all.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "mosaic_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "mosaic_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    cases = [(elem, ch, mode, mis, wt, len(MODEL_GEOMS)) for elem in (HG.ELEM_U8, HG.ELEM_F32) for ch in (1, 2, 3, 4)
             for mode, mis, wt in ((MM.LAST, 1, 0), (MM.MEAN, 0, 1), (MM.FEATHER, 1, 1))]
    cases += [(HG.ELEM_U8, 4, MM.FEATHER, 0, 1, len(MODEL_GEOMS)), (HG.ELEM_U8, 2, MM.LAST, 0, 0, len(MODEL_GEOMS)), (HG.ELEM_U8, 4, MM.MEAN, 0, 1, 0), (HG.ELEM_F32, 3, MM.LAST, 1, 1, 0)]
    for case, (elem, ch, mode, mis, wt, n) in enumerate(cases):
        es = 1 if elem == HG.ELEM_U8 else 4
        px = es * ch
        fields, frames = _model_set(elem, ch)
        geoms, fields, frames = MODEL_GEOMS[:n], fields[:n], frames[:n]
        feather = 2.5 if case % 2 else INF
        canvas = MODEL_CANVAS if case % 3 else (-3, -2, 67, 5)
        fo, po, f_end, p_end = [], [], 0, 0
        for f, g in enumerate(geoms):                             # mis: odd multiples of 8 / of the element size; exact ends
            fo.append(f_end + (8 * (2 * f + 1) if mis else 0))
            po.append(p_end + (es * (2 * f + 1) if mis else 0))
            f_end = fo[-1] + fields[f].nbytes
            p_end = po[-1] + frames[f].nbytes
        head = np.array([elem, ch, SW, SH, mode, n, *canvas, 16 + es if mis else 16, 16 + es if mis else 16, wt], np.int32).tobytes()
        head += np.array([feather], F32).tobytes() + np.array([f_end, p_end], np.uint64).tobytes()
        for g, a, b in zip(geoms, fo, po):
            head += np.array(g, np.int32).tobytes() + np.array([a, b], np.uint64).tobytes()
        fld, pix = np.zeros(f_end, np.uint8), np.full(p_end, 0xEE, np.uint8)
        for co, fr, a, b in zip(fields, frames, fo, po):
            fld[a:a + co.nbytes] = _bits(co).ravel()
            pix[b:b + fr.nbytes] = _bits(fr).ravel()
        fin, fout = tmp_path / f"case{case}.in", tmp_path / f"case{case}.out"
        fin.write_bytes(head + fld.tobytes() + pix.tobytes())
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (case, (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (case, (p.stdout + p.stderr)[-3000:])
        raw = np.frombuffer(fout.read_bytes(), np.uint8)
        n_px = canvas[2] * canvas[3]
        assert raw.size == n_px * px + (n_px * 4 if wt else 0), case
        if n:
            want, ww = MM.mosaic(geoms, fields, frames, SW, SH, mode, feather, canvas)
        else:
            want, ww = np.zeros(n_px * px, np.uint8), np.zeros(n_px, F32)
        bad = np.flatnonzero(raw[:n_px * px] != _bits(want).ravel())
        assert bad.size == 0, (case, elem, ch, mode, int(bad.size), (bad[:4] // px).tolist())
        if wt:
            assert np.array_equal(raw[n_px * px:], _bits(ww).ravel()), (case, "weight")


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_mosaic_over_the_recording_mock_addon():
    """tests/js/mosaic_class.mjs: h.mosaic reaches 'mosaicInverse' + family with the windows the class computes, the blend, the feather, the
    canvas (default: the bounding box of the non-blank windows) and the weight flag; it refuses an unknown blend, a bad feather, a canvas
    that is not four integers, `devices` and `sourcePoints`; and the instance ends in the state warpBatch(..., {inverse: true}) leaves."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "mosaic_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_mosaic_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["failures"] == [] and p.returncode == 0, (res["failures"], p.stderr[-2000:])
    assert res["checks"] >= 60
