"""CPU-side checks of the multi-band mosaic (include/hgwarp.h, hg_mosaic_multiband_device / hg_mosaic_multiband_layout): declaration, export
and the refusals that need no device; the numpy model of tests/hgtest/multiband.py against independent statements of what it must give
(n_bands == 1 is a paste by label, a single frame gives itself at any band count, a constant stays a constant); the seam step and the
ghosting it is built to remove, measured on the model; the layout of the work area against hand-worked sizes; and the kernels' source
text on the host under sanitizers."""
import ctypes as C
import functools
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
from hgtest import multiband as MB           # noqa: E402

INVALID = 1
F32 = np.float32
INF = float("inf")
SW, SH = 37, 23                               # the source whose border the ranks measure

MODEL_GEOMS = [(0, 0, 20, 14), (7, 3, 18, 12), (-5, -4, 12, 9), (0, 0, 0, 5), (7, 3, 18, 12), (22, 10, 1, 1), (30, -2, 16, 6), (100, 100, 4, 4), (3, 12, 25, 1)]
MODEL_CANVAS = (-3, -2, 41, 22)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _field(rng, w, h, f):
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    co = np.stack([(SW + 4.0) * i / max(w - 1, 1) - 2 + 0.25 * f, (SH + 3.0) * j / max(h - 1, 1) - 1.5 + 0.125 * f], -1).astype(F32)
    if w * h >= 20:
        co[rng.random((h, w)) < 0.15] = np.nan
        flat = co.reshape(-1, 2)
        flat[1:9] = [[np.nan, 3], [3, np.nan], [np.inf, 2], [2, -np.inf], [1e30, 5], [5, -1e30], [0, SH - 1], [SW - 1, 0]]
    return co.reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _model_set(elem, ch):
    rng = np.random.default_rng(300 + 10 * ch + elem)
    fields, frames = [], []
    for f, (_, _, w, h) in enumerate(MODEL_GEOMS):
        n = max(w, 0) * max(h, 0)
        fields.append(_field(rng, w, h, f) if n else np.zeros((0, 2), F32))
        frames.append(rng.integers(1, 160, (n, ch), dtype=np.uint8) if elem == HG.ELEM_U8 else (rng.standard_normal((n, ch)) * 40 + 3).astype(F32))
        fields[-1].setflags(write=False)
        frames[-1].setflags(write=False)
    return fields, frames


# ------------------------------------------------------------------------------------------------ symbols and host-only refusals
def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in ("hg_mosaic_multiband_device", "hg_mosaic_multiband_layout"):
        assert name in declared and hasattr(L, name) and name in HG.EXPORTS
    assert "hg_mosaic_multiband_device" in text[text.index("#define HG_VERSION"):text.index("enum {")]       # how the feature is detected
    assert re.search(r"int hg_mosaic_multiband_device\([^;]*float feather, int n_bands,\s*hg_geom canvas, void \*d_canvas, float \*d_weight, int32_t \*d_labels,"
                     r"\s*const float \*gains, void \*d_work, size_t work_bytes\);", code)
    assert callable(HG.Context.mosaic_multiband_device) and callable(HG.mosaic_multiband_layout)


def test_refusals_that_need_no_device():
    L = HG.lib()
    g = (HG.Geom * 1)(HG.Geom(0, 0, 4, 4))
    p = C.c_void_p(4096)
    cv = HG.Geom(0, 0, 4, 4)
    for bands, feather in ((5, 1.0), (0, 1.0), (9, 1.0), (3, -1.0), (3, float("nan"))):      # a NULL context is refused whatever else is passed
        assert L.hg_mosaic_multiband_device(None, g, 1, p, None, p, None, HG.ELEM_U8, 4, 4, 4, feather, bands, cv, p, None, None, None, p, 1 << 20) == INVALID
    assert b"ctx" in L.hg_last_error(None)
    n = C.c_size_t(77)
    ok = lambda *a: L.hg_mosaic_multiband_layout(*a)
    assert ok(g, 1, cv, 4, 5, C.byref(n)) == 0 and n.value > 0
    assert ok(g, 1, cv, 4, 5, None) == INVALID and b"work_bytes" in L.hg_last_error(None)
    for bands in (0, 9, -1):
        assert ok(g, 1, cv, 4, bands, C.byref(n)) == INVALID
    for ch in (0, 5):
        assert ok(g, 1, cv, ch, 3, C.byref(n)) == INVALID
    assert ok(g, -1, cv, 4, 3, C.byref(n)) == INVALID and ok(g, 65536, cv, 4, 3, C.byref(n)) == INVALID and ok(None, 1, cv, 4, 3, C.byref(n)) == INVALID
    assert ok(g, 1, HG.Geom((1 << 26) + 1, 0, 4, 4), 4, 3, C.byref(n)) == INVALID                 # beyond the hg_geom limits
    assert ok((HG.Geom * 1)(HG.Geom(0, 0, 1 << 16, (1 << 15) + 1)), 1, cv, 4, 3, C.byref(n)) == INVALID
    assert ok(None, 0, cv, 1, 1, C.byref(n)) == 0 and n.value == 256                               # no frames: the labels alone
    assert ok(g, 1, HG.Geom(0, 0, 0, 4), 4, 5, C.byref(n)) == 0 and n.value == 0                   # an empty canvas needs nothing
    with pytest.raises(HG.HgError):
        HG.mosaic_multiband_layout([(0, 0, 4, 4)], (0, 0, 4, 4), 4, 9)


# ------------------------------------------------------------------------------------------------ n_bands == 1, stated independently
def test_one_band_is_a_paste_by_label():
    """Three lines of numpy that do not call the pyramid code: the label is the argmax of the feather weight over the contributors, the
    lowest index on ties, and the canvas is the label frame's pixel."""
    for elem, ch in ((HG.ELEM_U8, 3), (HG.ELEM_F32, 2), (HG.ELEM_U8, 4)):
        fields, frames = _model_set(elem, ch)
        for feather in (INF, 2.5):
            cx, cy, cw, chh = MODEL_CANVAS
            rank = np.full((len(MODEL_GEOMS), chh, cw), -1, F32)
            pix = np.zeros((len(MODEL_GEOMS), chh, cw, ch), frames[0].dtype)
            for f, (x, y, w, h) in enumerate(MODEL_GEOMS):
                for v in range(max(h, 0)):
                    for u in range(max(w, 0)):
                        i, j = x + u - cx, y + v - cy
                        co = fields[f][v * w + u]
                        if 0 <= i < cw and 0 <= j < chh and np.isfinite(co).all():
                            rank[f, j, i] = MM.feather_weight(co, SW, SH, feather)
                            pix[f, j, i] = frames[f][v * w + u]
            label = np.where(rank.max(0) > 0, rank.argmax(0), -1)                                           # (argmax: the first of equals)
            paste = np.where((label >= 0)[..., None], np.take_along_axis(pix, np.maximum(label, 0)[None, ..., None], 0)[0], 0)
            out, wt, lab = MB.multiband(MODEL_GEOMS, fields, frames, SW, SH, feather, 1, MODEL_CANVAS)
            assert np.array_equal(lab, label) and (label == -1).any() and len(np.unique(label)) >= 6
            assert np.array_equal(_bits(out), _bits(paste.astype(out.dtype))), (elem, ch, feather)
            assert np.array_equal(wt, (label >= 0).astype(F32))
    g = [(0, 0, 6, 4), (6, 0, 5, 4), (0, 4, 11, 2)]                                                       # no overlap: HG_MOSAIC_LAST
    rng = np.random.default_rng(3)
    fr = [rng.integers(0, 256, (w * h, 3), dtype=np.uint8) for _, _, w, h in g]
    co = [np.full((w * h, 2), 5, F32) for _, _, w, h in g]
    assert np.array_equal(MB.multiband(g, co, fr, SW, SH, INF, 1, (-1, -1, 13, 8))[0], MM.mosaic(g, co, fr, SW, SH, MM.LAST, 1.0, (-1, -1, 13, 8))[0])
    gains = [1.25, 0.5, 2.0]                                                                              # gained u8: rounded as the gain mosaic rounds
    from hgtest import mosaic_gain as MG
    assert np.array_equal(MB.multiband(g, co, fr, SW, SH, INF, 1, (-1, -1, 13, 8), gains)[0], MG.mosaic_gain(g, co, fr, SW, SH, MM.LAST, 1.0, (-1, -1, 13, 8), gains)[0])


def test_a_single_u8_frame_with_a_nan_hole_gives_its_own_bytes():
    rng = np.random.default_rng(11)
    g = [(3, -2, 29, 17)]
    px = rng.integers(0, 256, (29 * 17, 3), dtype=np.uint8)
    co = np.full((17, 29, 2), 9, F32)
    co[5:9, 10:16] = np.nan
    cover = np.isfinite(co).all(-1)
    for bands in range(2, 7):
        for canvas in ((3, -2, 29, 17), (5, 0, 20, 9)):
            out, wt, lab = MB.multiband(g, [co.reshape(-1, 2)], [px], SW, SH, INF, bands, canvas)
            ys, xs = slice(canvas[1] + 2, canvas[1] + 2 + canvas[3]), slice(canvas[0] - 3, canvas[0] - 3 + canvas[2])
            want, cov = px.reshape(17, 29, 3)[ys, xs], cover[ys, xs]
            assert np.array_equal(out[cov], want[cov]) and not out[~cov].any(), (bands, canvas)
            assert np.array_equal(lab, np.where(cov, 0, -1)) and np.array_equal(wt, cov.astype(F32))


# ------------------------------------------------------------------------------------------------ what the blend is for
def split_fields(w=64, h=16, at=32):
    """Two full-coverage fields on one w x h window whose ranks make columns < at frame 0's: frame 0 looks at the middle of the source left of
    the split and at its border right of it, frame 1 the other way round."""
    i = np.tile(np.arange(w), (h, 1))
    mid, edge = [SW // 2, SH // 2], [0, SH // 2]
    co0 = np.where((i < at)[..., None], mid, edge).astype(F32).reshape(-1, 2)
    co1 = np.where((i < at)[..., None], edge, mid).astype(F32).reshape(-1, 2)
    return [(0, 0, w, h)] * 2, [co0, co1], (0, 0, w, h)


def seam_steps(run):
    """Largest difference between neighbouring columns of the 100 | 140 canvas for bands 1..5, from run(geoms, fields, frames, bands, canvas)."""
    g, co, cv = split_fields()
    fr = [np.full((64 * 16, 1), 100, np.uint8), np.full((64 * 16, 1), 140, np.uint8)]
    return [int(np.abs(np.diff(run(g, co, fr, b, cv)[0][..., 0].astype(int), axis=1)).max()) for b in range(1, 6)]


def check_seam_steps(steps):
    assert steps[0] == 40
    assert all(b <= a for a, b in zip(steps, steps[1:])), steps        # it does not grow with the band count
    assert steps[4] < 40


def test_the_seam_step_shrinks_with_the_band_count_and_a_constant_stays():
    """Measured on the model (EXPERIMENTS.md "Multi-band"): 40, 22, 18, 17, 16 for 1..5 bands."""
    run = lambda g, co, fr, b, cv: MB.multiband(g, co, fr, SW, SH, INF, b, cv)
    g, co, cv = split_fields()
    lab = MB.labels(g, co, SW, SH, INF, cv)[0]
    assert (lab[:, :32] == 0).all() and (lab[:, 32:] == 1).all()
    steps = seam_steps(run)
    print("seam steps, bands 1..5:", steps)
    check_seam_steps(steps)
    for value in (1, 77, 255):
        fr = [np.full((64 * 16, 3), value, np.uint8)] * 2
        for b in range(1, 6):
            assert (run(g, co, fr, b, cv)[0] == value).all(), (value, b)


GHOST_DISTANCE, GHOST_RESIDUAL = 0, 0         # measured on the model: from the seam's own columns on every pixel IS its own frame's stripe (both
#                                               frames have the same mean, so the low bands blend equal content and the stripes live in level 0 alone)


def ghosting(run):
    """Two frames of one-pixel vertical stripes in anti-phase, split at column 32: per column distance d = 0..31 from the seam the largest
    |canvas - own frame| at 5 bands, from run(geoms, fields, frames, bands, canvas)."""
    g, co, cv = split_fields()
    i = np.tile(np.arange(64), (16, 1))
    a = np.where(i % 2 == 0, 200, 50).astype(np.uint8)
    fr = [a.reshape(-1, 1), (250 - a).reshape(-1, 1)]
    out = run(g, co, fr, 5, cv)[0][..., 0].astype(int)
    own = np.where(i < 32, a, 250 - a).astype(int)
    err = np.abs(out - own).max(0)
    return np.array([max(err[31 - d], err[32 + d]) for d in range(32)])


def test_stripes_in_anti_phase_stay_stripes_where_feathering_gives_grey():
    g, co, cv = split_fields()
    i = np.tile(np.arange(64), (16, 1))
    a = np.where(i % 2 == 0, 200, 50).astype(np.uint8)
    fr = [a.reshape(-1, 1), (250 - a).reshape(-1, 1)]
    co_even = [np.full((64 * 16, 2), [SW // 2, SH // 2], F32)] * 2                                 # equal weights everywhere: the uncapped feather at a seam
    fe = MM.mosaic(g, co_even, fr, SW, SH, MM.FEATHER, INF, cv)[0][..., 0]
    assert (fe == 125).all()                                                                       # mid-grey: the stripes are gone
    err = ghosting(lambda g, co, fr, b, cv: MB.multiband(g, co, fr, SW, SH, INF, b, cv))
    print("ghosting residual by distance from the seam:", err.tolist())
    assert err[GHOST_DISTANCE:].max() <= GHOST_RESIDUAL + 1, err.tolist()
    own_contrast = 150
    assert err[GHOST_DISTANCE:].max() < own_contrast // 4                                          # the stripes (contrast 150) survive


# ------------------------------------------------------------------------------------------------ the layout
def test_layout_hand_worked_aligned_and_monotone():
    one = [(0, 0, 5, 3)]
    # L = 1, A = 1: labels 5 * 3 * 4 = 60 -> 256; the grid [-1, 6) x [-1, 4) = 35 flag bytes -> 256
    assert MB.layout(one, (0, 0, 5, 3), 3, 1)[1] == 512 == HG.mosaic_multiband_layout(one, (0, 0, 5, 3), 3, 1)
    # L = 3, A = 4: labels 256; grid [-4, 12) x [-4, 8) = 16 x 12 = 192 -> 256; level 1: 8 x 6 = 48 px: I 576 -> 768, M 192 -> 256; level 2: 4 x 3:
    # I 144 -> 256, M 48 -> 256; R on the canvas grid 16 x 12: level 1 576 -> 768, level 2 144 -> 256
    assert MB.layout(one, (0, 0, 5, 3), 3, 3)[1] == 256 + 256 + 768 + 256 + 256 + 256 + 768 + 256 == HG.mosaic_multiband_layout(one, (0, 0, 5, 3), 3, 3)
    for geoms, canvas in ((MODEL_GEOMS, MODEL_CANVAS), (MODEL_GEOMS, (9, 5, 7, 3)), ([], (0, 0, 70, 9)), (MODEL_GEOMS[:3], (400, 400, 5, 5)), (one, (-7, -9, 300, 200))):
        for ch in (1, 4):
            for bands in range(1, 9):
                parts, total = MB.layout(geoms, canvas, ch, bands)
                assert total == HG.mosaic_multiband_layout(geoms, canvas, ch, bands), (canvas, ch, bands)
                offs = [o for _, o, _ in parts]
                assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and len(set(offs)) == len(offs)
                assert all(o + n <= nxt for (_, o, n), nxt in zip(parts, offs[1:] + [total]))
                assert parts[0][0] == "labels" and [p[0] for p in parts if p[0][0] == "R"] == [("R", k) for k in range(1, bands)]
    # the header's figure: 64 frames of 3840 x 2160, u8 x 4, 5 bands
    assert HG.mosaic_multiband_layout([(0, 0, 3840, 2160)] * 64, (0, 0, 3840, 2160), 4, 5) == 4228678656


# ------------------------------------------------------------------------------------------------ the kernels' text on the host
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def write_case(path, geoms, fields, frames, elem, ch, feather, bands, canvas, gains=None, mis=0, weight=1, own_labels=1):
    """The input file of tests/cpp/multiband_check.cpp (its header comment names the words); fields and frames lie back to back, at odd
    multiples of 8 bytes / of the element size with `mis`, and both buffers end with their last byte."""
    es = 1 if elem == HG.ELEM_U8 else 4
    fo, po, f_end, p_end = [], [], 0, 0
    for f in range(len(geoms)):
        fo.append(f_end + (8 * (2 * f + 1) if mis else 0))
        po.append(p_end + (es * (2 * f + 1) if mis else 0))
        f_end, p_end = fo[-1] + fields[f].nbytes, po[-1] + frames[f].nbytes
    parts, total = MB.layout(geoms, canvas, ch, bands)
    at = {name: off for name, off, _ in parts}
    gr = MB.grids(geoms, canvas, bands)
    part = [f for f, g in enumerate(gr) if g is not None]
    pw, ph = MB.canvas_grid(canvas, bands)
    head = np.array([elem, ch, SW, SH, bands, len(geoms), *canvas, 16 + es if mis else 0, es if mis else 0, weight, own_labels, len(part), pw, ph], np.int32).tobytes()
    head += np.array([feather], F32).tobytes()
    head += np.array([f_end, p_end, at["labels"], total] + [at.get(("R", k), 0) for k in range(8)], np.uint64).tobytes()
    for f, g in enumerate(geoms):
        head += np.array(g, np.int32).tobytes() + np.array([fo[f], po[f]], np.uint64).tobytes() + np.array([1.0 if gains is None else gains[f]], F32).tobytes()
    for f in part:
        head += np.array([f, *gr[f]], np.int32).tobytes()
        head += np.array([at[("flags", f)]] + [at.get(("I", f, k), 0) for k in range(8)] + [at.get(("M", f, k), 0) for k in range(8)], np.uint64).tobytes()
    fld, pix = np.zeros(f_end, np.uint8), np.full(p_end, 0xEE, np.uint8)
    for co, fr, a, b in zip(fields, frames, fo, po):
        fld[a:a + co.nbytes] = _bits(co).ravel()
        pix[b:b + fr.nbytes] = _bits(fr).ravel()
    path.write_bytes(head + fld.tobytes() + pix.tobytes())


@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/multiband_check.cpp: hg_k_multiband.hip itself, compiled for the CPU behind the thread-index shim and run under ASan + UBSan
    on exact-size buffers, gives the model's canvas, weight plane and labels bit for bit.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "multiband_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    "-Wno-everything", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "multiband_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    rng = np.random.default_rng(21)
    one = lambda w, h, elem, ch: (rng.integers(1, 160, (w * h, ch), dtype=np.uint8) if elem == HG.ELEM_U8 else (rng.standard_normal((w * h, ch)) * 40 + 3).astype(F32))
    cases = []
    for elem, ch, bands, mis in ((HG.ELEM_U8, 4, 3, 0), (HG.ELEM_F32, 3, 2, 1), (HG.ELEM_U8, 2, 1, 1), (HG.ELEM_F32, 1, 4, 0), (HG.ELEM_U8, 3, 5, 1)):
        fields, frames = _model_set(elem, ch)
        cases.append((MODEL_GEOMS, fields, frames, elem, ch, 2.5 if mis else INF, bands, MODEL_CANVAS, [1.0 + 0.1 * f for f in range(len(MODEL_GEOMS))] if mis else None, mis))
    g = [(-9, -6, 11, 8), (-2, -3, 1, 1), (1, 1, 7, 3)]                       # a frame at negative offsets, a 1 x 1 frame, L = 8 on a 9 x 5 canvas
    cases.append((g, [np.full((w * h, 2), [3 + f, 4], F32) for f, (_, _, w, h) in enumerate(g)], [one(w, h, HG.ELEM_U8, 4) for _, _, w, h in g], HG.ELEM_U8, 4, INF, 8, (-4, -3, 9, 5), None, 0))
    cases.append(([], [], [], HG.ELEM_F32, 2, 1.0, 3, (0, 0, 7, 3), None, 0))   # no frames
    cases.append((g, cases[-2][1], cases[-2][2], HG.ELEM_U8, 4, INF, 2, (-4, -3, 1, 1), None, 1))      # a 1 x 1 canvas
    for case, (geoms, fields, frames, elem, ch, feather, bands, canvas, gains, mis) in enumerate(cases):
        fin, fout = tmp_path / f"case{case}.in", tmp_path / f"case{case}.out"
        write_case(fin, geoms, fields, frames, elem, ch, feather, bands, canvas, gains, mis, weight=case % 2 == 0, own_labels=case % 3 != 0)
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (case, (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (case, (p.stdout + p.stderr)[-3000:])
        raw = np.frombuffer(fout.read_bytes(), np.uint8)
        n_px, px = canvas[2] * canvas[3], ch * (1 if elem == HG.ELEM_U8 else 4)
        wt = n_px * 4 if case % 2 == 0 else 0
        assert raw.size == n_px * px + wt + n_px * 4, case
        want, ww, lab = MB.multiband(geoms, fields, frames, SW, SH, feather, bands, canvas, gains, like=(np.uint8 if elem == HG.ELEM_U8 else F32, ch))
        assert np.array_equal(raw[n_px * px + wt:].view(np.int32), lab.ravel()), (case, "labels")
        bad = np.flatnonzero(raw[:n_px * px] != _bits(want).ravel())
        assert bad.size == 0, (case, elem, ch, bands, int(bad.size), (bad[:4] // px).tolist())
        if wt:
            assert np.array_equal(raw[n_px * px:n_px * px + wt], _bits(ww).ravel()), (case, "weight")
