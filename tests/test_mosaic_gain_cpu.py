"""CPU-side checks of the mosaic's exposure entries (include/hgwarp.h: hg_mosaic_overlap_stats_device, hg_mosaic_solve_gains,
hg_mosaic_frames_gain_device): declaration, export and refusals that need no device, the vectorised numpy models of
tests/hgtest/mosaic_gain.py against scalar models written from the header text, hand-computed cases, the host solve against a float64
reference and its properties, the whole sequence on the model, the kernels' source text on the host under sanitizers, and the class's
mosaic({exposure}) over a recording mock."""
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
from hgtest import mosaic_gain as MG         # noqa: E402

INVALID = 1
F32 = np.float32
INF = float("inf")
SW, SH = 37, 23
NAMES = ("hg_mosaic_overlap_stats_device", "hg_mosaic_solve_gains", "hg_mosaic_frames_gain_device")


# ------------------------------------------------------------------------------------------------ symbols and host-only refusals
def test_header_declares_and_library_exports_the_three_entries():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NAMES:
        assert name in declared and hasattr(L, name) and name in HG.EXPORTS, name
    assert NAMES[0] in text[text.index("#define HG_VERSION"):text.index("enum {")]       # how the feature is detected
    assert re.search(r"int hg_mosaic_overlap_stats_device\([^;]*int channels, hg_geom canvas, uint64_t \*d_stats\);", code)
    assert re.search(r"int hg_mosaic_solve_gains\(const uint64_t \*stats, int n_frames, int channels,\s*double sigma_n, double sigma_g, float \*gains\);", code)
    assert re.search(r"int hg_mosaic_frames_gain_device\([^;]*hg_geom canvas, void \*d_canvas, float \*d_weight,\s*const float \*gains\);", code)
    assert callable(HG.Context.mosaic_overlap_stats_device) and callable(HG.mosaic_solve_gains)
    assert "gains" in HG.Context.mosaic_frames_device.__code__.co_varnames


def test_a_null_context_is_refused_whatever_else_is_passed():
    L = HG.lib()
    g = (HG.Geom * 1)(HG.Geom(0, 0, 4, 4))
    p = C.c_void_p(4096)
    one = (C.c_float * 1)(1.0)
    for gains in (None, one):
        assert L.hg_mosaic_frames_gain_device(None, g, 1, p, None, p, None, HG.ELEM_U8, 4, 4, 4, 1, 1.0, HG.Geom(0, 0, 4, 4), p, None, gains) == INVALID
        assert b"ctx" in L.hg_last_error(None)
    for ch in (4, 9):
        assert L.hg_mosaic_overlap_stats_device(None, g, 1, p, None, p, None, ch, HG.Geom(0, 0, 4, 4), p) == INVALID
        assert b"ctx" in L.hg_last_error(None)


def _solve_code(stats, n, channels, sn, sg, gains=True):
    st = np.ascontiguousarray(stats, np.uint64).ravel()
    out = np.full(max(n, 1), 7.0, F32)
    code = HG.lib().hg_mosaic_solve_gains(st.ctypes.data_as(C.POINTER(C.c_uint64)) if st.size else None, n, channels, sn, sg,
                                          out.ctypes.data_as(C.POINTER(C.c_float)) if gains else None)
    return code, out


def test_the_solve_refuses_bad_arguments_and_then_still_works():
    st = np.array([[[8, 800], [4, 300]], [[4, 500], [8, 900]]], np.uint64)
    ok, want = _solve_code(st, 2, 1, 10.0, 0.1)
    assert ok == 0 and (want > 0).all()
    for sn, sg in ((0.0, 0.1), (-1.0, 0.1), (float("nan"), 0.1), (INF, 0.1), (10.0, 0.0), (10.0, -0.1), (10.0, float("nan")), (10.0, INF)):
        assert _solve_code(st, 2, 1, sn, sg)[0] == INVALID, (sn, sg)
        assert b"hg_mosaic_solve_gains" in HG.lib().hg_last_error(None)
    assert _solve_code(st, -1, 1, 10.0, 0.1)[0] == INVALID and _solve_code(st, 257, 1, 10.0, 0.1)[0] == INVALID
    assert _solve_code(st, 2, 0, 10.0, 0.1)[0] == INVALID and _solve_code(st, 2, 5, 10.0, 0.1)[0] == INVALID
    assert _solve_code(np.zeros(0, np.uint64), 2, 1, 10.0, 0.1)[0] == INVALID and _solve_code(st, 2, 1, 10.0, 0.1, gains=False)[0] == INVALID      # NULL pointers
    assert _solve_code(np.zeros(0, np.uint64), 0, 1, 10.0, 0.1, gains=False)[0] == 0                                                            # ... are legal for F = 0
    skew = st.copy()
    skew[0, 1, 0] = 5
    assert _solve_code(skew, 2, 1, 10.0, 0.1)[0] == INVALID and b"symmetric" in HG.lib().hg_last_error(None)
    with pytest.raises(HG.HgError):
        HG.mosaic_solve_gains(skew, 1)
    again = _solve_code(st, 2, 1, 10.0, 0.1)
    assert again[0] == 0 and np.array_equal(again[1], want)
    assert np.array_equal(HG.mosaic_solve_gains(st, 1), want) and HG.mosaic_solve_gains(np.zeros(0, np.uint64), 3).size == 0


# ------------------------------------------------------------------------------------------------ the scalar models, from the header text
def _scalar_stats(geoms, fields, frames, ch, canvas):
    F = len(geoms)
    cx, cy, cw, chh = canvas
    st = np.zeros((F, F, 2), np.uint64)
    k = 3 if ch == 4 else ch
    for j in range(max(chh, 0)):
        for i in range(max(cw, 0)):
            X, Y = cx + i, cy + j
            con = []
            for f, (x, y, w, h) in enumerate(geoms):
                if w <= 0 or h <= 0:
                    continue
                u, v = X - x, Y - y
                if not (0 <= u < w and 0 <= v < h):
                    continue
                sx, sy = fields[f][v * w + u]
                if not (math.isfinite(sx) and math.isfinite(sy)):
                    continue
                con.append((f, sum(int(p) for p in frames[f].reshape(-1, ch)[v * w + u][:k])))
            for a, va in con:
                for b, _ in con:
                    st[a, b, 0] += 1
                    st[a, b, 1] += va
    return st


def _scalar_gain_mosaic(geoms, fields, frames, W, H, mode, feather, canvas, is_u8, ch, gains):
    cx, cy, cw, chh = canvas
    out = np.zeros((chh, cw, ch), np.uint8 if is_u8 else F32)
    weight = np.zeros((chh, cw), F32)
    k = 3 if ch == 4 else ch
    store = (lambda q: [int(min(F32(255), F32(math.floor(F32(v + F32(0.5)))))) for v in q]) if is_u8 else (lambda q: q)
    for j in range(chh):
        for i in range(cw):
            X, Y = cx + i, cy + j
            con = []
            for f, (x, y, w, h) in enumerate(geoms):
                if w <= 0 or h <= 0:
                    continue
                u, v = X - x, Y - y
                if not (0 <= u < w and 0 <= v < h):
                    continue
                sx, sy = fields[f][v * w + u]
                if not (math.isfinite(sx) and math.isfinite(sy)):
                    continue
                p = frames[f].reshape(-1, ch)[v * w + u]
                with np.errstate(all="ignore"):
                    q = [F32(F32(gains[f]) * F32(pc)) if c < k else F32(pc) for c, pc in enumerate(p)]
                con.append((F32(sx), F32(sy), q))
            if not con:
                continue
            if mode == MM.LAST:
                out[j, i] = store(con[-1][2])
                weight[j, i] = 1
                continue
            acc, wsum = [F32(0)] * ch, F32(0)
            with np.errstate(all="ignore"):
                for sx, sy, q in con:
                    if mode == MM.MEAN:
                        wf = F32(1)
                    else:
                        dx = min(F32(sx + F32(1)), F32(F32(W) - sx))
                        dy = min(F32(sy + F32(1)), F32(F32(H) - sy))
                        wf = max(min(min(dx, dy), F32(feather)), F32(2.0 ** -10))
                    acc = [F32(a + F32(wf * qc)) for a, qc in zip(acc, q)]
                    wsum = F32(wsum + wf)
                weight[j, i] = wsum
                if len(con) == 1:
                    out[j, i] = store(con[0][2])
                    continue
                r = [F32(a / wsum) for a in acc]
            out[j, i] = store(r)
    return out, weight


MODEL_GEOMS = [(0, 0, 20, 14), (7, 3, 18, 12), (-5, -4, 12, 9), (0, 0, 0, 5), (7, 3, 18, 12), (22, 10, 1, 9), (30, -2, 16, 6), (100, 100, 4, 4), (3, 12, 25, 1)]
MODEL_CANVAS = (-3, -2, 41, 22)
MODEL_GAINS = np.array([0.5, 2.0, 1.25, 1.0, 0.8125, 1.7, 0.6, 1.0, 1.9], F32)


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
    """(fields, frames) over MODEL_GEOMS; u8 values reach 255, so that a gain above 1 saturates some; none equals the host check's fills."""
    rng = np.random.default_rng(300 + 10 * ch + elem)
    fields, frames = [], []
    for f, (_, _, w, h) in enumerate(MODEL_GEOMS):
        n = max(w, 0) * max(h, 0)
        fields.append(_field(rng, w, h, f) if n else np.zeros((0, 2), F32))
        if elem == HG.ELEM_U8:
            px = rng.integers(0, 256, (n, ch), dtype=np.uint8)
            px[(px == 0xA5) | (px == 0xEE)] = 255
        else:
            px = (rng.standard_normal((n, ch)) * 40 + 3).astype(F32)
        frames.append(px)
        fields[-1].setflags(write=False)
        frames[-1].setflags(write=False)
    return fields, frames


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_the_vectorised_models_match_the_scalar_models():
    for ch in (1, 2, 3, 4):
        fields, frames = _model_set(HG.ELEM_U8, ch)
        for canvas in (MODEL_CANVAS, (9, 5, 7, 3), (0, 0, 0, 4)):
            got = MG.overlap_stats(MODEL_GEOMS, fields, frames, ch, canvas)
            want = _scalar_stats(MODEL_GEOMS, fields, frames, ch, canvas)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (ch, canvas)
    st = MG.overlap_stats(MODEL_GEOMS, *_model_set(HG.ELEM_U8, 4), 4, MODEL_CANVAS)
    N = st[..., 0]
    assert np.array_equal(N, N.T) and (N[np.triu_indices(9, 1)] == 0).any() and (N[np.triu_indices(9, 1)] > 0).any()
    assert not st[3].any() and not st[7].any() and 0 < N[1, 4] < min(N[1, 1], N[4, 4])      # an empty frame, one off the canvas, two windows alike with holes of their own
    for elem, ch in ((HG.ELEM_U8, 3), (HG.ELEM_F32, 2), (HG.ELEM_U8, 4), (HG.ELEM_F32, 4), (HG.ELEM_U8, 1)):
        fields, frames = _model_set(elem, ch)
        for mode in (MM.LAST, MM.MEAN, MM.FEATHER):
            for feather in ((INF, 2.5) if mode == MM.FEATHER else (1.0,)):
                got, gw = MG.mosaic_gain(MODEL_GEOMS, fields, frames, SW, SH, mode, feather, MODEL_CANVAS, MODEL_GAINS)
                want, ww = _scalar_gain_mosaic(MODEL_GEOMS, fields, frames, SW, SH, mode, feather, MODEL_CANVAS, elem == HG.ELEM_U8, ch, MODEL_GAINS)
                assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), (elem, ch, mode, feather, np.argwhere(_bits(got) != _bits(want))[:4].tolist())
                assert np.array_equal(_bits(gw), _bits(ww)), (elem, ch, mode, feather)
                plain, pw = MM.mosaic(MODEL_GEOMS, fields, frames, SW, SH, mode, feather, MODEL_CANVAS)
                ones, ow = MG.mosaic_gain(MODEL_GEOMS, fields, frames, SW, SH, mode, feather, MODEL_CANVAS, np.ones(9, F32))
                assert np.array_equal(_bits(ones), _bits(plain)) and np.array_equal(_bits(ow), _bits(pw)) and np.array_equal(_bits(gw), _bits(pw))
                assert not np.array_equal(_bits(got), _bits(plain))
                if ch == 4:                                       # alpha passes unscaled wherever one frame stands alone or paints last
                    lone = (MM.mosaic(MODEL_GEOMS, fields, frames, SW, SH, MM.MEAN, 1.0, MODEL_CANVAS)[1] == 1) | (mode == MM.LAST)
                    assert lone.any() and np.array_equal(_bits(got[..., 3][lone]), _bits(plain[..., 3][lone]))


def test_hand_computed_cases():
    # two 4 x 2 frames overlapping in 2 columns: frame 0 holds 10 everywhere, frame 1 holds 3
    g = [(0, 0, 4, 2), (2, 0, 4, 2)]
    co = [np.full((8, 2), 5, F32)] * 2
    px = [np.full((8, 1), 10, np.uint8), np.full((8, 1), 3, np.uint8)]
    st = MG.overlap_stats(g, co, px, 1, (0, 0, 6, 2))
    assert st.tolist() == [[[8, 80], [4, 40]], [[4, 12], [8, 24]]]
    assert MG.overlap_stats(g, co, px, 1, (3, 1, 3, 1)).tolist() == [[[1, 10], [1, 10]], [[1, 3], [3, 9]]]      # the canvas cuts both
    # a 4-channel frame: alpha (200) must not enter S; 3 channels: all three do
    rgba = np.tile(np.array([1, 2, 3, 200], np.uint8), (8, 1))
    assert MG.overlap_stats(g[:1], co[:1], [rgba], 4, (0, 0, 4, 2)).tolist() == [[[8, 48]]]
    assert MG.overlap_stats(g[:1], co[:1], [rgba[:, :3]], 3, (0, 0, 4, 2)).tolist() == [[[8, 48]]]
    assert MG.overlap_stats(g[:1], co[:1], [rgba[:, 2:]], 2, (0, 0, 4, 2)).tolist() == [[[8, 8 * 203]]]
    # a NaN coordinate in frame 1's first pixel (canvas column 2, row 0) removes one pixel from N_01, N_10 and N_11, not from N_00
    hole = co[1].copy()
    hole[0, 1] = np.nan
    assert MG.overlap_stats(g, [co[0], hole], px, 1, (0, 0, 6, 2)).tolist() == [[[8, 80], [3, 30]], [[3, 9], [7, 21]]]
    # the gained mosaic: 100 * 1.5 and 100 * 0.5 average to 100; alone they are 150 and 50; 200 * 1.5 saturates; 3 * 0.5 = 1.5 rounds up
    px = [np.full((8, 1), 100, np.uint8), np.full((8, 1), 100, np.uint8)]
    out, w = MG.mosaic_gain(g, co, px, 9, 7, MM.MEAN, 1.0, (0, 0, 6, 1), [1.5, 0.5])
    assert out.ravel().tolist() == [150, 150, 100, 100, 50, 50] and w.ravel().tolist() == [1, 1, 2, 2, 1, 1]
    out, _ = MG.mosaic_gain(g, co, px, 9, 7, MM.LAST, 1.0, (0, 0, 6, 1), [1.5, 0.5])
    assert out.ravel().tolist() == [150, 150, 50, 50, 50, 50]
    px = [np.full((8, 1), 200, np.uint8), np.full((8, 1), 3, np.uint8)]
    out, _ = MG.mosaic_gain(g, co, px, 9, 7, MM.MEAN, 1.0, (0, 0, 6, 1), [1.5, 0.5])
    assert out.ravel().tolist() == [255, 255, 151, 151, 2, 2]                              # (300 + 1.5) / 2 = 150.75
    out, _ = MG.mosaic_gain(g[:1], co[:1], [rgba], 9, 7, MM.MEAN, 1.0, (0, 0, 1, 1), [2.0])
    assert out.ravel().tolist() == [2, 4, 6, 200]


# ------------------------------------------------------------------------------------------------ the solve
def _exposure_set(exposures, channels=3, seed=5):
    """One smooth scene seen through len(exposures) overlapping windows in a row, each frame's bytes scaled by its exposure with u8 rounding.
    (geoms, fields, frames, canvas)"""
    rng = np.random.default_rng(seed)
    n, w, h, step = len(exposures), 24, 12, 16
    cw = step * (n - 1) + w
    yy, xx = np.meshgrid(np.arange(h), np.arange(cw), indexing="ij")
    scene = np.stack([90 + 30 * np.sin(yy / 3.0 + c) + 0.3 * xx + rng.uniform(-2, 2, xx.shape) for c in range(channels)], -1)
    geoms, fields, frames = [], [], []
    for f, e in enumerate(exposures):
        geoms.append((step * f, 0, w, h))
        fields.append(np.stack([xx[:, step * f:step * f + w], yy[:, :w]], -1).astype(F32).reshape(-1, 2))
        px = np.minimum(255, np.floor(scene[:, step * f:step * f + w] * e + 0.5)).astype(np.uint8).reshape(-1, channels)
        if channels == 4:
            px[:, 3] = 255
        frames.append(px)
    return geoms, fields, frames, (0, 0, cw, h)


def _neighbours(ref64):
    r = np.asarray(ref64, np.float64).astype(F32)
    return r, np.nextafter(r, F32(0)), np.nextafter(r, F32(4))


def test_solve_against_the_float64_reference():
    for exposures, ch, sn, sg in (((0.8, 1.0, 1.25), 3, 10.0, 0.1), ((1.2, 0.7, 1.0, 0.9, 1.1), 1, 10.0, 0.1), ((0.6, 1.3), 4, 5.0, 0.3), ((1.0, 0.5, 1.5, 1.0), 2, 20.0, 0.05)):
        geoms, fields, frames, canvas = _exposure_set(exposures, ch)
        geoms = geoms + [(500, 500, 4, 4)]                        # ... and a frame that covers nothing
        fields, frames = fields + [np.zeros((16, 2), F32)], frames + [np.full((16, ch), 9, np.uint8)]
        st = MG.overlap_stats(geoms, fields, frames, ch, canvas)
        A, b, live = MG.normal_equations(st, ch, sn, sg)
        assert live.tolist() == list(range(len(exposures))) and np.linalg.cond(A) < 1e6, np.linalg.cond(A)
        ref = MG.solve_gains(st, ch, sn, sg)
        got = HG.mosaic_solve_gains(st, ch, sn, sg)
        assert got.dtype == F32 and got.shape == ref.shape
        r, lo, hi = _neighbours(ref)
        assert ((got == r) | (got == lo) | (got == hi)).all(), (got.tolist(), ref.tolist())
        # the normal equations, for general inputs: the unrounded reference meets them to 1e-9 relative, and the returned float32 gains meet
        # them within what rounding g to float32 may add: |A| times one float32 spacing of g (the neighbour allowed above)
        x, scale = ref[live], np.abs(A) @ np.abs(ref[live]) + np.abs(b)
        assert (np.abs(A @ x - b) <= 1e-9 * scale).all()
        g64 = got[live].astype(np.float64)
        assert (np.abs(A @ g64 - b) <= 1e-9 * scale + np.abs(A) @ np.spacing(got[live]).astype(np.float64)).all(), (A @ g64 - b).tolist()
        assert got[-1] == 1.0 and np.abs(got[:-1] - 1).max() > 0.02


def test_properties_of_the_solve():
    sn, sg = 10.0, 0.1
    geoms, fields, frames, canvas = _exposure_set((0.8, 1.0, 1.25), 3)
    st = MG.overlap_stats(geoms, fields, frames, 3, canvas)
    g = HG.mosaic_solve_gains(st, 3, sn, sg)
    e0 = MG.gain_error(st, 3, sn, sg, g)
    for f in range(3):                                             # a minimum: every one of the 2F points around it lies higher
        for k in (0.99, 1.01):
            moved = g.astype(np.float64)
            moved[f] *= k
            assert e0 < MG.gain_error(st, 3, sn, sg, moved), (f, k)
    assert e0 < MG.gain_error(st, 3, sn, sg, np.ones(3))          # the exposures differ: better than no gains
    assert g[0] > g[1] > g[2]                                      # the darkest frame is raised most
    # the normal equations to 1e-9 relative: the result is float32, so the bare bound is asked where the exact solution IS a float32 (general
    # inputs: test_solve_against_the_float64_reference, within the float32 rounding of g).  Two frames,
    # one channel: I_01 = 100, I_10 = 50, N = [[700, 100], [100, 100]], sigma_g = 0.1, sigma_n^2 = 50 have the solution (0.875, 1.25) -- put into
    # the equations: 100 * 800 * (-0.125) + 0.04 * 100 * 100 * (87.5 - 62.5) = 0 and 100 * 200 * 0.25 + 0.04 * 100 * 50 * (62.5 - 87.5) = 0.
    # A third frame that overlaps neither keeps 1.0; equal exposures give 1.0 throughout.
    st2 = np.zeros((3, 3, 2), np.uint64)
    st2[0, 0], st2[0, 1], st2[1, 0], st2[1, 1], st2[2, 2] = (700, 70000), (100, 10000), (100, 5000), (100, 5000), (50, 999)
    for stats, chn, s_n in ((st2, 1, math.sqrt(50.0)), (MG.overlap_stats(*_exposure_set((1.0, 1.0, 1.0), 3)[:3], 3, canvas), 3, sn)):
        gg = HG.mosaic_solve_gains(stats, chn, s_n, sg)
        A, b, live = MG.normal_equations(stats, chn, s_n, sg)
        x = gg[live].astype(np.float64)
        res = np.abs(A @ x - b)
        assert (res <= 1e-9 * (np.abs(A) @ np.abs(x) + np.abs(b))).all(), (res.tolist(), gg.tolist())
    assert HG.mosaic_solve_gains(st2, 1, math.sqrt(50.0), sg).tolist() == [0.875, 1.25, 1.0]
    # frames without coverage get exactly 1.0f, wherever they stand
    geoms4 = [(900, 900, 3, 3)] + geoms[:2] + [(0, 0, 0, 7)] + geoms[2:]
    fields4 = [np.zeros((9, 2), F32)] + fields[:2] + [np.zeros((0, 2), F32)] + fields[2:]
    frames4 = [np.full((9, 3), 50, np.uint8)] + frames[:2] + [np.zeros((0, 3), np.uint8)] + frames[2:]
    g4 = HG.mosaic_solve_gains(MG.overlap_stats(geoms4, fields4, frames4, 3, canvas), 3, sn, sg)
    assert g4[0] == 1.0 and g4[3] == 1.0 and np.array_equal(g4[[1, 2, 4]], g)
    # equal exposures: all within 1e-6 of 1
    geq = HG.mosaic_solve_gains(MG.overlap_stats(*_exposure_set((1.0, 1.0, 1.0), 3)[:3], 3, canvas), 3, sn, sg)
    assert np.abs(geq.astype(np.float64) - 1).max() <= 1e-6, geq.tolist()


def test_end_to_end_on_the_model_the_steps_at_the_window_borders_shrink():
    geoms, fields, frames, canvas = _exposure_set((0.8, 1.0, 1.25), 3)
    st = MG.overlap_stats(geoms, fields, frames, 3, canvas)
    gains = HG.mosaic_solve_gains(st, 3)
    plain, _ = MM.mosaic(geoms, fields, frames, 64, 12, MM.MEAN, 1.0, canvas)
    fixed, _ = MG.mosaic_gain(geoms, fields, frames, 64, 12, MM.MEAN, 1.0, canvas, gains)
    borders = sorted({x for g in geoms for x in (g[0], g[0] + g[2]) if 0 < x < canvas[2]})
    assert borders == [16, 24, 32, 40]
    for x in borders:
        before = float(np.abs(plain[:, x].astype(np.float64) - plain[:, x - 1]).mean())
        after = float(np.abs(fixed[:, x].astype(np.float64) - fixed[:, x - 1]).mean())
        assert after < before, f"border at column {x}: mean absolute step {after:.3f} with gains {gains.tolist()}, {before:.3f} without"


# ------------------------------------------------------------------------------------------------ the kernels' text on the host
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def _case_file(path, kind, elem, ch, mode, feather, canvas, geoms, fields, frames, mis, wt, gains=None):
    es = 1 if elem == HG.ELEM_U8 else 4
    fo, po, f_end, p_end = [], [], 0, 0
    for f in range(len(geoms)):                                   # mis: odd multiples of 8 / of the element size; exact ends
        fo.append(f_end + (8 * (2 * f + 1) if mis else 0))
        po.append(p_end + (es * (2 * f + 1) if mis else 0))
        f_end = fo[-1] + fields[f].nbytes
        p_end = po[-1] + frames[f].nbytes
    head = np.array([kind, elem, ch, SW, SH, mode, len(geoms), *canvas, 16 + es if mis else 16, 16 + es if mis else 16, wt], np.int32).tobytes()
    head += np.array([feather], F32).tobytes() + np.array([f_end, p_end], np.uint64).tobytes()
    for g, a, b in zip(geoms, fo, po):
        head += np.array(g, np.int32).tobytes() + np.array([a, b], np.uint64).tobytes()
    if kind == 1:
        head += np.asarray(gains, F32).tobytes()
    fld, pix = np.zeros(f_end, np.uint8), np.full(p_end, 0xEE, np.uint8)
    for co, fr, a, b in zip(fields, frames, fo, po):
        fld[a:a + co.nbytes] = _bits(co).ravel()
        pix[b:b + fr.nbytes] = _bits(fr).ravel()
    path.write_bytes(head + fld.tobytes() + pix.tobytes())


@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/mosaic_gain_check.cpp: k_mosaic_stats -- hg_k_mosaic_stats.hip itself, a block as 256 host threads -- and the gained
    k_mosaic_frames, compiled for the CPU behind the thread-index shim and run under ASan + UBSan on exact-size buffers: no byte outside
    a buffer is touched, whatever the alignment, and what they compute is the models', exactly.  The statistics also on 150 small frames,
    more than the block's LDS table holds per side.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "mosaic_gain_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "mosaic_gain_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)

    def run(case, *a, **k):
        fin, fout = tmp_path / f"case{case}.in", tmp_path / f"case{case}.out"
        _case_file(fin, *a, **k)
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (case, (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (case, (p.stdout + p.stderr)[-3000:])
        return np.frombuffer(fout.read_bytes(), np.uint8)

    case = 0
    for ch in (1, 2, 3, 4):
        fields, frames = _model_set(HG.ELEM_U8, ch)
        for mis, canvas in ((0, MODEL_CANVAS), (1, (-3, -2, 67, 5))):
            want = MG.overlap_stats(MODEL_GEOMS, fields, frames, ch, canvas)
            raw = run(case, 0, HG.ELEM_U8, ch, 0, 1.0, canvas, MODEL_GEOMS, fields, frames, mis, 0)
            assert np.array_equal(raw.view(np.uint64), want.ravel()), (case, ch, canvas)
            case += 1
    rng = np.random.default_rng(46)                               # 150 frames of 2 x 2 over a 70 x 6 canvas: tiles that more than 64 frames hit
    canvas = (-5, 3, 70, 6)
    geoms = [(int(x), int(y), 2, 2) for x, y in zip(rng.integers(-9, 66, 150), rng.integers(1, 9, 150))]
    geoms[7] = (geoms[7][0], geoms[7][1], 0, 2)
    fields = [(rng.random((g[2] * g[3], 2)) * [SW, SH]).astype(F32) for g in geoms]
    for co in fields[::5]:
        co[:1] = np.nan
    frames = [rng.integers(0, 256, (g[2] * g[3], 3), dtype=np.uint8) for g in geoms]
    hits = sum(1 for g in geoms if g[2] > 0 and g[0] < 59 and g[0] + 2 > -5 and g[1] < 7 and g[1] + 2 > 3)
    assert hits > 64, hits                                        # the first tile's list is longer than the table's side
    for canvas in (canvas, (-5, 3, 70, 16)):                      # ... and with tile rows below that fewer frames hit
        raw = run(case, 0, HG.ELEM_U8, 3, 0, 1.0, canvas, geoms, fields, frames, 0, 0)
        assert np.array_equal(raw.view(np.uint64), MG.overlap_stats(geoms, fields, frames, 3, canvas).ravel()), canvas
        case += 1
    for elem in (HG.ELEM_U8, HG.ELEM_F32):
        px = 1 if elem == HG.ELEM_U8 else 4
        for ch in (1, 2, 3, 4):
            fields, frames = _model_set(elem, ch)
            for mode, mis, wt in ((MM.LAST, 1, 0), (MM.MEAN, 0, 1), (MM.FEATHER, 1, 1)):
                feather = 2.5 if case % 2 else INF
                canvas = MODEL_CANVAS if case % 3 else (-3, -2, 67, 5)
                raw = run(case, 1, elem, ch, mode, feather, canvas, MODEL_GEOMS, fields, frames, mis, wt, MODEL_GAINS)
                want, ww = MG.mosaic_gain(MODEL_GEOMS, fields, frames, SW, SH, mode, feather, canvas, MODEL_GAINS)
                n = canvas[2] * canvas[3] * px * ch
                assert raw.size == n + (canvas[2] * canvas[3] * 4 if wt else 0), case
                bad = np.flatnonzero(raw[:n] != _bits(want).ravel())
                assert bad.size == 0, (case, elem, ch, mode, int(bad.size), (bad[:4] // (px * ch)).tolist())
                if wt:
                    assert np.array_equal(raw[n:], _bits(ww).ravel()), (case, "weight")
                case += 1


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_mosaic_exposure_over_the_recording_mock_addon():
    """tests/js/mosaic_gain_class.mjs: h.mosaic(sets, {exposure}) reaches the addon with the exposure arguments behind the mosaic's own, in
    their order; 'none' is an absent option; the array form is validated (length, finite, > 0); the result carries `gains`."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "mosaic_gain_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_mosaic_gain_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["failures"] == [] and p.returncode == 0, (res["failures"], p.stderr[-2000:])
    assert res["checks"] >= 25
