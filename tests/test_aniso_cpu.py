"""CPU-side checks of the anisotropic remap (include/hgwarp.h, hg_remap_aniso_frames_device): declaration, export and refusals that need no
device, the vectorised numpy model of tests/hgtest/aniso.py against a scalar model written from the header text, the model's own
properties (max_aniso == 1 IS the trilinear model, the stripes shrunk 8x along their length stay stripes where trilinear gives grey, a
constant stays constant), the kernel's source text on the host under sanitizers, and the class's remap() with sampling 'anisotropic' over
a recording mock."""
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
from hgtest import aniso as AM               # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest import trilinear as TM           # noqa: E402

INVALID = 1
F32 = np.float32
SW, SH = 61, 43                               # the source of the model tests: 7 levels
LEVELS = 7
assert TM.n_levels(SW, SH) == LEVELS


# ------------------------------------------------------------------------------------------------ symbols and host-only refusals
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    name = "hg_remap_aniso_frames_device"
    assert name in declared and hasattr(L, name) and name in HG.EXPORTS
    assert name in text[text.index("#define HG_VERSION"):text.index("enum {")]       # how the feature is detected
    assert re.search(r"int hg_remap_aniso_frames_device\([^;]*int levels, int max_aniso\);", code)
    assert callable(HG.Context.remap_aniso_frames_device)


def test_max_aniso_out_of_range_and_a_null_context_are_refused():
    L = HG.lib()
    g = (HG.Geom * 1)(HG.Geom(0, 0, 4, 4))
    p = C.c_void_p(4096)
    for bad in (0, 17, -1):
        assert L.hg_remap_aniso_frames_device(None, g, 1, p, None, p, 4, 4, 1, 64, HG.ELEM_U8, 1, p, None, p, 256, 2, bad) == INVALID, bad
    for good in (1, 8, 16):
        assert L.hg_remap_aniso_frames_device(None, g, 1, p, None, p, 4, 4, 1, 64, HG.ELEM_U8, 1, p, None, p, 256, 2, good) == INVALID, good      # the NULL context


# ------------------------------------------------------------------------------------------------ the scalar model, from the header text
def _finite(c):
    return bool(np.isfinite(c[0]) and np.isfinite(c[1]))


def _scalar_step(co, i, j, cands):
    """Step 2: (dx, dy, q) to the first candidate that exists and is finite; zeros without one."""
    sx, sy = co[j, i]
    for exists, (x, y) in cands:
        if exists and _finite(co[y, x]):
            dx = F32(co[y, x, 0] - sx)
            dy = F32(co[y, x, 1] - sy)
            return dx, dy, F32(F32(dx * dx) + F32(dy * dy))
    return F32(0), F32(0), F32(0)


def _scalar_bilinear(level, u, v):
    """hg_remap_bilinear_f32_device's rule on one level ((H, W, C) float32) at the finite float32 coordinate (u, v)."""
    H, W, _ = level.shape
    x0, y0 = F32(math.floor(u)), F32(math.floor(v))
    fx, fy = F32(u - x0), F32(v - y0)
    gx, gy = F32(F32(1) - fx), F32(F32(1) - fy)

    def tap(t, n):
        return min(int(min(max(t, F32(0)), F32(2147483520.0))), n - 1)

    c0, c1, r0, r1 = tap(x0, W), tap(F32(x0 + F32(1)), W), tap(y0, H), tap(F32(y0 + F32(1)), H)
    out = []
    for p00, p01, p10, p11 in zip(level[r0, c0], level[r0, c1], level[r1, c0], level[r1, c1]):
        top = F32(F32(F32(p00 * gx) + F32(p01 * fx)) * gy)
        bot = F32(F32(F32(p10 * gx) + F32(p11 * fx)) * fy)
        out.append(F32(top + bot))
    return out


def _scalar_pixel(co, i, j, pyr_f32, is_u8, max_aniso, seen):
    levels = len(pyr_f32)
    C_ = pyr_f32[0].shape[2]
    h, w, _ = co.shape
    sx, sy = co[j, i]
    if not _finite((sx, sy)):                                                                  # 1
        return [0] * C_
    with np.errstate(all="ignore"):
        hx, hy, qh = _scalar_step(co, i, j, [(i + 1 < w, (min(i + 1, w - 1), j)), (i - 1 >= 0, (max(i - 1, 0), j))])      # 2
        vx, vy, qv = _scalar_step(co, i, j, [(j + 1 < h, (i, min(j + 1, h - 1))), (j - 1 >= 0, (i, max(j - 1, 0)))])
        if qh >= qv:                                                                           # 3
            mx, my, qM, qm = hx, hy, qh, qv
        else:
            mx, my, qM, qm = vx, vy, qv, qh
        if not (qM > F32(1)) or not np.isfinite(qM):                                           # 4
            N = 1
        else:
            qmc = max(qm, F32(1))
            N = max_aniso
            for n in range(1, max_aniso + 1):
                if F32(F32(n * n) * qmc) >= qM:
                    N = n
                    break
        q = F32(qM / F32(N * N))                                                               # 5

    def at(k, px, py):
        if k == 0:
            return _scalar_bilinear(pyr_f32[0], px, py)
        inv = F32(1.0 / (1 << k))
        return _scalar_bilinear(pyr_f32[k], F32(F32(F32(px + F32(0.5)) * inv) - F32(0.5)), F32(F32(F32(py + F32(0.5)) * inv) - F32(0.5)))

    if not q > F32(1):
        k, two, t = 0, False, F32(0)
    else:
        k = 64 if math.isinf(q) else (math.frexp(float(q))[1] - 1) >> 1
        if k >= levels - 1:
            k, two, t = levels - 1, False, F32(0)
        else:
            two, t = True, F32(F32(F32(math.ldexp(float(q), -2 * k)) - F32(1)) * F32(0.33333334))
    seen.add((N, k, two))
    acc = None
    for p in range(N):                                                                         # 6
        if N == 1:
            px, py = sx, sy
        else:
            o = F32(F32(F32(F32(p) + F32(0.5)) / F32(N)) - F32(0.5))
            px, py = F32(sx + F32(mx * o)), F32(sy + F32(my * o))
        r = at(k, px, py)
        if two:
            hi = at(k + 1, px, py)
            r = [F32(a + F32(F32(b - a) * t)) for a, b in zip(r, hi)]
        acc = r if acc is None else [F32(a + b) for a, b in zip(acc, r)]                       # 7
    r = [F32(a / F32(N)) for a in acc]
    if is_u8:
        return [int(min(F32(255), F32(math.floor(F32(v + F32(0.5)))))) for v in r]
    return r


@functools.lru_cache(maxsize=None)
def _model_planes():
    rng = np.random.default_rng(15)
    u8 = rng.integers(0, 256, (SH, SW, 2), dtype=np.uint8)
    f32 = (rng.standard_normal((SH, SW, 1)) * 50).astype(F32)
    for a in (u8, f32):
        a.setflags(write=False)
    return u8, f32


def _projective(w, h, rng, strength=1.0):
    """A projective-like field: the horizontal step grows down the frame, the vertical one much faster (an oblique floor)."""
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    den = 1.0 - (0.9 * strength) * j / max(h, 1) - 0.002 * i
    sx = (SW / 2 + (i - w / 2) * (SW / w) * 0.9 / den) + rng.random() * 0.5
    sy = (2.0 + 0.8 * j / den) + rng.random() * 0.5
    return np.stack([sx, sy], -1).astype(F32)


@functools.lru_cache(maxsize=None)
def _model_frames():
    """(name, (h, w, 2) float32) frames: projective-like fields with NaN holes, infinities and 1e30 entries inside and ON every frame edge,
    steps that overflow, exact anisotropic steps, and 1 x n / n x 1 frames."""
    rng = np.random.default_rng(16)
    out = []
    w, h = 44, 30
    pro = _projective(w, h, rng)
    pro[rng.random((h, w)) < 0.03] = np.nan
    pro[rng.random((h, w)) < 0.01] = [np.inf, 3]
    pro[rng.random((h, w)) < 0.01] = [2, -np.inf]
    pro[5:8, 0] = np.nan
    pro[5:8, w - 1] = np.nan
    pro[0, 20:23] = np.nan
    pro[h - 1, 20:23] = np.nan
    pro[12:15, 1] = np.nan
    pro[12:15, w - 2] = np.nan
    pro[1, 30:33] = np.nan
    pro[h - 2, 30:33] = np.nan
    pro[10, 10:14] = [[1e30, 5], [5, -1e30], [-1e30, 1e30], [3e38, 3e38]]
    pro[20, 20] = [-2e30, 4]                                     # beside (20, 21): a step of about 2e30 whose square overflows
    pro[20, 21] = [2e30, 4]
    out.append(("projective", pro))
    i, j = np.meshgrid(np.arange(24), np.arange(9))
    out.append(("8 by 1", np.stack([1.0 * i + 3, 8.0 * j + 3.5], -1).astype(F32)))
    out.append(("1 by 5.5, turned", np.stack([5.5 * j + 0.25 * i, 1.0 * i + 0.5], -1).astype(F32)))
    out.append(("20 by 2", np.stack([20.0 * i * 0.1 + 0.3 * j, 2.0 * j + 0.5], -1).astype(F32) * F32(1)))
    out.append(("40 by 3", np.stack([3.0 * i - 4, 40.0 * j * 0.2 + 0.1 * i], -1).astype(F32)))
    out.append(("1 by 14.5", np.stack([1.0 * i + 0.5, 14.5 * j - 20], -1).astype(F32)))          # N = 15, and taps above and below the plane
    out.append(("magnifying", np.stack([0.5 * i + 3, 0.25 * j + 1], -1).astype(F32)))
    line = np.stack([np.linspace(-3, SW + 3, 90), np.full(90, 7.3)], -1).astype(F32)
    line[::17] = np.nan
    out.append(("1 x n", line.copy().reshape(90, 1, 2)))
    out.append(("n x 1", np.ascontiguousarray(line[:, ::-1] * F32(3)).reshape(1, 90, 2)))
    out.append(("1 x 1", np.array([[[3.5, 2.5]]], F32)))
    for _, a in out:
        a.setflags(write=False)
    return out


def test_the_vectorised_model_matches_the_scalar_model():
    u8, f32 = _model_planes()
    seen = set()
    total = 0
    for plane in (u8, f32):
        pyr = TM.pyramid(plane, LEVELS)
        pyr_f32 = [p.astype(F32) for p in pyr]
        for max_aniso in (1, 4, 16) if plane is u8 else (8,):
            for name, co in _model_frames():
                h, w, _ = co.shape
                got = AM.remap_aniso(co, pyr, max_aniso)
                want = np.array([_scalar_pixel(co, i, j, pyr_f32, plane is u8, max_aniso, seen) for j in range(h) for i in range(w)], plane.dtype)
                assert got.dtype == plane.dtype and got.shape == want.shape
                same = got.view(np.uint32) == want.view(np.uint32) if plane is f32 else got == want
                assert same.all(), (name, plane.dtype, max_aniso, np.argwhere(~same)[:5].tolist())
                total += h * w
    assert total >= 8000, total
    # the premises: every probe count, one level and two, and the non-finite / missing neighbour cases
    assert {n for n, _, _ in seen} == set(range(1, 17)), sorted({n for n, _, _ in seen})
    assert {two for _, _, two in seen} == {False, True} and len({k for _, k, _ in seen}) >= 4, seen
    pro = dict(_model_frames())["projective"]
    fin = np.isfinite(pro).all(-1)
    assert np.isnan(pro).any() and np.isinf(pro).any() and (np.abs(pro[fin]) >= 1e30).any()
    assert (fin[:, :-1] & ~fin[:, 1:]).any() and (fin[:-1] & ~fin[1:]).any()
    assert (fin[:, 1] & ~fin[:, 0]).any() and (fin[:, -2] & ~fin[:, -1]).any() and (fin[1] & ~fin[0]).any() and (fin[-2] & ~fin[-1]).any()
    assert fin[:, 0].any() and fin[:, -1].any() and fin[0].any() and fin[-1].any()
    with np.errstate(all="ignore"):
        assert np.isinf(AM.probe_plan(pro, 16)[3][20, 20])      # the overflowing step: q' = +Inf, N = 1
    assert AM.probe_plan(pro, 16)[2][20, 20] == 1
    shapes = [a.shape[:2] for _, a in _model_frames()]
    assert any(s[1] == 1 and s[0] > 1 for s in shapes) and any(s[0] == 1 and s[1] > 1 for s in shapes) and (1, 1) in shapes


def test_probe_count_and_level_on_hand_computed_cases():
    def plan(qM, qm, max_aniso, levels=LEVELS):
        N = int(AM.probe_count(np.array([qM], F32), np.array([qm], F32), max_aniso)[0])
        with np.errstate(all="ignore"):
            q = F32(qM) / F32(N * N)
        k, two, t = TM.level_choice(np.array([q], F32), levels)
        return N, float(q), int(k[0]), bool(two[0])

    assert plan(64, 1, 16) == (8, 1.0, 0, False)                 # 8 probes from level 0
    assert plan(64, 0, 16) == (8, 1.0, 0, False)                 # no minor neighbour: qm' = 1
    assert plan(64, 16, 16) == (2, 16.0, 2, True)                # the minor axis shrinks 4x: 2 probes from level 2 (t == 0)
    assert plan(1000, 1, 4) == (4, 62.5, 2, True)                # capped: the rest of the shrink goes to the level
    assert plan(np.inf, 1, 16)[0] == 1 and plan(np.inf, 1, 16)[2:] == (LEVELS - 1, False)
    assert plan(1.0, 0, 16) == (1, 1.0, 0, False) and plan(0.25, 0.1, 16)[0] == 1
    assert plan(64.00001, 1, 16)[0] == 9 and plan(63.99999, 1, 16)[0] == 8
    assert plan(300, 1, 16)[0] == 16 and plan(256, 1, 16)[0] == 16 and plan(225, 1, 16)[0] == 15
    # through a field: the major axis is the vertical step of 8, the horizontal neighbour one pixel away
    i, j = np.meshgrid(np.arange(5), np.arange(4))
    co = np.stack([1.0 * i, 8.0 * j + 3.5], -1).astype(F32)
    mx, my, N, q = AM.probe_plan(co, 16)
    assert (N == 8).all() and (q == 1).all() and (mx == 0).all() and (my[:-1] == 8).all() and (my[-1] == -8).all()
    mx, my, N, q = AM.probe_plan(co, 4)
    assert (N == 4).all() and (q == 4).all()
    # a tie: the horizontal step is the major one
    co = np.stack([3.0 * i, 3.0 * j], -1).astype(F32)
    mx, my, N, q = AM.probe_plan(co, 16)
    assert (np.abs(mx) == 3).all() and (my == 0).all() and (N == 1).all() and (q == 9).all()


# ------------------------------------------------------------------------------------------------ properties of the model
def test_max_aniso_1_is_the_trilinear_model():
    for plane in _model_planes():
        for levels in (1, 3, LEVELS):
            pyr = TM.pyramid(plane, levels)
            for name, co in _model_frames():
                a, t = AM.remap_aniso(co, pyr, 1), TM.remap_trilinear(co, pyr)
                assert a.dtype == t.dtype and np.array_equal(a.view(np.uint8), t.view(np.uint8)), (name, plane.dtype, levels)
    # ... and with one level, or where nothing shrinks, every max_aniso is the bilinear remap
    for plane in _model_planes():
        fn = RF.remap_bilinear_u8 if plane.dtype == np.uint8 else RF.FM.remap_bilinear_f32
        for name, co in _model_frames():
            for max_aniso, levels in ((1, 1), (8, LEVELS)) if name == "magnifying" else ((1, 1),):
                assert np.array_equal(AM.remap_aniso(co, TM.pyramid(plane, levels), max_aniso).view(np.uint8), fn(co.reshape(-1, 2), plane).view(np.uint8)), name


def stripes_case():
    """A 64 x 64 u8 plane of one-pixel vertical stripes, shrunk 8x vertically and not at all horizontally."""
    plane = np.zeros((64, 64, 1), np.uint8)
    plane[:, 1::2] = 255
    i, j = np.meshgrid(np.arange(64), np.arange(8))
    co = np.stack([1.0 * i, 8.0 * j + 3.5], -1).astype(F32)
    return plane, co


def test_the_stripes_shrunk_along_their_length_stay_stripes_where_trilinear_gives_grey():
    plane, co = stripes_case()
    pyr = TM.pyramid(plane, TM.n_levels(64, 64))
    assert (AM.probe_plan(co, 16)[2] == 8).all()
    got = AM.remap_aniso(co, pyr, 16).reshape(8, 64)
    assert np.array_equal(got, np.broadcast_to(plane[0, :, 0], (8, 64)))
    assert np.array_equal(AM.remap_aniso(co, pyr, 8), got.reshape(-1, 1))
    assert (TM.remap_trilinear(co, pyr) == 128).all()


def test_a_constant_u8_plane_stays_constant():
    rng = np.random.default_rng(17)
    co = _projective(44, 30, rng).copy()
    co[3, 4] = np.nan
    fin = np.isfinite(co).all(-1).ravel()
    assert len(set(AM.probe_plan(co, 16)[2][np.isfinite(co).all(-1)].tolist())) >= 6
    for value in (0, 1, 127, 128, 255):
        pyr = TM.pyramid(np.full((SH, SW, 3), value, np.uint8), LEVELS)
        for max_aniso in (1, 3, 7, 16):
            out = AM.remap_aniso(co, pyr, max_aniso)
            assert (out[fin] == value).all() and not out[~fin].any(), (value, max_aniso)


# ------------------------------------------------------------------------------------------------ the kernel's text on the host
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/aniso_check.cpp: k_remap_aniso_frames over k_pyr_down's pyramids -- hg_k_aniso.hip and hg_k_pyramid.hip themselves --,
    compiled for the CPU behind a thread-index shim and run under ASan + UBSan on exact-size buffers -- no byte outside a
    buffer is touched, whatever the alignment -- and what it computes is the model's, bit for bit: every element type and channel count,
    misaligned planes, pyramids, offsets and strides, the frames of the model test.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "aniso_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "aniso_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    frames = [co for _, co in _model_frames()]
    geoms = [(0, 0, co.shape[1], co.shape[0]) for co in frames] + [(0, 0, 0, 3)]
    fields = [co.reshape(-1, 2) for co in frames] + [np.zeros((0, 2), F32)]
    rng = np.random.default_rng(18)
    for case, (elem, ch, n_planes, levels, misalign, max_aniso) in enumerate((
            (1, 1, 1, 7, 0, 16), (1, 2, 3, 7, 1, 8), (1, 3, 2, 7, 1, 5), (1, 4, 3, 7, 1, 16), (1, 4, 1, 7, 0, 2), (1, 2, 1, 2, 0, 16),
            (0, 1, 3, 7, 1, 16), (0, 2, 1, 7, 0, 3), (0, 3, 2, 3, 1, 8), (0, 4, 3, 7, 1, 16), (1, 4, 2, 1, 1, 16), (0, 1, 1, 7, 1, 1))):
        es = 1 if elem else 4
        px = es * ch
        if elem:
            planes = [rng.integers(0, 256, (SH, SW, ch), dtype=np.uint8) for _ in range(n_planes)]
        else:
            planes = [(rng.standard_normal((SH, SW, ch)) * 30).astype(F32) for _ in range(n_planes)]
        blk_px = 1024
        plane_stride = planes[0].nbytes + (256 + 3 * es if misalign else 0)
        plane_front, pyr_front = (16 + es, 16 + es) if misalign else (16, 16)
        offs, total = TM.layout(SW, SH, px, levels)
        pyr_stride = total + (3 * es if misalign else 0)
        fo, oo, f_end, o_end = [], [], 0, 0
        for f, g in enumerate(geoms):
            fo.append(f_end + (8 * (2 * f + 1) if misalign else 0))
            oo.append(o_end + (es * (2 * f + 1) if misalign else 0))
            f_end = fo[-1] + RF.n_px(g) * 8
            o_end = oo[-1] + RF.n_px(g) * px + (7 * es if misalign else 0)
        head = np.array([elem, ch, SW, SH, levels, n_planes, len(geoms), plane_front, max_aniso, 0], np.int32).tobytes()
        head += np.array([blk_px, plane_stride, pyr_front, pyr_stride, f_end, o_end], np.uint64).tobytes()
        for g, a, b in zip(geoms, fo, oo):
            head += np.array([g[2], g[3]], np.int32).tobytes() + np.array([a, b], np.uint64).tobytes()
        fld = np.zeros(f_end, np.uint8)
        for co, a in zip(fields, fo):
            fld[a:a + co.size * 4] = np.ascontiguousarray(co).view(np.uint8).ravel()
        pl = np.full((n_planes - 1) * plane_stride + planes[0].nbytes, 0xEE, np.uint8)
        for k, p_ in enumerate(planes):
            pl[k * plane_stride:k * plane_stride + p_.nbytes] = p_.view(np.uint8).ravel()
        fin, fout = tmp_path / f"case{case}.in", tmp_path / f"case{case}.out"
        fin.write_bytes(head + fld.tobytes() + pl.tobytes())
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (case, (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (case, (p.stdout + p.stderr)[-3000:])
        raw = np.frombuffer(fout.read_bytes(), np.uint8)
        pyr_bytes = (n_planes - 1) * pyr_stride + total if levels > 1 else 0
        assert raw.size == pyr_bytes + o_end, case
        pyrs = [TM.pyramid(p_, levels) for p_ in planes]
        out = raw[pyr_bytes:]
        want = AM.aniso_frames(geoms, fields, pyrs, max_aniso)
        untouched = np.ones(o_end, bool)
        for f, g in enumerate(geoms):
            n = RF.n_px(g) * px
            untouched[oo[f]:oo[f] + n] = False
            w_ = np.ascontiguousarray(want[f]).view(np.uint8).ravel()
            got = out[oo[f]:oo[f] + n]
            assert np.array_equal(got, w_), (case, "frame", f, g, int((got != w_).sum()), np.flatnonzero(got != w_)[:4].tolist())
        assert (out[untouched] == 0xA5).all(), case


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_anisotropic_over_the_recording_mock_addon():
    """tests/js/aniso_class.mjs: sampling 'anisotropic' reaches 'remapAniso' + entry with the trilinear call's arguments and maxAniso
    (default 8), refuses a bad maxAniso and what 'trilinear' refuses, and leaves the calls of the other three samplings as they were."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "aniso_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_aniso_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["failures"] == [] and p.returncode == 0, (res["failures"], p.stderr[-2000:])
    assert res["checks"] >= 300
