"""CPU-side checks of the bicubic remap (include/hgwarp.h, hg_remap_bicubic_frames_device): declaration, export and refusals that need no
device, the vectorised numpy model of tests/hgtest/bicubic.py against a scalar model written from the header text, hand-checked numbers,
the model's own properties (Catmull-Rom interpolates, a constant stays constant, the overshoot beside an edge is clamped on both sides,
a sinusoid enlarged 4x lies four times closer to the function than the bilinear remap's), the kernel's source text on the host under
sanitizers, and the class's remap() with sampling 'bicubic' over a recording mock."""
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
from hgtest import bicubic as BM             # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402

INVALID = 1
F32 = np.float32
SW, SH = 23, 17                               # the source of the model tests
PARAMS = ((0.0, 0.5), (1 / 3, 1 / 3), (1.0, 0.0), (0.37, 0.81))
NAME = "hg_remap_bicubic_frames_device"


# ------------------------------------------------------------------------------------------------ symbols and host-only refusals
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    assert NAME in declared and hasattr(L, NAME) and NAME in HG.EXPORTS
    assert NAME in text[text.index("#define HG_VERSION"):text.index("enum {")]       # how the feature is detected
    assert re.search(r"int hg_remap_bicubic_frames_device\([^;]*const size_t \*out_offsets,\s*float B, float C\);", code)
    assert "#define HG_VERSION 100 " in text
    assert callable(HG.Context.remap_bicubic_frames_device)
    assert HG.CUBIC_CATMULL_ROM == (0.0, 0.5) and HG.CUBIC_MITCHELL == (1 / 3, 1 / 3) and HG.CUBIC_BSPLINE == (1.0, 0.0)


def test_b_or_c_out_of_range_and_a_null_context_are_refused():
    L = HG.lib()
    g = (HG.Geom * 1)(HG.Geom(0, 0, 4, 4))
    p = C.c_void_p(4096)

    def call(b, c):
        return L.hg_remap_bicubic_frames_device(None, g, 1, p, None, p, 4, 4, 1, 64, HG.ELEM_U8, 1, p, None, b, c)

    for bad in (float("nan"), -0.1, 1.5, float("inf")):
        assert call(bad, 0.5) == INVALID, bad
        assert b"B must" in L.hg_last_error(None), bad
        assert call(0.5, bad) == INVALID, bad
        assert b"C must" in L.hg_last_error(None), bad
    for b, c in PARAMS + ((0.0, 0.0), (1.0, 1.0)):
        assert call(b, c) == INVALID, (b, c)                                      # the NULL context
        assert b"must lie" not in L.hg_last_error(None), (b, c)


# ------------------------------------------------------------------------------------------------ the scalar model, from the header text
def _scalar_coefficients(B, Cc):
    B, Cc = float(F32(B)), float(F32(Cc))                                         # 2: in double, each rounded once
    return [F32(v) for v in (((12 - 9 * B) - 6 * Cc) / 6, ((-18 + 12 * B) + 6 * Cc) / 6, (6 - 2 * B) / 6,
                             (-B - 6 * Cc) / 6, (6 * B + 30 * Cc) / 6, (-12 * B - 48 * Cc) / 6, (8 * B + 24 * Cc) / 6)]


def _scalar_weights(t, k):
    p3, p2, p0, q3, q2, q1, q0 = k

    def near(x):
        return F32(F32(F32(F32(F32(p3 * x) + p2) * x) * x) + p0)

    def far(x):
        return F32(F32(F32(F32(F32(F32(q3 * x) + q2) * x) + q1) * x) + q0)

    return [far(F32(F32(1) + t)), near(t), near(F32(F32(1) - t)), far(F32(F32(2) - t))]         # 4


def _scalar_tap(v, n):
    return min(int(min(max(v, F32(0)), F32(2147483520.0))), n - 1)


def _scalar_pixel(sx, sy, plane_f32, is_u8, k, seen):
    H, W, Cn = plane_f32.shape
    if not (np.isfinite(sx) and np.isfinite(sy)):                                 # 1
        seen["nonfinite"] += 1
        return [0] * Cn
    x0, y0 = F32(math.floor(sx)), F32(math.floor(sy))                             # 3
    fx, fy = F32(sx - x0), F32(sy - y0)
    wx, wy = _scalar_weights(fx, k), _scalar_weights(fy, k)
    xs = [F32(x0 - F32(1)), x0, F32(x0 + F32(1)), F32(x0 + F32(2))]               # 5
    ys = [F32(y0 - F32(1)), y0, F32(y0 + F32(1)), F32(y0 + F32(2))]
    cols, rows = [_scalar_tap(v, W) for v in xs], [_scalar_tap(v, H) for v in ys]
    for n in range(4):
        seen["col_lo"][n] |= bool(xs[n] < 0)
        seen["col_hi"][n] |= bool(xs[n] > W - 1)
        seen["row_lo"][n] |= bool(ys[n] < 0)
        seen["row_hi"][n] |= bool(ys[n] > H - 1)
    seen["fx0"] += int(fx == 0)
    seen["fx1"] += int(fx > F32(0.99))
    out = []
    for ch in range(Cn):                                                          # 6
        r = None
        for n in range(4):
            p = [plane_f32[rows[n], c, ch] for c in cols]
            h = F32(F32(F32(F32(p[0] * wx[0]) + F32(p[1] * wx[1])) + F32(p[2] * wx[2])) + F32(p[3] * wx[3]))
            r = F32(h * wy[0]) if n == 0 else F32(r + F32(h * wy[n]))
        if is_u8:                                                                 # 7
            out.append(int(min(F32(255), max(F32(0), F32(math.floor(F32(r + F32(0.5))))))))
        else:
            out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def _model_planes():
    rng = np.random.default_rng(25)
    u8 = rng.integers(0, 256, (SH, SW, 2), dtype=np.uint8)
    f32 = (rng.standard_normal((SH, SW, 1)) * 50).astype(F32)
    for a in (u8, f32):
        a.setflags(write=False)
    return u8, f32


def enlarging_projective(w, h, sw, sh, rng):
    """A projective-like ENLARGING field over a sw x sh source: steps of about sw / (1.6 w) that grow across the frame."""
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    den = 1.0 + 0.3 * j / max(h, 1) + 0.2 * i / max(w, 1)
    sx = sw * 0.15 + (i / max(w, 1)) * sw * 0.9 / den + rng.random() * 0.5
    sy = sh * 0.1 + (j / max(h, 1)) * sh * 0.9 / den + rng.random() * 0.5
    return np.stack([sx, sy], -1).astype(F32)


@functools.lru_cache(maxsize=None)
def _model_frames():
    """(name, (h, w, 2) float32) frames: an enlarging projective-like field with NaN holes, infinities, 1e30 and 3e38 entries, 1 x n, n x 1
    and 1 x 1 frames, and a field that runs 3 pixels beyond every edge of the plane."""
    rng = np.random.default_rng(26)
    out = []
    w, h = 44, 30
    pro = enlarging_projective(w, h, SW, SH, rng)
    pro[rng.random((h, w)) < 0.03] = np.nan
    pro[rng.random((h, w)) < 0.01] = [np.inf, 3]
    pro[rng.random((h, w)) < 0.01] = [2, -np.inf]
    pro[10, 10:14] = [[1e30, 5], [5, -1e30], [-1e30, 1e30], [3e38, 3e38]]
    pro[11, 10:12] = [[-3e38, 2.5], [4.25, 3e38]]
    pro[3, 3:7] = [[4, 6], [4.5, 6.999999], [5.9999995, 2], [0, 0]]              # integer coordinates and fractions next to 1
    out.append(("projective", pro))
    line = np.stack([np.linspace(-3, SW + 3, 90), np.full(90, 7.3)], -1).astype(F32)
    line[::17] = np.nan
    out.append(("1 x n", line.copy().reshape(90, 1, 2)))
    out.append(("n x 1", np.ascontiguousarray(line[:, ::-1] * F32(0.7)).reshape(1, 90, 2)))
    out.append(("1 x 1", np.array([[[3.5, 2.5]]], F32)))
    i, j = np.meshgrid(np.arange(30), np.arange(24))
    beyond = np.stack([-3 + i * (SW + 6) / 29, -3 + j * (SH + 6) / 23], -1).astype(F32)
    out.append(("beyond every edge", beyond))
    for _, a in out:
        a.setflags(write=False)
    return out


def _new_seen():
    return {"nonfinite": 0, "fx0": 0, "fx1": 0, "col_lo": [False] * 4, "col_hi": [False] * 4, "row_lo": [False] * 4, "row_hi": [False] * 4}


def test_the_vectorised_model_matches_the_scalar_model():
    u8, f32 = _model_planes()
    seen = _new_seen()
    total = 0
    for plane in (u8, f32):
        pf = plane.astype(F32)
        for B, Cc in PARAMS:
            k = _scalar_coefficients(B, Cc)
            assert [float(v) for v in k] == [float(v) for v in BM.coefficients(B, Cc)]
            for name, co in _model_frames():
                flat = co.reshape(-1, 2)
                got = BM.remap_bicubic(flat, plane, B, Cc)
                with np.errstate(all="ignore"):
                    want = np.array([_scalar_pixel(sx, sy, pf, plane is u8, k, seen) for sx, sy in flat], plane.dtype)
                assert got.dtype == plane.dtype and got.shape == want.shape
                same = got.view(np.uint32) == want.view(np.uint32) if plane is f32 else got == want
                assert same.all(), (name, plane.dtype, B, Cc, np.argwhere(~same)[:5].tolist())
                total += flat.shape[0]
    assert total >= 15000, total
    # the premises: every tap column and row is clamped at both ends somewhere, non-finite pixels, integer coordinates and fractions next to 1
    assert all(seen["col_lo"]) and all(seen["col_hi"]) and all(seen["row_lo"]) and all(seen["row_hi"]), seen
    assert seen["nonfinite"] > 100 and seen["fx0"] > 10 and seen["fx1"] > 10, seen
    pro = dict(_model_frames())["projective"]
    fin = np.isfinite(pro).all(-1)
    assert np.isnan(pro).any() and (pro == np.inf).any() and (pro == -np.inf).any()
    assert (np.abs(pro[fin]) == F32(1e30)).any() and (np.abs(pro[fin]) == F32(3e38)).any()
    steps = np.diff(pro[:, :, 0], axis=1)[fin[:, 1:] & fin[:, :-1]]
    assert 0 < np.median(steps) < 0.6                                             # an enlargement
    shapes = [a.shape[:2] for _, a in _model_frames()]
    assert any(s[1] == 1 and s[0] > 1 for s in shapes) and any(s[0] == 1 and s[1] > 1 for s in shapes) and (1, 1) in shapes


def test_the_models_agree_on_tiny_planes():
    rng = np.random.default_rng(27)
    for (w, h) in ((1, 5), (5, 1), (2, 2)):
        u8 = rng.integers(0, 256, (h, w, 2), dtype=np.uint8)
        f32 = (rng.standard_normal((h, w, 1)) * 50).astype(F32)
        co = np.stack([rng.uniform(-3, w + 3, 300), rng.uniform(-3, h + 3, 300)], -1).astype(F32)
        co[:4] = [[0, 0], [w - 1, h - 1], [np.nan, 0], [1e30, -1e30]]
        for plane in (u8, f32):
            for B, Cc in PARAMS:
                k = _scalar_coefficients(B, Cc)
                got = BM.remap_bicubic(co, plane, B, Cc)
                want = np.array([_scalar_pixel(sx, sy, plane.astype(F32), plane is u8, k, _new_seen()) for sx, sy in co], plane.dtype)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (w, h, plane.dtype, B, Cc)


# ------------------------------------------------------------------------------------------------ hand-checked numbers
def test_coefficients_and_weights_on_hand_computed_cases():
    k = BM.coefficients(0.0, 0.5)
    assert [float(v) for v in k] == [1.5, -2.5, 1.0, -0.5, 2.5, -4.0, 2.0] and all(v.dtype == F32 for v in k)
    assert [float(w) for w in BM.weights(F32(0), k)] == [0.0, 1.0, 0.0, 0.0]
    assert [float(w) for w in BM.weights(F32(0.5), k)] == [-0.0625, 0.5625, 0.5625, -0.0625]
    t = (np.arange(100001) / 100001).astype(F32)
    assert t.max() < 1 and t.size == 100001
    for B, Cc in ((1 / 3, 1 / 3), (1.0, 0.0)):
        w = BM.weights(t, BM.coefficients(B, Cc))
        s = ((w[0] + w[1]) + w[2]) + w[3]
        assert s.dtype == F32 and np.abs(s.astype(np.float64) - 1).max() <= 2e-6, (B, Cc)
    # the B-spline at t = 0: 1/6, 4/6, 1/6, 0
    w = [float(v) for v in BM.weights(F32(0), BM.coefficients(1.0, 0.0))]
    assert np.allclose(w, [1 / 6, 4 / 6, 1 / 6, 0], atol=3e-7)


# ------------------------------------------------------------------------------------------------ properties of the model
def test_catmull_rom_at_integer_coordinates_is_the_plane_and_the_bilinear_remap():
    for plane in _model_planes():
        j, i = np.meshgrid(np.arange(SH), np.arange(SW), indexing="ij")
        co = np.stack([i, j], -1).astype(F32).reshape(-1, 2)
        got = BM.remap_bicubic(co, plane, 0.0, 0.5)
        assert got.dtype == plane.dtype and np.array_equal(got.view(np.uint8), plane.reshape(got.shape).view(np.uint8))
        fn = RF.remap_bilinear_u8 if plane.dtype == np.uint8 else RF.FM.remap_bilinear_f32
        assert np.array_equal(got.view(np.uint8), fn(co, plane).view(np.uint8))


def test_a_constant_u8_plane_stays_constant():
    rng = np.random.default_rng(28)
    co = rng.uniform(-2, 10, (20000, 2)).astype(F32)
    assert co.min() >= -2 and co.max() < 10
    for value in (0, 1, 127, 128, 255):
        plane = np.full((9, 9, 1), value, np.uint8)
        for B, Cc in ((0.0, 0.5), (1 / 3, 1 / 3), (1.0, 0.0), (0.37, 0.81), (0.0, 1.0), (1.0, 1.0)):
            out = BM.remap_bicubic(co, plane, B, Cc)
            assert (out == value).all(), (value, B, Cc, np.unique(out).tolist())


def step_edge_case():
    """A 16 x 6 u8 plane, 0 left of column 8 and 255 from it on, enlarged 4x (pixel centres aligned): the plane and the (h, w, 2) field."""
    plane = np.zeros((6, 16, 1), np.uint8)
    plane[:, 8:] = 255
    i, j = np.meshgrid(np.arange(64), np.arange(24))
    co = np.stack([(i + 0.5) / 4 - 0.5, (j + 0.5) / 4 - 0.5], -1).astype(F32)
    return plane, co


def test_the_overshoot_beside_a_step_edge_is_clamped_on_both_sides():
    plane, co = step_edge_case()
    flat = co.reshape(-1, 2)
    raw = BM.remap_bicubic(flat, plane, 0.0, 0.5, unrounded=True)
    assert raw.dtype == F32 and raw.min() < -0.5 and raw.max() > 255.5, (raw.min(), raw.max())
    out = BM.remap_bicubic(flat, plane, 0.0, 0.5)
    assert out.dtype == np.uint8 and (out[raw < -0.5] == 0).all() and (out[raw > 255.5] == 255).all()
    assert (raw < -0.5).sum() >= 24 and (raw > 255.5).sum() >= 24
    smooth = BM.remap_bicubic(flat, plane, 1.0, 0.0).reshape(24, 64).astype(np.int32)
    assert (np.diff(smooth, axis=1) >= 0).all() and smooth[:, 0].max() == 0 and smooth[:, -1].min() == 255
    assert len(np.unique(smooth)) > 8                                             # ... through a ramp, not a jump


def sinusoid_rms(remap):
    """RMS distance between a 64 x 64 plane of 100 sin(2 pi x / 8) cos(2 pi y / 10) enlarged 4x by `remap` and the function itself."""
    y, x = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    plane = (100 * np.sin(2 * np.pi * x / 8) * np.cos(2 * np.pi * y / 10)).astype(F32)[:, :, None]
    j, i = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    sx, sy = (i + 0.5) / 4 - 0.5, (j + 0.5) / 4 - 0.5
    inside = (sx >= 1) & (sx <= 62) & (sy >= 1) & (sy <= 62)                       # away from the clamped border
    exact = 100 * np.sin(2 * np.pi * sx / 8) * np.cos(2 * np.pi * sy / 10)
    got = remap(np.stack([sx, sy], -1).astype(F32).reshape(-1, 2), plane).reshape(256, 256).astype(np.float64)
    return float(np.sqrt(np.mean((got - exact)[inside] ** 2)))


def test_catmull_rom_enlarges_a_sinusoid_four_times_closer_than_bilinear():
    bil = sinusoid_rms(RF.FM.remap_bilinear_f32)
    cr = sinusoid_rms(lambda co, p: BM.remap_bicubic(co, p, 0.0, 0.5))
    mit = sinusoid_rms(lambda co, p: BM.remap_bicubic(co, p, 1 / 3, 1 / 3))
    print(f"RMS error: bilinear {bil:.3f}, Catmull-Rom {cr:.3f}, Mitchell {mit:.3f}")
    assert cr <= bil / 4 and cr < mit < bil, (bil, cr, mit)
    # the figures the header and the README quote (this setup: pixel centres aligned, the clamped border left out)
    assert abs(bil - 4.35) < 0.02 and abs(cr - 0.49) < 0.01 and abs(mit - 2.89) < 0.02, (bil, cr, mit)


# ------------------------------------------------------------------------------------------------ the kernel's text on the host
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def _host_case(tmp_path, exe, case, elem, planes, geoms, fields, B, Cc, misalign):
    """Runs bicubic_check on one case and compares every frame with the model; bytes between frames must keep their fill."""
    ch = planes[0].shape[2]
    H, W = planes[0].shape[:2]
    es = 1 if elem else 4
    px = es * ch
    n_planes = len(planes)
    plane_stride = planes[0].nbytes + (256 + 3 * es if misalign else 0)
    plane_front = 16 + es if misalign else 16
    fo, oo, f_end, o_end = [], [], 0, 0
    for f, g in enumerate(geoms):
        fo.append(f_end + (8 * (2 * f + 1) if misalign else 0))
        oo.append(o_end + (es * (2 * f + 1) if misalign else 0))
        f_end = fo[-1] + RF.n_px(g) * 8
        o_end = oo[-1] + RF.n_px(g) * px + (7 * es if misalign else 0)
    head = np.array([elem, ch, W, H, n_planes, len(geoms), plane_front, 0], np.int32).tobytes()
    head += np.array(list(BM.coefficients(B, Cc)) + [0], F32).tobytes()
    head += np.array([1024, plane_stride, f_end, o_end], np.uint64).tobytes()
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
    out = np.frombuffer(fout.read_bytes(), np.uint8)
    assert out.size == o_end, case
    want = BM.bicubic_frames(geoms, fields, planes, B, Cc)
    untouched = np.ones(o_end, bool)
    for f, g in enumerate(geoms):
        n = RF.n_px(g) * px
        untouched[oo[f]:oo[f] + n] = False
        w_ = np.ascontiguousarray(want[f]).view(np.uint8).ravel()
        got = out[oo[f]:oo[f] + n]
        assert np.array_equal(got, w_), (case, "frame", f, g, int((got != w_).sum()), np.flatnonzero(got != w_)[:4].tolist())
    assert (out[untouched] == 0xA5).all(), case
    return out


@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/bicubic_check.cpp: k_remap_bicubic_frames -- hg_k_bicubic.hip itself --, compiled for the CPU behind a thread-index shim and
    run under ASan + UBSan on exact-size buffers -- no byte outside a buffer is touched, whatever the alignment, and no negative value is
    converted to a byte -- and what it computes is the model's, bit for bit: every element type and channel count, 1 to 3 planes,
    misaligned plane fronts, offsets and strides, the frames of the model test plus an empty one, the four parameter pairs, and the
    Catmull-Rom step edge on u8.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "bicubic_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "bicubic_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    frames = [co for _, co in _model_frames()]
    geoms = [(0, 0, co.shape[1], co.shape[0]) for co in frames] + [(0, 0, 0, 3)]
    fields = [co.reshape(-1, 2) for co in frames] + [np.zeros((0, 2), F32)]
    rng = np.random.default_rng(29)
    cases = ((1, 1, 1, 0, 0), (1, 2, 3, 1, 1), (1, 3, 2, 1, 2), (1, 4, 3, 1, 3), (1, 4, 1, 0, 0), (1, 2, 1, 0, 1),
             (0, 1, 3, 1, 0), (0, 2, 1, 0, 1), (0, 3, 2, 1, 2), (0, 4, 3, 1, 3), (0, 1, 1, 1, 1), (1, 1, 2, 1, 2))
    assert {c[4] for c in cases} == {0, 1, 2, 3} and {(c[0], c[1]) for c in cases} == {(e, n) for e in (0, 1) for n in (1, 2, 3, 4)}
    for case, (elem, ch, n_planes, misalign, par) in enumerate(cases):
        if elem:
            planes = [rng.integers(0, 256, (SH, SW, ch), dtype=np.uint8) for _ in range(n_planes)]
        else:
            planes = [(rng.standard_normal((SH, SW, ch)) * 30).astype(F32) for _ in range(n_planes)]
        _host_case(tmp_path, exe, case, elem, planes, geoms, fields, *PARAMS[par], misalign)
    # the negative-value store: the Catmull-Rom step edge on u8, 1 and 4 channels
    plane, co = step_edge_case()
    for n, ch in enumerate((1, 4)):
        pl = np.ascontiguousarray(np.repeat(plane, ch, axis=2))
        out = _host_case(tmp_path, exe, 100 + n, 1, [pl], [(0, 0, co.shape[1], co.shape[0])], [co.reshape(-1, 2)], 0.0, 0.5, 0)
        assert (out == 0).any() and (out == 255).any()


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_bicubic_over_the_recording_mock_addon():
    """tests/js/bicubic_class.mjs: sampling 'bicubic' reaches 'remapBicubic' + entry with the bilinear call's arguments plus B and C (the
    three preset names, an array, Catmull-Rom by default), refuses a bad `cubic` and what 'bilinear' refuses without reaching an entry
    point, and leaves the calls of the other four samplings as they were."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "bicubic_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_bicubic_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["failures"] == [] and p.returncode == 0, (res["failures"], p.stderr[-2000:])
    assert res["checks"] >= 100
