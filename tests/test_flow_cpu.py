"""CPU-side checks of the dense flow (include/hgwarp.h, "dense optical flow"): the header declares and the library exports the entries,
hg_flow_layout's values, every refusal that needs no device in the header's order, the numpy model of tests/hgtest/flow.py pinned by the
properties the design rests on (identical planes, a rolled plane, a flat plane, the endpoint error on a known smooth flow, no divergence with
more iterations), the kernel text itself on the host under sanitizers, and the JS class over a recording mock addon.
tests/test_gpu_flow.py compares the device with the model byte for byte."""
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
from hgtest import flow as FM                # noqa: E402

NEW = ["hg_flow_layout", "hg_flow_dense_frames_device", "hg_field_compose_frames_device"]
INVALID = 1
F32 = np.float32
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def test_header_declares_and_library_exports_the_flow_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in HG.EXPORTS, name
    assert "dense optical flow" in text and "hg_flow_dense_frames_device," in text.split("enum {")[0]      # the section; the note beside HG_VERSION
    assert callable(HG.flow_layout) and callable(HG.Context.flow_dense_frames_device) and callable(HG.Context.field_compose_frames_device)
    dev = open(os.path.join(CSRC, "hg_flow_dev.h")).read()
    assert f"kFlowTileW = {FM.TILE_W}, kFlowTileH = {FM.TILE_H}" in dev      # the tile the GPU test picks its sizes around


def test_flow_layout_values():
    pad = lambda b: (b + 255) // 256 * 256
    # one level, one channel: two flow buffers and nothing else
    assert HG.flow_layout(1, 1, 1, 1, 1, 1) == 2 * 256
    assert HG.flow_layout(10, 10, 1, 3, 1, 1) == 2 * pad(3 * 100 * 8)
    # RGBA adds the luma copies of every FROM and TO plane
    assert HG.flow_layout(10, 10, 4, 3, 2, 1) == pad(300) + pad(200) + 2 * pad(2400)
    # levels add the pyramids of both sets (hg_pyramid_layout's bytes each) and two flow buffers per level
    _, pyr = HG.pyramid_layout(33, 17, HG.ELEM_U8, 1, 4)
    assert pyr == pad(17 * 9) + pad(9 * 5) + pad(5 * 3)
    assert HG.flow_layout(33, 17, 1, 5, 2, 4) == 7 * pyr + 2 * sum(pad(5 * w * h * 8) for w, h in ((33, 17), (17, 9), (9, 5), (5, 3)))
    for a in ((160, 224, 1, 3, 1, 4), (33, 17, 4, 5, 2, 7), (1920, 1080, 4, 64, 1, 7), (3840, 2160, 4, 8, 8, 8), (5, 7, 4, 0, 1, 4), (32768, 32768, 1, 4096, 4096, 12)):
        assert HG.flow_layout(*a) == FM.layout(*a), a
    assert [HG.flow_default_levels(w, h) for w, h in ((1920, 1080), (3840, 2160), (160, 224), (31, 400), (15, 400), (32, 32), (1, 1))] == [7, 8, 4, 2, 1, 2, 1]
    assert [FM.default_levels(w, h) for w, h in ((1920, 1080), (3840, 2160), (160, 224), (31, 400), (15, 400), (32, 32), (1, 1))] == [7, 8, 4, 2, 1, 2, 1]
    sz = C.c_size_t()
    for bad in ((0, 8, 1, 1, 1, 1), (8, 32769, 1, 1, 1, 1), (32768, 32769, 1, 1, 1, 1), (8, 8, 2, 1, 1, 1), (8, 8, 1, 1, 1, 0), (8, 8, 1, 1, 1, 5), (8192, 8192, 1, 1, 1, 13),
                (8, 8, 1, -1, 1, 1), (8, 8, 1, 4097, 1, 1), (8, 8, 1, 2, 0, 1), (8, 8, 1, 2, 3, 1), (8, 8, 1, 0, 2, 1)):
        assert HG.lib().hg_flow_layout(*bad, C.byref(sz)) == INVALID, bad
    assert HG.lib().hg_flow_layout(8, 8, 1, 1, 1, 1, None) == INVALID
    assert HG.lib().hg_flow_layout(8, 8, 1, 1, 1, 4, C.byref(sz)) == 0 and HG.lib().hg_flow_layout(8192, 8192, 1, 1, 1, 12, C.byref(sz)) == 0


def test_refusals_without_a_device_in_the_headers_order():
    """Every shape check is made before the context is looked at (ctx is NULL throughout) and names itself in hg_last_error; a call that
    passes them all is refused for the NULL context.  Each bad argument is paired with a LATER one that is bad too: the earlier one must be
    the one reported."""
    L = HG.lib()
    good = dict(n_frames=3, fs=64 * 48, n_to=1, ts=64 * 48, W=64, H=48, ch=1, levels=3, n_iter=4, radius=3, min_eig=1.0, max_update=1.0)

    def call(**k):
        a = dict(good, **k)
        code = L.hg_flow_dense_frames_device(None, None, a["n_frames"], a["fs"], None, a["n_to"], a["ts"], a["W"], a["H"], a["ch"], a["levels"], a["n_iter"],
                                             a["radius"], a["min_eig"], a["max_update"], None, None, None, None, None, None)
        return code, L.hg_last_error(None).decode()

    inf, nan = float("inf"), float("nan")
    order = [(dict(W=0), "W and H"), (dict(H=32769), "W and H"), (dict(W=32768, H=32769), "W and H"),
             (dict(ch=3), "channels must"), (dict(ch=0), "channels must"), (dict(ch=2), "channels must"),
             (dict(levels=0), "levels must"), (dict(levels=8), "levels must"), (dict(W=8192, H=8192, levels=13, fs=1 << 26, ts=1 << 26), "levels must"),
             (dict(n_iter=0), "n_iter must"), (dict(n_iter=33), "n_iter must"),
             (dict(radius=0), "radius must"), (dict(radius=8), "radius must"),
             (dict(min_eig=-1.0), "min_eig must"), (dict(min_eig=nan), "min_eig must"), (dict(min_eig=inf), "min_eig must"),
             (dict(max_update=0.0), "max_update must"), (dict(max_update=4.0001), "max_update must"), (dict(max_update=nan), "max_update must"), (dict(max_update=-1.0), "max_update must"),
             (dict(n_frames=-1), "n_frames must"), (dict(n_frames=4097), "n_frames must"),
             (dict(n_to=0), "n_to_sets must"), (dict(n_to=4), "n_to_sets must"), (dict(n_frames=0, n_to=2), "n_to_sets must"),
             (dict(fs=64 * 48 - 1), "stride must"), (dict(ts=64 * 48 - 1), "stride must"), (dict(ch=4), "stride must")]
    for k, (bad, word) in enumerate(order):
        code, msg = call(**bad)
        assert code == INVALID and word in msg, (bad, msg)
        for later, word2 in order[k + 1:]:
            if word2 == word or set(later) & set(bad):
                continue
            code, msg = call(**dict(later, **bad))
            assert code == INVALID and word in msg, (bad, later, msg)
    for ok in (dict(), dict(min_eig=0.0), dict(max_update=4.0), dict(n_iter=32), dict(n_iter=1), dict(radius=1), dict(radius=7), dict(levels=7), dict(levels=1),
               dict(n_frames=0), dict(n_frames=4096, n_to=4096), dict(ch=4, fs=64 * 48 * 4, ts=64 * 48 * 4), dict(W=1, H=1, levels=1),
               dict(W=8192, H=8192, levels=12, fs=1 << 26, ts=1 << 26)):
        code, msg = call(**ok)
        assert code == INVALID and "ctx is NULL" in msg, (ok, msg)   # the limits themselves are legal: only the context is missing
    # the chained field refuses a NULL context like the remap it follows
    assert L.hg_field_compose_frames_device(None, None, 0, None, None, None, 4, 4, 1, 128, None, None) == INVALID
    assert "ctx is NULL" in L.hg_last_error(None).decode()


# ------------------------------------------------------------------------------------------------ the model, pinned
@pytest.mark.parametrize("W,H", [(1, 1), (2, 3), (5, 7), (9, 130)])
def test_identical_planes_give_a_zero_flow_and_the_identity_field(W, H):
    p = np.ascontiguousarray(FM.texture(max(W, 8), max(H, 8), 1 + W, 0.2)[:H, :W])
    xs, ys = FM.grid(W, H)
    for levels in range(1, FM.max_levels(W, H) + 1):
        for radius in (1, 3, 7):
            r = FM.flow(p, p, levels, 4, radius)
            assert not r.flow.any() and not r.residual.any()
            assert np.array_equal(r.field.view(np.uint32), np.stack([xs, ys], -1).view(np.uint32))


def test_a_plane_rolled_by_two_columns_gives_exactly_two():
    to = FM.texture(96, 64, 3)
    r = FM.flow(np.roll(to, 2, 1), to, 3, 4, 3)                       # FROM(x + 2, y) = TO(x, y)
    inner = r.flow[16:-16, 16:-16]
    assert np.median(inner[..., 0]) == 2.0 and np.median(inner[..., 1]) == 0.0
    assert np.median(r.residual[16:-16, 16:-16]) == 0


def test_a_flat_region_is_never_good_and_keeps_what_it_inherited():
    to = FM.texture(96, 64, 5)
    to[16:48, 24:72] = 120                                            # a flat block inside a textured plane
    frm = np.roll(to, 1, 1)
    r = FM.flow(frm, to, 3, 4, 3)
    assert not r.good[20:44, 28:68].any() and r.good[:12].mean() > 0.9
    one = FM.flow(frm, to, 1, 4, 3)                                   # one level: nothing to inherit, so the flat block stays at 0
    assert not one.flow[20:44, 28:68].any() and one.flow[:12].any()
    flat = np.full((20, 30), 77, np.uint8)
    z = FM.flow(to[:20, :30].copy(), flat, 3, 4, 3)
    assert not z.good.any() and not z.flow.any()


def test_min_eig_zero_cannot_divide_by_zero():
    """Vertical stripes: Gyy = Gxy = 0, so det = 0 with a positive trace; min_eig 0 would pass det >= 0, det > 0 does not."""
    to = np.tile((np.arange(40) % 8 * 30).astype(np.uint8), (24, 1))
    r = FM.flow(np.roll(to, 1, 1), to, 2, 3, 3, min_eig=0.0)
    assert not r.good.any() and not r.flow.any() and np.isfinite(r.flow).all()


def test_endpoint_error_on_a_known_smooth_flow_and_no_divergence():
    """The fixture of the design: a band-limited texture of 160 x 224 and its bilinear resampling through sinusoids of 5 and 3 px plus an
    offset of 1.5 px.  The cap is 0.1 x the mean length of the true flow; with more iterations the error may not grow by more than a tenth."""
    frm, to, u, v = FM.fixture()
    zero = float(np.hypot(u, v).mean())
    e4 = FM.epe(FM.flow(frm, to, 4, 4, 3).flow, u, v)
    e8 = FM.epe(FM.flow(frm, to, 4, 8, 4).flow, u, v)
    e16 = FM.epe(FM.flow(frm, to, 4, 16, 4).flow, u, v)
    e1 = FM.epe(FM.flow(frm, to, 1, 8, 4).flow, u, v)
    print(f"zero-flow EPE {zero:.3f} px; 4 levels / 4 iterations / radius 3: {e4:.4f}; radius 4, 8 iterations {e8:.4f}, 16 iterations {e16:.4f}; 1 level {e1:.4f}")
    assert 2.5 < zero < 3.5
    assert e4 <= 0.1 * zero
    assert e16 <= 1.1 * e8
    assert e1 > 2 * e4                                                # the pyramid is needed


def test_compose_model_by_hand():
    inner = np.zeros((2, 3, 2), F32)
    inner[..., 0] = [[0, 10, 20], [100, 110, 120]]
    inner[..., 1] = [[1, 2, 3], [4, 5, np.nan]]
    out = FM.compose(np.array([[0.5, 0.5], [np.nan, 0], [0, np.inf], [1.5, 0.5], [-9, -9], [1e30, -5]], F32), inner)
    assert out[0].tolist() == [55.0, 3.0] and out[4].tolist() == [0.0, 1.0] and out[5].tolist() == [20.0, 3.0]
    assert (out[[1, 2, 3]].view(np.uint32) == FM.NAN_WORD).all()      # NaN / Inf coordinates, and a NaN tap


# ------------------------------------------------------------------------------------------------ the kernel text on the host
@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/flow_check.cpp: hg_k_flow.hip itself (and hg_k_pyramid.hip for the levels), compiled for the CPU behind the thread-index shim
    -- a workgroup of k_flow_iter as 256 host threads -- and run under ASan + UBSan on exact-size heap buffers: no byte outside a buffer is
    touched, and what the kernels compute is the model's, byte for byte.  Shapes smaller than a tile and smaller than the window, a tile
    and a bit, both LDS sizes.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "flow_check")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", os.path.join(cpp, "hip_stub"), "-I", CSRC, os.path.join(cpp, "flow_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    rng = np.random.default_rng(4)
    cases = [(1, 1, 1, 1, 1, 2, 7), (2, 3, 1, 1, 3, 2, 7), (5, 7, 2, 1, 4, 2, 7), (5, 7, 1, 1, 2, 3, 1), (33, 17, 2, 2, 4, 2, 3), (FM.TILE_W + 1, FM.TILE_H + 1, 1, 1, 2, 2, 4),
             (FM.TILE_W - 1, 2 * FM.TILE_H + 1, 2, 1, 3, 3, 2)]
    for k, (W, H, F, S, levels, n_iter, radius) in enumerate(cases):
        tos = [np.ascontiguousarray(FM.texture(max(W, 8), max(H, 8), 20 + 3 * k + s, 0.2)[:H, :W]) for s in range(S)]
        frms = [np.ascontiguousarray(np.roll(tos[f % S], (1, f), (1, 0))) for f in range(F)]
        outer = rng.uniform(-2, max(W, H) + 2, (40, 2)).astype(F32)
        outer[:4] = [[np.nan, 0], [0, np.inf], [0, 0], [W - 1, H - 1]]
        fin, fout = tmp_path / f"case{k}.in", tmp_path / f"case{k}.out"
        fin.write_bytes(struct.pack("<8i2d", W, H, F, S, levels, n_iter, radius, len(outer), 0.5, 1.5) + b"".join(p.tobytes() for p in frms + tos) + outer.tobytes())
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (k, (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (k, (p.stdout + p.stderr)[-3000:])
        raw, n = fout.read_bytes(), W * H
        assert len(raw) == F * n * 18 + len(outer) * 8
        want = FM.flow_frames(frms, tos, 1, levels, n_iter=n_iter, radius=radius, min_eig=0.5, max_update=1.5)
        for f, w in enumerate(want):
            b = raw[f * n * 18:(f + 1) * n * 18]
            assert b[:n * 8] == w.field.tobytes(), (k, f, "field")
            assert b[n * 8:n * 16] == np.ascontiguousarray(w.flow).tobytes(), (k, f, "flow")
            assert b[n * 16:n * 17] == w.residual.tobytes(), (k, f, "residual")
            assert b[n * 17:] == w.good.tobytes(), (k, f, "good")
        assert raw[F * n * 18:] == FM.compose(outer, want[0].field).tobytes(), (k, "chained")


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_dense_flow_over_the_recording_mock_addon():
    """tests/js/flow_class.mjs: h.denseFlow(fromImages, toImages, options) over a recording mock addon: the option defaults, the bare strings
    it throws, the arguments the addon gets and the shape of the result."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "flow_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_flow_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ok"] and res["fails"] == [] and p.returncode == 0, (res["fails"], p.stderr[-2000:])
    assert res["checks"] >= 20
