"""CPU-side checks of the remaps of whole frame sets and the 8-bit bilinear remap (include/hgwarp.h, hg_remap_*_frames_device,
hg_remap_bilinear_u8_device, hg_pack_plane_offsets): declarations and exports, the host-only packing, the refusal of a NULL context,
the u8 model of tests/hgtest/remap_frames.py on hand-computed cases, and the class's remap() over a recording mock addon."""
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
from hgtest import field as FM               # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402

NEW = ["hg_pack_plane_offsets", "hg_remap_index_frames_device", "hg_remap_bilinear_frames_device", "hg_remap_bilinear_u8_device"]
INVALID = 1
F32 = np.float32


def test_header_declares_and_library_exports_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in HG.EXPORTS, name
    assert re.search(r"HG_ELEM_F32\s*=\s*0\b", code) and re.search(r"HG_ELEM_U8\s*=\s*1\b", code)
    assert (HG.ELEM_F32, HG.ELEM_U8) == (0, 1)
    for name in ("remap_index_frames_device", "remap_bilinear_frames_device", "remap_bilinear_u8_device"):
        assert callable(getattr(HG.Context, name)), name


def test_pack_plane_offsets():
    geoms = [(0, 0, 7, 3), (-5, 2, 0, 9), (1, 1, 64, 1), (3, -3, 5, -1), (0, 0, 100, 100), (9, 9, 256, 1)]
    # hand-computed: 21, 0, 64, 0, 10000 and 256 pixels, each frame rounded up to 256 bytes
    want = {1: ([0, 256, 256, 512, 512, 10752], 11008),
            3: ([0, 256, 256, 512, 512, 30720], 31488),
            16: ([0, 512, 512, 1536, 1536, 161536], 165632)}
    for px_bytes, (offs, total) in want.items():
        assert HG.pack_plane_offsets(geoms, px_bytes) == (offs, total), px_bytes
        assert RF.pack(geoms, px_bytes) == (offs, total), px_bytes                    # (the tests' own packing is the same rule)
    assert HG.pack_plane_offsets(geoms, 4) == HG.pack_field_offsets(geoms, HG.FIELD_INDEX)
    assert HG.pack_plane_offsets(geoms, 8) == HG.pack_field_offsets(geoms, HG.FIELD_COORDS)
    assert HG.pack_plane_offsets([], 4) == ([], 0)                                  # n = 0
    L = HG.lib()
    g = (HG.Geom * 1)(HG.Geom(0, 0, 4, 4))
    offs, total = (C.c_size_t * 1)(), C.c_size_t(7)
    assert L.hg_pack_plane_offsets(g, 0, 4, offs, C.byref(total)) == 0 and total.value == 0
    assert L.hg_pack_plane_offsets(g, 1, 3, offs, C.byref(total)) == 0 and (offs[0], total.value) == (0, 256)
    assert L.hg_pack_plane_offsets(None, 1, 4, offs, C.byref(total)) == INVALID
    assert L.hg_pack_plane_offsets(g, 1, 4, None, C.byref(total)) == INVALID
    assert L.hg_pack_plane_offsets(g, 1, 4, offs, None) == INVALID
    assert L.hg_pack_plane_offsets(g, -1, 4, offs, C.byref(total)) == INVALID
    assert L.hg_pack_plane_offsets(g, 1, 0, offs, C.byref(total)) == INVALID
    with pytest.raises(HG.HgError) as e:
        HG.pack_plane_offsets([(0, 0, 4, 4)], 0)
    assert e.value.code == INVALID


def test_a_null_context_is_refused():
    L = HG.lib()
    g = (HG.Geom * 1)(HG.Geom(0, 0, 4, 4))
    p = C.c_void_p(4096)
    assert L.hg_remap_index_frames_device(None, g, 1, p, None, p, 16, 1, 64, 4, p, None) == INVALID
    assert L.hg_remap_bilinear_frames_device(None, g, 1, p, None, p, 4, 4, 1, 64, HG.ELEM_U8, 1, p, None) == INVALID
    assert L.hg_remap_bilinear_u8_device(None, p, 16, p, 4, 4, 1, p) == INVALID


def test_u8_model_on_hand_computed_cases():
    def one(src, sx, sy):
        return RF.remap_bilinear_u8(np.array([[sx, sy]], F32), np.asarray(src, np.uint8))[0]

    # the tie: p = (0, 1), fx = 0.5 -> v = 0.5 -> floor(0.5 + 0.5) = 1
    assert one([[[0], [1]]], 0.5, 0)[0] == 1
    assert one([[[0], [1]], [[0], [1]]], 0.5, 0.5)[0] == 1
    # all-255 taps give 255 at any fraction (the clamp: the f32 blend may exceed 255 by an ulp, never the result)
    full = np.full((2, 2, 3), 255, np.uint8)
    for sx, sy in ((0.3, 0.7), (0.5, 0.5), (0.1, 0.9), (1 / 3, 2 / 3)):
        assert (one(full, sx, sy) == 255).all()
    # fx = fy = 0 gives p00
    src = np.array([[[10, 200], [20, 100]], [[30, 50], [40, 25]]], np.uint8)
    assert one(src, 0, 0).tolist() == [10, 200] and one(src, 1, 1).tolist() == [40, 25] and one(src, 1, 0).tolist() == [20, 100]
    # by hand: (10 * .75 + 20 * .25) * .5 + (30 * .75 + 40 * .25) * .5 = 22.5 -> 23; (200 * .75 + 100 * .25) * .5 + (50 * .75 + 25 * .25) * .5 = 109.375 -> 109
    assert one(src, 0.25, 0.5).tolist() == [23, 109]
    # -1e-30: x0 = -1, fx = -1e-30 - (-1) rounds to 1: the f32 model's own choice -- weight 1 on the tap clamp(x0 + 1) = column 0
    tiny = F32(-1e-30)
    assert np.floor(tiny) == -1 and tiny - np.floor(tiny) == F32(1)
    f = FM.remap_bilinear_f32(np.array([[tiny, 0]], F32), src.astype(F32))[0]
    assert f.tolist() == [10.0, 200.0] and one(src, tiny, 0).tolist() == [10, 200]
    assert one(src, 0, tiny).tolist() == [10, 200]
    # NaN / infinite coordinates give 0 in every channel; huge ones clamp
    for sx, sy in ((np.nan, 0), (0, np.inf), (-np.inf, 1)):
        assert one(src, sx, sy).tolist() == [0, 0]
    assert one(src, 1e30, -1e30).tolist() == [20, 100]
    # the model is the f32 model rounded: on random data never further than half a step from it
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (9, 11, 4), dtype=np.uint8)
    co = (rng.random((500, 2)) * [13, 11] - 1).astype(F32)
    v = FM.remap_bilinear_f32(co, img.astype(F32))
    got = RF.remap_bilinear_u8(co, img)
    assert got.dtype == np.uint8 and (np.abs(got.astype(np.float64) - v) <= 0.5 + 1e-4).all()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "homography.js_amd", "lib", "hgwarp.node")),
                    reason="node or the N-API addon is missing")
def test_js_class_remap_over_the_recording_mock_addon():
    """tests/js/remap_class.mjs: remap() makes the field-side addon calls sourceField() makes, for each loop and transform, with the same
    arguments; no forward entry call under {loop: 'inverse'}; every bad plane or option throws a bare string; the empty window works."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "remap_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_remap_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["failures"] == [] and p.returncode == 0, (res["failures"], p.stderr[-2000:])
    assert res["checks"] >= 150


CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)


@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/remap_frames_check.cpp: the frame-set remap kernels -- hg_k_remap.hip itself --, compiled for the CPU behind a thread-index
    shim and run under ASan + UBSan against a scalar loop -- no byte outside a buffer is touched, whatever the alignment."""
    exe = str(tmp_path / "remap_frames_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "remap_frames_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "host check passed" in p.stdout, (p.stdout + p.stderr)[-3000:]
    assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (p.stdout + p.stderr)[-3000:]
