"""CPU-side checks of the source-field feature (include/hgwarp.h, HG_FIELD_*): the header declares and the library exports the new
entry points, hg_pack_field_offsets, and -- without any GPU -- the numpy model of tests/hgtest/field.py pinned to the reference through
the CPU oracle on the edge-case inputs of tests/hgtest/edges.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import edges as E                # noqa: E402
from hgtest import field as FM               # noqa: E402
from hgtest import oracle as O               # noqa: E402

NEW = ["hg_pack_field_offsets", "hg_field_inverse_geometric", "hg_field_inverse_geometric_device", "hg_field_inverse_geometric_frames_device",
       "hg_field_inverse_piecewise", "hg_field_inverse_piecewise_frames_device", "hg_remap_index_device", "hg_remap_bilinear_f32_device"]


def test_header_declares_and_library_exports_the_field_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in HG.EXPORTS, name
    assert re.search(r"HG_FIELD_INDEX\s*=\s*0\b", code) and re.search(r"HG_FIELD_COORDS\s*=\s*1\b", code)
    assert (HG.FIELD_INDEX, HG.FIELD_COORDS) == (0, 1)
    assert re.search(r"#define\s+HG_VERSION\s+100\b", code) and L.hg_version() == 100


def test_pack_field_offsets():
    geoms = [(0, 0, 7, 3), (-5, 2, 0, 9), (1, 1, 64, 1), (3, -3, 5, -1), (0, 0, 100, 100)]
    px = [7 * 3, 0, 64, 0, 100 * 100]
    for fmt, per in ((HG.FIELD_INDEX, 4), (HG.FIELD_COORDS, 8)):
        offs, total = HG.pack_field_offsets(geoms, fmt)
        want, off = [], 0
        for n in px:
            want.append(off)
            off += (n * per + 255) // 256 * 256
        assert offs == want and total == off
        assert all(o % 256 == 0 for o in offs)
        assert offs[1] == offs[2] and offs[3] == offs[4]        # empty frames take no room
    L = HG.lib()
    g = (HG.Geom * 1)(HG.Geom(0, 0, 4, 4))
    offs, total = (C.c_size_t * 1)(), C.c_size_t(0)
    assert L.hg_pack_field_offsets(g, 1, 0, offs, C.byref(total)) == 0 and total.value == 256
    for bad_fmt in (2, -1):
        assert L.hg_pack_field_offsets(g, 1, bad_fmt, offs, C.byref(total)) == 1        # HG_ERR_INVALID
        with pytest.raises(HG.HgError) as e:
            HG.pack_field_offsets([(0, 0, 4, 4)], bad_fmt)
        assert e.value.code == 1
    assert L.hg_pack_field_offsets(None, 1, 0, offs, C.byref(total)) == 1
    assert L.hg_pack_field_offsets(g, 1, 0, None, C.byref(total)) == 1
    assert L.hg_pack_field_offsets(g, 1, 0, offs, None) == 1


def _check_model(img, sx, sy, valid, msx, msy, want, what):
    H, W = img.shape[:2]
    idx = FM.index_field(sx, sy, valid, W, H, msx, msy)
    co = FM.coords_field(sx, sy, valid, W, H, msx, msy)
    got = FM.remap_index(idx, img.reshape(-1, 4)).reshape(want.shape)
    assert np.array_equal(got, want), what
    nan = co.view(np.uint32) == FM.NAN_BITS
    assert np.array_equal(nan[..., 0], nan[..., 1]), what
    assert not nan[..., 0][idx >= 0].any(), what              # index >= 0 implies "not NaN"
    assert np.array_equal(~nan[..., 0], FM.covered(sx, sy, valid, W, H, msx, msy)), what
    fin = ~nan[..., 0]
    assert np.array_equal(co[..., 0][fin], sx[fin].astype(np.float32)) and np.array_equal(co[..., 1][fin], sy[fin].astype(np.float32)), what


def test_model_is_pinned_to_the_reference_on_every_edge_case():
    total = {}

    def add(c):
        for k, v in c.items():
            total[k] = total.get(k, 0) + v

    for name, build in E.GEOMETRIC.items():
        case = build()
        kind, m, img, geom = case
        sx, sy, valid = E.geometric_coords(case)
        _check_model(img, sx, sy, valid, 0, 0, O.warp_inverse_geometric(kind, m, img, *geom), name)
        add(E.classify(sx, sy, valid, img.shape[1], img.shape[0]))
    for name in E.PIECEWISE:
        for twin in (False, True):
            case = E.piecewise(name, twin)
            sp, tris, msx, msy, dp, geom, img = case
            out, wmap, inv, sx, sy, valid = E.piecewise_taps(case)
            assert np.array_equal(out, O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom))
            _check_model(img, sx, sy, valid, msx, msy, out, (name, twin))
            add(E.classify(sx, sy, valid, img.shape[1], img.shape[0], msx, msy))
    for cls in ("E1", "E2", "E3", "E4", "E6"):
        keys = [k for k in total if k.startswith(cls)]
        assert keys and all(total[k] > 0 for k in keys), (cls, {k: total[k] for k in keys})


def test_remap_models():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 255, (50, 3), dtype=np.uint8)
    f = np.array([0, 49, 50, -1, 2 ** 31 - 1, -2 ** 31, 7], np.int32)
    got = FM.remap_index(f, src)
    assert np.array_equal(got[[0, 1, 6]], src[[0, 49, 7]]) and not got[[2, 3, 4, 5]].any()
    # bilinear: at integer coordinates the tap itself; outside the image the clamped border; NaN / Inf give zeros; 1e30 is legal
    img = rng.standard_normal((5, 7, 2)).astype(np.float32)
    co = np.array([[2, 3], [-4, 1], [1e30, 2], [6, 4], [7, 4], [np.nan, 1], [1, np.inf], [-0.0, 0], [2.5, 1]], np.float32)
    out = FM.remap_bilinear_f32(co, img)
    assert np.array_equal(out[0], img[3, 2]) and np.array_equal(out[1], img[1, 0]) and np.array_equal(out[2], img[2, 6])
    assert np.array_equal(out[3], img[4, 6]) and np.array_equal(out[4], img[4, 6]) and not out[5].any() and not out[6].any()
    assert np.array_equal(out[7], img[0, 0])
    half = np.float32(0.5)
    assert np.array_equal(out[8], (img[1, 2] * half + img[1, 3] * half) * np.float32(1) + (img[2, 2] * half + img[2, 3] * half) * np.float32(0))
