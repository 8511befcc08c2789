"""The source field of the FORWARD warps (hg_field_forward_*) against the model of tests/hgtest/fwd_field.py (the oracle's forward warp of
an image that names every source pixel; judged on the CPU by tests/test_forward_field_cpu.py), on the edge cases of tests/hgtest/fwd_edges.py:
tile borders, Math.round ties, alias columns, 256-row pass boundaries, admission limits, tile capacities.  Both paths -- the tile-binned
kernels' field tails (fwd_tiles 1) and scatter + k_fwd_win_field (fwd_tiles 0) -- bit-exact, with the path that ran
(hg_last_forward_field_kernel) and the frames redone (hg_redone_frames) asserted in every case, so that no case can pass on the other path."""
import ctypes as C

import numpy as np
import pytest

from hgtest import fwd_edges as F
from hgtest import fwd_field as M
from hgtest import gpu_frames as GF
from hgtest import hip
from hgtest import oracle as O

pytestmark = pytest.mark.gpu

HG = hip.load()
GEO = F.geometric_cases()
PW = F.piecewise_cases()
FUZZ_SEED, FUZZ_DRAWS = 2025, 420          # (tests/test_forward_field_cpu.py: at least 300 of these draws are admitted)
SENTINEL = 0x5A

_models = {}


def _model(name):
    """The model of a named case, computed once and handed out read-only."""
    if name not in _models:
        m = M.geometric_case(GEO[name]) if name in GEO else M.piecewise_case(PW[name])
        m.setflags(write=False)
        _models[name] = m
    return _models[name]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, want.shape, got.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        h, w = want.shape
        first = [(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in bad[:6]]
        where = {"alias columns": int(((bad[:, 1] < F.WRAP) | (bad[:, 1] >= w - F.WRAP)).sum()),
                 "tile borders": int(((bad % F.TILE == 0) | (bad % F.TILE == F.TILE - 1)).any(1).sum()),
                 "got -1": int((got[bad[:, 0], bad[:, 1]] == -1).sum())}
        raise AssertionError(f"{what}: {len(bad)} of {h * w} field entries differ, {where}; (row, col, got, want): {first}")


def _ctx(tiles):
    c = HG.Context(0)
    c.set_option("fwd_tiles", tiles)
    return c


def _field(c, d_field, geom, off=0):
    return c.to_host(d_field, geom[2] * geom[3] * 4, off).view(np.int32).reshape(geom[3], geom[2])


def _rgba(c, d_out, geom, off=0):
    return c.to_host(d_out, geom[2] * geom[3] * 4, off).reshape(geom[3], geom[2], 4)


# ------------------------------------------------------------------------------------------------ geometric

@pytest.mark.parametrize("name", list(GEO))
def test_geometric_cases(name):
    """Every geometric case: the host form (one frame: parameters in the kernel arguments), the device batch with one frame, and the frame
    twice with swapped offsets (uploaded parameters), with the tile kernel forced and switched off."""
    case = GEO[name]
    kind, m, geom = case["kind"], case["m"], case["geom"]
    want = _model(name)
    assert (want >= 0).any()
    m8 = np.zeros(8)
    m8[:m.size] = m
    nbytes = geom[2] * geom[3] * 4
    for tiles in (1, 0):
        expect = 2 if tiles and case["admit"] else 1
        c = _ctx(tiles)
        d_field = c.alloc(2 * nbytes)
        try:
            c.set_image(F.image(case))
            assert c.last_forward_field_kernel() == 0
            _same(c.field_forward_geometric(kind, m, geom), want, (name, tiles, "host"))
            assert c.last_forward_field_kernel() == expect, (name, tiles, c.last_forward_field_kernel())
            c.field_forward_geometric_batch_device(kind, m8, [geom], [0], d_field)
            assert c.last_forward_field_kernel() == expect, (name, tiles, c.last_forward_field_kernel())
            _same(_field(c, d_field, geom), want, (name, tiles, "device"))
            c.field_forward_geometric_batch_device(kind, np.concatenate([m8, m8]), [geom, geom], [nbytes, 0], d_field)
            assert c.last_forward_field_kernel() == expect, (name, tiles, c.last_forward_field_kernel())
            for f in (0, 1):
                _same(_field(c, d_field, geom, f * nbytes), want, (name, tiles, "batch", f))
            assert c.last_forward_kernel() == 0                       # the warps' own tap: no forward warp ran on this context
        finally:
            c.free(d_field); c.close()


def test_geometric_fuzz_at_the_limits():
    """Every admitted draw: the field of k_fwd_tiles' field form under fwd_tiles 1 and of scatter + k_fwd_win_field equals the model."""
    cases, _, _ = F.fuzz(FUZZ_SEED, FUZZ_DRAWS, HG.forward_tiles_admissible)
    assert len(cases) >= 300
    wrong = []
    ct, cs = _ctx(1), _ctx(0)
    try:
        for case in cases:
            kind, m, geom = case["kind"], case["m"], case["geom"]
            img = np.zeros((case["H"], case["W"], 4), np.uint8)       # (only the size is read)
            want = M.geometric_case(case)
            for c, code in ((ct, 2), (cs, 1)):
                c.set_image(img)
                got = c.field_forward_geometric(kind, m, geom)
                assert c.last_forward_field_kernel() == code, (case["name"], code, c.last_forward_field_kernel())
                if not np.array_equal(got, want):
                    wrong.append((case["name"], code, kind, m.tolist(), case["W"], case["H"], geom, int((got != want).sum())))
        assert not wrong, (len(wrong), wrong[:4])
        assert ct.last_forward_kernel() == 0 and cs.last_forward_kernel() == 0
    finally:
        ct.close(); cs.close()


# ------------------------------------------------------------------------------------------------ piecewise

def _pw_field(c, case, host):
    """One forward piecewise field through the host form, or through the device batch form (settled inside the call: no sync)."""
    if host:
        return c.field_forward_piecewise(case["dp"], case["Mx"], case["My"], case["geom"])
    g = case["geom"]
    d_field = c.alloc(g[2] * g[3] * 4)
    try:
        c.field_forward_piecewise_batch_device(case["dp"], case["Mx"], case["My"], [g], [0], d_field)
        return _field(c, d_field, g)
    finally:
        c.free(d_field)


def _pw_warp(c, case):
    return c.warp_forward_piecewise(case["dp"], case["Mx"], case["My"], case["geom"])


def _set(c, case):
    c.set_image(F.image(case))
    c.piecewise_set_mesh(case["sp"], case["tris"], case["msx"], case["msy"])          # (also re-arms the tile path and its first capacity)


def _taps(c):
    return (c.last_forward_field_kernel(), c.redone_frames())


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", [n for n in PW if "entries" not in PW[n]])
def test_piecewise_cases(name, host):
    """The first field call on a fresh mesh reports the path and redoes the frames the case claims; a frame the bins kernel could not
    bound switches the tile path off for the mesh: the next call takes the scatter path and redoes nothing -- as test_piecewise_edges
    expects of the warps."""
    case = PW[name]
    want = _model(name)
    assert (want >= 0).any()
    c = _ctx(0)
    try:
        _set(c, case)
        _same(_pw_field(c, case, host), want, (name, "scatter"))
        assert _taps(c) == (1, 0)
        assert c.last_forward_kernel() == 0
    finally:
        c.close()
    c = _ctx(1)
    try:
        _set(c, case)
        _same(_pw_field(c, case, host), want, (name, "tiles"))
        assert _taps(c) == (case["kernel"], case["flagged"]), (name, _taps(c))
        _same(_pw_field(c, case, host), want, (name, "tiles, second call"))
        again = 1 if case["flagged"] else case["kernel"]
        assert _taps(c) == (again, case["flagged"]), (name, _taps(c))
        assert c.last_forward_kernel() == 0
        if case["flagged"]:                                           # another mesh re-arms the tile path (the same mesh sent again does not)
            _set(c, PW["rotated_90"])
            _same(_pw_field(c, PW["rotated_90"], host), _model("rotated_90"), (name, "re-armed"))
            assert _taps(c) == (2, case["flagged"])
    finally:
        c.close()


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", [n for n in PW if "entries" in PW[n]])
def test_piecewise_tile_capacity_is_learned_by_field_calls(name, host):
    """test_piecewise_tile_capacity with the field calls doing the learning: an overfull tile list flags the frame (redone through the
    scatter path inside the call), the capacity doubles, 64 -> 128 -> 256; a tile past 256 entries is flagged once at each capacity, then
    the tile path is off for the mesh.  One forward WARP after the ladder finds what the field calls learned: it redoes nothing."""
    case = PW[name]
    n = case["entries"]
    flags = 0 if n <= F.PW_CAP0 else 1 if n <= 2 * F.PW_CAP0 else 2 if n <= F.PW_CAP_MAX else 3
    want = _model(name)
    c = _ctx(1)
    try:
        _set(c, case)
        for call in range(flags + 2):
            _same(_pw_field(c, case, host), want, (name, "call", call))
            off = n > F.PW_CAP_MAX and call >= flags
            assert _taps(c) == (1 if off else 2, min(call + 1, flags)), (name, call, _taps(c))
        img = F.image(case)
        assert np.array_equal(_pw_warp(c, case), F.piecewise_oracle(case, img)), (name, "warp after the ladder")
        assert (c.last_forward_kernel(), c.redone_frames()) == (1 if n > F.PW_CAP_MAX else 2, flags), (name, c.last_forward_kernel(), c.redone_frames())
        small = F.dense(F.DENSE["65-128"] // 2)                       # 48 entries: fits the first capacity
        assert small["entries"] <= F.PW_CAP0
        _set(c, small)
        _same(_pw_field(c, small, host), M.piecewise_case(small), (name, "re-armed"))
        assert _taps(c) == (2, flags)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ batches

def _padded_offsets(geoms):
    """Explicit offsets with gaps between the frames and in front of the first one; (offsets, total bytes)."""
    offs, off = [], 260
    for g in geoms:
        offs.append(off)
        off += (max(g[2], 0) * max(g[3], 0) * 4 + 255) // 256 * 256 + 516
    return offs, off


def _check_batch(c, d_field, d_out, d_remap, d_src, stride, W, H, n_imgs, geoms, offs, total, models, what):
    """Frames equal the model, every byte outside them is the sentinel, and the remap of frame f's image through frame f's field equals
    the bytes of the forward warp of the same inputs (both computed on the device, compared on the host)."""
    raw = c.to_host(d_field, total)
    outside = np.ones(total, bool)
    for f, g in enumerate(geoms):
        if g[2] <= 0 or g[3] <= 0: continue
        nb = g[2] * g[3] * 4
        outside[offs[f]:offs[f] + nb] = False
        _same(raw[offs[f]:offs[f] + nb].view(np.int32).reshape(g[3], g[2]), models[f], (what, "frame", f))
        c.remap_index_device(d_field + offs[f], g[2] * g[3], d_src + (f % n_imgs) * stride, W * H, 4, d_remap + offs[f])
    assert (raw[outside] == SENTINEL).all(), (what, "bytes outside the frames were written", int((raw[outside] != SENTINEL).sum()))
    c.sync()
    warped, remapped = c.to_host(d_out, total), c.to_host(d_remap, total)
    for f, g in enumerate(geoms):
        if g[2] <= 0 or g[3] <= 0: continue
        nb = g[2] * g[3] * 4
        assert np.array_equal(remapped[offs[f]:offs[f] + nb], warped[offs[f]:offs[f] + nb]), (what, "remap != warp", f)
        assert warped[offs[f]:offs[f] + nb].any(), (what, f)


def test_geometric_batch_of_mixed_windows():
    """G8: five frames in one call, an empty one in the middle, two source images (frame f reads image f mod 2), padded offsets."""
    b = F.batch()
    W, H, kind = b["W"], b["H"], b["kind"]
    imgs = [O.lcg_image(W, H, s) for s in b["seeds"]]
    mats = np.concatenate([m for m, _ in b["frames"]])
    geoms = [g for _, g in b["frames"]]
    models = [M.geometric(kind, m, W, H, g) if g[2] > 0 else None for m, g in b["frames"]]
    offs, total = _padded_offsets(geoms)
    stride = W * H * 4
    for tiles in (1, 0):
        c = _ctx(tiles)
        d_src, d_field, d_out, d_remap = c.alloc(2 * stride), c.alloc(total), c.alloc(total), c.alloc(total)
        try:
            for k in (0, 1): c.to_device(d_src, imgs[k], k * stride)
            c.set_images_device(d_src, W, H, 2, stride)
            c.to_device(d_field, np.full(total, SENTINEL, np.uint8))
            c.field_forward_geometric_batch_device(kind, mats, geoms, offs, d_field)
            assert c.last_forward_field_kernel() == (2 if tiles else 1) and c.last_forward_kernel() == 0
            c.warp_forward_geometric_batch_device(kind, mats, geoms, offs, d_out)
            _check_batch(c, d_field, d_out, d_remap, d_src, stride, W, H, 2, geoms, offs, total, models, ("G8", tiles))
        finally:
            c.free(d_remap); c.free(d_out); c.free(d_field); c.free(d_src); c.close()


def _p9():
    b = F.piecewise_batch()
    box = b["box"]
    geoms = [g for _, g in b["frames"]]
    cases = [{"sp": b["sp"], "tris": b["tris"], "dp": d, "W": b["W"], "H": b["H"], "msx": box[0], "msy": box[1], "Mx": box[2], "My": box[3], "geom": g}
             for d, g in b["frames"]]
    models = [M.piecewise_case(k) if k["geom"][2] > 0 else None for k in cases]
    return b, geoms, cases, models


def test_piecewise_batch_of_mixed_windows():
    """P9: five frames (an empty one in the middle) with one source per frame, padded offsets."""
    b, geoms, cases, models = _p9()
    W, H, box, n = b["W"], b["H"], b["box"], len(geoms)
    imgs = [O.lcg_image(W, H, s) for s in b["seeds"]]
    dps = np.concatenate([d for d, _ in b["frames"]])
    offs, total = _padded_offsets(geoms)
    stride = W * H * 4
    for tiles in (1, 0):
        c = _ctx(tiles)
        d_src, d_field, d_out, d_remap = c.alloc(n * stride), c.alloc(total), c.alloc(total), c.alloc(total)
        try:
            for k in range(n): c.to_device(d_src, imgs[k], k * stride)
            c.set_images_device(d_src, W, H, n, stride)
            c.piecewise_set_mesh(b["sp"], b["tris"], box[0], box[1])
            c.to_device(d_field, np.full(total, SENTINEL, np.uint8))
            c.field_forward_piecewise_batch_device(dps, box[2], box[3], geoms, offs, d_field)
            assert _taps(c) == (2 if tiles else 1, 0) and c.last_forward_kernel() == 0
            c.warp_forward_piecewise_batch_device(dps, box[2], box[3], geoms, offs, d_out)
            _check_batch(c, d_field, d_out, d_remap, d_src, stride, W, H, n, geoms, offs, total, models, ("P9", tiles))
            assert c.redone_frames() == 0
        finally:
            c.free(d_remap); c.free(d_out); c.free(d_field); c.free(d_src); c.close()


def test_a_field_call_leaves_a_queued_warp_batch_alone():
    """A tile-path forward piecewise batch is queued and not synced; the field of the same frames goes into another buffer; then sync.  The
    warp's frames are the oracle's, the field is the model's, and the warps' tap and the sampling mode are what they were."""
    b, geoms, cases, models = _p9()
    W, H, box, n = b["W"], b["H"], b["box"], len(geoms)
    imgs = [O.lcg_image(W, H, s) for s in b["seeds"]]
    dps = np.concatenate([d for d, _ in b["frames"]])
    offs, total = HG.pack_offsets(geoms)
    stride = W * H * 4
    c = _ctx(1)
    d_src, d_out, d_field = c.alloc(n * stride), c.alloc(total), c.alloc(total)
    try:
        for k in range(n): c.to_device(d_src, imgs[k], k * stride)
        c.set_images_device(d_src, W, H, n, stride)
        c.piecewise_set_mesh(b["sp"], b["tris"], box[0], box[1])
        c.set_sampling(HG.SAMPLE_BILINEAR)
        c.set_option("fwd_tiles", 0)
        c.field_forward_piecewise_batch_device(dps, box[2], box[3], geoms, None, d_field)       # (the field tap differs from the warp's below)
        c.set_option("fwd_tiles", 1)
        c.warp_forward_piecewise_batch_device(dps, box[2], box[3], geoms, offs, d_out)
        assert c.last_forward_kernel() == 2
        c.set_option("fwd_tiles", 0)
        c.field_forward_piecewise_batch_device(dps, box[2], box[3], geoms, None, d_field)       # packed: the same offsets as pack_offsets'
        c.sync()
        assert c.last_forward_kernel() == 2 and c.last_forward_field_kernel() == 1 and c.sampling == HG.SAMPLE_BILINEAR
        assert c.redone_frames() == 0
        assert HG.pack_field_offsets(geoms, HG.FIELD_INDEX) == (offs, total)
        for f, g in enumerate(geoms):
            if g[2] <= 0: continue
            assert np.array_equal(_rgba(c, d_out, g, offs[f]), F.piecewise_oracle(cases[f], imgs[f])), ("queued warp", f)
            _same(_field(c, d_field, g, offs[f]), models[f], ("field beside a queued warp", f))
        c.set_option("fwd_tiles", 1)                                                            # ... and the tile-path field beside a queued tile-path warp
        c.warp_forward_piecewise_batch_device(dps, box[2], box[3], geoms, offs, d_out)
        c.field_forward_piecewise_batch_device(dps, box[2], box[3], geoms, offs, d_field)
        c.sync()
        assert c.last_forward_kernel() == 2 and _taps(c) == (2, 0) and c.sampling == HG.SAMPLE_BILINEAR
        for f, g in enumerate(geoms):
            if g[2] <= 0: continue
            assert np.array_equal(_rgba(c, d_out, g, offs[f]), F.piecewise_oracle(cases[f], imgs[f])), ("queued warp, tiles", f)
            _same(_field(c, d_field, g, offs[f]), models[f], ("tile field beside a queued warp", f))
    finally:
        c.free(d_field); c.free(d_out); c.free(d_src); c.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals():
    case = PW["rotated_90"]
    g, m6 = (0, 0, 64, 16), np.float64([1, 0, 0, 1, 0, 0])
    L = HG.lib()
    dp = np.ascontiguousarray(case["dp"], np.float32)
    dpp = dp.ctypes.data_as(C.POINTER(C.c_float))
    geoms = (HG.Geom * 1)(HG.Geom(*case["geom"]))
    c = HG.Context(0)
    d_field = c.alloc(64 * 16 * 4 + case["geom"][2] * case["geom"][3] * 4 + 16)
    try:
        assert GF.refusal_code(c.field_forward_geometric, 0, m6, g) == 4                                  # HG_ERR_STATE: no image
        assert L.hg_field_forward_piecewise_batch_device(c._h, dpp, case["Mx"], case["My"], geoms, None, 1, C.c_void_p(d_field)) == 4
        c.set_image(F.image(case))
        assert L.hg_field_forward_piecewise_batch_device(c._h, dpp, case["Mx"], case["My"], geoms, None, 1, C.c_void_p(d_field)) == 4      # no mesh
        assert GF.refusal_code(c.field_forward_geometric, 2, np.zeros(8), g) == 1                         # HG_ERR_INVALID: unknown kind
        assert GF.refusal_code(c.field_forward_geometric_batch_device, 0, np.zeros(8), [g], [0], 0) == 1  # NULL field
        assert L.hg_field_forward_geometric(c._h, 0, m6.ctypes.data_as(C.POINTER(C.c_double)), HG.Geom(*g), None) == 1
        assert L.hg_field_forward_geometric(c._h, 0, None, HG.Geom(*g), C.c_void_p(d_field)) == 1
        assert GF.refusal_code(c.field_forward_geometric_batch_device, 0, np.zeros(8), [g], [6], d_field) == 1      # offset not a multiple of 4
        _set(c, case)
        assert GF.refusal_code(c.field_forward_piecewise_batch_device, case["dp"], case["Mx"], case["My"], [case["geom"]], [0], 0) == 1
        assert L.hg_field_forward_piecewise_batch_device(c._h, None, case["Mx"], case["My"], geoms, None, 1, C.c_void_p(d_field)) == 1
        assert L.hg_field_forward_piecewise(c._h, dpp, case["Mx"], case["My"], geoms[0], None) == 1
        assert GF.refusal_code(c.field_forward_piecewise_batch_device, case["dp"], case["Mx"], case["My"], [case["geom"]], [2], d_field) == 1
        assert c.last_forward_field_kernel() == 0 and c.last_forward_kernel() == 0
    finally:
        c.free(d_field); c.close()


def test_source_taller_than_65535_is_refused():
    img = np.zeros((F.SRC_MAX + 1, 16, 4), np.uint8)
    for tiles in (1, 0):
        c = _ctx(tiles)
        try:
            c.set_image(img)
            assert GF.refusal_code(c.field_forward_geometric, 0, np.float64([0, 1, 1, 0, 0, 0]), (0, 0, F.SRC_MAX + 1, 16)) == 1
        finally:
            c.close()


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_source_field_loops():
    """tests/js/field_forward_gpu.mjs: sourceField(format, {loop}) of js/Homography.mjs on the real addon -- a same-size piecewise and a
    same-size affine instance: the 'warp' field gathers warp().data, the 'inverse' field warp(null, false, true).data; refusals are strings."""
    res = GF.run_node_case("field_forward_gpu.mjs")
    assert set(res["report"]) == {"piecewise", "affine"}
    assert res["report"]["piecewise"]["forward_holes"] > 0


def test_host_forms_with_an_empty_window_write_nothing():
    """An empty window: both host forms return an empty field, launch nothing and leave the field tap alone."""
    case = PW["rotated_90"]
    for tiles in (1, 0):
        c = _ctx(tiles)
        try:
            _set(c, case)
            for g in ((0, 0, 0, 16), (3, -2, 16, 0)):
                assert c.field_forward_geometric(0, np.float64([1, 0, 0, 1, 0, 0]), g).shape == (max(g[3], 0), max(g[2], 0))
                assert c.field_forward_piecewise(case["dp"], case["Mx"], case["My"], g).shape == (max(g[3], 0), max(g[2], 0))
            assert _taps(c) == (0, 0) and c.last_forward_kernel() == 0
            _same(_pw_field(c, case, True), _model("rotated_90"), ("after empty windows", tiles))      # the context still works
        finally:
            c.close()


def test_source_of_2_to_the_31_pixels_is_refused():
    """An int32 cannot name the pixels of a 65536 x 32768 source: both forms refuse it before anything is launched (the source is only
    declared, over a small allocation that is never read: the refusal comes first)."""
    case = PW["rotated_90"]
    c = HG.Context(0)
    d_small = c.alloc(4096)
    try:
        c.set_image_device(d_small, 65536, 32768)
        c.piecewise_set_mesh(case["sp"], case["tris"], case["msx"], case["msy"])
        assert GF.refusal_code(c.field_forward_piecewise, case["dp"], case["Mx"], case["My"], case["geom"]) == 1
        assert GF.refusal_code(c.field_forward_geometric, 0, np.float64([1, 0, 0, 1, 0, 0]), (0, 0, 64, 16)) == 1
        assert c.last_forward_field_kernel() == 0
    finally:
        c.set_image(np.zeros((1, 1, 4), np.uint8))                    # drop the alias before the buffer goes away
        c.free(d_small); c.close()
