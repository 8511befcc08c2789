"""The forward tile kernels at the edges of their candidate bounds and at their admission limits (tests/hgtest/fwd_edges.py; the builders
are checked on the CPU by tests/test_forward_edges_cpu.py): k_fwd_tiles and k_fwd_pw_bins + k_fwd_pw_tiles (fwd_tiles 1) and scatter +
gather (fwd_tiles 0) against the oracle, bit-exact, with the kernel that ran (hg_last_forward_kernel) and the frames redone
(hg_redone_frames) asserted in every case, so that no case can pass on the other path."""
import numpy as np
import pytest

from hgtest import fwd_edges as F
from hgtest import hip
from hgtest import oracle as O

pytestmark = pytest.mark.gpu

HG = hip.load()
GEO = F.geometric_cases()
PW = F.piecewise_cases()
FUZZ_SEED, FUZZ_DRAWS = 2025, 420          # (tests/test_forward_edges_cpu.py: at least 300 of these draws are admitted)


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        h, w = want.shape[:2]
        first = [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:6]]
        where = {"alias columns": int(((bad[:, 1] < F.WRAP) | (bad[:, 1] >= w - F.WRAP)).sum()),
                 "tile borders": int(((bad % F.TILE == 0) | (bad % F.TILE == F.TILE - 1)).any(1).sum()),
                 "got 0": int((~got[bad[:, 0], bad[:, 1]].any(-1)).sum())}
        raise AssertionError(f"{what}: {len(bad)} of {h * w} pixels differ, {where}; (row, col, got, want): {first}")


def _ctx(tiles):
    c = HG.Context(0)
    c.set_option("fwd_tiles", tiles)
    return c


def _frame(c, d_out, geom, off=0):
    return c.to_host(d_out, geom[2] * geom[3] * 4, off).reshape(geom[3], geom[2], 4)


# ------------------------------------------------------------------------------------------------ geometric

@pytest.mark.parametrize("name", list(GEO))
def test_geometric_edges(name):
    """Every G1 .. G7 case: the host entry point (one frame: parameters in the kernel arguments) and the device batch entry point (one
    frame, and the frame twice: uploaded parameters), with the tile kernel forced and switched off."""
    case = GEO[name]
    kind, m, geom = case["kind"], case["m"], case["geom"]
    img = F.image(case)
    want = O.warp_forward_geometric(kind, m, img, *geom)
    assert want.any()
    m8 = np.zeros(8)
    m8[:m.size] = m
    nbytes = geom[2] * geom[3] * 4
    for tiles in (1, 0):
        expect = 2 if tiles and case["admit"] else 1
        c = _ctx(tiles)
        d_out = c.alloc(2 * nbytes)
        try:
            c.set_image(img)
            _same(c.warp_forward_geometric(kind, m, geom), want, (name, tiles, "host"))
            assert c.last_forward_kernel() == expect, (name, tiles, c.last_forward_kernel())
            c.warp_forward_geometric_batch_device(kind, m8, [geom], [0], d_out)
            c.sync()
            assert c.last_forward_kernel() == expect, (name, tiles, c.last_forward_kernel())
            _same(_frame(c, d_out, geom), want, (name, tiles, "device"))
            c.warp_forward_geometric_batch_device(kind, np.concatenate([m8, m8]), [geom, geom], [nbytes, 0], d_out)
            c.sync()
            assert c.last_forward_kernel() == expect, (name, tiles, c.last_forward_kernel())
            for f in (0, 1):
                _same(_frame(c, d_out, geom, f * nbytes), want, (name, tiles, "batch", f))
        finally:
            c.free(d_out); c.close()


def test_source_taller_than_65535_is_refused():
    img = np.zeros((F.SRC_MAX + 1, 16, 4), np.uint8)
    for tiles in (1, 0):
        c = _ctx(tiles)
        try:
            c.set_image(img)
            with pytest.raises(HG.HgError) as e:
                c.warp_forward_geometric(0, np.float64([0, 1, 1, 0, 0, 0]), (0, 0, F.SRC_MAX + 1, 16))
            assert e.value.code == 1                                  # HG_ERR_INVALID
        finally:
            c.close()


def test_geometric_batch_of_mixed_windows():
    """G8: five frames in one launch, an empty one in the middle, two source images (frame f reads image f mod 2)."""
    b = F.batch()
    W, H, kind = b["W"], b["H"], b["kind"]
    imgs = [O.lcg_image(W, H, s) for s in b["seeds"]]
    mats = np.concatenate([m for m, _ in b["frames"]])
    geoms = [g for _, g in b["frames"]]
    for f, (m, g) in enumerate(b["frames"]):
        assert g[2] == 0 or HG.forward_tiles_admissible(kind, m, W, H, g) == 2, f
    offs, total = HG.pack_offsets(geoms)
    stride = W * H * 4
    for tiles in (1, 0):
        c = _ctx(tiles)
        d_src, d_out = c.alloc(2 * stride), c.alloc(total)
        try:
            for k in (0, 1): c.to_device(d_src, imgs[k], k * stride)
            c.set_images_device(d_src, W, H, 2, stride)
            c.warp_forward_geometric_batch_device(kind, mats, geoms, offs, d_out)
            c.sync()
            assert c.last_forward_kernel() == (2 if tiles else 1)
            for f, (m, g) in enumerate(b["frames"]):
                if g[2] > 0:
                    _same(_frame(c, d_out, g, offs[f]), O.warp_forward_geometric(kind, m[:6], imgs[f % 2], *g), ("batch", tiles, f))
        finally:
            c.free(d_out); c.free(d_src); c.close()


def test_geometric_fuzz_at_the_limits():
    """G9: every admitted draw runs k_fwd_tiles under fwd_tiles 1 (that option leaves host admission as the only gate) and equals the
    oracle, as does scatter + gather."""
    cases, refused, _ = F.fuzz(FUZZ_SEED, FUZZ_DRAWS, HG.forward_tiles_admissible)
    assert len(cases) >= 300
    wrong = []
    ct, cs = _ctx(1), _ctx(0)
    try:
        for case in cases:
            kind, m, geom = case["kind"], case["m"], case["geom"]
            img = F.image(case)
            want = O.warp_forward_geometric(kind, m, img, *geom)
            for c, code in ((ct, 2), (cs, 1)):
                c.set_image(img)
                got = c.warp_forward_geometric(kind, m, geom)
                assert c.last_forward_kernel() == code, (case["name"], code, c.last_forward_kernel())
                if not np.array_equal(got, want):
                    wrong.append((case["name"], code, kind, m.tolist(), case["W"], case["H"], geom, int((got != want).any(-1).sum())))
        assert not wrong, (len(wrong), wrong[:4])
    finally:
        ct.close(); cs.close()


# ------------------------------------------------------------------------------------------------ piecewise

def _pw_run(c, case, host):
    """One forward piecewise frame through the host entry point, or through the device batch entry point and a sync."""
    if host:
        return c.warp_forward_piecewise(case["dp"], case["Mx"], case["My"], case["geom"])
    g = case["geom"]
    d_out = c.alloc(g[2] * g[3] * 4)
    try:
        c.warp_forward_piecewise_batch_device(case["dp"], case["Mx"], case["My"], [g], [0], d_out)
        c.sync()
        return _frame(c, d_out, g)
    finally:
        c.free(d_out)


def _set(c, case, img):
    c.set_image(img)
    c.piecewise_set_mesh(case["sp"], case["tris"], case["msx"], case["msy"])          # (also re-arms the tile path and its first capacity)


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", [n for n in PW if "entries" not in PW[n]])
def test_piecewise_edges(name, host):
    """P1 .. P3, P6 .. P8 and the meshes of P4 that fit the first capacity: the first call on a fresh mesh reports the kernel and redoes
    the frames the case claims; a frame the bins kernel could not bound (k = +-3, an entry above 1e6, NaN) switches the tile path off
    for the mesh: the next call runs scatter + gather and redoes nothing."""
    case = PW[name]
    img = F.image(case)
    want = F.piecewise_oracle(case, img)
    assert want.any()
    c = _ctx(0)
    try:
        _set(c, case, img)
        _same(_pw_run(c, case, host), want, (name, "scatter"))
        assert (c.last_forward_kernel(), c.redone_frames()) == (1, 0)
    finally:
        c.close()
    c = _ctx(1)
    try:
        _set(c, case, img)
        _same(_pw_run(c, case, host), want, (name, "tiles"))
        assert (c.last_forward_kernel(), c.redone_frames()) == (case["kernel"], case["flagged"]), (name, c.last_forward_kernel(), c.redone_frames())
        _same(_pw_run(c, case, host), want, (name, "tiles, second call"))
        again = 1 if case["flagged"] else case["kernel"]
        assert (c.last_forward_kernel(), c.redone_frames()) == (again, case["flagged"]), (name, c.last_forward_kernel(), c.redone_frames())
        if case["flagged"]:                                           # another mesh re-arms the tile path (the same mesh sent again does not)
            other = PW["rotated_90"]
            oimg = F.image(other)
            _set(c, other, oimg)
            _same(_pw_run(c, other, host), F.piecewise_oracle(other, oimg), (name, "re-armed"))
            assert (c.last_forward_kernel(), c.redone_frames()) == (2, case["flagged"])
    finally:
        c.close()


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", [n for n in PW if "entries" in PW[n]])
def test_piecewise_tile_capacity(name, host):
    """P5 and the 8 x 8 mesh of P4: a tile with more entries than the capacity flags its frame (redone through scatter + gather) and
    the capacity doubles at the sync, 64 -> 128 -> 256; a tile past 256 entries is flagged once at each capacity, then the tile path is
    switched off for the mesh (kernel 1, nothing redone) until hg_piecewise_set_mesh re-arms it."""
    case = PW[name]
    n = case["entries"]
    flags = 0 if n <= F.PW_CAP0 else 1 if n <= 2 * F.PW_CAP0 else 2 if n <= F.PW_CAP_MAX else 3
    img = F.image(case)
    want = F.piecewise_oracle(case, img)
    c = _ctx(1)
    try:
        _set(c, case, img)
        for call in range(flags + 2):
            _same(_pw_run(c, case, host), want, (name, "call", call))
            off = n > F.PW_CAP_MAX and call >= flags
            assert (c.last_forward_kernel(), c.redone_frames()) == (1 if off else 2, min(call + 1, flags)), (name, call, c.last_forward_kernel(), c.redone_frames())
        small = F.dense(F.DENSE["65-128"] // 2)                       # 48 entries: fits the first capacity
        assert small["entries"] <= F.PW_CAP0
        simg = F.image(small)
        _set(c, small, simg)
        _same(_pw_run(c, small, host), F.piecewise_oracle(small, simg), (name, "re-armed"))
        assert (c.last_forward_kernel(), c.redone_frames()) == (2, flags)
    finally:
        c.close()


def test_piecewise_batches_of_mixed_windows():
    """P9: five frames (an empty one in the middle) with one source per frame, and two batches queued without a sync between them."""
    b = F.piecewise_batch()
    W, H, box = b["W"], b["H"], b["box"]
    imgs = [O.lcg_image(W, H, s) for s in b["seeds"]]
    n = len(b["frames"])
    geoms = [g for _, g in b["frames"]]
    offs, total = HG.pack_offsets(geoms)
    moved = [(d.reshape(-1, 2) + np.float32([1.5, -0.5])).ravel() for d, _ in b["frames"]]      # the second batch: the same windows, the points moved
    sets = [[d for d, _ in b["frames"]], moved]
    stride = W * H * 4
    for tiles in (1, 0):
        c = _ctx(tiles)
        d_src, d_a, d_b = c.alloc(n * stride), c.alloc(total), c.alloc(total)
        try:
            for k in range(n): c.to_device(d_src, imgs[k], k * stride)
            c.set_images_device(d_src, W, H, n, stride)
            c.piecewise_set_mesh(b["sp"], b["tris"], box[0], box[1])
            for d_out, dps in ((d_a, sets[0]), (d_b, sets[1])):
                c.warp_forward_piecewise_batch_device(np.concatenate(dps), box[2], box[3], geoms, offs, d_out)
                assert c.last_forward_kernel() == (2 if tiles else 1)
            c.sync()
            assert c.redone_frames() == 0
            for d_out, dps in ((d_a, sets[0]), (d_b, sets[1])):
                for f, g in enumerate(geoms):
                    if g[2] <= 0: continue
                    case = {"sp": b["sp"], "tris": b["tris"], "dp": dps[f], "msx": box[0], "msy": box[1], "Mx": box[2], "My": box[3], "geom": g}
                    _same(_frame(c, d_out, g, offs[f]), F.piecewise_oracle(case, imgs[f]), ("batch", tiles, dps is moved, f))
        finally:
            c.free(d_b); c.free(d_a); c.free(d_src); c.close()
