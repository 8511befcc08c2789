"""The forward piecewise tile kernels (k_fwd_pw_bins + k_fwd_pw_tiles, fwd_tiles 1) and scatter + gather (fwd_tiles 0) on the turned,
mirrored, sheared, sloped and nearly singular frames of tests/hgtest/fwd_turns.py (judged on the CPU by tests/test_forward_turns_cpu.py):
warps and source fields against the oracle, bit-exact, with the kernel that ran and the frames redone asserted in every case -- a named
case must run the tile kernels with nothing redone, a fuzz draw is redone exactly where the model of the bins kernel says so."""
import numpy as np
import pytest

from hgtest import fwd_edges as F
from hgtest import fwd_field as M
from hgtest import fwd_turns as T
from hgtest import hip
from hgtest import oracle as O

pytestmark = pytest.mark.gpu

HG = hip.load()
NAMED = T.named_cases()
FUZZ_SEED, FUZZ_DRAWS = 2026, 240          # (tests/test_forward_turns_cpu.py: what these draws reach)

_wants = {}


def _want(name):
    """(image, oracle's warp of it, model of the field) of a named case, computed once and handed out read-only."""
    if name not in _wants:
        case = NAMED[name]
        img = F.image(case)
        w = (img, F.piecewise_oracle(case, img), M.piecewise_case(case))
        for a in w: a.setflags(write=False)
        _wants[name] = w
    return _wants[name]


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        h, w = want.shape[:2]
        first = [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:6]]
        where = {"alias columns": int(((bad[:, 1] < F.WRAP) | (bad[:, 1] >= w - F.WRAP)).sum()),
                 "tile borders": int(((bad % F.TILE == 0) | (bad % F.TILE == F.TILE - 1)).any(1).sum()),
                 "got 0": int((~got[bad[:, 0], bad[:, 1]].any(-1)).sum())}
        raise AssertionError(f"{what}: {len(bad)} of {h * w} pixels differ, {where}; (row, col, got, want): {first}")


def _same_field(got, want, what):
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, want.shape, got.dtype)
    _same(got[..., None], want[..., None], what)


def _ctx(tiles):
    c = HG.Context(0)
    c.set_option("fwd_tiles", tiles)
    return c


def _frame(c, d_out, geom, off=0):
    return c.to_host(d_out, geom[2] * geom[3] * 4, off).reshape(geom[3], geom[2], 4)


def _field(c, d_field, geom, off=0):
    return c.to_host(d_field, geom[2] * geom[3] * 4, off).view(np.int32).reshape(geom[3], geom[2])


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


def _set(c, case, img):
    c.set_image(img)
    c.piecewise_set_mesh(case["sp"], case["tris"], case["msx"], case["msy"])          # (also re-arms the tile path and its first capacity)


def _warp_taps(c):
    return (c.last_forward_kernel(), c.redone_frames())


def _field_taps(c):
    return (c.last_forward_field_kernel(), c.redone_frames())


# ------------------------------------------------------------------------------------------------ T1 .. T3

@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", list(NAMED))
def test_named_warps(name, host):
    """Scatter + gather, then the tile kernels on a fresh context and mesh, twice: the oracle's bytes each time, kernel 2 with nothing
    redone -- no case passes by being handed to the scatter path."""
    case = NAMED[name]
    img, want, _ = _want(name)
    assert want.any()
    c = _ctx(0)
    try:
        _set(c, case, img)
        _same(_pw_run(c, case, host), want, (name, "scatter"))
        assert _warp_taps(c) == (1, 0)
    finally:
        c.close()
    c = _ctx(1)
    try:
        _set(c, case, img)
        first = _pw_run(c, case, host)
        _same(first, want, (name, "tiles"))
        assert _warp_taps(c) == (2, 0), (name, _warp_taps(c))
        again = _pw_run(c, case, host)
        assert _warp_taps(c) == (2, 0), (name, "second call", _warp_taps(c))
        assert np.array_equal(again, first), (name, "second call")
    finally:
        c.close()


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", list(NAMED))
def test_named_fields(name, host):
    """The source field of the same frames from k_fwd_pw_tiles' field form and from scatter + k_fwd_win_field: the model's field, and the
    source gathered through it is the warp."""
    case = NAMED[name]
    img, want, model = _want(name)
    assert (model >= 0).any()
    for tiles in (1, 0):
        c = _ctx(tiles)
        try:
            _set(c, case, img)
            got = _pw_field(c, case, host)
            _same_field(got, model, (name, tiles, "field"))
            assert _field_taps(c) == (2 if tiles else 1, 0), (name, tiles, _field_taps(c))
            assert c.last_forward_kernel() == 0                       # the warps' own tap: no forward warp ran on this context
            assert np.array_equal(M.gather(got, img), want), (name, tiles, "gathered field != warp")
        finally:
            c.close()


# ------------------------------------------------------------------------------------------------ T4

def test_batch_of_turned_frames():
    """Six frames of one mesh in one launch, each in its own window, three sources (frame f reads source f mod 3): one warp batch and one
    field batch, with the tile kernels forced (nothing redone) and off."""
    b = T.turns_batch()
    cases = T.batch_cases(b)
    W, H, box = b["W"], b["H"], b["box"]
    imgs = [O.lcg_image(W, H, s) for s in b["seeds"]]
    n_img = len(imgs)
    geoms = [g for _, g in b["frames"]]
    dps = np.concatenate([d for d, _ in b["frames"]])
    wants = [F.piecewise_oracle(k, imgs[f % n_img]) for f, k in enumerate(cases)]
    models = [M.piecewise_case(k) for k in cases]
    offs, total = HG.pack_offsets(geoms)
    stride = W * H * 4
    for tiles in (1, 0):
        code = 2 if tiles else 1
        c = _ctx(tiles)
        d_src, d_out, d_field = c.alloc(n_img * stride), c.alloc(total), c.alloc(total)
        try:
            for k in range(n_img): c.to_device(d_src, imgs[k], k * stride)
            c.set_images_device(d_src, W, H, n_img, stride)
            c.piecewise_set_mesh(b["sp"], b["tris"], box[0], box[1])
            c.warp_forward_piecewise_batch_device(dps, box[2], box[3], geoms, offs, d_out)
            c.sync()
            assert _warp_taps(c) == (code, 0), (tiles, _warp_taps(c))
            c.field_forward_piecewise_batch_device(dps, box[2], box[3], geoms, offs, d_field)
            assert _field_taps(c) == (code, 0), (tiles, _field_taps(c))
            for f, g in enumerate(geoms):
                assert wants[f].any()
                _same(_frame(c, d_out, g, offs[f]), wants[f], ("batch", tiles, f))
                got = _field(c, d_field, g, offs[f])
                _same_field(got, models[f], ("batch field", tiles, f))
                assert np.array_equal(M.gather(got, imgs[f % n_img]), wants[f]), ("batch", tiles, f, "gathered field != warp")
        finally:
            c.free(d_field); c.free(d_out); c.free(d_src); c.close()


# ------------------------------------------------------------------------------------------------ T5

def _worst_triangle(case, got, want):
    """The forward matrix that owns most of the differing pixels' reference winners (the one of smallest |det| when none has a winner)."""
    maps = F.piecewise_maps(case)
    _, win, _ = F.classify_piecewise(case, maps)
    bad = np.flatnonzero((got != want).any(-1).ravel())
    w = win[bad]
    ids = maps[0].ravel().astype(np.int64)[w[w >= 0]]
    t = int(np.bincount(ids).argmax()) if ids.size else int(np.abs(T.dets(maps[1])).argmin())
    return t, maps[1][t].astype(np.float64).tolist()


def test_fuzz_of_turned_frames():
    """Every draw on two contexts (tile kernels forced, and off) equals the oracle.  Every draw sets a new mesh, which re-arms the tile
    path: the first call always reports kernel 2, and redoes its frame exactly where the model of k_fwd_pw_bins flags the draw."""
    cases, _ = T.fuzz(FUZZ_SEED, FUZZ_DRAWS)
    assert len(cases) >= 220
    wrong, taps, flagged, unflagged = [], [], 0, 0
    ct, cs = _ctx(1), _ctx(0)
    try:
        for case in cases:
            img = F.image(case)
            maps = F.piecewise_maps(case)
            want = O.warp_forward_piecewise(maps[0].ravel(), maps[1], img, case["msx"], case["msy"], case["Mx"], case["My"], *case["geom"])
            flag = T.bins_model(case, maps)[0]
            flagged += flag is not None
            unflagged += flag is None
            for c, code, redo in ((ct, 2, int(flag is not None)), (cs, 1, 0)):
                _set(c, case, img)
                before = c.redone_frames()
                got = _pw_run(c, case, True)
                seen = (c.last_forward_kernel(), c.redone_frames() - before)
                if seen != (code, redo):
                    taps.append((case["name"], "(kernel, redone) is", seen, "the model says", (code, redo), flag))
                if not np.array_equal(got, want):
                    t, m = _worst_triangle(case, got, want)
                    wrong.append((case["name"], code, "angle", case["ang"], "mode", case["mode"], "triangle", t, m, "window", case["geom"],
                                  "source", (case["W"], case["H"]), int((got != want).any(-1).sum()), "pixels differ"))
        print(len(cases), "draws:", unflagged, "on the tile kernels unflagged,", flagged, "redone")
        assert not wrong, (len(wrong), wrong[:4])
        assert not taps, (len(taps), taps[:4])
        assert unflagged >= 200 and flagged >= 1
    finally:
        ct.close(); cs.close()
