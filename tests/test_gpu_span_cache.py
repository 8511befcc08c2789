"""The span cache of k_pw_rows<SELF> (csrc/hg_span_cache.h): a frame set that stays on the context is warped from the per-row span slots an
earlier warp of it wrote to device memory.  Results never depend on it: every comparison here is bit-exact against the oracle, every warp that
ran from the cache is also compared with the bytes of the set's first warp, and every case asserts the statistics it relies on (a case that
never reached "use" would prove nothing).  Shapes are tiny; the path is forced through the options (self_spans, min_row_groups, span_cache = 1:
build on the first warp, use from the second) except in the default-policy and fresh-points cases."""
import functools

import numpy as np
import pytest

from hgtest import edges as E
from hgtest import folds as FO
from hgtest import golden as G
from hgtest import hip
from hgtest import oracle as O
from hgtest import workloads as WL

pytestmark = pytest.mark.gpu

HG = hip.load()
SELF_ROWS = {"self_spans": 1, "patch": 0, "tile": 0, "compact": 0, "min_row_groups": 0}
SW, SH = 260, 12                                      # source; the 4 x 3-cell grid has cells of 65 x 4 source pixels
WIN = (520, 22)                                       # 520 is no multiple of 256 (ragged last window); 22 rows: the last group has 2 rows


@functools.lru_cache(maxsize=None)
def _image(w=SW, h=SH, seed=5):
    img = G.lcg_image(w, h, seed).copy()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _mesh():
    sp, tris = WL.grid_points(SW, SH, 4, 3), WL.grid_triangles(4, 3)
    assert tris.size // 3 == 24
    return sp, tris, WL.src_min(sp)


def _frames(long_form, shift=0):
    """Three frames of the mesh at twice its size: frame 1 is empty (obj_w = 0), frame 2 sits at a window offset of its own and has one interior
    vertex pulled 6 pixels aside.  long_form: an interior vertex of frames 0 and 2 moved by one f32 unit in the last place (a shear some 2^20
    below the scale: the :1383 sums are no longer exact and the frame's records take the long form)."""
    sp = _mesh()[0].reshape(-1, 2).astype(np.float64)
    frames = []
    for f in range(3):
        d = 2.0 * sp + [3 * f + shift, f]
        if f == 2:
            d[7] += [6, 0]
        d = d.astype(np.float32).ravel()
        frames.append(E.nudge(d, 6, 1) if long_form and f != 1 else d)
    geoms = [(shift, 0, WIN[0], WIN[1]), (0, 0, 0, WIN[1]), (4 + shift, 1, WIN[0], WIN[1])]
    return frames, geoms


def _one_fma(sp, tris, dp, geom):
    fwd = HG.solve_affine_triangles(sp, dp, tris).reshape(-1, 6)
    return all(HG.affine_one_fma_form(HG.invert_affine(m), geom) for m in fwd)


def _want(sp, tris, ms, frames, geoms, img):
    return [O.warp_inverse_piecewise(sp, frames[f], tris, img, ms[0], ms[1], *g) if g[2] > 0 and g[3] > 0 else None for f, g in enumerate(geoms)]


@functools.lru_cache(maxsize=None)
def _base_want(long_form):
    sp, tris, ms = _mesh()
    frames, geoms = _frames(long_form)
    return _want(sp, tris, ms, frames, geoms, _image())


def _ctx(options=(), eager=True):
    c = HG.Context(0)
    for k, v in dict(SELF_ROWS, **dict(options)).items():
        c.set_option(k, v)
    if eager:
        c.set_option("span_cache", 1)
    return c


def _download(c, d_out, geoms, offs):
    return [c.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4) if g[2] > 0 and g[3] > 0 else None for f, g in enumerate(geoms)]


def _same(got, want, what):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        if b is None:
            assert a is None
            continue
        assert a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes(), (what, "frame", f)


def _warps(c, n, geoms, offs, total, sync=True):
    """n warps of the staged set into n buffers of their own; returns the frames of every warp."""
    bufs = [c.alloc(total) for _ in range(n)]
    try:
        for d in bufs:
            c.warp_inverse_piecewise_frames_device(d)
            if sync:
                c.sync()
        c.sync()
        return [_download(c, d, geoms, offs) for d in bufs]
    finally:
        for d in bufs:
            c.free(d)


# ------------------------------------------------------------------------------------------------ the base shape
@pytest.mark.parametrize("sync", [True, False], ids=["synced", "queued"])
@pytest.mark.parametrize("long_form", [False, True], ids=["one_fma", "long_form"])
@pytest.mark.parametrize("safe", [0, 1], ids=["unsafe", "safe"])
@pytest.mark.parametrize("hi_bounds", [0, 1], ids=["fp64_bounds", "hi_bounds"])
def test_base_shape_build_then_use(hi_bounds, safe, long_form, sync):
    """One warp as ever (span_cache = 0), then the build and two warps from the cache, into four buffers: all four equal the oracle, and the
    cached ones the first."""
    sp, tris, ms = _mesh()
    frames, geoms = _frames(long_form)
    assert _one_fma(sp, tris, frames[0], geoms[0]) != long_form and _one_fma(sp, tris, frames[2], geoms[2]) != long_form
    offs, total = HG.pack_offsets(geoms)
    with _ctx({"hi_bounds": hi_bounds, "safe_spans": safe}, eager=False) as c:
        c.set_option("span_cache", 0)
        c.set_image(_image())
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        first = _warps(c, 1, geoms, offs, total)[0]
        assert c.span_cache_stats()["state"] == "off" and c.span_cache_stats()["builds"] == 0
        variant = c.last_piecewise_variant()
        assert variant == (104011 if hi_bounds else 101001) and c.last_piecewise_self() == 1
        c.set_option("span_cache", 1)
        later = _warps(c, 3, geoms, offs, total, sync)
        st = c.span_cache_stats()
        print(st)
        assert (st["builds"], st["use_calls"], st["groups_not_cached"], st["state"]) == (1, 2, 0, "use"), st
        assert st["groups_valid"] == 2 * ((WIN[1] + 3) // 4) and st["bytes"] > 0, st
        assert c.last_piecewise_variant() == variant and c.last_piecewise_self() == 1 and c.redone_frames() == 0
        want = _base_want(long_form)
        _same(first, want, "first warp")
        for k, got in enumerate(later):
            _same(got, want, ("warp", k + 2))
            _same(got, first, ("warp", k + 2, "against the first"))


# ------------------------------------------------------------------------------------------------ default policy
@functools.lru_cache(maxsize=None)
def _policy_set():
    """16 frames of 320 x 288 on a 6 x 6 grid: 1152 four-row groups, the policy's own threshold for the self-span form."""
    W, H, F = 160, 144, 16
    sp, tris = WL.grid_points(W, H, 6, 6), WL.grid_triangles(6, 6)
    p = sp.reshape(-1, 2).astype(np.float64)
    inner = ((p[:, 0] > 0) & (p[:, 0] < W) & (p[:, 1] > 0) & (p[:, 1] < H))[:, None]
    i = np.arange(p.shape[0])
    frames = [(2.0 * p + inner * np.stack([np.sin(1.0 + i + f), np.cos(2.0 + 3 * i - f)], 1) * 5.0).astype(np.float32).ravel() for f in range(F)]
    geoms = [(0, 0, 320, 288)] * F
    img = G.lcg_image(W, H, 9)
    ms = WL.src_min(sp)
    want = _want(sp, tris, ms, frames, geoms, img)
    return sp, tris, ms, frames, geoms, img, want


def test_default_policy_builds_on_the_second_warp():
    sp, tris, ms, frames, geoms, img, want = _policy_set()
    offs, total = HG.pack_offsets(geoms)
    with HG.Context(0) as c:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        d_out = c.alloc(total)
        try:
            variants, states, first = [], [], None
            for k in range(5):
                c.warp_inverse_piecewise_frames_device(d_out)
                variants.append(c.last_piecewise_variant())
                states.append(c.span_cache_stats()["state"])
                got = _download(c, d_out, geoms, offs)
                _same(got, want, ("warp", k))
                first = got if first is None else first
                _same(got, first, ("warp", k, "against the first"))
        finally:
            c.free(d_out)
        st = c.span_cache_stats()
        print(st, variants)
        assert states == ["off", "build", "use", "use", "use"], states
        assert (st["builds"], st["use_calls"], st["groups_not_cached"]) == (1, 3, 0) and st["groups_valid"] == 16 * 72, st
        assert len(set(variants)) == 1 and c.last_piecewise_self() == 1 and c.last_piecewise_kernel() == 1, variants


# ------------------------------------------------------------------------------------------------ invalidation
def test_every_change_of_an_input_rebuilds():
    """After "use" is reached: a change, two eager warps (build, use) against the oracle of the changed state, and the build counter must have
    moved -- a warp from the old records would have the old bytes."""
    sp, tris, ms = _mesh()
    frames, geoms = _frames(False)
    state = {"sp": sp, "tris": tris, "ms": ms, "frames": frames, "geoms": geoms, "img": _image(), "src": None, "mins": None}

    def upload(c):
        s = state
        offs, _ = HG.pack_offsets(s["geoms"])
        if s["src"] is None:
            c.piecewise_set_frames(np.concatenate(s["frames"]), s["geoms"], offs)
        else:
            c.piecewise_set_frames_src(np.concatenate(s["src"]), np.int32(s["mins"]).ravel(), np.concatenate(s["frames"]), s["geoms"], offs)

    def want():
        s = state
        if s["src"] is None:
            return _want(s["sp"], s["tris"], s["ms"], s["frames"], s["geoms"], s["img"])
        return [O.warp_inverse_piecewise(s["src"][f], s["frames"][f], s["tris"], s["img"], s["mins"][f][0], s["mins"][f][1], *g)
                if g[2] > 0 and g[3] > 0 else None for f, g in enumerate(s["geoms"])]

    def new_points(c):
        state["frames"] = [d if f == 1 else (d.reshape(-1, 2) + np.float32([[0, 0]] * 8 + [[5, 0]] + [[0, 0]] * 11)).ravel() for f, d in enumerate(state["frames"])]
        upload(c)

    def other_windows(c):
        state["geoms"] = [(g[0], g[1], 500 if g[2] else 0, 20) for g in state["geoms"]]
        upload(c)

    def moved_minima(c):
        state["src"] = [state["sp"]] * 3
        state["mins"] = [(state["ms"][0] + 1 + f, state["ms"][1] + (f & 1)) for f in range(3)]
        upload(c)

    def new_mesh(c):
        p = state["sp"].reshape(-1, 2).copy()
        p[6] += np.float32([4, 0])
        state["sp"], state["src"], state["mins"] = p.ravel(), None, None
        state["ms"] = WL.src_min(state["sp"])
        c.piecewise_set_mesh(state["sp"], state["tris"], *state["ms"])
        upload(c)

    def other_source(c):
        state["img"] = _image(SW + 4, SH + 1, 6)
        c.set_image(state["img"])

    flips = {"safe_spans": 1, "hi_bounds": 1}

    def flip(key):
        def go(c):
            flips[key] ^= 1
            c.set_option(key, flips[key])
        return go

    def sampling_and_back(c):
        c.set_sampling(HG.SAMPLE_BILINEAR)
        c.set_sampling(HG.SAMPLE_NEAREST)

    changes = [("new destination points", new_points), ("other windows", other_windows), ("moved source minima", moved_minima),
               ("another mesh", new_mesh), ("a source of other dimensions", other_source), ("safe_spans flipped", flip("safe_spans")),
               ("hi_bounds flipped", flip("hi_bounds")), ("bilinear and back", sampling_and_back)]
    with _ctx({"safe_spans": 1, "hi_bounds": 1}) as c:
        c.set_image(state["img"])
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        upload(c)
        offs, total = HG.pack_offsets(state["geoms"])
        for got in _warps(c, 2, state["geoms"], offs, total):
            _same(got, _base_want(False), "before any change")
        st = c.span_cache_stats()
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 1, "use"), st
        for name, change in changes:
            before = c.span_cache_stats()
            change(c)
            offs, total = HG.pack_offsets(state["geoms"])
            w = want()
            a, b = _warps(c, 2, state["geoms"], offs, total)
            _same(a, w, (name, "build"))
            _same(b, w, (name, "use"))
            st = c.span_cache_stats()
            print(name, st)
            assert st["builds"] == before["builds"] + 1 and st["use_calls"] == before["use_calls"] + 1 and st["state"] == "use", (name, before, st)
            assert st["groups_not_cached"] == 0 and st["groups_valid"] > 0, (name, st)
            assert c.last_piecewise_self() == 1 and c.redone_frames() == 0, name


def test_new_content_and_new_pointer_in_the_same_dimensions_keep_the_cache():
    sp, tris, ms = _mesh()
    frames, geoms = _frames(True)
    offs, total = HG.pack_offsets(geoms)
    with _ctx() as c:
        c.set_image(_image())
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        for got in _warps(c, 2, geoms, offs, total):
            _same(got, _base_want(True), "first content")
        other = _image(SW, SH, 77)
        c.set_image(other)                                          # new content, the context's own copy
        _same(_warps(c, 1, geoms, offs, total)[0], _want(sp, tris, ms, frames, geoms, other), "new content")
        third = _image(SW, SH, 78)
        d_img = c.alloc(third.size)
        try:
            c.to_device(d_img, third)
            c.set_image_device(d_img, SW, SH)                       # another pointer
            _same(_warps(c, 1, geoms, offs, total)[0], _want(sp, tris, ms, frames, geoms, third), "new pointer")
            st = c.span_cache_stats()
            assert (st["builds"], st["use_calls"], st["state"], st["groups_not_cached"]) == (1, 3, "use", 0), st
        finally:
            c.set_image(_image())
            c.free(d_img)


# ------------------------------------------------------------------------------------------------ budget
def test_a_budget_that_holds_part_of_the_groups():
    """span_cache_mb = -4: a budget of 4 KB that the host's estimate does not veto.  Some groups find room, the others evaluate their spans
    as ever; the bytes are the same."""
    sp, tris, ms = _mesh()
    frames, geoms = _frames(True)
    offs, total = HG.pack_offsets(geoms)
    with _ctx() as c:
        c.set_option("span_cache_mb", -4)
        c.set_image(_image())
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        for k, got in enumerate(_warps(c, 3, geoms, offs, total)):
            _same(got, _base_want(True), ("warp", k))
        st = c.span_cache_stats()
        print(st)
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 2, "use"), st
        assert st["groups_valid"] > 0 and st["groups_not_cached"] > 0 and st["groups_valid"] + st["groups_not_cached"] == 12, st
        assert st["bytes"] <= 4096 + 16 * (1 + 3 * 6), st
        # ... and a budget the estimate does veto: no build at all
        c.set_option("span_cache_mb", 0)
        _same(_warps(c, 2, geoms, offs, total)[1], _base_want(True), "no budget")
        st = c.span_cache_stats()
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 2, "off"), st


# ------------------------------------------------------------------------------------------------ flagged frames inside a cached set
@functools.lru_cache(maxsize=None)
def _flagged_set():
    """The mesh of hgtest.folds' deep stacks at depth 20 (400 triangles) in three frames: the blocks spread over a grid of 5 x 4 (20 spans a
    row), the same with a NaN vertex (k_tri_setup flags the frame), and the blocks stacked on one another as in folds' deep20: 80 spans in
    every row, which the 63 slots of a row block do not hold (the prologue flags the frame).  A first set of three spread frames has the
    same extents: the layout estimate of that set is kept for this one, which is how a packed plan meets rows it cannot hold."""
    blocks = FO.deep_blocks(20)
    spread = [b[:6] + ((2 + 400 * (k % 5), 2 + 44 * (k // 5)),) for k, b in enumerate(blocks)]
    sp, tris, stacked = E.tie_mesh(blocks)
    sp2, tris2, flat = E.tie_mesh(spread)
    assert np.array_equal(sp, sp2) and np.array_equal(tris, tris2)
    geom = WL.piecewise_geom(flat)
    nan = flat.copy()
    nan[2 * 7] = np.nan
    img = G.lcg_image(FO.W, FO.H, 11)
    ms = WL.src_min(sp)
    frames = [flat, nan, stacked]
    want = [O.warp_inverse_piecewise(sp, d, tris, img, ms[0], ms[1], *geom) for d in frames]
    return sp, tris, ms, frames, [geom] * 3, img, want


def test_flagged_frames_flag_again_on_every_cached_call():
    sp, tris, ms, frames, geoms, img, want = _flagged_set()
    offs, total = HG.pack_offsets(geoms)
    with _ctx() as c:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        c.piecewise_set_frames(np.concatenate([frames[0]] * 3), geoms, offs)        # the estimate: 20 spans a row, packed groups
        _same(_warps(c, 1, geoms, offs, total)[0], [want[0]] * 3, "the spread set")
        assert c.redone_frames() == 0 and c.last_piecewise_variant() in (104011, 101001)
        builds = c.span_cache_stats()["builds"]
        c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        got = _warps(c, 4, geoms, offs, total, sync=False)                          # queued: one plan for all four
        st = c.span_cache_stats()
        print(st, c.redone_frames(), c.last_piecewise_flag())
        for k, g in enumerate(got):
            _same(g, want, ("warp", k))
        assert (st["builds"], st["use_calls"], st["state"]) == (builds + 1, 3, "use"), st
        assert c.redone_frames() == 4 * 2, c.redone_frames()                        # the NaN frame and the stacked frame, on every call


# ------------------------------------------------------------------------------------------------ fresh points every step
def test_a_loop_over_fresh_point_sets_never_builds():
    sp, tris, ms = _mesh()
    sets = [_frames(k % 2 == 1, shift=k) for k in range(8)]
    with _ctx(eager=False) as c:
        c.set_image(_image())
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        args = [c.frame_set_args(np.concatenate(fr), gm, HG.pack_offsets(gm)[0]) for fr, gm in sets]
        total = max(HG.pack_offsets(gm)[1] for _, gm in sets)
        bufs = [c.alloc(total) for _ in range(8)]
        try:
            for k in range(24):
                c.piecewise_set_frames_prepared(args[k % 8])
                c.warp_inverse_piecewise_frames_device(bufs[k % 8])
            c.sync()
            st = c.span_cache_stats()
            assert (st["builds"], st["use_calls"], st["state"]) == (0, 0, "off"), st
            assert c.last_piecewise_self() == 1
            for k, (fr, gm) in enumerate(sets):
                _same(_download(c, bufs[k], gm, HG.pack_offsets(gm)[0]), _want(sp, tris, ms, fr, gm, _image()), ("set", k))
        finally:
            for d in bufs:
                c.free(d)


# ------------------------------------------------------------------------------------------------ other calls in between
def test_field_point_and_forward_calls_between_cached_warps():
    """A field call and a point-list call on the same set, and a forward geometric warp, between warps from the cache: the next warp still
    runs from it and its bytes are right.  (A forward PIECEWISE warp uploads a frame set of its own: a new set like any other.)"""
    sp, tris, ms = _mesh()
    frames, geoms = _frames(False)
    offs, total = HG.pack_offsets(geoms)
    foffs, ftotal = HG.pack_field_offsets(geoms, HG.FIELD_INDEX)
    pts = np.float32([[10.5, 3.25], [300, 11], [519, 21], [-4, 2]])
    with _ctx() as c:
        c.set_image(_image())
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        for got in _warps(c, 2, geoms, offs, total):
            _same(got, _base_want(False), "before")
        d_field, d_pts, d_res = c.alloc(max(ftotal, 16)), c.alloc(pts.nbytes), c.alloc(3 * pts.nbytes)
        try:
            c.to_device(d_pts, pts)
            c.field_inverse_piecewise_frames_device(HG.FIELD_INDEX, d_field, foffs)
            _same(_warps(c, 1, geoms, offs, total)[0], _base_want(False), "after the field call")
            c.points_to_source_piecewise_frames_device(d_pts, len(pts), 1, d_res)
            _same(_warps(c, 1, geoms, offs, total)[0], _base_want(False), "after the point list")
            fwd = c.warp_forward_geometric(HG.HG_AFFINE, np.float64([2, 0, 0, 2, 0, 0]), (0, 0, 64, 24))
            assert fwd.shape[:2] == (24, 64)
            _same(_warps(c, 1, geoms, offs, total)[0], _base_want(False), "after the forward warp")
        finally:
            c.free(d_field); c.free(d_pts); c.free(d_res)
        st = c.span_cache_stats()
        assert (st["builds"], st["use_calls"], st["state"], st["groups_not_cached"]) == (1, 4, "use", 0), st
