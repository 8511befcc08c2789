"""The run form of the span cache (csrc/hg_span_runs.h): the build resolves a row's overlapping spans into disjoint sorted runs with their
winners, and later warps of the set find a pixel's record by counting run starts.  Results never depend on it: every warp here is compared bit
for bit with the oracle, every warp that ran from the cache also with the set's first warp, and every case asserts the statistics it relies on.
Shapes are tiny (a 300 x 14 source, windows of 520 x 22: a ragged last window, a short last group); the path is forced through the options
(self_spans, min_row_groups, span_cache = 1: build on the first warp, use from the second).

One mesh serves every frame: BASE (4 x 3 cells, ids 0 .. 23), INNER (2 x 1 cells, ids 24 .. 27) and 40 thin triangles of their own points
(ids 28 .. 67).  A frame places each part in its window or parks it a thousand rows below.  (The folded meshes of hgtest.folds are built the
same way from edges.tie_mesh, but from 16-pixel cells: more than 56 triangles reach one of their rows, the planner gives such sets one-row groups,
and the span cache takes 4-row groups only -- they never reach this code.)"""
import functools

import numpy as np
import pytest

from hgtest import edges as E
from hgtest import golden as G
from hgtest import hip
from hgtest import oracle as O
from hgtest import workloads as WL

pytestmark = pytest.mark.gpu

HG = hip.load()
SELF_ROWS = {"self_spans": 1, "patch": 0, "tile": 0, "compact": 0, "min_row_groups": 0}
SW, SH = 300, 14
WIN = (0, 0, 520, 22)
GROUPS = (WIN[3] + 3) // 4
BASE = (0.0, 0.0, 4, 3, 64, 4)                        # 256 x 12 source pixels -> 512 x 24 output pixels
INNER = (100.0, 2.0, 2, 1, 32, 4)                     # 64 x 4 -> 128 x 8
THIN = 40                                             # tests/test_span_runs_cpu.py checks this row shape on the host: 41 spans, 81 runs
PARK = 1000
RUN_LIMIT = 64


@functools.lru_cache(maxsize=None)
def _image():
    img = G.lcg_image(SW, SH, 9).copy()
    img.setflags(write=False)
    return img


def _with_triangle(mesh, src3, dst3):
    """The mesh with one more triangle on three points of its own, listed last."""
    sp, tris, dp = mesh
    n = sp.size // 2
    return np.concatenate([sp, np.float32(src3)]), np.concatenate([tris, np.uint32([n, n + 1, n + 2])]), np.concatenate([dp, np.float32(dst3)])


@functools.lru_cache(maxsize=None)
def _mesh(reverse=False):
    """(sp, tris, ms, dp0): dp0 has BASE at (0, 0), INNER at (0, 0) and thin triangle b with its upright edge at x = 0."""
    mesh = E.tie_mesh([BASE + ((0, 0),), INNER + ((0, 0),)])
    for b in range(THIN):                             # source 3 x 11 -> output 6 x 44 from row 0 (a row above the window would wrap into its last row): the inverse is [0.5, 0, 0, 0.25, c, d]
        mesh = _with_triangle(mesh, [10 + 6 * b, 2, 13 + 6 * b, 2, 10 + 6 * b, 13], [0, 0, 6, 0, 0, 44])
    sp, tris, dp = mesh
    if reverse:
        tris = tris.reshape(-1, 3)[::-1].ravel().copy()
    for a in (sp, tris, dp):
        a.setflags(write=False)
    return sp, tris, WL.src_min(sp), dp


N_BASE, N_INNER = 5 * 4, 3 * 2                        # points


def _frame(base=None, inner=None, thin=(), long_form=False):
    """Destination points: BASE / INNER moved to the given output position (None: parked), thin triangle b to x = thin[b] (absent: parked)."""
    d = np.array(_mesh()[3], np.float64).reshape(-1, 2)
    d[:N_BASE] += base if base is not None else (0, PARK)
    d[N_BASE:N_BASE + N_INNER] += inner if inner is not None else (0, PARK)
    thin = dict(thin)
    for b in range(THIN):
        d[N_BASE + N_INNER + 3 * b:N_BASE + N_INNER + 3 * b + 3] += (thin[b], 0) if b in thin else (0, PARK)
    d = d.astype(np.float32).ravel()
    return E.nudge(d, 6, 1) if long_form and base is not None else d      # (vertex 6: an interior point of BASE)


# name -> frame.  INNER has the higher ids: where it lies on BASE it splits BASE's spans into two runs.
def _frames(long_form):
    f = {
        "nested": _frame((4, 0), (200, 4), long_form=long_form),
        "edge255": _frame((4, 0), (255, 4), long_form=long_form),            # a run boundary on, one before and one behind a window edge ...
        "edge256": _frame((4, 0), (256, 4), long_form=long_form),
        "edge257": _frame((4, 0), (257, 4), long_form=long_form),
        "piece64": _frame((4, 0), (64, 4), long_form=long_form),             # ... and on 64-pixel piece edges (INNER is 128 wide: both its ends)
        "to_edge": _frame((8, 0), (200, 4), long_form=long_form),            # BASE reaches the row end: the ragged last window ends in a record-bearing run
        "split": _frame((4, 0), None, {0: 60, 1: 300}, long_form=long_form),  # a thin triangle inside one span of BASE: the span is split into two runs
        "gaps": _frame(None, (60, 2), {0: 250, 1: 262, 2: 300}),              # gaps at both ends and in the middle of rows, over a window edge
        "no_spans": _frame(None, (200, 8)),                                   # rows 0 .. 7 and 16 .. 21 hold no span at all
        "over_limit": _frame((4, 0), None, {b: 6 + 12 * b for b in range(THIN)}, long_form=long_form),
    }
    return f


ORDER = ["nested", "edge255", "edge256", "edge257", "piece64", "to_edge", "split", "gaps", "no_spans", "over_limit"]


@functools.lru_cache(maxsize=None)
def _want(long_form, reverse=False):
    """Per frame (rgba, runs per row, winner of the last column per row) on the oracle: the runs of a row are the changes of the winner along it."""
    sp, tris, ms, _ = _mesh(reverse)
    frames = _frames(long_form)
    out = {}
    for name in ORDER:
        rgba, wmap, _, _ = O.warp_inverse_piecewise(sp, frames[name], tris, _image(), ms[0], ms[1], *WIN, taps=True)
        wmap = np.asarray(wmap).reshape(WIN[3], WIN[2])
        out[name] = (rgba, 1 + (wmap[:, 1:] != wmap[:, :-1]).sum(axis=1), wmap[:, -1].copy())
    return out


def _ctx(options):
    c = HG.Context(0)
    for k, v in dict(SELF_ROWS, **dict(options)).items():
        c.set_option(k, v)
    c.set_option("span_cache", 1)
    return c


def _run_set(c, names, frames, n=3):
    """n warps of the frames `names` into n buffers; returns [warp][frame] arrays."""
    geoms = [WIN] * len(names)
    offs, total = HG.pack_offsets(geoms)
    c.piecewise_set_frames(np.concatenate([frames[k] for k in names]), geoms, offs)
    bufs = [c.alloc(total) for _ in range(n)]
    try:
        for d in bufs:
            c.warp_inverse_piecewise_frames_device(d)
        c.sync()
        return [[c.to_host(d, WIN[2] * WIN[3] * 4, offs[f]).reshape(WIN[3], WIN[2], 4) for f in range(len(names))] for d in bufs]
    finally:
        for d in bufs:
            c.free(d)


def _check(warps, names, want):
    for k, got in enumerate(warps):
        for f, name in enumerate(names):
            assert got[f].tobytes() == np.ascontiguousarray(want[name][0]).tobytes(), ("warp", k, "frame", name, "against the oracle")
            assert got[f].tobytes() == warps[0][f].tobytes(), ("warp", k, "frame", name, "against the first warp")


@pytest.mark.parametrize("long_form", [False, True], ids=["one_fma", "long_form"])
@pytest.mark.parametrize("safe", [0, 1], ids=["unsafe", "safe"])
@pytest.mark.parametrize("hi_bounds", [0, 1], ids=["fp64_bounds", "hi_bounds"])
def test_runs_of_nested_split_gapped_and_empty_rows(hi_bounds, safe, long_form):
    """Every frame but the over-limit one: all their groups are held in run form, and three warps (the build, two from the cache) give the
    oracle's bytes."""
    sp, tris, ms, _ = _mesh()
    frames, want = _frames(long_form), _want(long_form)
    names = ORDER[:-1]
    for name in names:
        assert want[name][1].max() <= RUN_LIMIT, name
    assert (want["to_edge"][2] >= 0).all() and (want["nested"][2] < 0).all()      # a triangle in the last column of every row; a gap there
    assert (want["split"][1][:4] == want["nested"][1][:4] + 4).all()      # rows above INNER: each thin triangle adds itself and the second piece of the span under it
    assert want["nested"][1].max() >= 5 and want["no_spans"][1].min() == 1 and want["gaps"][1].max() >= 7      # split spans; rows of one gap run; gaps
    fwd = HG.solve_affine_triangles(sp, frames["nested"], tris).reshape(-1, 6)[:24]
    assert all(HG.affine_one_fma_form(HG.invert_affine(m), WIN) for m in fwd) != long_form
    with _ctx({"hi_bounds": hi_bounds, "safe_spans": safe}) as c:
        c.set_image(_image())
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        warps = _run_set(c, names, frames)
        st = c.span_cache_stats()
        print(st)
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 2, "use"), st
        assert st["groups_valid"] == len(names) * GROUPS and st["groups_not_cached"] == 0, st
        assert c.last_piecewise_variant() == (104011 if hi_bounds else 101001) and c.last_piecewise_self() == 1 and c.redone_frames() == 0
        _check(warps, names, want)


@pytest.mark.parametrize("long_form", [False, True], ids=["one_fma", "long_form"])
@pytest.mark.parametrize("hi_bounds,safe", [(0, 0), (1, 1)], ids=["fp64_unsafe", "hi_safe"])
def test_lower_span_wholly_hidden(hi_bounds, safe, long_form):
    """The same frames with the triangle list reversed: BASE has the higher ids and hides INNER, whose spans own no run."""
    sp, tris, ms, _ = _mesh(True)
    frames, want = _frames(long_form), _want(long_form, True)
    names = ["nested", "edge256", "no_spans"]
    assert np.array_equal(want["nested"][1], _want(long_form, True)["edge256"][1])      # wherever INNER lies under BASE, the rows' runs are BASE's
    with _ctx({"hi_bounds": hi_bounds, "safe_spans": safe}) as c:
        c.set_image(_image())
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        warps = _run_set(c, names, frames)
        st = c.span_cache_stats()
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 2, "use"), st
        assert st["groups_valid"] == len(names) * GROUPS and st["groups_not_cached"] == 0 and c.redone_frames() == 0, st
        _check(warps, names, want)


@pytest.mark.parametrize("long_form", [False, True], ids=["one_fma", "long_form"])
@pytest.mark.parametrize("hi_bounds,safe", [(0, 1), (1, 0), (1, 1)], ids=["fp64_safe", "hi_unsafe", "hi_safe"])
def test_rows_of_more_runs_than_the_limit_stay_in_span_form(hi_bounds, safe, long_form):
    """40 separated thin triangles over BASE: fewer than 64 spans in a row, more than 64 runs.  The frame's groups are not cached and walk
    their spans on every warp, beside a frame whose groups are cached; the bytes are right."""
    sp, tris, ms, _ = _mesh()
    frames, want = _frames(long_form), _want(long_form)
    names = ["nested", "over_limit"]
    assert want["over_limit"][1].min() > RUN_LIMIT, want["over_limit"][1]      # every row, so every group
    with _ctx({"hi_bounds": hi_bounds, "safe_spans": safe}) as c:
        c.set_image(_image())
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        warps = _run_set(c, names, frames, n=4)
        st = c.span_cache_stats()
        print(st)
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 3, "use"), st
        assert st["groups_valid"] == GROUPS and st["groups_not_cached"] == GROUPS, st
        assert c.last_piecewise_self() == 1 and c.redone_frames() == 0      # (fewer than 64 spans: no row overflowed its block)
        _check(warps, names, want)

