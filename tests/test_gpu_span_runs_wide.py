"""The run form of the span cache (csrc/hg_span_runs.h) where tests/test_gpu_span_runs.py does not reach: rows of five to nine 256-pixel windows
-- the second and third trips of k_pw_rows' window loop, which takes four windows a trip in the hi-bounds form --, rows at the capacities of a
row block (64 runs, 63 spans) and bounded random stacks.  The shapes come from tests/hgtest/span_rows.py and tests/test_span_runs_shapes_cpu.py
proves on the oracle alone what the cases here rely on.

The protocol is that of tests/test_gpu_span_runs.py: self_spans = 1, patch = tile = compact = min_row_groups = 0, span_cache = 1 (build on the
first warp, use from the second); every warp goes into a buffer of its own and is compared bit for bit with the oracle and with the set's
first warp; every case asserts the cache statistics, the variant and the self-span form it relies on."""
import numpy as np
import pytest

from hgtest import hip
from hgtest import span_rows as S

pytestmark = pytest.mark.gpu

HG = hip.load()
SELF_ROWS = {"self_spans": 1, "patch": 0, "tile": 0, "compact": 0, "min_row_groups": 0}
# (hi_bounds, safe_spans, long form): hi_bounds = 1 is the four-windows-a-trip form and takes the whole cross product
FORMS = [(1, 0, False), (1, 0, True), (1, 1, False), (1, 1, True), (0, 0, False), (0, 1, True)]
FORM_IDS = ["hi_unsafe_one_fma", "hi_unsafe_long", "hi_safe_one_fma", "hi_safe_long", "fp64_unsafe_one_fma", "fp64_safe_long"]
FEWER = [(1, 1, False), (1, 0, True), (0, 1, False), (0, 0, True)]
FEWER_IDS = ["hi_safe_one_fma", "hi_unsafe_long", "fp64_safe_one_fma", "fp64_unsafe_long"]


def _ctx(hi_bounds, safe):
    c = HG.Context(0)
    for k, v in dict(SELF_ROWS, hi_bounds=hi_bounds, safe_spans=safe).items():
        c.set_option(k, v)
    c.set_option("span_cache", 1)
    return c


def _one_fma(sp, tris, dp, geom, mask):
    """Do the placed triangles of a frame all have an inverse of the one-fma form in its window?"""
    fwd = HG.solve_affine_triangles(sp, dp, tris).reshape(-1, 6)[mask]
    return all(HG.affine_one_fma_form(HG.invert_affine(m), geom) for m in fwd)


def _warps(c, n, geoms, offs, total, sync=True, queued=None):
    """n warps of the staged set into n buffers of their own; returns [warp][frame] arrays (None for a frame without pixels).  queued: called
    behind the last launch, before the context settles its queued warps."""
    bufs = [c.alloc(total) for _ in range(n)]
    try:
        junk = np.full(total, 0xA5, np.uint8)                 # a pixel no warp stores keeps this: a zero store that went elsewhere shows
        for d in bufs:
            c.to_device(d, junk)
        for d in bufs:
            c.warp_inverse_piecewise_frames_device(d)
            if sync:
                c.sync()
        if queued is not None:
            queued()
        c.sync()
        return [[c.to_host(d, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4) if g[2] > 0 and g[3] > 0 else None for f, g in enumerate(geoms)]
                for d in bufs]
    finally:
        for d in bufs:
            c.free(d)


def _check(warps, want, names):
    for k, got in enumerate(warps):
        for f, name in enumerate(names):
            if want[f] is None:
                assert got[f] is None
                continue
            assert got[f].shape == want[f].shape and got[f].tobytes() == np.ascontiguousarray(want[f]).tobytes(), ("warp", k, "frame", name, "against the oracle")
            assert got[f].tobytes() == warps[0][f].tobytes(), ("warp", k, "frame", name, "against the first warp")


def _variant_ok(c, hi_bounds):
    return c.last_piecewise_variant() == (104011 if hi_bounds else 101001) and c.last_piecewise_self() == 1


# ------------------------------------------------------------------------------------------------ 1. wide rows
@pytest.mark.parametrize("hi_bounds,safe,long_form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("width", S.WIDTHS)
def test_rows_of_more_windows_than_one_trip(width, hi_bounds, safe, long_form):
    """The frames of one width (hgtest.span_rows.wide_places) in one set: run boundaries on, before and behind the window edges 1024, 1280 and
    2048 and on the piece edges 1088 and 1152; windows of the later trips inside one record-bearing run, inside a gap run (the 16-byte zero
    stores of window 4 and up; none at the odd width 1153) and with five and more interior run starts; rows that end in a run and in a gap; the
    ragged last window and its dead pieces in a later trip; at width 40 a row narrower than one 64-pixel piece (22 rows: a frame whose map is smaller than its widest triangle goes through the map path)."""
    S.check_wide_placement(width, long_form)
    P = S.wide_parts()
    frames, want = S.wide_frames(width, long_form), S.wide_want(width, long_form)
    names = list(frames)
    geoms = [frames[k][1] for k in names]
    for k in names:
        if S.wide_places(width)[k]:
            assert _one_fma(P.sp, P.tris, frames[k][0], frames[k][1], P.placed_mask(S.wide_places(width)[k])) != long_form, k
    offs, total = HG.pack_offsets(geoms)
    with _ctx(hi_bounds, safe) as c:
        c.set_image(S.image())
        c.piecewise_set_mesh(P.sp, P.tris, P.ms[0], P.ms[1])
        c.piecewise_set_frames(np.concatenate([frames[k][0] for k in names]), geoms, offs)
        warps = _warps(c, 3, geoms, offs, total)
        st = c.span_cache_stats()
        print(st)
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 2, "use"), st
        assert st["groups_valid"] == len(names) * S.group_count(S.wide_height(width)) and st["groups_not_cached"] == 0, st
        assert _variant_ok(c, hi_bounds) and c.redone_frames() == 0
        _check(warps, [want[k][0] for k in names], names)


@pytest.mark.parametrize("hi_bounds,safe,long_form", FEWER, ids=FEWER_IDS)
def test_frames_of_different_sizes_in_one_set(hi_bounds, safe, long_form):
    """2052 x 10 at a window origin of its own, 1300 x 3 at a byte offset that is no multiple of 16 (the 16-byte zero stores are off for a width
    that would allow them), 40 x 22 and an empty frame.  The directory has six groups a frame, those of the tallest; hg_span_cache_stats counts a
    frame's own groups only -- the groups beyond its rows are never launched and are neither valid nor "not cached": 3 + 1 + 6 + 0."""
    P = S.wide_parts()
    dps, geoms, offs, total, want = S.mixed_set(long_form)
    assert [g[2:] for g in geoms] == [(2052, 10), (1300, 3), (40, 22), (0, 22)] and geoms[0][:2] != (0, 0)
    groups = sum(S.group_count(g[3]) for g in geoms if g[2] > 0)
    assert groups == 10
    with _ctx(hi_bounds, safe) as c:
        c.set_image(S.image())
        c.piecewise_set_mesh(P.sp, P.tris, P.ms[0], P.ms[1])
        c.piecewise_set_frames(np.concatenate(dps), geoms, offs)
        warps = _warps(c, 3, geoms, offs, total)
        st = c.span_cache_stats()
        print(st)
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 2, "use"), st
        assert st["groups_valid"] == groups and st["groups_not_cached"] == 0, st
        assert _variant_ok(c, hi_bounds) and c.redone_frames() == 0
        _check(warps, want, ["2052x10", "1300x3", "40x22", "empty"])


# ------------------------------------------------------------------------------------------------ 2. capacities
def _capacity_set(c, names, long_form, n, sync, queued=None):
    """A set of three "low" frames first (40 spans a row): the planner's estimate of that set is kept for the next one of the same extents,
    which is how 4-row groups meet rows of 63 and 64 spans (the estimate of such a set alone gives one-row groups, which the cache does not
    take).  Then n warps of the frames `names`.  Returns (warps, builds before the set)."""
    P, frames, want = S.cap_parts(), S.cap_frames(long_form), S.cap_want(long_form)
    places = S.cap_places()
    geoms = [S.CAP_WIN] * 3
    offs, total = HG.pack_offsets(geoms)
    for k in set(names) | {"low"}:
        assert _one_fma(P.sp, P.tris, frames[k], S.CAP_WIN, P.placed_mask(places[k])) != long_form, k
    c.set_image(S.image())
    c.piecewise_set_mesh(P.sp, P.tris, P.ms[0], P.ms[1])
    c.piecewise_set_frames(np.concatenate([frames["low"]] * 3), geoms, offs)
    _check(_warps(c, 1, geoms, offs, total), [want["low"][0]] * 3, ["low"] * 3)
    assert c.redone_frames() == 0 and c.last_piecewise_variant() in (104011, 101001)
    builds = c.span_cache_stats()["builds"]
    c.piecewise_set_frames(np.concatenate([frames[k] for k in names]), geoms, offs)
    return _warps(c, n, geoms, offs, total, sync, queued), builds


@pytest.mark.parametrize("hi_bounds,safe,long_form", FEWER, ids=FEWER_IDS)
def test_rows_of_exactly_64_runs_beside_rows_of_65(hi_bounds, safe, long_form):
    """63 spans resolving to 64 runs, in both forms -- run 63 the trailing gap; run 63 a record of the tail cell, with live pixels: lane 63 copies
    it into slot 63 of the row's block, the place of the NaN record in span form -- are cached and flag nothing.  The third frame has a gap at
    either end of the same 63 spans, 65 runs: its groups are not cached and walk their spans on every warp."""
    S.check_capacities(long_form)
    names = ["gap63", "rec64", "runs65"]
    want = S.cap_want(long_form)
    groups = S.group_count(S.CAP_WIN[3])
    with _ctx(hi_bounds, safe) as c:
        warps, builds = _capacity_set(c, names, long_form, 3, True)
        st = c.span_cache_stats()
        print(st)
        assert (st["builds"], st["use_calls"], st["state"]) == (builds + 1, 2, "use"), st
        assert st["groups_valid"] == 2 * groups and st["groups_not_cached"] == groups, st
        assert _variant_ok(c, hi_bounds) and c.redone_frames() == 0
        _check(warps, [want[k][0] for k in names], names)


@pytest.mark.parametrize("hi_bounds,safe,long_form", FEWER, ids=FEWER_IDS)
def test_a_row_of_64_spans_flags_its_frame_on_every_cached_call(hi_bounds, safe, long_form):
    """One more span than a row block holds: the prologue of the build flags the frame (FRAME_LDS_OVERFLOW), the frame is redone through the
    map, and every warp from the cache flags it again; the 63-span frame beside it is cached.  (Queued: one plan for all four warps.  The
    directory is read behind the last launch: settling the flagged frames redoes them one by one, and the statistics of a context whose last
    upload was such a frame count no groups.)"""
    S.check_capacities(long_form)
    names = ["gap63", "spans64", "low"]
    want = S.cap_want(long_form)
    groups = S.group_count(S.CAP_WIN[3])
    with _ctx(hi_bounds, safe) as c:
        seen = []
        warps, builds = _capacity_set(c, names, long_form, 4, False, lambda: seen.append(c.span_cache_stats()))
        st = c.span_cache_stats()
        print(seen, st, c.redone_frames(), c.last_piecewise_flag())
        assert (st["builds"], st["use_calls"], st["state"]) == (builds + 1, 3, "use"), st
        assert seen[0]["groups_valid"] == 2 * groups and seen[0]["groups_not_cached"] == 0, seen      # (an overflowed group is neither)
        assert _variant_ok(c, hi_bounds)
        assert c.redone_frames() == 4, c.redone_frames()
        _check(warps, [want[k][0] for k in names], names)


# ------------------------------------------------------------------------------------------------ 3. bounded random differential
# every seed in the hi-bounds form, every fourth in the fp64 form as well; safe_spans alternates
RANDOM = [(seed, 1, (seed >> 1) & 1) for seed in S.SEEDS] + [(seed, 0, seed & 1) for seed in S.SEEDS[::4]]


@pytest.mark.parametrize("seed,hi_bounds,safe", RANDOM, ids=["seed%d_%s_%s" % (s, "hi" if h else "fp64", "safe" if f else "unsafe") for s, h, f in RANDOM])
def test_random_stacks_from_the_cache(seed, hi_bounds, safe):
    """hgtest.span_rows.random_set: grid layers and thin triangles in shuffled id order, two or three windows of 700 .. 1300 x 10 .. 18 at
    offsets of their own; odd seeds in the long record form, multiples of three with source points and minima per frame.  The groups held in
    run form are exactly those the oracle's winner maps allow (tests/test_span_runs_shapes_cpu.py: at least one per seed, at least three
    quarters over all seeds)."""
    s, want = S.random_set(seed), S.random_want(seed)
    frames = s["frames"]
    geoms = [f[1] for f in frames]
    ok = np.concatenate([S.cacheable_groups(m) for _, m in want])
    assert ok.any()
    assert all(_one_fma(f[2], s["tris"], f[0], f[1], m) != s["long_form"] for f, m in zip(frames, s["placed"]))
    with _ctx(hi_bounds, safe) as c:
        c.set_image(S.image())
        c.piecewise_set_mesh(s["sp"], s["tris"], s["ms"][0], s["ms"][1])
        dst = np.concatenate([f[0] for f in frames])
        if s["own_src"]:
            c.piecewise_set_frames_src(np.concatenate([f[2] for f in frames]), np.int32([f[3] for f in frames]).ravel(), dst, geoms, s["offs"])
        else:
            c.piecewise_set_frames(dst, geoms, s["offs"])
        warps = _warps(c, 3, geoms, s["offs"], s["total"])
        st = c.span_cache_stats()
        print(st)
        assert (st["builds"], st["use_calls"], st["state"]) == (1, 2, "use"), st
        assert st["groups_valid"] == int(ok.sum()) and st["groups_not_cached"] == int((~ok).sum()), (st, ok)
        assert _variant_ok(c, hi_bounds) and c.redone_frames() == 0
        _check(warps, [w[0] for w in want], list(range(len(frames))))
