"""The thin-plate splines on the GPU against the numpy model of tests/hgtest/tps.py (written from the header's text; pinned by
tests/test_tps_cpu.py).  Shapes are the smallest at which the kernels can go wrong: a handful of frames, windows around the 256-pixel row
walk, point counts around the wave's 64 lanes and around the LDS capacity of the solve (read from hg_tps_dev.h), one frame at 1024 points.

Evaluation tolerance (derived, not measured).  For a record DOWNLOADED FROM THE DEVICE, v = the model's float64 value at a position and
delta = (N + 16) 2^-52 (sum_i |w_i| q_i (|log q_i| + 1) + |a0| + |a1 x'| + |a2 y'| + |t|): the device's float32 must lie between
float32(v - delta) and float32(v + delta) -- any summation order, any logarithm good to a few ulp -- and the coverage decision may differ
from the model's only where |v - bound| <= delta.  Lattice pixels: the same against the model's blend of the device's own nodes, delta = the
largest of the four nodes' plus 8 x 2^-53 x max |node|; pixels on nodes equal the step-1 field bit for bit.

Solve tolerance (the fit test's precedent).  Metric: R = max_i |spline(from_i) - to_i| px at lambda == 0 (the residual of the linear system
at lambda > 0), evaluated in longdouble; base: R of the model's float64 solve; the device may reach 16 x the base (a base of 0 is replaced by
the smallest non-zero base of this file's sweep).  The largest device / base ratio measured over this file on an MI355X: 3.94
(EXPERIMENTS.md, "Thin-plate")."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import tps as TM                 # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import FILL, INVALID  # noqa: E402

pytestmark = pytest.mark.gpu
IX, CO = HG.FIELD_INDEX, HG.FIELD_COORDS
TAIL = 256                                   # canary bytes behind every output
SRC_W, SRC_H = 180, 120                      # the source: smaller than the landmarks' box, so a good share of the pixels is uncovered
WORST = [0.0]
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")
CAP = int(re.search(r"kTpsLdsCap = (\d+);", open(os.path.join(CSRC, "hg_tps_dev.h")).read()).group(1))
LDS_N = max(n for n in range(3, 1025) if (n + 3) ** 2 <= CAP)            # the most points whose system stays in LDS
SWEEP = (3, 4, 5, 63, 64, 65, LDS_N - 1, LDS_N, LDS_N + 1)
_floor = []


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()
    print(f"largest device / base ratio of this file: {WORST[0]:.3g}")


def landmarks(n, seed, w=300.0, h=200.0, amp=6.0, variant=0):
    """n pairs: destiny points over a w x h box, source points a smooth deformation of them plus 0.5 px of noise, moved by (-40, -3) so that
    windows near the origin straddle the source's left and top borders.  variant k > 0: the same destiny points jittered by 2 px."""
    rng = np.random.default_rng(seed)
    frm = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    to = frm + amp * np.stack([np.sin(frm[:, 1] / 40.0), np.cos(frm[:, 0] / 55.0)], 1) + rng.normal(0, 0.5, (n, 2)) - [40.0, 3.0]
    if variant:
        frm = frm + np.random.default_rng(seed * 1000 + variant).normal(0, 2.0, (n, 2))
    return frm.astype(np.float32), to.astype(np.float32)


def floor_base():
    """The smallest non-zero base of the sweep's cases: what a base of 0 is replaced by."""
    if not _floor:
        _floor.append(min(b for b in (TM.solve_base(*landmarks(n, 100 + n), 0.0)[2] for n in SWEEP) if b))
    return _floor[0]


# ------------------------------------------------------------------------------------------------ run
def solve(ctx, frm_sets, to_sets, n_frames, lam=0.0):
    """Upload the lists, fill records, status and scratch with FILL (a canary behind each), solve, download.  Returns (records (F, 16 + 4 N),
    status (F), the device pointer of the records -- to be freed by the caller)."""
    frm_sets, to_sets = np.ascontiguousarray(frm_sets, np.float32), np.ascontiguousarray(to_sets, np.float32)
    n = frm_sets.shape[1]
    rec_b, scr_b = HG.tps_layout(n, n_frames)
    assert rec_b == TM.record_doubles(n) * 8
    d_a, d_b = ctx.alloc(frm_sets.nbytes), ctx.alloc(to_sets.nbytes)
    d_r, d_s, d_w = ctx.alloc(rec_b * n_frames + TAIL), ctx.alloc(4 * n_frames + TAIL), (ctx.alloc(scr_b + TAIL) if scr_b else 0)
    try:
        ctx.to_device(d_a, frm_sets.view(np.uint8).ravel())
        ctx.to_device(d_b, to_sets.view(np.uint8).ravel())
        ctx.to_device(d_r, np.full(rec_b * n_frames + TAIL, FILL, np.uint8))
        ctx.to_device(d_s, np.full(4 * n_frames + TAIL, FILL, np.uint8))
        if scr_b:
            ctx.to_device(d_w, np.full(scr_b + TAIL, FILL, np.uint8))
        ctx.tps_solve_frames_device(d_a, frm_sets.shape[0], d_b, to_sets.shape[0], n, n_frames, d_r, d_s, smoothing=lam, d_scratch=d_w)
        ctx.sync()
        raw_r, raw_s = ctx.to_host(d_r, rec_b * n_frames + TAIL), ctx.to_host(d_s, 4 * n_frames + TAIL)
        if scr_b:
            assert (ctx.to_host(d_w + scr_b, TAIL) == FILL).all(), "the canary behind the scratch"
        assert np.array_equal(ctx.to_host(d_a, frm_sets.nbytes), frm_sets.view(np.uint8).ravel()), "the inputs must not be written"
    except BaseException:
        ctx.free(d_r)
        raise
    finally:
        for p in (d_a, d_b, d_s) + ((d_w,) if d_w else ()):
            ctx.free(p)
    assert (raw_r[rec_b * n_frames:] == FILL).all() and (raw_s[4 * n_frames:] == FILL).all(), "the canaries behind the records and the status"
    recs = raw_r[:rec_b * n_frames].view(np.float64).reshape(n_frames, -1).copy()
    return recs, raw_s[:4 * n_frames].view(np.int32).copy(), d_r


def field(ctx, d_r, n, geoms, fmt, step=1, offs=None, W=SRC_W, H=SRC_H):
    """The field of the records at d_r into an allocation full of FILL; every byte outside the frames must still be FILL afterwards.  Returns
    (per-frame bytes, per-frame node bytes or None)."""
    px = 4 if fmt == IX else 8
    fo = list(offs) if offs is not None else HG.pack_field_offsets(geoms, fmt)[0]
    assert offs is not None or fo == TM.pack256(geoms, px)[0]
    total = max([o + max(g[2], 0) * max(g[3], 0) * px for o, g in zip(fo, geoms)] + [0]) + TAIL
    scr = HG.tps_field_layout(geoms, step)
    no, ntotal = TM.pack256([(0, 0, TM.nodes(g[2], step), TM.nodes(g[3], step)) if g[2] > 0 and g[3] > 0 else (0, 0, 0, 0) for g in geoms], 16)
    assert scr == (ntotal if step > 1 else 0)
    d_f, d_n = ctx.alloc(total), (ctx.alloc(scr + TAIL) if scr else 0)
    try:
        ctx.to_device(d_f, np.full(total, FILL, np.uint8))
        if scr:
            ctx.to_device(d_n, np.full(scr + TAIL, FILL, np.uint8))
        ctx.field_tps_frames_device(d_r, n, geoms, W, H, fmt, d_f, step=step, field_offsets=offs, d_scratch=d_n)
        ctx.sync()
        raw = ctx.to_host(d_f, total)
        nraw = ctx.to_host(d_n, scr + TAIL) if scr else None
    finally:
        ctx.free(d_f)
        if d_n:
            ctx.free(d_n)
    untouched = np.ones(total, bool)
    frames = []
    for o, g in zip(fo, geoms):
        k = max(g[2], 0) * max(g[3], 0) * px
        untouched[o:o + k] = False
        frames.append(raw[o:o + k].copy())
    assert (raw[untouched] == FILL).all(), "bytes between the frames, the padding and the tail must not be written"
    nodes = None
    if scr:
        assert (nraw[scr:] == FILL).all(), "the canary behind the nodes"
        nodes = [nraw[o:o + TM.nodes(g[2], step) * TM.nodes(g[3], step) * 16].copy() if g[2] > 0 and g[3] > 0 else None for o, g in zip(no, geoms)]
    return frames, nodes


def points(ctx, d_r, n, n_frames, pts):
    pts = np.ascontiguousarray(pts, np.float32)
    n_sets, n_pts = pts.shape[0], pts.shape[1]
    out_b = n_frames * n_pts * 8
    d_p, d_o = ctx.alloc(pts.nbytes), ctx.alloc(out_b + TAIL)
    try:
        ctx.to_device(d_p, pts.view(np.uint8).ravel())
        ctx.to_device(d_o, np.full(out_b + TAIL, FILL, np.uint8))
        ctx.points_tps_frames_device(d_r, n, n_frames, d_p, n_pts, n_sets, d_o)
        ctx.sync()
        raw = ctx.to_host(d_o, out_b + TAIL)
    finally:
        ctx.free(d_p)
        ctx.free(d_o)
    assert (raw[out_b:] == FILL).all(), "the canary behind the point results"
    return raw[:out_b].view(np.float32).reshape(n_frames, n_pts, 2).copy()


def check_records(recs, status, frm_sets, to_sets, lam, what):
    for f in range(recs.shape[0]):
        r = TM.check_record(recs[f], status[f], frm_sets[f % len(frm_sets)], to_sets[f % len(to_sets)], lam, floor_base(), (what, f))
        WORST[0] = max(WORST[0], r)
        print(f"{what} frame {f}: device / base {r:.3g}")


# ------------------------------------------------------------------------------------------------ the solve and the step-1 field
@pytest.mark.parametrize("n", SWEEP)
def test_point_counts_around_the_wave_and_the_lds_capacity(ctx, n):
    a, b = landmarks(n, 100 + n)
    a2, _ = landmarks(n, 100 + n, variant=1)
    frm_sets, to_sets = [a, a2], [b]
    geoms = [(-4, 3, 70, 9), (60, 40, 33, 6), (-20, -10, 5, 4)]
    recs, status, d_r = solve(ctx, frm_sets, to_sets, 3)
    try:
        check_records(recs, status, frm_sets, to_sets, 0.0, f"N = {n}")
        assert (status == TM.OK).all()
        frames, _ = field(ctx, d_r, n, geoms, CO)
    finally:
        ctx.free(d_r)
    covered = 0
    for f, g in enumerate(geoms):
        TM.check_field_frame(frames[f], recs[f], True, g, SRC_W, SRC_H, False, (n, f))
        covered += int((~np.isnan(frames[f].view(np.float32))).sum()) // 2
    total = sum(g[2] * g[3] for g in geoms)
    if n >= 63:                                              # (a handful of random pairs extrapolates anywhere; dense landmarks follow the deformation)
        assert 0.1 * total < covered < 0.9 * total, (covered, total)         # the coverage test decides in both directions


def test_1024_points_solve_in_scratch(ctx):
    a, b = landmarks(1024, 7, w=900.0, h=700.0)
    recs, status, d_r = solve(ctx, [a], [b], 1)
    try:
        check_records(recs, status, [a], [b], 0.0, "N = 1024")
        assert status[0] == TM.OK
        frames, _ = field(ctx, d_r, 1024, [(100, 100, 64, 4)], CO, W=900, H=700)
    finally:
        ctx.free(d_r)
    assert not np.isnan(frames[0].view(np.float32)).any()   # (inside the landmarks' box and the source: the spline is sane there)


@pytest.mark.parametrize("sets", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_frame_f_reads_list_f_modulo_the_set_count(ctx, sets):
    n = 12
    frm_sets = [landmarks(n, 30 + k)[0] for k in range(sets[0])]
    to_sets = [landmarks(n, 40 + k)[1] for k in range(sets[1])]
    recs, status, d_r = solve(ctx, frm_sets, to_sets, 3, lam=0.25 if sets == (2, 2) else 0.0)
    ctx.free(d_r)
    check_records(recs, status, frm_sets, to_sets, 0.25 if sets == (2, 2) else 0.0, f"sets {sets}")
    assert (status == TM.OK).all()
    if sets == (1, 1):
        assert np.array_equal(recs[0].view(np.uint64), recs[1].view(np.uint64)) and np.array_equal(recs[0].view(np.uint64), recs[2].view(np.uint64))
    if sets == (2, 2):
        assert np.array_equal(recs[0].view(np.uint64), recs[2].view(np.uint64)) and not np.array_equal(recs[0], recs[1])


WINDOWS = [(-3, -2, 1, 1), (5, 7, 70, 9), (0, 0, 0, 4), (-100, 50, 257, 5), (20, 2, 513, 3)]


@pytest.mark.parametrize("fmt", [IX, CO])
def test_windows_around_the_row_walk_with_an_empty_frame(ctx, fmt):
    n = 16
    frm_sets = [landmarks(n, 50 + k, w=500.0)[0] for k in range(5)]
    to_sets = [landmarks(n, 50 + k, w=500.0)[1] for k in range(5)]
    recs, status, d_r = solve(ctx, frm_sets, to_sets, 5)
    try:
        assert (status == TM.OK).all()
        frames, _ = field(ctx, d_r, n, WINDOWS, fmt, W=400, H=SRC_H)
        # caller-given offsets: reversed order, gaps of odd sizes (multiples of the pixel size), which must keep their bytes
        px = 4 if fmt == IX else 8
        offs, o = [0] * 5, 24
        for f in (4, 2, 0, 3, 1):
            offs[f] = o
            o += max(WINDOWS[f][2], 0) * max(WINDOWS[f][3], 0) * px + 8 * (f + 1)
        moved, _ = field(ctx, d_r, n, WINDOWS, fmt, offs=offs, W=400, H=SRC_H)
    finally:
        ctx.free(d_r)
    for f, g in enumerate(WINDOWS):
        assert frames[f].size == max(g[2], 0) * max(g[3], 0) * px
        if frames[f].size:
            TM.check_field_frame(frames[f], recs[f], True, g, 400, SRC_H, fmt == IX, (fmt, f))
        assert np.array_equal(frames[f], moved[f]), (fmt, f, "the same values wherever the frame is put")


# ------------------------------------------------------------------------------------------------ the stepped field
LATTICE = [(0, 0, 1, 1), (-4, 3, 70, 9), (2, 2, 0, 5), (35, -3, 33, 37), (0, 0, 3, 2), (30, 20, 65, 17)]


@pytest.mark.parametrize("fmt", [IX, CO])
@pytest.mark.parametrize("step", [2, 4, 8, 16, 32])
def test_every_step_on_windows_smaller_than_the_step_and_no_multiple_of_it(ctx, step, fmt):
    n = 20
    frm_sets = [landmarks(n, 60)[0], landmarks(n, 60, variant=1)[0]]
    to_sets = [landmarks(n, 60)[1]]
    F = len(LATTICE)
    bad = frm_sets[1].copy()
    bad[3, 0] = np.nan
    frm_sets = [frm_sets[0], frm_sets[1], bad]                # frames 2 and 5 fail
    recs, status, d_r = solve(ctx, frm_sets, to_sets, F)
    try:
        assert status.tolist() == [0, 0, 2, 0, 0, 2]
        one, _ = field(ctx, d_r, n, LATTICE, fmt)
        frames, nodes = field(ctx, d_r, n, LATTICE, fmt, step=step)
    finally:
        ctx.free(d_r)
    for f, g in enumerate(LATTICE):
        if g[2] > 0 and g[3] > 0:
            TM.check_lattice_frame(frames[f], one[f], nodes[f], recs[f], status[f] == TM.OK, g, SRC_W, SRC_H, fmt == IX, step, (step, fmt, f))


# ------------------------------------------------------------------------------------------------ failed frames
def test_failed_frames_leave_their_neighbours_alone(ctx):
    n = 10
    good = [landmarks(n, 70 + k) for k in range(3)]
    nan_from = good[0][0].copy(); nan_from[4, 1] = np.nan
    inf_to = good[0][1].copy(); inf_to[0, 0] = -np.inf
    same = np.tile(good[1][0][:1], (n, 1))
    dup = good[2][0].copy(); dup[7] = dup[2]
    frm_sets = [good[0][0], nan_from, good[1][0], same, good[2][0], dup, good[0][0]]
    to_sets = [good[0][1], good[0][1], good[1][1], good[1][1], good[2][1], good[2][1], inf_to]
    F = len(frm_sets)
    geoms = [(-4, 3, 40, 5)] * F
    recs, status, d_r = solve(ctx, frm_sets, to_sets, F)
    try:
        assert status.tolist() == [TM.OK, TM.BAD_INPUT, TM.OK, TM.SINGULAR, TM.OK, TM.SINGULAR, TM.BAD_INPUT]
        check_records(recs, status, frm_sets, to_sets, 0.0, "failed frames")
        frames = {fmt: field(ctx, d_r, n, geoms, fmt)[0] for fmt in (IX, CO)}
        pts = np.array([[[0, 0], [10.5, 3.25], [100, 50]]], np.float32)
        got = points(ctx, d_r, n, F, pts)
    finally:
        ctx.free(d_r)
    for fmt in (IX, CO):
        for f in range(F):
            TM.check_field_frame(frames[fmt][f], recs[f], status[f] == TM.OK, geoms[f], SRC_W, SRC_H, fmt == IX, (fmt, f))
    for f in range(F):
        TM.check_points_frame(got[f], recs[f], status[f] == TM.OK, pts[0], f)
    # the good frames alone give the same bits
    alone, st, d_r = solve(ctx, [g[0] for g in good], [g[1] for g in good], 3)
    ctx.free(d_r)
    assert (st == TM.OK).all()
    for k, f in enumerate((0, 2, 4)):
        assert np.array_equal(alone[k].view(np.uint64), recs[f].view(np.uint64)), f
    # the duplicate at lambda > 0 solves
    recs, status, d_r = solve(ctx, [dup], [good[2][1]], 1, lam=0.05)
    ctx.free(d_r)
    assert status[0] == TM.OK and np.isfinite(recs).all()
    check_records(recs, status, [dup], [good[2][1]], 0.05, "duplicate, lambda 0.05")


# ------------------------------------------------------------------------------------------------ point lists
@pytest.mark.parametrize("n", [5, 64, LDS_N + 1])
def test_point_lists_repeat_the_coords_field_and_take_any_float(ctx, n):
    frm_sets = [landmarks(n, 80)[0], landmarks(n, 80, variant=1)[0]]
    to_sets = [landmarks(n, 80)[1]]
    g = (-4, 3, 70, 9) if n > 5 else (0, 0, 70, 9)
    X, Y = TM.window_positions(g)
    grid = np.stack([X.ravel(), Y.ravel()], 1).astype(np.float32)
    odd = np.array([[np.nan, 1], [2, np.nan], [np.inf, 0], [0, -np.inf], [1e30, 5], [-1e30, 1e30], [13.5, 7.25], [-1000.75, 2000.5]], np.float32)
    lists = np.stack([np.concatenate([grid, odd]), np.concatenate([grid, odd[::-1]])])
    recs, status, d_r = solve(ctx, frm_sets, to_sets, 3)
    try:
        assert (status == TM.OK).all()
        frames, _ = field(ctx, d_r, n, [g] * 3, CO)
        one = points(ctx, d_r, n, 3, lists[:1])
        two = points(ctx, d_r, n, 3, lists)
    finally:
        ctx.free(d_r)
    k = grid.shape[0]
    for f in range(3):
        fld = frames[f].view(np.uint32).reshape(-1, 2)
        cov = fld[:, 0] != 0x7FC00000
        assert n == 5 or (cov.any() and (~cov).any())        # (five random pairs extrapolate anywhere)
        for got, lst in ((one[f], lists[0]), (two[f], lists[f % 2])):
            assert np.array_equal(got[:k].view(np.uint32)[cov], fld[cov]), (n, f, "an integer position equals the coords field where it is covered, bit for bit")
            TM.check_points_frame(got, recs[f], True, lst, (n, f))
            assert not np.isnan(got[:k]).any()             # there is no coverage test
    assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(one[2].view(np.uint32), two[2].view(np.uint32))


# ------------------------------------------------------------------------------------------------ determinism, refusals
@pytest.mark.parametrize("n", [64, LDS_N + 1])
def test_the_same_bytes_on_two_runs(ctx, n):
    frm_sets, to_sets = [landmarks(n, 90)[0], landmarks(n, 90, variant=1)[0]], [landmarks(n, 90)[1]]
    geoms = [(-4, 3, 70, 9), (60, 40, 33, 6), (0, 0, 5, 4)]
    pts = np.array([[[0.5, 0.25], [100, 50], [-7, 300]]], np.float32)
    runs = []
    for _ in range(2):
        recs, status, d_r = solve(ctx, frm_sets, to_sets, 3, lam=0.0)
        try:
            runs.append((recs.view(np.uint64), status, field(ctx, d_r, n, geoms, CO)[0], field(ctx, d_r, n, geoms, IX, step=4)[0], points(ctx, d_r, n, 3, pts).view(np.uint32)))
        finally:
            ctx.free(d_r)
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])
    for k in (2, 3):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))


def test_refusals_on_the_device(ctx):
    n = 8
    a, b = landmarks(n, 95)
    recs, status, d_r = solve(ctx, [a], [b], 1)
    d_f = ctx.alloc(4096)
    try:
        g = [(0, 0, 8, 8)]
        code = lambda fn, *x, **k: GF.refusal_code(fn, *x, **k)
        assert code(ctx.field_tps_frames_device, d_r, n, g, SRC_W, SRC_H, CO, 0) == INVALID                        # d_field NULL
        assert code(ctx.field_tps_frames_device, 0, n, g, SRC_W, SRC_H, CO, d_f) == INVALID                        # d_records NULL
        assert code(ctx.field_tps_frames_device, d_r + 4, n, g, SRC_W, SRC_H, CO, d_f) == INVALID                  # misaligned records
        assert code(ctx.field_tps_frames_device, d_r, n, g, SRC_W, SRC_H, CO, d_f + 4) == INVALID                  # coords field off its 8 bytes
        assert code(ctx.field_tps_frames_device, d_r, n, g, SRC_W, SRC_H, CO, d_f, step=4) == INVALID              # a stepped field needs its scratch
        assert code(ctx.field_tps_frames_device, d_r, n, g, SRC_W, SRC_H, CO, d_f, step=5) == INVALID
        assert code(ctx.field_tps_frames_device, d_r, n, g, 0, SRC_H, CO, d_f) == INVALID
        assert code(ctx.field_tps_frames_device, d_r, n, g, SRC_W, SRC_H, 2, d_f) == INVALID
        assert code(ctx.points_tps_frames_device, d_r, n, 1, 0, 4, 1, d_f) == INVALID
        assert code(ctx.points_tps_frames_device, d_r, n, 1, d_f + 4, 4, 1, d_f) == INVALID
        assert code(ctx.points_tps_frames_device, d_r, n, 1, d_f, 4, 0, d_f) == INVALID
        assert code(ctx.tps_solve_frames_device, d_f, 1, d_f, 1, n, 1, 0, d_f) == INVALID                          # d_records NULL
        assert code(ctx.tps_solve_frames_device, d_f, 1, d_f, 1, n, 1, d_r, d_f, smoothing=-1.0) == INVALID
        assert code(ctx.tps_solve_frames_device, d_f, 1, d_f, 1, LDS_N + 1, 1, d_r, d_f) == INVALID                # beyond LDS the scratch is required
        assert code(ctx.tps_solve_frames_device, d_f, 0, d_f, 1, n, 1, d_r, d_f) == INVALID
        ctx.tps_solve_frames_device(0, 1, 0, 1, n, 0, 0, 0)                                                       # no frames: HG_OK, nothing is looked at
        ctx.field_tps_frames_device(0, n, [], SRC_W, SRC_H, CO, 0)
        ctx.points_tps_frames_device(0, n, 1, 0, 0, 1, 0)
        ctx.sync()
        assert np.array_equal(ctx.to_host(d_r, recs.nbytes).view(np.uint64), recs.view(np.uint64).ravel()), "a refused call writes nothing"
    finally:
        ctx.free(d_r)
        ctx.free(d_f)


def test_a_tps_call_leaves_the_warp_state_alone(ctx):
    before = GF.tap_state(ctx)
    a, b = landmarks(9, 96)
    recs, status, d_r = solve(ctx, [a], [b], 1)
    try:
        field(ctx, d_r, 9, [(0, 0, 20, 6)], CO, step=2)
        points(ctx, d_r, 9, 1, np.zeros((1, 3, 2), np.float32))
    finally:
        ctx.free(d_r)
    assert GF.tap_state(ctx) == before


def test_js_warp_thin_plate_equals_the_gather_through_its_own_index_field():
    """tests/js/tps_gpu.mjs: warpThinPlate(..., { output: 'image' }) on the real addon equals gathering the picture through the call's own
    index field; a failed frame is empty and alone."""
    GF.run_node_case("tps_gpu.mjs")
