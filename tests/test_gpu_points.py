"""Point lists through the warp geometry of a frame set on the GPU (include/hgwarp.h, hg_points_*), bit for bit (results are compared as
uint32 views) against two anchors: the library's own HG_FIELD_COORDS fields at every integer window pixel, and the numpy model of
tests/hgtest/points.py (pinned to the field model and to the oracle's forward warps by tests/test_points_cpu.py) everywhere else.  The
model's maps and matrices come from the CPU oracle, never from the library under test."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import folds as FO               # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import moving as M               # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import points as P               # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
CO = HG.FIELD_COORDS
W, H = 160, 96
WIN = (-3, -5, W + 9, H + 6)                 # the window of test_gpu_sampling
NAN = np.uint32(0x7FC00000)
CAP = 0.005


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    g, w = GF.u32(got).reshape(-1, 2), GF.u32(want).reshape(-1, 2)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(1))
    if bad.size:
        gf, wf = g.view(np.float32), w.view(np.float32)
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} points differ; (i, got, want): "
                             f"{[(int(i), gf[i].tolist(), wf[i].tolist()) for i in bad[:6]]}")


def grid(x0, y0, w, h):
    x, y = np.meshgrid(np.arange(w) + x0, np.arange(h) + y0)
    return np.stack([x, y], -1).reshape(-1, 2).astype(np.float32)


def run(ctx, call, pts, n_frames, n_sets=1):
    """call(d_points, n_points, n_sets, d_out) over `pts` ((n_sets *) n x 2 float32); returns (n_frames, n, 2) float32.  The results sit in a
    buffer pre-filled with 0xA5 with a tail that must stay as it was."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(n_sets, -1, 2)
    n = pts.shape[1]
    nb, slack = n_frames * n * 8, 256
    d_p, d_o = ctx.alloc(max(pts.nbytes, 8)), ctx.alloc(nb + slack)
    try:
        if pts.nbytes:
            ctx.to_device(d_p, pts)
        ctx.to_device(d_o, np.full(nb + slack, 0xA5, np.uint8))
        call(d_p, n, n_sets, d_o)
        ctx.sync()
        raw = ctx.to_host(d_o, nb + slack)
    finally:
        ctx.free(d_p)
        ctx.free(d_o)
    assert (raw[nb:] == 0xA5).all(), "bytes behind the results"
    return raw[:nb].view(np.float32).reshape(n_frames, n, 2)


def fields(ctx, call, geoms):
    """The HG_FIELD_COORDS fields of the staged set through call(fmt, d_field, offsets): list of (h, w, 2) float32."""
    offs, total = HG.pack_field_offsets(geoms, CO)
    d = ctx.alloc(max(total, 8))
    try:
        call(CO, d, offs)
        ctx.sync()
        return [ctx.to_host(d, max(g[2], 0) * max(g[3], 0) * 8, offs[f]).view(np.float32).reshape(max(g[3], 0), max(g[2], 0), 2)
                for f, g in enumerate(geoms)]
    finally:
        ctx.free(d)


def anchor(ctx, pcall, fcall, geoms, what):
    """Every integer pixel of the LARGEST window through pcall: inside frame f's window the result is frame f's coords field, bit for bit;
    outside it (and in an empty window) the quiet NaN."""
    mw, mh = max(max(g[2], 0) for g in geoms), max(max(g[3], 0) for g in geoms)
    got = run(ctx, pcall, grid(0, 0, mw, mh), len(geoms)).reshape(len(geoms), mh, mw, 2)
    flds = fields(ctx, fcall, geoms)
    for f, g in enumerate(geoms):
        want = np.full((mh, mw, 2), NAN, np.uint32).view(np.float32)
        want[:max(g[3], 0), :max(g[2], 0)] = flds[f]
        _same(got[f], want, (what, f))
        if g[2] > 0 and g[3] > 0:
            nan = GF.u32(flds[f])[..., 0] == NAN
            assert not nan.all(), (what, f, "nothing mapped")
    return got


# ------------------------------------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def sin_mesh(nx=6, ny=4, amp=7.0):
    sp, tris = WL.grid_points(W, H, nx, ny), WL.grid_triangles(nx, ny)
    return sp, tris, WL.sin_dst(sp, amp, 8), WL.src_min(sp)


def src_box(sp):
    mm = O.minmax_xy(sp)
    return int(mm[0]), int(mm[1]), int(mm[2]), int(mm[3])


def with_nan_triangle(sp, tris, dp):
    """The mesh plus one triangle, listed last, with a NaN destination x: k_tri_setup flags the frame irregular."""
    n = sp.size // 2
    s3 = np.float32([40, 8, 80, 12, 60, 30])
    d3 = np.float32([np.nan, 10, 90, 14, 60, 40])
    return np.concatenate([sp, s3]), np.concatenate([tris, np.uint32([n, n + 1, n + 2])]), np.concatenate([dp, d3])


GEO_INV = [(0, [0.9, 0.05, -0.1, 1.1, 3.25, -2.5, 0, 0]), (1, [1.02, 0.03, -4.0, -0.02, 0.97, 2.5, 1e-4, -2e-4])]
GEO_FWD = [(0, [0.8317, 0.1093, -0.0719, 0.9133, 5.3071, 2.2113, 0, 0]), (1, [0.9013, 0.0417, 3.0331, -0.0309, 0.8821, 4.0173, 2.1e-4, 1.3e-4])]


def fractional(seed, x0, y0, w, h):
    """1000 seeded positions over a w x h box from (x0, y0), some outside it by up to 2 pixels, the cell-rule edge values and the non-finite inputs."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(x0 - 2, x0 + w + 2, 1000), rng.uniform(y0 - 2, y0 + h + 2, 1000)], 1).astype(np.float32)
    edge = np.float32([[x0 - 0.5, y0], [x0 + w - 0.5, y0], [x0 + 3.5, y0 + 2], [x0, y0 - 0.5], [x0, y0 + h - 0.5], [x0 + 2.5, y0 + 3.5],
                       [np.nan, y0 + 1], [x0 + 1, np.nan], [np.inf, y0 + 1], [-np.inf, y0 + 1], [x0 + 1, np.inf], [1e30, y0 + 1], [x0 + 1, -1e30],
                       [-0.0, 0.0]])
    return np.concatenate([p, edge])


# ------------------------------------------------------------------------------------------------ field anchor
def test_field_anchor_geometric(ctx):
    ctx.set_image(WL.lcg_image(W, H, 3))
    geoms = [WIN, WIN, (WIN[0], WIN[1], 0, WIN[3]), WIN]                 # an empty window among them
    for kind, _ in GEO_INV:
        mats = np.array([GEO_INV[kind][1]] * 4, np.float64)
        mats[:, 2 if kind else 4] += 0.75 * np.arange(4)                 # different matrices: the x translation moves with the frame
        ctx.geometric_set_frames(kind, mats, geoms)
        anchor(ctx, ctx.points_to_source_geometric_frames_device, ctx.field_inverse_geometric_frames_device, geoms, ("matrices", kind))
    # frames given as point sets: the matrices are solved on the device first
    s4 = WL.corners(W, H)
    d4s = [WL.projective_dst(W, H, 0.03 * k) for k in range(3)]
    ctx.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, 3), [WIN] * 3)
    anchor(ctx, ctx.points_to_source_geometric_frames_device, ctx.field_inverse_geometric_frames_device, [WIN] * 3, "point sets")


def test_field_anchor_piecewise(ctx):
    sp, tris, dp, (msx, msy) = sin_mesh()
    ctx.set_image(WL.lcg_image(W, H, 3))
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    dsts = [WL.sin_dst(sp, 5.0 + 2 * f, 8 + f) for f in range(3)] + [dp]
    geoms = [WIN, WL.piecewise_geom(dsts[1]), WIN, (WIN[0], WIN[1], WIN[2], 0)]
    ctx.piecewise_set_frames(np.concatenate(dsts), geoms)
    anchor(ctx, ctx.points_to_source_piecewise_frames_device, ctx.field_inverse_piecewise_frames_device, geoms, "piecewise set")


def test_field_anchor_frames_with_their_own_source_points(ctx):
    ms = M.set_a(-12, 3)
    ctx.set_image(ms.imgs[0])
    ctx.piecewise_set_mesh(ms.base, ms.tris, *WL.src_min(ms.base))
    ctx.piecewise_set_frames_src(ms.src_all, ms.min_all, ms.dst_all, ms.geoms)
    assert len(set(ms.mins)) > 1
    got = anchor(ctx, ctx.points_to_source_piecewise_frames_device, ctx.field_inverse_piecewise_frames_device, ms.geoms, "own source")
    f = 1                                                                # ... and one frame against the model over the oracle's taps
    _, _, _, wmap, _, inv = ms.want(f, 1)
    g = ms.geoms[f]
    mw, mh = got.shape[2], got.shape[1]
    _same(got[f], P.to_source_piecewise(wmap, inv, grid(0, 0, mw, mh), g, ms.W, ms.H, *ms.mins[f]), "own source, model")


@pytest.mark.parametrize("name", ["fold_over", "fold_over_neg"])
def test_field_anchor_folded_and_wrapping_meshes(ctx, name):
    """Where "largest id wins" (fold_over) and the second image of a span, fill()'s wrap of negative indices (fold_over_neg), decide."""
    sp, tris, msx, msy, dp, geom, img = FO.case(name)
    ctx.set_image(img)
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    ctx.piecewise_set_frames(dp, [geom])
    got = anchor(ctx, ctx.points_to_source_piecewise_frames_device, ctx.field_inverse_piecewise_frames_device, [geom], name)
    _, wmap, _, inv, _, _, _ = FO.taps(name)
    _same(got[0], P.to_source_piecewise(wmap, inv, grid(0, 0, geom[2], geom[3]), geom, FO.W, FO.H, msx, msy), (name, "model"))


# ------------------------------------------------------------------------------------------------ fractional points
@pytest.mark.parametrize("kind", (0, 1))
def test_fractional_points_geometric(ctx, kind):
    ctx.set_image(WL.lcg_image(W, H, 3))
    geoms = [WIN, (4, -2, W - 20, H - 7)]
    inv = np.array([GEO_INV[kind][1], GEO_INV[kind][1]], np.float64)
    inv[1, 2 if kind else 4] += 1.5
    ctx.geometric_set_frames(kind, inv, geoms)
    pts = fractional(11 + kind, 0, 0, WIN[2], WIN[3])
    got = run(ctx, ctx.points_to_source_geometric_frames_device, pts, 2)
    for f in range(2):
        want = P.to_source_geometric(kind, inv[f], pts, geoms[f], W, H)
        nan = (GF.u32(want) == NAN).all(1)
        assert nan[1000:].sum() >= 8 and 100 < nan[:1000].sum() < 1000
        _same(got[f], want, ("to source", kind, f))
    fwd = np.array([GEO_FWD[kind][1], GEO_FWD[kind][1]], np.float64)
    fwd[1, 2 if kind else 4] -= 2.25
    pts = fractional(21 + kind, 0, 0, W, H)
    got = run(ctx, lambda p, n, s, o: ctx.points_to_output_geometric_batch_device(kind, fwd, geoms, p, n, s, o), pts, 2)
    for f in range(2):
        want = P.to_output_geometric(kind, fwd[f], pts, geoms[f], W, H)
        assert 0 < (GF.u32(want) == NAN).all(1).sum() < 400
        _same(got[f], want, ("to output", kind, f))
    # one list per frame (n_sets = F): frame f reads list f, in both directions
    lists = np.stack([fractional(31 + kind, 0, 0, W, H), fractional(41 + kind, 0, 0, W, H)])
    assert not np.array_equal(GF.u32(lists[0]), GF.u32(lists[1]))
    got = run(ctx, ctx.points_to_source_geometric_frames_device, lists, 2, 2)
    gout = run(ctx, lambda p, n, s, o: ctx.points_to_output_geometric_batch_device(kind, fwd, geoms, p, n, s, o), lists, 2, 2)
    for f in range(2):
        _same(got[f], P.to_source_geometric(kind, inv[f], lists[f], geoms[f], W, H), ("to source, own list", kind, f))
        _same(gout[f], P.to_output_geometric(kind, fwd[f], lists[f], geoms[f], W, H), ("to output, own list", kind, f))
        assert not np.array_equal(GF.u32(got[f]), GF.u32(P.to_source_geometric(kind, inv[f], lists[1 - f], geoms[f], W, H)))


def test_fractional_points_piecewise(ctx):
    sp, tris, dp, (msx, msy) = sin_mesh()
    img = WL.lcg_image(W, H, 3)
    ctx.set_image(img)
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    dsts = [dp, WL.sin_dst(sp, 4.0, 9)]
    geoms = [WL.piecewise_geom(dsts[0]), WIN]
    ctx.piecewise_set_frames(np.concatenate(dsts), geoms)
    pts = fractional(31, 0, 0, WIN[2], WIN[3])
    got = run(ctx, ctx.points_to_source_piecewise_frames_device, pts, 2)
    for f in range(2):
        want = P.to_source_piecewise_mesh(sp, dsts[f], tris, pts, geoms[f], W, H, msx, msy)
        assert 100 < (GF.u32(want) == NAN).all(1).sum() < 1000
        _same(got[f], want, ("to source", f))
    x0, y0, x1, y1 = src_box(sp)
    pts = fractional(41, x0, y0, x1 - x0, y1 - y0)
    got = run(ctx, lambda p, n, s, o: ctx.points_to_output_piecewise_batch_device(np.concatenate(dsts), x1, y1, geoms, p, n, s, o), pts, 2)
    fmap = P.forward_map(sp, tris, x0, y0, x1, y1)
    for f in range(2):
        want = P.to_output_piecewise(fmap, O.piecewise_matrices(sp, dsts[f], tris), pts, geoms[f], x0, y0, x1, y1)
        assert 0 < (GF.u32(want) == NAN).all(1).sum() < 400
        _same(got[f], want, ("to output", f))


# ------------------------------------------------------------------------------------------------ block and chunk tails, list sets
def test_block_and_chunk_tails_and_list_sets(ctx):
    """N around the 64-lane wave and the 256-point block; a mesh of 257 triangles -- 256 grid triangles and one more on top of them, listed
    last -- which is one more than k_pw_points_src stages per step; n_sets 1, F and a value that does not divide F."""
    nx, ny = 16, 8                                                       # 256 triangles
    sp, tris = WL.grid_points(W, H, nx, ny), WL.grid_triangles(nx, ny)
    n = sp.size // 2                                                     # + one triangle on top of the others, listed last: id 256 wins there
    sp = np.concatenate([sp, np.float32([20, 10, 60, 14, 40, 50])])
    tris = np.concatenate([tris, np.uint32([n, n + 1, n + 2])])
    assert tris.size // 3 == 257
    F = 3
    dsts = [np.concatenate([WL.sin_dst(sp[:2 * n], 3.0 + f, 8), np.float32([30 + f, 20, 90, 24, 50, 70])]) for f in range(F)]
    msx, msy = WL.src_min(sp)
    ctx.set_image(WL.lcg_image(W, H, 3))
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    ctx.piecewise_set_frames(np.concatenate(dsts), [WIN] * F)
    x0, y0, x1, y1 = src_box(sp)
    fmap = P.forward_map(sp, tris, x0, y0, x1, y1)
    rng = np.random.default_rng(51)
    for N in (1, 63, 64, 255, 257):
        for n_sets in (1, F, 2):
            pts = np.stack([rng.uniform(-2, WIN[2] + 2, (n_sets, N)), rng.uniform(-2, WIN[3] + 2, (n_sets, N))], -1).astype(np.float32)
            ctx.piecewise_set_frames(np.concatenate(dsts), [WIN] * F)
            got = run(ctx, ctx.points_to_source_piecewise_frames_device, pts, F, n_sets)
            gout = run(ctx, lambda p, k, s, o: ctx.points_to_output_piecewise_batch_device(np.concatenate(dsts), x1, y1, [WIN] * F, p, k, s, o),
                       pts, F, n_sets)
            for f in range(F):
                own = pts[f % n_sets]
                want = P.to_source_piecewise_mesh(sp, dsts[f], tris, own, WIN, W, H, msx, msy)
                _same(got[f], want, ("to source", N, n_sets, f))
                _same(gout[f], P.to_output_piecewise(fmap, O.piecewise_matrices(sp, dsts[f], tris), own, WIN, x0, y0, x1, y1), ("to output", N, n_sets, f))
    # the last triangle is seen: points inside it resolve to id 256
    inside = np.float32([[(30 + 90 + 50) / 3 - WIN[0], (20 + 24 + 70) / 3 - WIN[1]]])
    wmap = O.build_tri_map(dsts[0], tris, WIN[2], WIN[1], WIN[2] * WIN[3])
    cx, cy = P.cells(inside)
    assert wmap[int(cy[0]) * WIN[2] + int(cx[0])] == 256
    ctx.piecewise_set_frames(np.concatenate(dsts), [WIN] * F)
    _same(run(ctx, ctx.points_to_source_piecewise_frames_device, inside, F)[0],
          P.to_source_piecewise_mesh(sp, dsts[0], tris, inside, WIN, W, H, msx, msy), "id 256")


# ------------------------------------------------------------------------------------------------ redo through the map
def test_irregular_frames_are_redone_through_the_map(ctx):
    sp, tris, dp, (msx, msy) = sin_mesh()
    sp2, tr2, dp2 = with_nan_triangle(sp, tris, dp)
    clean2 = np.concatenate([WL.sin_dst(sp, 5.0, 9), dp2[-6:]])
    clean2[-6] = 20.0                                                    # the same triangle with a finite vertex: this frame is not flagged
    assert WL.src_min(sp2) == (msx, msy)
    ctx.set_image(WL.lcg_image(W, H, 3))
    ctx.piecewise_set_mesh(sp2, tr2, msx, msy)
    dsts, geoms = [dp2, clean2, dp2], [WIN, WIN, WL.piecewise_geom(dp)]
    ctx.piecewise_set_frames(np.concatenate(dsts), geoms)
    pts = np.concatenate([grid(0, 0, WIN[2], WIN[3]), fractional(61, 0, 0, WIN[2], WIN[3])])
    r0 = ctx.redone_frames()
    got = run(ctx, ctx.points_to_source_piecewise_frames_device, pts, 3)
    assert ctx.redone_frames() == r0 + 2                                 # frames 0 and 2
    for f in range(3):
        _same(got[f], P.to_source_piecewise_mesh(sp2, dsts[f], tr2, pts, geoms[f], W, H, msx, msy), ("redo", f))
    # one list per frame (n_sets = F): a redone frame reads its own list, not the first
    lists = np.stack([fractional(62 + f, 0, 0, WIN[2], WIN[3]) for f in range(3)])
    r0 = ctx.redone_frames()
    own = run(ctx, ctx.points_to_source_piecewise_frames_device, lists, 3, 3)
    assert ctx.redone_frames() == r0 + 2
    for f in range(3):
        _same(own[f], P.to_source_piecewise_mesh(sp2, dsts[f], tr2, lists[f], geoms[f], W, H, msx, msy), ("redo, own list", f))
    assert not np.array_equal(GF.u32(own[2]), GF.u32(P.to_source_piecewise_mesh(sp2, dsts[2], tr2, lists[0], geoms[2], W, H, msx, msy)))
    # the unflagged mesh without that triangle agrees wherever the triangle covers nothing
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    ctx.piecewise_set_frames(dp, [WIN])
    r0 = ctx.redone_frames()
    plain = run(ctx, ctx.points_to_source_piecewise_frames_device, pts, 1)[0]
    assert ctx.redone_frames() == r0
    alone = O.build_tri_map(dp2, tr2[-3:], WIN[2], WIN[1], WIN[2] * WIN[3]) >= 0
    cx, cy = P.cells(pts)
    ins = P._inside(cx, cy, 0, 0, WIN[2], WIN[3])
    free = ~ins
    free[ins] = ~alone[cy[ins].astype(np.int64) * WIN[2] + cx[ins].astype(np.int64)]
    assert free.sum() > pts.shape[0] // 2
    assert np.array_equal(GF.u32(plain)[free], GF.u32(got[0])[free])


# ------------------------------------------------------------------------------------------------ to output, piecewise
def test_to_output_piecewise_paints_the_forward_warp_and_reuses_the_map(ctx):
    sp, tris, dp, (msx, msy) = sin_mesh()
    img = WL.lcg_image(W, H, 9)
    x0, y0, x1, y1 = src_box(sp)
    g = WL.piecewise_geom(dp)
    ctx.set_image(img)
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    before = ctx.warp_forward_piecewise(dp, x1, y1, g)
    fmap, fwd = P.forward_map(sp, tris, x0, y0, x1, y1), O.piecewise_matrices(sp, dp, tris)
    assert np.array_equal(before, O.warp_forward_piecewise(fmap, fwd, img, x0, y0, x1, y1, *g))
    pts = grid(x0, y0, x1 - x0, y1 - y0)
    call = lambda p, n, s, o: ctx.points_to_output_piecewise_batch_device(dp, x1, y1, [g], p, n, s, o)      # noqa: E731
    res = run(ctx, call, pts, 1)[0]
    again = run(ctx, call, pts, 1)[0]                                    # the cached forward map
    assert np.array_equal(GF.u32(res), GF.u32(again))
    _same(res, P.to_output_piecewise(fmap, fwd, pts, g, x0, y0, x1, y1), "model")
    x, y, ok = P.to_output_piecewise(fmap, fwd, pts, g, x0, y0, x1, y1, raw=True)
    p64 = pts.astype(np.int64)
    vals = img.reshape(-1, 4)[p64[:, 1] * W + p64[:, 0]]
    painted, left_out = P.paint(res, vals, g[2], g[3], exact=(x, y))
    print("painted at the f64 position:", left_out, "of", int(ok.sum()))
    assert left_out <= CAP * ok.sum()
    assert np.array_equal(painted, before)
    # ... and against the forward index field: the gather through it is the same picture
    fld = ctx.field_forward_piecewise(dp, x1, y1, g)
    gathered = np.where((fld >= 0)[..., None], img.reshape(-1, 4)[np.where(fld >= 0, fld, 0)], 0).astype(np.uint8)
    assert np.array_equal(painted, gathered)
    assert np.array_equal(ctx.warp_forward_piecewise(dp, x1, y1, g), before)


# ------------------------------------------------------------------------------------------------ neutrality
def _taps(ctx):
    return (ctx.last_piecewise_kernel(), ctx.last_piecewise_variant(), ctx.last_piecewise_self(), ctx.last_geometric_kernel(),
            ctx.last_forward_kernel(), ctx.last_forward_field_kernel(), ctx.sampling, ctx.layout_walks())


def test_points_calls_leave_the_taps_the_mode_and_the_layout_alone(ctx):
    sp, tris, dp, (msx, msy) = sin_mesh()
    img = WL.lcg_image(W, H, 3)
    x0, y0, x1, y1 = src_box(sp)
    g = WL.piecewise_geom(dp)
    ctx.set_sampling(HG.SAMPLE_BILINEAR)
    try:
        ctx.set_image(img)
        ctx.piecewise_set_mesh(sp, tris, msx, msy)
        ctx.warp_forward_piecewise(dp, x1, y1, g)
        ctx.field_forward_piecewise(dp, x1, y1, g)
        ctx.warp_inverse_geometric(0, np.array(GEO_INV[0][1][:6]), WIN)
        ctx.geometric_set_frames(0, np.array([GEO_INV[0][1]]), [WIN])
        ctx.piecewise_prepare(dp, g)
        ctx.warp_inverse_piecewise()
        taps = _taps(ctx)
        assert taps[0] != 0 and taps[3] != -1 and taps[4] != 0 and taps[5] != 0
        pts = fractional(71, 0, 0, g[2], g[3])
        run(ctx, ctx.points_to_source_piecewise_frames_device, pts, 1)
        assert _taps(ctx) == taps
        run(ctx, ctx.points_to_source_geometric_frames_device, pts, 1)
        assert _taps(ctx) == taps
        run(ctx, lambda p, n, s, o: ctx.points_to_output_geometric_batch_device(0, np.array([GEO_FWD[0][1]]), [WIN], p, n, s, o), pts, 1)
        assert _taps(ctx) == taps
        run(ctx, lambda p, n, s, o: ctx.points_to_output_piecewise_batch_device(dp, x1, y1, [g], p, n, s, o), pts, 1)
        assert _taps(ctx) == taps                                        # (it stages its frame set without a host walk over the triangles)
    finally:
        ctx.set_sampling(HG.SAMPLE_NEAREST)


def test_a_queued_flagged_batch_is_settled_by_the_points_call(ctx):
    sp, tris, dp, (msx, msy) = sin_mesh()
    sp2, tr2, dp2 = with_nan_triangle(sp, tris, dp)
    img = WL.lcg_image(W, H, 3)
    ctx.set_sampling(HG.SAMPLE_NEAREST)
    ctx.set_image(img)
    ctx.piecewise_set_mesh(sp2, tr2, msx, msy)
    want = O.warp_inverse_piecewise(sp2, dp2, tr2, img, msx, msy, *WIN)
    offs, total = HG.pack_offsets([WIN])
    d = ctx.alloc(total)
    try:
        ctx.piecewise_set_frames(dp2, [WIN], offs)
        ctx.warp_inverse_piecewise_frames_device(d)                      # queued; its flagged frame is redone when the run is settled
        pts = fractional(81, 0, 0, WIN[2], WIN[3])
        got = run(ctx, ctx.points_to_source_piecewise_frames_device, pts, 1)[0]
        _same(got, P.to_source_piecewise_mesh(sp2, dp2, tr2, pts, WIN, W, H, msx, msy), "points behind a queued batch")
        ctx.sync()
        assert np.array_equal(ctx.to_host(d, WIN[2] * WIN[3] * 4).reshape(WIN[3], WIN[2], 4), want)
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    INVALID, STATE = 1, 4
    m8 = np.array([[1, 0, 0, 1, 0, 0, 0, 0]], np.float64)
    g = (0, 0, 8, 8)
    sp, tris = WL.grid_points(16, 16, 2, 2), WL.grid_triangles(2, 2)
    with HG.Context(0) as c:
        c._n_pts = sp.size // 2
        d = c.alloc(4096)
        try:
            src_g, src_p = c.points_to_source_geometric_frames_device, c.points_to_source_piecewise_frames_device
            out_g = lambda *a: c.points_to_output_geometric_batch_device(0, m8, [g], *a)        # noqa: E731
            out_p = lambda *a: c.points_to_output_piecewise_batch_device(sp, 16, 16, [g], *a)   # noqa: E731
            calls = (src_g, src_p, out_g, out_p)
            for fn in calls:                                             # no image / mesh / frame set yet
                assert GF.refusal_code(fn, d, 4, 1, d + 1024) == STATE
                fn(d, 0, 1, d + 1024)                                    # n_points == 0: nothing happens, whatever the state
                fn(0, 0, 1, 0)
            c.set_image(WL.lcg_image(16, 16, 1))
            assert GF.refusal_code(src_g, d, 4, 1, d + 1024) == STATE              # no frame set
            assert GF.refusal_code(src_p, d, 4, 1, d + 1024) == STATE              # no mesh
            assert GF.refusal_code(out_p, d, 4, 1, d + 1024) == STATE
            c.piecewise_set_mesh(sp, tris, 0, 0)
            assert GF.refusal_code(src_p, d, 4, 1, d + 1024) == STATE              # no frame set
            c.piecewise_prepare(sp, (0, 0, 16, 16))
            c.geometric_set_frames(0, m8, [g])
            for fn in calls:
                assert GF.refusal_code(fn, 0, 4, 1, d + 1024) == INVALID           # NULL pointers with work to do
                assert GF.refusal_code(fn, d, 4, 1, 0) == INVALID
                assert GF.refusal_code(fn, d, -1, 1, d + 1024) == INVALID
                assert GF.refusal_code(fn, d, (1 << 24) + 1, 1, d + 1024) == INVALID
                assert GF.refusal_code(fn, d, 4, 0, d + 1024) == INVALID
                assert GF.refusal_code(fn, d + 4, 4, 1, d + 1024) == INVALID       # misaligned
                assert GF.refusal_code(fn, d, 4, 1, d + 1028) == INVALID
            assert GF.refusal_code(c.points_to_output_geometric_batch_device, 2, m8, [g], d, 4, 1, d + 1024) == INVALID     # unknown kind
            # the context still works
            pts = np.float32([[1, 2], [3.5, 4.25], [7.5, 0], [15.5, 3], [np.nan, 0]])
            fmap, fwd = P.forward_map(sp, tris, 0, 0, 16, 16), O.piecewise_matrices(sp, sp, tris)
            want = {src_g: P.to_source_geometric(0, m8[0], pts, g, 16, 16), src_p: P.to_source_piecewise_mesh(sp, sp, tris, pts, (0, 0, 16, 16), 16, 16, 0, 0),
                    out_g: P.to_output_geometric(0, m8[0], pts, g, 16, 16), out_p: P.to_output_piecewise(fmap, fwd, pts, g, 0, 0, 16, 16)}
            for fn in calls:
                nan = (GF.u32(want[fn]) == NAN).all(1)
                assert nan[4] and not nan[:2].any(), want[fn]
                _same(run(c, fn, pts, 1)[0], want[fn], "after the refusals")
        finally:
            c.free(d)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_transform_points():
    """tests/js/points_gpu.mjs: transformPoints() of js/Homography.mjs on the real addon, both directions, the three transforms; the ctypes
    calls on the same state give the same bits."""
    res = GF.run_node_case("points_gpu.mjs")
    W2, H2 = res["W"], res["H"]
    pts_src, pts_out = np.float32(res["points_source"]), np.float32(res["points_output"])
    with HG.Context(0) as c:
        c.set_image(WL.lcg_image(W2, H2, res["seed"]))
        for name, rep in res["report"].items():
            g = tuple(rep["geom"])
            if name == "piecewise":
                sp, dp, tris = np.float32(rep["src"]), np.float32(rep["dst"]), np.uint32(rep["tris"])
                c.piecewise_set_mesh(sp, tris, *rep["min_src"])
                c.piecewise_set_frames(dp, [g])
                to_src = run(c, c.points_to_source_piecewise_frames_device, pts_src, 1)[0]
                to_out = run(c, lambda p_, n, s, o: c.points_to_output_piecewise_batch_device(dp, rep["max_src"][0], rep["max_src"][1], [g], p_, n, s, o),
                             pts_out, 1)[0]
            else:
                kind = 0 if name == "affine" else 1
                inv, fwd = np.zeros((1, 8)), np.zeros((1, 8))
                inv[0, :len(rep["inverse"])] = rep["inverse"]
                fwd[0, :len(rep["forward"])] = rep["forward"]
                c.geometric_set_frames(kind, inv, [g])
                to_src = run(c, c.points_to_source_geometric_frames_device, pts_src, 1)[0]
                to_out = run(c, lambda p_, n, s, o: c.points_to_output_geometric_batch_device(kind, fwd, [g], p_, n, s, o), pts_out, 1)[0]
            _same(np.array(rep["to_source_bits"], np.uint32).view(np.float32), to_src, (name, "to source"))
            _same(np.array(rep["to_output_bits"], np.uint32).view(np.float32), to_out, (name, "to output"))
    assert set(res["report"]) == {"affine", "projective", "piecewise"}
