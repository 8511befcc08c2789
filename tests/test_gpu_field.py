"""The source fields of the inverse warps and the remaps through them on the GPU (include/hgwarp.h, HG_FIELD_*) against the numpy model of
tests/hgtest/field.py, byte for byte (coordinates are compared as uint32 views).  The model's piecewise maps and inverse matrices come from
the CPU oracle's taps, never from the library under test; tests/test_field_cpu.py pins the model itself to the reference."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import bilinear as B             # noqa: E402
from hgtest import edges as E                # noqa: E402
from hgtest import field as FM               # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import moving as M               # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
IDX, CO = HG.FIELD_INDEX, HG.FIELD_COORDS
NEAR, BIL = HG.SAMPLE_NEAREST, HG.SAMPLE_BILINEAR
PX = {IDX: 4, CO: 8}


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    """Bit-equal fields.  On a mismatch: how many pixels, and the first few (row, col, got, want)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = GF.u32(got), GF.u32(want)
    if not np.array_equal(g, w):
        diff = g != w
        bad = np.argwhere(diff.any(-1) if diff.ndim == 3 else diff)
        first = [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ; (row, col, got, want): {first}")


def _model(sx, sy, valid, img, msx=0, msy=0):
    H, W = img.shape[:2]
    return {IDX: FM.index_field(sx, sy, valid, W, H, msx, msy), CO: FM.coords_field(sx, sy, valid, W, H, msx, msy)}


def _gather(idx, img):
    return FM.remap_index(idx, img.reshape(-1, 4)).reshape(idx.shape + (4,))


def _field_from(raw, fmt, g):
    """The (h, w[, 2]) field of window g out of downloaded bytes."""
    return raw.view(np.int32).reshape(g[3], g[2]) if fmt == IDX else raw.view(np.float32).reshape(g[3], g[2], 2)


def _pw_setup(ctx, case):
    sp, tris, msx, msy, dp, geom, img = case
    ctx.set_image(img)
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    ctx.piecewise_prepare(dp, geom)


@functools.lru_cache(maxsize=None)
def _pw_edge(name, twin):
    case = E.piecewise(name, twin)
    out, wmap, inv, sx, sy, valid = E.piecewise_taps(case)
    for a in (out, sx, sy, valid):
        a.setflags(write=False)
    return case, out, sx, sy, valid


# ------------------------------------------------------------------------------------------------ 1, 2: the edge cases
@pytest.mark.parametrize("name", sorted(E.GEOMETRIC))
def test_geometric_edge_cases(ctx, name):
    case = E.GEOMETRIC[name]()
    kind, m, img, geom = case
    sx, sy, valid = E.geometric_coords(case)
    want = _model(sx, sy, valid, img)
    ctx.set_sampling(NEAR)
    ctx.set_image(img)
    got = {fmt: ctx.field_inverse_geometric(kind, m, geom, fmt) for fmt in (IDX, CO)}
    for fmt in (IDX, CO):
        _same(got[fmt], want[fmt], (name, fmt))
    assert np.array_equal(_gather(got[IDX], img), ctx.warp_inverse_geometric(kind, m, geom)), name


@pytest.mark.parametrize("twin", (False, True))
@pytest.mark.parametrize("name", sorted(E.PIECEWISE))
def test_piecewise_edge_cases(ctx, name, twin):
    case, out, sx, sy, valid = _pw_edge(name, twin)
    sp, tris, msx, msy, dp, geom, img = case
    H, W = img.shape[:2]
    want = _model(sx, sy, valid, img, msx, msy)
    ctx.set_sampling(NEAR)
    _pw_setup(ctx, case)
    got = {fmt: ctx.field_inverse_piecewise(fmt) for fmt in (IDX, CO)}
    for fmt in (IDX, CO):
        _same(got[fmt], want[fmt], (name, twin, fmt))
    warped = ctx.warp_inverse_piecewise()
    assert np.array_equal(warped, out) and np.array_equal(_gather(got[IDX], img), warped), (name, twin)
    # covered pixels whose flat index leaves the array: -1 in the index field, a real coordinate in the other
    cov = FM.covered(sx, sy, valid, W, H, msx, msy)
    raw = np.where(cov, E.js_round(np.where(cov, sy, 0)) * W + E.js_round(np.where(cov, sx, 0)), 0)
    neg, past = cov & (raw < 0), cov & (raw >= W * H)
    if name in ("neg", "negy"):
        assert neg.any(), name
    if name == "pos":
        assert past.any(), name
    outside = neg | past
    assert (got[IDX][outside] == -1).all() and not np.isnan(got[CO][outside]).any(), (name, twin)


# ------------------------------------------------------------------------------------------------ 3: lane-map tails
def test_lane_map_tails(ctx):
    """An affine half-pixel shift over windows around the 64-lane store and the 256-pixel window, at negative offsets: nothing is written
    past obj_w (the row after it, and the bytes behind the frame, stay as they were)."""
    img = WL.lcg_image(300, 9, 61)
    m = np.array([1, 0, 0, 1, 0.5, 0.5], np.float64)
    ctx.set_sampling(NEAR)
    ctx.set_image(img)
    slack = 256
    d = ctx.alloc(257 * 5 * 8 + slack)
    try:
        for w in (1, 3, 63, 64, 65, 255, 257):
            for h in (1, 5):
                g = (-2, -1, w, h)
                sx, sy = B.geometric_coords(0, m, *g)
                want = _model(sx, sy, np.ones(sx.shape, bool), img)
                for fmt in (IDX, CO):
                    _same(ctx.field_inverse_geometric(0, m, g, fmt), want[fmt], ("host", w, h, fmt))
                    n = w * h * PX[fmt]
                    ctx.to_device(d, np.full(n + slack, 0xA5, np.uint8))
                    ctx.field_inverse_geometric_device(0, m, g, fmt, d)
                    ctx.sync()
                    raw = ctx.to_host(d, n + slack)
                    _same(_field_from(raw[:n], fmt, g), want[fmt], ("device", w, h, fmt))
                    assert (raw[n:] == 0xA5).all(), ("bytes behind the frame", w, h, fmt)
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ 4: general transforms
W4, H4 = 200, 120


@functools.lru_cache(maxsize=None)
def _projective4():
    img = WL.lcg_image(W4, H4, 71)
    s4, d4 = WL.corners(W4, H4), WL.projective_dst(W4, H4)
    m = O.projective_from_squares(d4, s4)
    g = tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W4, H4))
    sx, sy = B.geometric_coords(1, m, *g)
    return img, m, g, sx, sy


@functools.lru_cache(maxsize=None)
def _sin_mesh4():
    img = WL.lcg_image(W4, H4, 72)
    sp, tris = WL.grid_points(W4, H4, 6, 4), WL.grid_triangles(6, 4)
    dp = WL.sin_dst(sp, 9.0, 8)
    g = WL.piecewise_geom(dp)
    msx, msy = WL.src_min(sp)
    out, wmap, _, inv = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *g, taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *g)
    return (sp, tris, msx, msy, dp, g, img), out, sx, sy, valid


def test_general_projective_and_sin_mesh(ctx):
    ctx.set_sampling(NEAR)
    img, m, g, sx, sy = _projective4()
    valid = np.ones(sx.shape, bool)
    cov = FM.covered(sx, sy, valid, W4, H4)
    assert cov.any() and not cov.all()
    want = _model(sx, sy, valid, img)
    ctx.set_image(img)
    for fmt in (IDX, CO):
        _same(ctx.field_inverse_geometric(1, m, g, fmt), want[fmt], ("projective", fmt))
    case, out, sx, sy, valid = _sin_mesh4()
    msx, msy, img = case[2], case[3], case[6]
    cov = FM.covered(sx, sy, valid, W4, H4, msx, msy)
    assert cov.any() and not cov.all()
    want = _model(sx, sy, valid, img, msx, msy)
    _pw_setup(ctx, case)
    for fmt in (IDX, CO):
        _same(ctx.field_inverse_piecewise(fmt), want[fmt], ("sin mesh", fmt))
    assert np.array_equal(_gather(want[IDX], img), out)


# ------------------------------------------------------------------------------------------------ 5: frame sets
def _gapped(geoms, fmt):
    """Explicit field offsets that leave gaps: the packed layout with 512 * (f + 1) more bytes in front of frame f, and a tail."""
    packed, total = HG.pack_field_offsets(geoms, fmt)
    return [o + 512 * (f + 1) for f, o in enumerate(packed)], total + 512 * (len(geoms) + 2)


def _check_set(ctx, run, geoms, fmt, singles, what):
    """run(fmt, d_field, offs) into a buffer pre-filled with 0xA5: every frame equals singles[f], every other byte stays 0xA5."""
    offs, total = _gapped(geoms, fmt)
    d = ctx.alloc(total)
    try:
        ctx.to_device(d, np.full(total, 0xA5, np.uint8))
        run(fmt, d, offs)
        ctx.sync()
        raw = ctx.to_host(d, total)
    finally:
        ctx.free(d)
    untouched = np.ones(total, bool)
    for f, g in enumerate(geoms):
        n = max(g[2], 0) * max(g[3], 0) * PX[fmt]
        untouched[offs[f]:offs[f] + n] = False
        if n:
            _same(_field_from(raw[offs[f]:offs[f] + n], fmt, g), singles[f], (what, fmt, f))
    assert (raw[untouched] == 0xA5).all(), (what, fmt, "gaps and tail")
    return raw, offs


def test_geometric_frame_sets(ctx):
    W, H, F = 256, 160, 5
    img = WL.lcg_image(W, H, 81)
    ctx.set_sampling(NEAR)
    ctx.set_image(img)
    s4 = WL.corners(W, H)
    d4s = [WL.projective_dst(W, H, 0.03 * k) for k in range(F)]
    gg = [tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W, H)) for d4 in d4s]
    gg = [(g[0] - 3 * f, g[1] + f - 2, g[2] - 11 * f, g[3] - 5 * f) for f, g in enumerate(gg)]      # different windows (negative offsets, odd widths)
    gg[3] = (gg[3][0], gg[3][1], 0, gg[3][3])                # an empty frame in the middle
    a3s = np.array([0, 0, 0, H, W, 0], np.float32)
    a3d = [WL.affine_dst(W, H, 0.01 * k) for k in range(F)]
    ma = [HG.solve_affine(d, a3s).astype(np.float64) for d in a3d]
    ag = [tuple(int(v) for v in O.transform_limits(0, O.affine_from_triangles(a3s, d).astype(np.float64), W, H)) for d in a3d]
    assert len(set(gg)) == F and len(set(ag)) == F          # different windows
    for fmt in (IDX, CO):
        singles = [ctx.field_inverse_geometric(1, HG.solve_projective(d4s[f], s4), gg[f], fmt) for f in range(F)]
        for f in (0, 4):                                     # ... which are the model's
            sx, sy = B.geometric_coords(1, O.projective_from_squares(d4s[f], s4), *gg[f])
            _same(singles[f], _model(sx, sy, np.ones(sx.shape, bool), img)[fmt], ("projective single", fmt, f))
        ctx.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg)       # device-solved matrices
        _check_set(ctx, ctx.field_inverse_geometric_frames_device, gg, fmt, singles, "projective points")
        singles = [ctx.field_inverse_geometric(0, ma[f], ag[f], fmt) for f in range(F)]
        mats = np.zeros((F, 8))
        mats[:, :6] = ma
        ctx.geometric_set_frames(0, mats, ag)
        _check_set(ctx, ctx.field_inverse_geometric_frames_device, ag, fmt, singles, "affine")
    # packed layout (offsets = None) == hg_pack_field_offsets
    offs, total = HG.pack_field_offsets(ag, IDX)
    d = ctx.alloc(total)
    try:
        ctx.field_inverse_geometric_frames_device(IDX, d)
        ctx.sync()
        for f in (0, F - 1):
            got = _field_from(ctx.to_host(d, ag[f][2] * ag[f][3] * 4, offs[f]), IDX, ag[f])
            _same(got, ctx.field_inverse_geometric(0, ma[f], ag[f], IDX), ("affine packed", f))
    finally:
        ctx.free(d)


def test_piecewise_frame_sets_and_one_source_per_frame(ctx):
    W, H, nx, ny, F, NI = 256, 160, 8, 5, 5, 3
    imgs = [WL.lcg_image(W, H, 500 + k) for k in range(NI)]
    sp, tris = WL.grid_points(W, H, nx, ny), WL.grid_triangles(nx, ny)
    frames = [WL.sin_dst(sp, 5.0 + f, 8 + (f % 4)) for f in range(F)]
    geoms = [WL.piecewise_geom(d) for d in frames]
    assert len(set(geoms)) > 1
    msx, msy = WL.src_min(sp)
    ctx.set_sampling(NEAR)
    singles = {IDX: [], CO: []}
    for f in range(F):
        _pw_setup(ctx, (sp, tris, msx, msy, frames[f], geoms[f], imgs[f % NI]))
        for fmt in (IDX, CO):
            singles[fmt].append(ctx.field_inverse_piecewise(fmt))
    out, wmap, _, inv = O.warp_inverse_piecewise(sp, frames[2], tris, imgs[2], msx, msy, *geoms[2], taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *geoms[2])
    for fmt in (IDX, CO):
        _same(singles[fmt][2], _model(sx, sy, valid, imgs[2], msx, msy)[fmt], ("piecewise single", fmt))
    stride = W * H * 4 + 256
    roffs, rtotal = HG.pack_offsets(geoms)
    d_src, d_out = ctx.alloc(stride * NI), ctx.alloc(rtotal)
    try:
        for k in range(NI):
            ctx.to_device(d_src, imgs[k], k * stride)
        ctx.set_images_device(d_src, W, H, NI, stride)
        ctx.piecewise_set_mesh(sp, tris, msx, msy)
        ctx.piecewise_set_frames(np.concatenate(frames), geoms, roffs)
        fields = {}
        for fmt in (IDX, CO):
            fields[fmt] = _check_set(ctx, ctx.field_inverse_piecewise_frames_device, geoms, fmt, singles[fmt], "piecewise set")
        # one source per frame: the index of frame f is relative to image f % 3
        ctx.warp_inverse_piecewise_frames_device(d_out)
        ctx.sync()
        raw, offs = fields[IDX]
        for f, g in enumerate(geoms):
            warped = ctx.to_host(d_out, g[2] * g[3] * 4, roffs[f]).reshape(g[3], g[2], 4)
            idx = _field_from(raw[offs[f]:offs[f] + g[2] * g[3] * 4], IDX, g)
            assert np.array_equal(_gather(idx, imgs[f % NI]), warped), ("gather from image f % 3", f)
            if f == 2:
                assert np.array_equal(warped, out)
    finally:
        ctx.set_image(imgs[0])
        ctx.free(d_out)
        ctx.free(d_src)


def test_frame_set_with_its_own_source_points(ctx):
    ms = M.set_a(-12, 3)
    assert min(v for mn in ms.mins for v in mn) < 0 < max(v for mn in ms.mins for v in mn)      # minima of both signs
    ctx.set_sampling(NEAR)
    ctx.set_image(ms.imgs[0])
    ctx.piecewise_set_mesh(ms.base, ms.tris, *WL.src_min(ms.base))
    want = {IDX: [], CO: []}
    for f in range(ms.F):
        near, _, _, wmap, _, inv = ms.want(f, 1)
        sx, sy, valid = B.piecewise_coords(wmap, inv, *ms.geoms[f])
        mod = _model(sx, sy, valid, ms.imgs[0], *ms.mins[f])
        assert np.array_equal(_gather(mod[IDX], ms.imgs[0]), near)
        ctx.piecewise_set_frames_src(ms.srcs[f], ms.min_all[2 * f:2 * f + 2], ms.dsts[f], [ms.geoms[f]])
        for fmt in (IDX, CO):
            want[fmt].append(mod[fmt])
            _same(ctx.field_inverse_piecewise(fmt), mod[fmt], ("own source, single", fmt, f))
    ctx.piecewise_set_frames_src(ms.src_all, ms.min_all, ms.dst_all, ms.geoms)
    for fmt in (IDX, CO):
        _check_set(ctx, ctx.field_inverse_piecewise_frames_device, ms.geoms, fmt, want[fmt], "own source, set")


# ------------------------------------------------------------------------------------------------ 6, 7: redo through the map, Int16 wrap
def _overflow_mesh():
    """1100 triangles side by side on a 2400 x 8 source: every output row crosses more spans than the general kernel's LDS list holds."""
    n, W2, H2 = 1100, 2400, 8
    img = WL.lcg_image(W2, H2, 10)
    xs = np.linspace(0, W2, n + 1)
    sp = np.stack([np.repeat(xs, 2), np.tile([0.0, H2], n + 1)], 1).astype(np.float32).ravel()
    tr = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(n)], np.uint32).ravel()
    dp = sp.copy()
    dp[1::2] *= 1.5
    mm, md = O.minmax_xy(sp), O.minmax_xy(dp)
    g = (int(md[0]), int(md[1]), int(md[2] - md[0]), int(md[3] - md[1]))
    return img, sp, tr, dp, g, int(mm[0]), int(mm[1])


def test_span_list_overflow_is_redone_through_the_map(ctx):
    img, sp, tr, dp, g, msx, msy = _overflow_mesh()
    out, wmap, _, inv = O.warp_inverse_piecewise(sp, dp, tr, img, msx, msy, *g, taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *g)
    want = _model(sx, sy, valid, img, msx, msy)
    ctx.set_sampling(NEAR)
    _pw_setup(ctx, (sp, tr, msx, msy, dp, g, img))
    for fmt in (IDX, CO):
        r0 = ctx.redone_frames()
        _same(ctx.field_inverse_piecewise(fmt), want[fmt], ("overflow", fmt))
        assert ctx.redone_frames() > r0, fmt
    assert np.array_equal(ctx.warp_inverse_piecewise(), out)


def test_beyond_32767_triangles(ctx):
    sp, tris, msx, msy, dp, geom, img = E.piecewise("pos")
    sp2, tr2, dp2 = E.pad_triangles(sp, tris, dp, geom)
    assert tr2.size // 3 == 32769
    out, wmap, _, inv = O.warp_inverse_piecewise(sp2, dp2, tr2, img, msx, msy, *geom, taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *geom)
    want = _model(sx, sy, valid, img, msx, msy)
    ctx.set_sampling(NEAR)
    _pw_setup(ctx, (sp2, tr2, msx, msy, dp2, geom, img))
    for fmt in (IDX, CO):
        _same(ctx.field_inverse_piecewise(fmt), want[fmt], ("32769 triangles", fmt))
    assert np.array_equal(_gather(want[IDX], img), out)


# ------------------------------------------------------------------------------------------------ 8: independence
def test_fields_are_independent_of_the_sampling_mode_and_leave_the_taps_alone(ctx):
    case, out, sx, sy, valid = _sin_mesh4()
    sp, tris, msx, msy, dp, g, img = case
    pimg, m, pg, _, _ = _projective4()
    ctx.set_sampling(NEAR)
    _pw_setup(ctx, case)
    assert np.array_equal(ctx.warp_inverse_piecewise(), out)
    ctx.set_image(pimg)
    ctx.warp_inverse_geometric(1, m, pg)
    ctx.set_image(img)
    taps = (ctx.last_piecewise_kernel(), ctx.last_piecewise_variant(), ctx.last_piecewise_self(), ctx.last_geometric_kernel(), ctx.last_forward_kernel())
    assert taps[0] != 0 and taps[3] != -1
    got = {}
    for mode in (NEAR, BIL):
        ctx.set_sampling(mode)
        got[mode] = [ctx.field_inverse_piecewise(IDX), ctx.field_inverse_piecewise(CO),
                     ctx.field_inverse_geometric(1, m, pg, IDX), ctx.field_inverse_geometric(1, m, pg, CO)]
        assert ctx.sampling == mode
        assert taps == (ctx.last_piecewise_kernel(), ctx.last_piecewise_variant(), ctx.last_piecewise_self(), ctx.last_geometric_kernel(),
                        ctx.last_forward_kernel())
    for a, b in zip(got[NEAR], got[BIL]):
        assert np.array_equal(GF.u32(a), GF.u32(b))
    ctx.set_sampling(NEAR)
    # a warp run queued before a field call and synced after it keeps its result
    offs, total = HG.pack_offsets([g])
    d = ctx.alloc(total)
    try:
        ctx.piecewise_set_frames(dp, [g], offs)
        ctx.warp_inverse_piecewise_frames_device(d)
        queued = (ctx.last_piecewise_kernel(), ctx.last_piecewise_variant(), ctx.last_piecewise_self())
        fld = ctx.field_inverse_piecewise(IDX)
        assert queued == (ctx.last_piecewise_kernel(), ctx.last_piecewise_variant(), ctx.last_piecewise_self())
        ctx.sync()
        assert np.array_equal(ctx.to_host(d, g[2] * g[3] * 4).reshape(g[3], g[2], 4), out)
        assert np.array_equal(_gather(fld, img), out)
        # ... and the next warp of the set lays itself out as the one before the field call did
        ctx.warp_inverse_piecewise_frames_device(d)
        ctx.sync()
        assert (ctx.last_piecewise_kernel(), ctx.last_piecewise_variant(), ctx.last_piecewise_self()) == queued
        assert np.array_equal(ctx.to_host(d, g[2] * g[3] * 4).reshape(g[3], g[2], 4), out)
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ 9, 10: the remaps
@pytest.mark.parametrize("pixel_bytes", (1, 2, 4, 8, 16))
def test_remap_index_pixel_sizes_and_caller_made_fields(ctx, pixel_bytes):
    n, n_src = 4099, 1031
    rng = np.random.default_rng(90 + pixel_bytes)
    src = rng.integers(0, 256, (n_src, pixel_bytes), dtype=np.uint8)
    fld = rng.integers(-3, n_src + 3, n).astype(np.int32)
    fld[:8] = [-1, n_src, 2 ** 31 - 1, -2 ** 31, 0, n_src - 1, n_src + 1, -2]
    want = FM.remap_index(fld, src)
    assert not want[[0, 1, 2, 3, 6, 7]].any() and np.array_equal(want[4], src[0]) and np.array_equal(want[5], src[-1])
    d_f, d_s, d_o = ctx.alloc(n * 4), ctx.alloc(n_src * pixel_bytes), ctx.alloc(n * pixel_bytes)
    try:
        ctx.to_device(d_f, fld)
        ctx.to_device(d_s, src)
        ctx.to_device(d_o, np.full(n * pixel_bytes, 0xA5, np.uint8))
        ctx.remap_index_device(d_f, n, d_s, n_src, pixel_bytes, d_o)
        ctx.sync()
        got = ctx.to_host(d_o, n * pixel_bytes).reshape(n, pixel_bytes)
    finally:
        for p in (d_f, d_s, d_o):
            ctx.free(p)
    assert np.array_equal(got, want)


def test_remap_index_of_the_rgba_source_is_the_device_warp(ctx):
    img, m, g, sx, sy = _projective4()
    n = g[2] * g[3]
    ctx.set_sampling(NEAR)
    ctx.set_image(img)
    d_f, d_s, d_o, d_w = ctx.alloc(n * 4), ctx.alloc(img.nbytes), ctx.alloc(n * 4), ctx.alloc(n * 4)
    try:
        ctx.to_device(d_s, img)
        ctx.field_inverse_geometric_device(1, m, g, IDX, d_f)
        ctx.remap_index_device(d_f, n, d_s, W4 * H4, 4, d_o)
        ctx.warp_inverse_geometric_device(1, m, g, d_w)
        ctx.sync()
        got, warped = ctx.to_host(d_o, n * 4), ctx.to_host(d_w, n * 4)
    finally:
        for p in (d_f, d_s, d_o, d_w):
            ctx.free(p)
    assert np.array_equal(got, warped)
    assert np.array_equal(got.reshape(g[3], g[2], 4), O.warp_inverse_geometric(1, m, img, *g))


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_remap_bilinear_f32(ctx, channels):
    W, H = 37, 23
    src = np.random.default_rng(100 + channels).standard_normal((H, W, channels)).astype(np.float32)
    img, m, g, sx, sy = _projective4()
    # the coordinate field of the projective case, scaled onto the small source (NaN where uncovered), plus every special value on either axis
    co = FM.coords_field(sx, sy, np.ones(sx.shape, bool), W4, H4).reshape(-1, 2).copy()
    co *= np.float32([W / W4, H / H4])
    special = np.float32([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, W - 1, W, -1, H - 1, H, 0.5, W - 0.5])
    pairs = [(a, b) for a in special for b in (np.float32(3.25),) + tuple(special)] + [(np.float32(3.25), a) for a in special]
    co[:len(pairs)] = np.float32(pairs)
    assert np.isnan(co).any() and np.isfinite(co).all(-1).sum() > 1000
    want = FM.remap_bilinear_f32(co, src)
    n = co.shape[0]
    d_c, d_s, d_o = ctx.alloc(n * 8), ctx.alloc(src.nbytes), ctx.alloc(n * channels * 4)
    try:
        ctx.to_device(d_c, co)
        ctx.to_device(d_s, src)
        ctx.to_device(d_o, np.full(n * channels * 4, 0xA5, np.uint8))
        ctx.remap_bilinear_f32_device(d_c, n, d_s, W, H, channels, d_o)
        ctx.sync()
        got = ctx.to_host(d_o, n * channels * 4).view(np.float32).reshape(n, channels)
    finally:
        for p in (d_c, d_s, d_o):
            ctx.free(p)
    bad = np.flatnonzero((GF.u32(got) != GF.u32(want)).any(-1))
    assert bad.size == 0, (bad.size, [(int(i), co[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:6]])
    nan_rows = ~np.isfinite(co).all(-1)
    assert nan_rows.any() and not got[nan_rows].any()


# ------------------------------------------------------------------------------------------------ 11: refusals
def test_refusals():
    INVALID, STATE = 1, 4
    m = np.array([1, 0, 0, 1, 0, 0], np.float64)
    g = (0, 0, 8, 8)
    with HG.Context(0) as c:
        d = c.alloc(4096)
        try:
            # before any image size / mesh / frame set
            assert GF.refusal_code(c.field_inverse_geometric, 0, m, g, IDX) == STATE
            assert GF.refusal_code(c.field_inverse_geometric_device, 0, m, g, CO, d) == STATE
            assert GF.refusal_code(c.field_inverse_geometric_frames_device, IDX, d) == STATE
            assert GF.refusal_code(c.field_inverse_piecewise_frames_device, IDX, d) == STATE
            c.set_image(WL.lcg_image(16, 16, 1))
            assert GF.refusal_code(c.field_inverse_geometric_frames_device, IDX, d) == STATE         # no frame set
            assert GF.refusal_code(c.field_inverse_piecewise_frames_device, CO, d) == STATE          # no mesh
            sp, tris = WL.grid_points(16, 16, 2, 2), WL.grid_triangles(2, 2)
            c.piecewise_set_mesh(sp, tris, 0, 0)
            assert GF.refusal_code(c.field_inverse_piecewise_frames_device, CO, d) == STATE          # no frame set
            c.piecewise_prepare(sp, (0, 0, 16, 16))
            c.geometric_set_frames(0, np.concatenate([m, [0, 0]]), [g])
            # unknown formats, NULL pointers
            for fmt in (2, -1):
                assert GF.refusal_code(c.field_inverse_geometric, 0, m, g, fmt) == INVALID
                assert GF.refusal_code(c.field_inverse_geometric_device, 0, m, g, fmt, d) == INVALID
                assert GF.refusal_code(c.field_inverse_geometric_frames_device, fmt, d) == INVALID
                assert GF.refusal_code(c.field_inverse_piecewise, fmt) == INVALID
                assert GF.refusal_code(c.field_inverse_piecewise_frames_device, fmt, d) == INVALID
            assert GF.refusal_code(c.field_inverse_geometric_device, 0, m, g, IDX, 0) == INVALID
            assert GF.refusal_code(c.field_inverse_geometric_frames_device, IDX, 0) == INVALID
            assert GF.refusal_code(c.field_inverse_piecewise_frames_device, IDX, 0) == INVALID
            assert GF.refusal_code(c.field_inverse_geometric_frames_device, CO, d, [4]) == INVALID   # an offset that is no multiple of the pixel size
            # remaps
            assert GF.refusal_code(c.remap_index_device, d, 16, d + 1024, 16, 3, d + 2048) == INVALID
            assert GF.refusal_code(c.remap_index_device, d, 16, d + 1024, 16, 0, d + 2048) == INVALID
            assert GF.refusal_code(c.remap_index_device, d, 16, d + 1024, 16, 8, d + 2048 + 4) == INVALID     # misaligned d_out
            assert GF.refusal_code(c.remap_index_device, d, 16, d + 1024 + 2, 16, 4, d + 2048) == INVALID     # misaligned d_src
            assert GF.refusal_code(c.remap_index_device, 0, 16, d + 1024, 16, 4, d + 2048) == INVALID
            for ch in (0, 5):
                assert GF.refusal_code(c.remap_bilinear_f32_device, d, 16, d + 1024, 4, 4, ch, d + 2048) == INVALID
            assert GF.refusal_code(c.remap_bilinear_f32_device, d, 16, d + 1024, 0, 4, 1, d + 2048) == INVALID
            assert GF.refusal_code(c.remap_bilinear_f32_device, d + 4, 16, d + 1024, 4, 4, 1, d + 2048) == INVALID   # misaligned coordinates
            # the context still works
            idx = c.field_inverse_geometric(0, m, g, IDX)
            assert np.array_equal(idx, np.arange(8)[None, :] + 16 * np.arange(8)[:, None])
        finally:
            c.free(d)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_source_field():
    """tests/js/field_gpu.mjs: sourceField() of js/Homography.mjs on the real addon (gather == warp, NaN pattern, refusals as strings)."""
    res = GF.run_node_case("field_gpu.mjs")
    assert set(res["report"]) == {"projective", "piecewise"}
