"""hg_flow_dense_frames_device and hg_field_compose_frames_device on the device against the numpy model of tests/hgtest/flow.py, BYTE FOR
BYTE: field, flow pairs, residual and good bytes of every frame; every output, the planes and the scratch lie between guard bytes that must
survive, and so must the bytes between frames.  Window sums are integers and everything else is IEEE in a fixed order, so no tolerance is
involved anywhere in this file."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import flow as FM                # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
FILL, POISON, GUARD = GF.FILL, GF.POISON, 256
TW, TH = FM.TILE_W, FM.TILE_H
pad256 = lambda b: (b + 255) // 256 * 256


@pytest.fixture(scope="module")
def ctx():
    with HG.Context(0) as c:
        yield c


def planes(seed, W, H, n, ch=1):
    """n textured planes (H, W) or (H, W, 4) of u8; the texture generator needs two pixels a side, so tiny planes are cut from a larger one."""
    out = []
    for k in range(n * ch):
        out.append(np.ascontiguousarray(FM.texture(max(W, 8), max(H, 8), seed + k, 0.2)[:H, :W]))
    if ch == 1:
        return out
    return [np.ascontiguousarray(np.stack(out[4 * k:4 * k + 4], -1)) for k in range(n)]


def shifted(p, dx, dy):
    """p moved by whole pixels with its border repeated: FROM(x + dx, y + dy) = p(x, y)."""
    H, W = p.shape[:2]
    return np.ascontiguousarray(p[np.clip(np.arange(H) - dy, 0, H - 1)][:, np.clip(np.arange(W) - dx, 0, W - 1)])


class Ran:
    pass


def run(ctx, frms, tos, ch, levels, n_iter=2, radius=3, min_eig=1.0, max_update=1.0, foffs=None, gap=0, flow=True, residual=True, good=True):
    """One call between guards.  Returns the raw field / flow extents (guards checked and cut off), the residual and good planes."""
    F, S = len(frms), len(tos)
    H, W = frms[0].shape[:2]
    n = W * H
    stride = n * ch + gap
    fo = list(foffs) if foffs is not None else [f * pad256(n * 8) for f in range(F)]
    ext = max(o + n * 8 for o in fo)
    scratch = HG.flow_layout(W, H, ch, F, S, levels)
    assert scratch == FM.layout(W, H, ch, F, S, levels)
    sizes = dict(frm=F * stride, to=S * stride, field=ext, flow=ext, res=F * n, good=F * n, scratch=scratch)
    d = {k: ctx.alloc(v + 2 * GUARD) for k, v in sizes.items()}
    try:
        ctx.to_device(d["frm"], GF.place(frms, [GUARD + k * stride for k in range(F)], sizes["frm"] + 2 * GUARD, POISON))
        ctx.to_device(d["to"], GF.place(tos, [GUARD + k * stride for k in range(S)], sizes["to"] + 2 * GUARD, POISON))
        for k in ("field", "flow", "res", "good", "scratch"):
            ctx.to_device(d[k], np.full(sizes[k] + 2 * GUARD, FILL, np.uint8))
        ctx.flow_dense_frames_device(d["frm"] + GUARD, F, d["to"] + GUARD, S, W, H, ch, d["field"] + GUARD, d["scratch"] + GUARD, levels=levels, n_iter=n_iter,
                                     radius=radius, min_eig=min_eig, max_update=max_update, field_offsets=foffs,
                                     d_flow=d["flow"] + GUARD if flow else 0, d_residual=d["res"] + GUARD if residual else 0,
                                     d_good=d["good"] + GUARD if good else 0, from_stride_bytes=stride, to_stride_bytes=stride)
        ctx.sync()
        raw = {k: ctx.to_host(d[k], sizes[k] + 2 * GUARD) for k in ("field", "flow", "res", "good", "scratch")}
    finally:
        for p in d.values():
            ctx.free(p)
    r = Ran()
    for k, b in raw.items():
        assert (b[:GUARD] == FILL).all() and (b[GUARD + sizes[k]:] == FILL).all(), (k, "guard bytes were written")
        setattr(r, k, b[GUARD:GUARD + sizes[k]])
    r.fo, r.n, r.F, r.shape = fo, n, F, (H, W)
    if not flow:
        assert (r.flow == FILL).all()
    if not residual:
        assert (r.res == FILL).all()
    if not good:
        assert (r.good == FILL).all()
    return r


def check(r, want, what, flow=True, residual=True, good=True):
    """Every frame equals the model; the bytes between the frames are untouched."""
    n, (H, W) = r.n, r.shape
    for name, on in (("field", True), ("flow", flow)):
        raw = getattr(r, name)
        untouched = np.ones(raw.size, bool)
        for f, w in enumerate(want):
            o = r.fo[f]
            untouched[o:o + n * 8] = False
            if on:
                got = raw[o:o + n * 8].view(np.uint32)
                ww = np.ascontiguousarray(getattr(w, name)).view(np.uint32).ravel()
                if not np.array_equal(got, ww):
                    bad = np.flatnonzero(got != ww)
                    raise AssertionError(f"{what}: {name} of frame {f}: {bad.size} of {2 * n} words differ, first at pixel {int(bad[0]) // 2} (width {W}): "
                                         f"got {got[bad[:4]].view(F32).tolist()}, want {ww[bad[:4]].view(F32).tolist()}")
        assert (raw[untouched] == FILL).all(), (what, name, "bytes between the frames must not be written")
    for f, w in enumerate(want):
        if residual:
            assert np.array_equal(r.res[f * n:(f + 1) * n], w.residual.ravel()), (what, "residual", f)
        if good:
            assert np.array_equal(r.good[f * n:(f + 1) * n], w.good.ravel()), (what, "good", f)


def pair(seed, W, H, dx=1, dy=0):
    to = planes(seed, W, H, 1)[0]
    return shifted(to, dx, dy), to


# ------------------------------------------------------------------------------------------------ sizes, at every legal number of levels
SIZES = [(1, 1, 7), (2, 3, 7), (5, 7, 7), (33, 17, 3), (TW - 1, TH - 1, 3), (TW, TH, 3), (TW + 1, TH + 1, 7), (TW - 1, TH + 1, 2), (2 * TW + 1, TH - 1, 4),
         (TW + 1, 2 * TH + 1, 3)]


@pytest.mark.parametrize("W,H,radius", SIZES)
def test_sizes_at_every_legal_number_of_levels(ctx, W, H, radius):
    frm, to = pair(11 + W, W, H)
    top = FM.max_levels(W, H)
    assert top == HG.pyramid_levels(W, H) or top == 12
    if (W, H) == (33, 17):
        assert [p.shape[::-1] for p in FM.pyramid(to, 4)] == [(33, 17), (17, 9), (9, 5), (5, 3)]
    for levels in range(1, top + 1):
        want = [FM.flow(frm, to, levels, 2, radius)]
        check(run(ctx, [frm], [to], 1, levels, 2, radius), want, (W, H, radius, levels))
    if top < 12:
        assert GF.refusal_code(run, ctx, [frm], [to], 1, top + 1) == GF.INVALID


@pytest.mark.parametrize("radius", [1, 7])
def test_radius_one_and_seven_over_several_tiles(ctx, radius):
    W, H = 2 * TW + 5, 2 * TH + 3
    frm, to = pair(5, W, H, 1, 1)
    want = [FM.flow(frm, to, 3, 3, radius, 0.5, 0.75)]
    assert want[0].good.any() and want[0].flow.any()
    check(run(ctx, [frm], [to], 1, 3, 3, radius, 0.5, 0.75), want, ("radius", radius))


def test_many_iterations_and_a_large_step(ctx):
    W, H = 70, 45
    frm, to = pair(9, W, H, 3, -2)
    want = [FM.flow(frm, to, 3, 9, 4, 2.0, 4.0)]
    check(run(ctx, [frm], [to], 1, 3, 9, 4, 2.0, 4.0), want, "9 iterations, max_update 4")
    inner = want[0].flow[12:-12, 12:-12]
    assert abs(np.median(inner[..., 0]) - 3.0) < 0.25 and abs(np.median(inner[..., 1]) + 2.0) < 0.25      # (the model found the shift)


# ------------------------------------------------------------------------------------------------ the set rule, luma, strides
@pytest.mark.parametrize("n_to", [1, 2, 5])
def test_set_rule_five_frames(ctx, n_to):
    W, H = 40, 21
    tos = planes(40, W, H, n_to)
    frms = [shifted(tos[f % n_to], 1 + f % 2, f % 3 - 1) for f in range(5)]
    want = FM.flow_frames(frms, tos, 1, 2, n_iter=2, radius=2)
    check(run(ctx, frms, tos, 1, 2, 2, 2, gap=13), want, ("sets", n_to))
    if n_to > 1:
        assert not np.array_equal(want[0].flow, FM.flow(frms[0], tos[1], 2, 2, 2).flow)      # the rule matters on these planes


def test_an_empty_set_writes_nothing(ctx):
    d = ctx.alloc(1024)
    try:
        ctx.to_device(d, np.full(1024, FILL, np.uint8))
        ctx.flow_dense_frames_device(0, 0, 0, 1, 8, 8, 1, d, d, levels=1, d_flow=d, d_residual=d, d_good=d)
        ctx.flow_dense_frames_device(0, 0, 0, 1, 8, 8, 1, 0, 0, levels=1)
        ctx.sync()
        assert (ctx.to_host(d, 1024) == FILL).all()
    finally:
        ctx.free(d)


def test_rgba_planes_give_the_bytes_of_their_luma_planes(ctx):
    W, H = 37, 19
    tos = planes(70, W, H, 2, 4)
    frms = [shifted(tos[f % 2], 1, f - 1) for f in range(3)]
    a = run(ctx, frms, tos, 4, 3, 2, 3, gap=8)
    b = run(ctx, [FM.luma(p) for p in frms], [FM.luma(p) for p in tos], 1, 3, 2, 3)
    for k in ("field", "flow", "res", "good"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    check(a, FM.flow_frames(frms, tos, 4, 3, n_iter=2, radius=3), "rgba")


# ------------------------------------------------------------------------------------------------ coverage, flat and identical planes
def test_a_flow_that_leaves_the_plane_on_all_four_sides_gives_the_nan_pattern_there(ctx):
    W, H = 64, 48
    to = planes(90, W, H, 1)[0]
    xs, ys = FM.grid(W, H)
    cx, cy = F32((W - 1) / 2), F32((H - 1) / 2)
    # FROM is TO shrunk by 1.12 about the centre: FROM(c + (p - c) * 1.12) would be TO(p), so the field points outwards at every border
    src = FM.bilinear(to[..., None], cx + (xs - cx) / F32(1.12), cy + (ys - cy) / F32(1.12))[..., 0]
    frm = np.minimum(F32(255), np.floor(src + F32(0.5))).astype(np.uint8)
    want = FM.flow(frm, to, 3, 4, 3)
    nanw = np.ascontiguousarray(want.field).view(np.uint32)[..., 0] == FM.NAN_WORD
    assert nanw[0].any() and nanw[-1].any() and nanw[:, 0].any() and nanw[:, -1].any() and not nanw[H // 4:-H // 4, W // 4:-W // 4].any()
    assert (np.ascontiguousarray(want.field).view(np.uint32)[nanw] == FM.NAN_WORD).all()
    check(run(ctx, [frm], [to], 1, 3, 4, 3), [want], "coverage")


def test_flat_and_identical_planes(ctx):
    W, H = TW + 7, TH + 5
    flat = np.full((H, W), 93, np.uint8)
    tex = planes(3, W, H, 1)[0]
    r = run(ctx, [tex, tex], [flat, tex], 1, 3, 3, 3)
    check(r, [FM.flow(tex, flat, 3, 3, 3), FM.flow(tex, tex, 3, 3, 3)], "flat, identical")
    n = W * H
    assert not r.good[:n].any() and not r.flow[r.fo[0]:r.fo[0] + n * 8].any()            # flat TO: no good pixel, a zero flow
    xs, ys = FM.grid(W, H)
    ident = np.stack([xs, ys], -1)
    assert np.array_equal(r.field[r.fo[1]:r.fo[1] + n * 8].view(np.uint32), ident.view(np.uint32).ravel())      # identical planes: the identity field
    assert not r.res[n:].any() and r.good[n:].any()


# ------------------------------------------------------------------------------------------------ gaps, optional outputs, determinism, state
def test_caller_made_offsets_with_gaps_and_optional_outputs(ctx):
    W, H = 35, 18
    n = W * H
    tos = planes(50, W, H, 1)
    frms = [shifted(tos[0], 1, 0), shifted(tos[0], 0, 1), shifted(tos[0], -1, 1)]
    foffs = [2 * pad256(n * 8) + 72, 8, pad256(n * 8) + 40]
    want = FM.flow_frames(frms, tos, 1, 2, n_iter=2, radius=3)
    check(run(ctx, frms, tos, 1, 2, 2, 3, foffs=foffs), want, "gaps")
    for keep in ("flow", "residual", "good", None):
        on = {k: k == keep for k in ("flow", "residual", "good")}
        check(run(ctx, frms, tos, 1, 2, 2, 3, foffs=foffs, **on), want, ("optional", keep), **on)


def test_two_runs_give_the_same_bytes_and_the_warp_state_is_left_alone(ctx):
    W, H = 3 * TW + 3, 2 * TH + 9
    tos = planes(60, W, H, 1)
    frms = [shifted(tos[0], 2, 1), shifted(tos[0], -1, 2)]
    before = GF.tap_state(ctx)
    a = run(ctx, frms, tos, 1, 3, 4, 3)
    b = run(ctx, frms, tos, 1, 3, 4, 3)
    assert GF.tap_state(ctx) == before
    for k in ("field", "flow", "res", "good"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    check(a, FM.flow_frames(frms, tos, 1, 3, n_iter=4, radius=3), "determinism")


def test_refusals_on_the_device(ctx):
    d = ctx.alloc(1 << 16)
    try:
        ctx.to_device(d, np.zeros(1 << 16, np.uint8))
        ok = dict(d_from=d, n_frames=2, d_to=d + 4096, n_to_sets=1, w=16, h=12, channels=1, d_field=d + 8192, d_scratch=d + 16384, levels=2)
        assert HG.flow_layout(16, 12, 1, 2, 1, 2) <= (1 << 16) - 16384
        call = lambda **k: ctx.flow_dense_frames_device(**dict(ok, **k))
        call()
        ctx.sync()
        for bad in (dict(w=0), dict(h=32769), dict(channels=3), dict(levels=0), dict(levels=6), dict(n_iter=0), dict(n_iter=33), dict(radius=0), dict(radius=8),
                    dict(min_eig=-1.0), dict(min_eig=float("nan")), dict(max_update=0.0), dict(max_update=4.5), dict(n_frames=-1), dict(n_frames=4097),
                    dict(n_to_sets=0), dict(n_to_sets=3), dict(from_stride_bytes=16 * 12 - 1), dict(to_stride_bytes=1), dict(d_from=0), dict(d_to=0),
                    dict(d_field=0), dict(d_scratch=0), dict(d_field=d + 4), dict(d_flow=d + 4), dict(d_scratch=d + 8), dict(field_offsets=[0, 4])):
            assert GF.refusal_code(call, **bad) == GF.INVALID, bad
        g = [(0, 0, 4, 4)]
        comp = lambda **k: ctx.field_compose_frames_device(**dict(dict(geoms=g, d_outer=d, d_inner=d + 1024, wi=4, hi=4, n_inner=1, inner_stride_bytes=128, d_out=d + 2048), **k))
        comp()
        ctx.sync()
        for bad in (dict(wi=0), dict(hi=0), dict(n_inner=0), dict(d_outer=0), dict(d_inner=0), dict(d_out=0), dict(d_outer=d + 4), dict(d_out=d + 4),
                    dict(d_inner=d + 2), dict(inner_stride_bytes=130), dict(outer_offsets=[4]), dict(out_offsets=[4])):
            assert GF.refusal_code(comp, **bad) == GF.INVALID, bad
        ctx.field_compose_frames_device([], 0, 0, 4, 4, 1, 128, 0)
    finally:
        ctx.free(d)


# ------------------------------------------------------------------------------------------------ the chained field
def compose_case():
    rng = np.random.default_rng(77)
    Wi, Hi = 23, 14
    geoms = [(3, -2, 19, 11), (0, 0, 0, 5), (-4, 9, 33, 7), (1, 1, 5, 40)]
    inner = [(rng.uniform(-5, 40, (Hi, Wi, 2))).astype(F32) for _ in range(2)]
    inner[0][4, 7, 0] = np.nan
    inner[1][9, 20, 1] = np.inf
    inner[1][0, 0] = -np.inf
    outer = []
    for k, g in enumerate(geoms):
        n = RF.n_px(g)
        co = rng.uniform(-3, 26, (n, 2)).astype(F32)
        co[:, 1] = rng.uniform(-3, 17, n).astype(F32)
        if n:
            co[rng.integers(0, n, 6), rng.integers(0, 2, 6)] = [np.nan, np.inf, -np.inf, 1e30, -1e30, np.nan]
            co[0] = [7.0, 4.0] if k % 2 == 0 else [20.0, 9.0]      # exactly on the tap that is not finite
        outer.append(co)
    for p in inner + outer:
        p.setflags(write=False)
    return geoms, outer, tuple(inner), Wi, Hi


@pytest.mark.parametrize("gaps", [False, True])
def test_compose_equals_the_two_channel_remap_where_finite_and_the_nan_pattern_elsewhere(ctx, gaps):
    geoms, outer, inner, Wi, Hi = compose_case()
    foffs = ooffs = None
    if gaps:
        fo, _ = RF.pack(geoms, 8)
        foffs, ooffs = [o + 8 * (k + 1) for k, o in enumerate(fo)], [o + 16 * (k + 2) for k, o in enumerate(fo)][::-1]
    comp = lambda b: ctx.field_compose_frames_device(geoms, b.d_f, b.d_p, Wi, Hi, len(inner), b.stride, b.d_o, foffs, ooffs)
    remap = lambda b: ctx.remap_bilinear_frames_device(geoms, b.d_f, b.d_p, Wi, Hi, len(inner), b.stride, GF.F32E, 2, b.d_o, foffs, ooffs)
    got = GF.run_frames(ctx, geoms, outer, 8, inner, 8, comp, foffs, ooffs)
    ref = GF.run_frames(ctx, geoms, outer, 8, inner, 8, remap, foffs, ooffs)
    want = [FM.compose(co, inner[f % len(inner)]) for f, co in enumerate(outer)]
    GF.check_frames(got.raw, got.oo, geoms, want, 8, "compose")
    kinds = set()
    for f, (g, co) in enumerate(zip(geoms, outer)):
        n = RF.n_px(g)
        a = got.raw[got.oo[f]:got.oo[f] + n * 8].view(np.uint32).reshape(-1, 2)
        b = ref.raw[ref.oo[f]:ref.oo[f] + n * 8].view(np.uint32).reshape(-1, 2)
        fin = np.isfinite(co).all(1) & np.isfinite(b.view(F32)).all(1)
        assert np.array_equal(a[fin], b[fin]) and (a[~fin] == FM.NAN_WORD).all(), f
        kinds |= {"outer nan"} if np.isnan(co).any() else set()
        kinds |= {"outer inf"} if np.isinf(co).any() else set()
        kinds |= {"inner tap"} if (np.isfinite(co).all(1) & ~np.isfinite(b.view(F32)).all(1)).any() else set()
    assert kinds == {"outer nan", "outer inf", "inner tap"}
    # the set rule: frame 2 reads inner field 0, not 1
    assert not np.array_equal(want[2], FM.compose(outer[2], inner[1]))


# ------------------------------------------------------------------------------------------------ the drop-in class on the real addon
def test_js_dense_flow_with_warp_equals_the_bilinear_gather_through_its_own_field():
    """tests/js/flow_gpu.mjs: h.denseFlow(..., { warp: true, field: true }) on the real addon: every picture that comes down is the bilinear
    gather of its FROM picture through the call's own field, a picture moved by two columns gives a flow of two columns, identical pictures
    the identity field."""
    GF.run_node_case("flow_gpu.mjs")
