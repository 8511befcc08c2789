"""The bicubic remap on the GPU (include/hgwarp.h: hg_remap_bicubic_frames_device) against the numpy model of tests/hgtest/bicubic.py --
frame by frame, byte for byte (bit for bit for f32) --, against hg_remap_bilinear_frames_device and hg_remap_index_frames_device where
they must agree, and the drop-in class on the real addon against the ctypes result.  tests/test_bicubic_cpu.py pins the model itself
against a scalar model written from the header.  Small shapes throughout: planes of 67 x 45 at most, frames of 48 x 32 at most."""
import base64
import functools
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import bicubic as BM             # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
CO = HG.FIELD_COORDS
F32E, U8E = HG.ELEM_F32, HG.ELEM_U8
F32 = np.float32
INVALID = 1
FILL, POISON = 0xA5, 0xEE                    # the output before a call; the bytes around the source planes
SW, SH = 67, 45                              # the source
GRID = [(0, 0, 48, 32), (0, 0, 1, 7), (2, 1, 33, 5), (0, 0, 47, 1), (-1, 0, 17, 31)]
PARAMS = ((0.0, 0.5), (1 / 3, 1 / 3), (1.0, 0.0), (0.37, 0.81))


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def _es(elem):
    return 1 if elem == U8E else 4


# ------------------------------------------------------------------------------------------------ inputs, made once and never modified
@functools.lru_cache(maxsize=None)
def _planes(elem, ch, n=3, w=SW, h=SH):
    """n planes (h, w, ch); f32: normal-range values.  uint8 planes hold 1..159, so that no byte of a result equals POISON: the positive
    weights of an axis sum to at most P = 1.188 and the negative ones to at least -N = -0.188 for every pair of PARAMS (the largest lobes:
    (0.37, 0.81)), so a blend stays below 159 * (P * P + N * N) < 231 < POISON, while values near 1 beside larger ones still go below 0 and
    meet the lower clamp."""
    rng = np.random.default_rng(5000 + 10 * ch + elem + 100 * w + 7 * h)
    if elem == U8E:
        ps = [rng.integers(1, 160, (h, w, ch), dtype=np.uint8) for _ in range(n)]
    else:
        ps = [(rng.standard_normal((h, w, ch)) * 40 + 3).astype(F32) for _ in range(n)]
    for p in ps:
        p.setflags(write=False)
    return tuple(ps)


def _split(raw, offs, geoms):
    out = []
    for o, g in zip(offs, geoms):
        a = raw[o:o + RF.n_px(g) * 8].view(F32).reshape(-1, 2).copy()
        a.setflags(write=False)
        out.append(a)
    return out


PW_SCALES = ((3.0, 3.0), (2.5, 3.5), (4.0, 2.0))
PW_GEOMS = [(-3, -2, 48, 10)] + [(int(SW * kx) + 2 - 30, int(SH * ky) + 1 - 20, 48, 32) for kx, ky in PW_SCALES[1:]]


@functools.lru_cache(maxsize=None)
def _library_fields():
    """The HG_FIELD_COORDS fields the library makes over the SW x SH source, downloaded once: an ENLARGING projective set on GRID (steps of
    about 0.3 source pixels) and an enlarging piecewise set (2-4x) whose windows reach beyond the mesh (uncovered pixels are NaN)."""
    out = {}
    with HG.Context(0) as c:
        c.set_image(np.zeros((SH, SW, 4), np.uint8))             # (a field reads the source's SIZE only)
        pro = np.concatenate([[0.3 + 0.02 * f, 0.01 * f, 3 + 2 * f, 0.005, 0.32, 2 + f, 0.0004 * f, 0.002] for f in range(len(GRID))])
        offs, total = HG.pack_field_offsets(GRID, CO)
        d = c.alloc(total)
        try:
            c.geometric_set_frames(1, pro, GRID)
            c.field_inverse_geometric_frames_device(CO, d)
            c.sync()
            out["projective"] = (GRID, _split(c.to_host(d, total), offs, GRID))
        finally:
            c.free(d)
        nx, ny = 3, 2
        sp, tris = WL.grid_points(SW, SH, nx, ny), WL.grid_triangles(nx, ny)
        p = sp.reshape(-1, 2).astype(np.float64)
        dps = [np.stack([p[:, 0] * kx + 2, p[:, 1] * ky + 1 + 0.4 * np.sin(p[:, 0] / 20 + f)], 1).astype(F32).ravel()
               for f, (kx, ky) in enumerate(PW_SCALES)]
        offs, total = HG.pack_field_offsets(PW_GEOMS, CO)
        d = c.alloc(total)
        try:
            c.piecewise_set_mesh(sp, tris, *WL.src_min(sp))
            c.piecewise_set_frames(np.concatenate(dps), PW_GEOMS)
            c.field_inverse_piecewise_frames_device(CO, d)
            c.sync()
            out["piecewise"] = (PW_GEOMS, _split(c.to_host(d, total), offs, PW_GEOMS))
        finally:
            c.free(d)
    return out


def _enlarges(geoms, fields):
    """The median horizontal step of the finite neighbours of the frames wider than one pixel: below 0.6 source pixels."""
    steps = []
    for g, co in zip(geoms, fields):
        if g[2] > 1 and g[3] > 0:
            a = co.reshape(g[3], g[2], 2)
            ok = np.isfinite(a).all(-1)
            steps.append(np.abs(np.diff(a[:, :, 0], axis=1))[ok[:, 1:] & ok[:, :-1]])
    return float(np.median(np.concatenate(steps)))


@functools.lru_cache(maxsize=None)
def _caller_fields(w=SW, h=SH):
    """Caller-made fields on GRID over a w x h plane: enlargements that run 3 pixels beyond every edge of the plane, with NaN, +-Inf, 1e30
    and 3e38 entries and integer coordinates."""
    rng = np.random.default_rng(51)
    out = []
    for f, (_, _, fw, fh) in enumerate(GRID):
        i, j = np.meshgrid(np.arange(fw), np.arange(fh))
        sx = -3 + i * (w + 6) / max(fw - 1, 1) + 0.1 * f
        sy = -3 + j * (h + 6) / max(fh - 1, 1) + 0.05 * i / max(fw, 1)
        if f == 4:
            sx, sy = sy * w / h, sx * h / w                      # turned
        co = np.stack([sx, sy], -1).astype(F32)
        if fw >= 33:
            co[rng.random((fh, fw)) < 0.04] = np.nan
            co[0, 5:15] = [[np.nan, 3], [3, np.nan], [np.inf, 2], [2, -np.inf], [1e30, 5], [5, -1e30], [-1e30, 1e30], [3e38, -3e38], [4, 2], [0, 0]]
            co[fh - 1, 20] = [1e30, 1e30]
            co[fh - 1, fw - 1] = np.inf
            co[0, 0] = np.nan
        co = co.reshape(-1, 2)
        co.setflags(write=False)
        out.append(co)
    return out


def _place(parts, offs, total, fill):
    buf = np.full(total, fill, np.uint8)
    for p, o in zip(parts, offs):
        b = np.ascontiguousarray(p).view(np.uint8).ravel()
        buf[o:o + b.size] = b
    return buf


def _run(ctx, geoms, fields, planes, elem, ch, B=0.0, C=0.5, foffs=None, ooffs=None, stride=None, front=256, call=None):
    """Upload the fields (at foffs, or packed) and the planes (inside an allocation full of POISON, `front` bytes in, `stride` apart), fill
    the output with FILL, remap (call, or the bicubic remap), and return (output bytes, offsets)."""
    px = ch * _es(elem)
    h, w = planes[0].shape[:2]
    fo = list(foffs) if foffs is not None else RF.pack(geoms, 8)[0]
    oo = list(ooffs) if ooffs is not None else RF.pack(geoms, px)[0]
    stride = stride if stride is not None else (planes[0].nbytes + 255) // 256 * 256 + 256
    f_total = max([o + RF.n_px(g) * 8 for o, g in zip(fo, geoms)] + [0]) + 256
    o_total = max([o + RF.n_px(g) * px for o, g in zip(oo, geoms)] + [0]) + 512
    p_total = front + stride * len(planes) + 256
    d_f, d_p, d_o = ctx.alloc(f_total), ctx.alloc(p_total), ctx.alloc(o_total)
    try:
        ctx.to_device(d_f, _place(fields, fo, f_total, 0x11))
        ctx.to_device(d_p, _place(planes, [front + k * stride for k in range(len(planes))], p_total, POISON))
        ctx.to_device(d_o, np.full(o_total, FILL, np.uint8))
        if call is not None:
            call(d_f, d_p + front, stride, d_o)
        else:
            ctx.remap_bicubic_frames_device(geoms, d_f, d_p + front, w, h, len(planes), stride, elem, ch, d_o, B, C, foffs, ooffs)
        ctx.sync()
        return ctx.to_host(d_o, o_total), oo
    finally:
        for p in (d_f, d_p, d_o):
            ctx.free(p)


def _check(raw, oo, geoms, want, px_bytes, what):
    """Every frame equals the model, bit for bit, and every byte outside the frames is still FILL."""
    untouched = np.ones(raw.size, bool)
    for f, g in enumerate(geoms):
        n = RF.n_px(g) * px_bytes
        untouched[oo[f]:oo[f] + n] = False
        w = np.ascontiguousarray(want[f]).view(np.uint8).ravel()
        assert w.size == n, (what, f)
        got = raw[oo[f]:oo[f] + n]
        if not np.array_equal(got, w):
            bad = np.flatnonzero(got != w)
            raise AssertionError(f"{what}: frame {f} {g}: {bad.size} of {n} bytes differ, first at pixel {int(bad[0]) // px_bytes}: "
                                 f"got {got[bad[:8]].tolist()}, want {w[bad[:8]].tolist()}")
    assert (raw[untouched] == FILL).all(), (what, "bytes between the frames, the padding and the tail must not be written")


# ------------------------------------------------------------------------------------------------ the remap against the model
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_bicubic_frames_of_the_librarys_projective_fields(ctx, elem, channels):
    px = channels * _es(elem)
    geoms, fields = _library_fields()["projective"]
    assert _enlarges(geoms, fields) < 0.6 and sum(int(np.isfinite(f).all(-1).sum()) for f in fields) > 1500      # on the CPU, before anything is compared
    first = (channels + 2 * elem) % 4
    for n_planes, (B, C) in ((3, PARAMS[first]), (1, PARAMS[(first + 1) % 4])):
        planes = _planes(elem, channels)[:n_planes]
        want = BM.bicubic_frames(geoms, fields, planes, B, C)
        raw, oo = _run(ctx, geoms, fields, planes, elem, channels, B, C)
        _check(raw, oo, geoms, want, px, ("projective", elem, channels, n_planes, B, C))


@pytest.mark.parametrize("elem,channels,par", ((U8E, 4, 0), (F32E, 1, 1), (U8E, 3, 2), (F32E, 2, 3)))
def test_bicubic_frames_of_a_piecewise_field_with_uncovered_pixels(ctx, elem, channels, par):
    geoms, fields = _library_fields()["piecewise"]
    px = channels * _es(elem)
    nan = sum(int((~np.isfinite(f).all(-1)).sum()) for f in fields)
    assert nan > 50 and sum(int(np.isfinite(f).all(-1).sum()) for f in fields) > 300
    assert _enlarges(geoms, fields) < 0.6
    B, C = PARAMS[par]
    for n_planes in (1, 3):
        planes = _planes(elem, channels)[:n_planes]
        want = BM.bicubic_frames(geoms, fields, planes, B, C)
        assert any(not w_[~np.isfinite(f).all(-1)].any() and w_.any() for w_, f in zip(want, fields))
        raw, oo = _run(ctx, geoms, fields, planes, elem, channels, B, C)
        _check(raw, oo, geoms, want, px, ("piecewise", elem, channels, n_planes, B, C))


@pytest.mark.parametrize("elem,channels,par", ((U8E, 1, 0), (U8E, 2, 1), (U8E, 4, 3), (F32E, 1, 2), (F32E, 3, 0), (F32E, 4, 1)))
def test_caller_made_fields_with_nan_infinite_and_huge_entries_beyond_every_edge(ctx, elem, channels, par):
    px = channels * _es(elem)
    fields = _caller_fields()
    planes = _planes(elem, channels)
    f0 = fields[0].reshape(32, 48, 2)
    fin = np.isfinite(f0).all(-1)
    assert np.isnan(f0).any() and (f0 == np.inf).any() and (f0 == -np.inf).any()
    assert (np.abs(f0[fin]) == F32(1e30)).any() and (np.abs(f0[fin]) == F32(3e38)).any()
    assert f0[fin][:, 0].min() <= -2.9 and f0[fin][:, 1].min() <= -2.9
    assert (f0[fin][:, 0] >= SW + 2.9).any() and (f0[fin][:, 1] >= SH + 2.9).any()
    B, C = PARAMS[par]
    want = BM.bicubic_frames(GRID, fields, planes, B, C)
    w0 = want[0].reshape(32, 48, channels)
    assert not w0[0, 5:9].any() and w0[0, 9:13].any()                   # NaN / Inf: zeros; 1e30: clamped taps
    raw, oo = _run(ctx, GRID, fields, planes, elem, channels, B, C, stride=planes[0].nbytes, front=16)      # planes back to back
    _check(raw, oo, GRID, want, px, ("caller-made", elem, channels, B, C))
    if elem == U8E:
        frames = np.concatenate([raw[o:o + RF.n_px(g) * px] for o, g in zip(oo, GRID)])
        assert not (frames == POISON).any()


def test_explicit_offsets_and_strides_that_break_every_wider_alignment(ctx):
    fields = _caller_fields()
    fo8 = [o + 8 * (2 * f + 1) + 512 * f for f, o in enumerate(RF.pack(GRID, 8)[0])]            # odd multiples of 8: no 16-byte alignment
    assert all(o % 8 == 0 and o % 16 != 0 for o in fo8)
    for elem in (U8E, F32E):
        es = _es(elem)
        for ch in (1, 2, 3, 4):
            planes = _planes(elem, ch)
            oo = [o + 640 * f + es * (2 * f + 1) for f, o in enumerate(RF.pack(GRID, ch * es)[0])]  # odd element offsets: no 2- or 4-byte store fits (u8)
            assert all(o % es == 0 and (o // es) % 2 == 1 for o in oo)
            stride = planes[0].nbytes + 256 + es * 3
            B, C = PARAMS[(ch + elem) % 4]
            want = BM.bicubic_frames(GRID, fields, planes, B, C)
            raw, used = _run(ctx, GRID, fields, planes, elem, ch, B, C, fo8, oo, stride, front=256 + es)
            _check(raw, used, GRID, want, ch * es, ("explicit offsets", elem, ch))


@pytest.mark.parametrize("w,h", ((1, 5), (5, 1), (2, 2)))
def test_tiny_planes(ctx, w, h):
    fields = _caller_fields(w, h)
    for elem, ch, par in ((U8E, 2, 0), (F32E, 1, 1), (U8E, 3, 2), (F32E, 4, 3)):
        planes = _planes(elem, ch, 2, w, h)
        B, C = PARAMS[par]
        want = BM.bicubic_frames(GRID, fields, planes, B, C)
        raw, oo = _run(ctx, GRID, fields, planes, elem, ch, B, C, stride=planes[0].nbytes, front=16)
        _check(raw, oo, GRID, want, ch * _es(elem), ("tiny", w, h, elem, ch))


# ------------------------------------------------------------------------------------------------ where it IS another remap
@pytest.mark.parametrize("elem,channels", ((U8E, 1), (U8E, 4), (F32E, 1), (F32E, 4), (U8E, 3), (F32E, 2)))
def test_catmull_rom_on_integer_coordinates_is_the_bilinear_and_the_index_remap(ctx, elem, channels):
    planes = _planes(elem, channels)
    px = channels * _es(elem)
    rng = np.random.default_rng(52)
    fields, index = [], []
    for g in GRID:
        n = RF.n_px(g)
        x, y = rng.integers(0, SW, n), rng.integers(0, SH, n)
        x[:2], y[:2] = [0, SW - 1], [0, SH - 1]
        fields.append(np.stack([x, y], -1).astype(F32))
        index.append((y * SW + x).astype(np.int32))
    a, oo = _run(ctx, GRID, fields, planes, elem, channels, 0.0, 0.5)
    b, _ = _run(ctx, GRID, fields, planes, elem, channels,
                call=lambda d_f, d_p, stride, d_o: ctx.remap_bilinear_frames_device(GRID, d_f, d_p, SW, SH, 3, stride, elem, channels, d_o))
    assert np.array_equal(a, b) and (a != FILL).any()
    _check(a, oo, GRID, [planes[f % 3].reshape(-1, channels)[index[f]] for f in range(len(GRID))], px, ("integer coordinates", elem, channels))
    if px == 4:
        # the same gather through the matching index field (fields of 4 bytes per pixel at the packed offsets of that format)
        fo4 = RF.pack(GRID, 4)[0]
        d_i = ctx.alloc(fo4[-1] + RF.n_px(GRID[-1]) * 4 + 256)
        try:
            ctx.to_device(d_i, _place(index, fo4, fo4[-1] + RF.n_px(GRID[-1]) * 4 + 256, 0))
            c_, _ = _run(ctx, GRID, fields, planes, elem, channels,
                         call=lambda d_f, d_p, stride, d_o: ctx.remap_index_frames_device(GRID, d_i, d_p, SW * SH, 3, stride, 4, d_o))
        finally:
            ctx.free(d_i)
        assert np.array_equal(a, c_)


def step_edge_case():
    """A 16 x 6 u8 plane, 0 left of column 8 and 255 from it on, enlarged 4x (pixel centres aligned), cut into frames of 48 x 24 and 16 x 24."""
    plane = np.zeros((6, 16, 1), np.uint8)
    plane[:, 8:] = 255
    i, j = np.meshgrid(np.arange(64), np.arange(24))
    co = np.stack([(i + 0.5) / 4 - 0.5, (j + 0.5) / 4 - 0.5], -1).astype(F32)
    return plane, [(0, 0, 48, 24), (48, 0, 16, 24)], [np.ascontiguousarray(co[:, :48]).reshape(-1, 2), np.ascontiguousarray(co[:, 48:]).reshape(-1, 2)]


@pytest.mark.parametrize("channels", (1, 2, 4))
def test_the_step_edge_is_clamped_on_both_sides_on_the_device(ctx, channels):
    plane, geoms, fields = step_edge_case()
    planes = (np.ascontiguousarray(np.repeat(plane, channels, axis=2)),)
    raw = np.concatenate([BM.remap_bicubic(f, planes[0], 0.0, 0.5, unrounded=True) for f in fields])
    assert raw.min() < -0.5 and raw.max() > 255.5                        # the premise: the lower clamp is needed
    want = BM.bicubic_frames(geoms, fields, planes, 0.0, 0.5)
    got, oo = _run(ctx, geoms, fields, planes, U8E, channels, 0.0, 0.5)
    _check(got, oo, geoms, want, channels, ("step edge", channels))
    frame = got[oo[0]:oo[0] + RF.n_px(geoms[0]) * channels]
    assert (frame == 0).any() and (frame == 255).any()
    assert (frame[raw[:frame.size // channels].ravel() < -0.5] == 0).all()


def test_a_constant_u8_plane_stays_constant(ctx):
    fields = _caller_fields()
    for value, (B, C) in ((1, (0.0, 0.5)), (127, (1 / 3, 1 / 3)), (255, (1.0, 0.0)), (128, (0.0, 1.0)), (254, (1.0, 1.0))):
        planes = tuple(np.full((SH, SW, 3), value, np.uint8) for _ in range(2))
        raw, oo = _run(ctx, GRID, fields, planes, U8E, 3, B, C)
        for f, g in enumerate(GRID):
            got = raw[oo[f]:oo[f] + RF.n_px(g) * 3].reshape(-1, 3)
            fin = np.isfinite(fields[f]).all(-1)
            assert (got[fin] == value).all() and not got[~fin].any(), (value, f)


# ------------------------------------------------------------------------------------------------ refusals
def _code(fn, *a):
    with pytest.raises(HG.HgError) as e:
        fn(*a)
    return e.value.code


def test_refusals():
    g = [(0, 0, 8, 2), (0, 0, 4, 1)]
    W, H = 8, 4
    with HG.Context(0) as c:
        d = c.alloc(16384)
        d_f, d_p, d_o = d, d + 4096, d + 8192
        co = (np.random.default_rng(2).random((20, 2)) * [9, 5] - 1).astype(F32)
        plane = np.arange(1, 33, dtype=np.float32).reshape(H, W, 1)
        c.to_device(d_f, _place([co[:16], co[16:]], [0, 256], 512, 0))
        c.to_device(d_p, plane)
        want = BM.bicubic_frames(g, [co[:16], co[16:]], [plane], 1 / 3, 1 / 3)

        def still_works():
            c.to_device(d_o, np.full(512, FILL, np.uint8))
            c.remap_bicubic_frames_device(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, 1 / 3, 1 / 3)
            c.sync()
            raw = c.to_host(d_o, 512)
            assert np.array_equal(raw[:64].view(F32), want[0].ravel()) and np.array_equal(raw[256:272].view(F32), want[1].ravel()) and (raw[64:256] == FILL).all()

        def refused(*a):
            assert _code(c.remap_bicubic_frames_device, *a) == INVALID, a
            still_works()

        try:
            still_works()
            # (geoms, d_coords, d_planes, w, h, n_planes, stride, elem, channels, d_out, B, C, field_offsets, out_offsets)
            for bad in (float("nan"), -0.1, 1.5, float("inf"), -float("inf")):
                refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, bad, 0.5)
                refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, 0.5, bad)
            # ... and what the bilinear frames form refuses
            refused(g, d_f, d_p, W, H, 1, 0, 2, 1, d_o, 0.0, 0.5)                  # elem
            for ch in (0, 5):
                refused(g, d_f, d_p, W, H, 1, 0, F32E, ch, d_o, 0.0, 0.5)
            refused(g, d_f, d_p, 0, H, 1, 0, F32E, 1, d_o, 0.0, 0.5)
            refused(g, d_f, d_p, W, 0, 1, 0, F32E, 1, d_o, 0.0, 0.5)
            refused(g, d_f, d_p, W, H, 0, 0, F32E, 1, d_o, 0.0, 0.5)               # n_planes
            refused(g, 0, d_p, W, H, 1, 0, F32E, 1, d_o, 0.0, 0.5)                 # NULL pointers
            refused(g, d_f, 0, W, H, 1, 0, F32E, 1, d_o, 0.0, 0.5)
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, 0, 0.0, 0.5)
            refused(g, d_f + 4, d_p, W, H, 1, 0, F32E, 1, d_o, 0.0, 0.5)           # misaligned coordinates, planes, output, stride, offsets
            refused(g, d_f, d_p + 2, W, H, 1, 0, F32E, 1, d_o, 0.0, 0.5)
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o + 1, 0.0, 0.5)
            refused(g, d_f, d_p, W, H, 1, 130, F32E, 1, d_o, 0.0, 0.5)
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, 0.0, 0.5, [0, 260])
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, 0.0, 0.5, None, [0, 258])
            L = HG.lib()
            geoms = HG._geoms(g)
            vp = HG.C.c_void_p
            assert L.hg_remap_bicubic_frames_device(c._h, geoms, -1, vp(d_f), None, vp(d_p), W, H, 1, 0, 0, 1, vp(d_o), None, 0.0, 0.5) == INVALID
            assert L.hg_remap_bicubic_frames_device(c._h, geoms, 65536, vp(d_f), None, vp(d_p), W, H, 1, 0, 0, 1, vp(d_o), None, 0.0, 0.5) == INVALID
            assert L.hg_remap_bicubic_frames_device(c._h, None, 2, vp(d_f), None, vp(d_p), W, H, 1, 0, 0, 1, vp(d_o), None, 0.0, 0.5) == INVALID
            assert L.hg_remap_bicubic_frames_device(c._h, None, 0, None, None, None, W, H, 1, 0, 0, 1, None, None, 0.0, 0.5) == 0      # n_frames == 0
            assert L.hg_remap_bicubic_frames_device(c._h, None, 0, None, None, None, W, H, 1, 0, 0, 1, None, None, 0.0, 1.5) == INVALID
            assert b"C must" in L.hg_last_error(c._h)
            assert L.hg_remap_bicubic_frames_device(c._h, None, 0, None, None, None, W, H, 1, 0, 0, 1, None, None, float("nan"), 0.5) == INVALID
            assert b"B must" in L.hg_last_error(c._h)
            still_works()
        finally:
            c.free(d)


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def _state(c):
    return (c.last_piecewise_kernel(), c.last_piecewise_variant(), c.last_piecewise_self(), c.last_piecewise_flag(), c.last_geometric_kernel(),
            c.last_forward_kernel(), c.last_forward_field_kernel(), c.sampling, c.redone_frames(), c.layout_walks())


def test_state_is_untouched_and_a_queued_nearest_warp_keeps_its_bytes():
    W, H, F = 24, 16, 3
    img = WL.lcg_image(W, H, 81)
    s4 = WL.corners(W, H)
    d4s = [WL.projective_dst(W, H, 0.03 * k) * np.tile([1.9, 1.9], 4) for k in range(F)]                     # an enlargement: the inverse loop
    gg = [tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W, H)) for d4 in d4s]
    assert all(24 < g[2] <= 48 and 16 < g[3] <= 32 for g in gg), gg
    offs, total = HG.pack_offsets(gg)
    with HG.Context(0) as c:
        d_src, d_f, d_w, d_r = c.alloc(img.nbytes), c.alloc(2 * total), c.alloc(total), c.alloc(total)
        try:
            c.set_sampling(HG.SAMPLE_BILINEAR)
            c.set_sampling(HG.SAMPLE_NEAREST)
            c.to_device(d_src, img)
            c.set_image_device(d_src, W, H)
            c.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, offs)
            c.warp_inverse_geometric_frames_device(d_w)
            c.sync()
            alone = c.to_host(d_w, total)
            assert alone.any()
            c.field_inverse_geometric_frames_device(CO, d_f)
            c.sync()
            fo = HG.pack_field_offsets(gg, CO)[0]
            fields = _split(c.to_host(d_f, 2 * total), fo, gg)
            assert _enlarges(gg, fields) < 0.7
            c.to_device(d_w, np.zeros(total, np.uint8))
            c.warp_inverse_geometric_frames_device(d_w)                   # queued ...
            mid = _state(c)
            c.remap_bicubic_frames_device(gg, d_f, d_src, W, H, 1, 0, U8E, 4, d_r, 1 / 3, 1 / 3)      # ... in front of the remap of the picture itself
            assert _state(c) == mid
            c.sync()
            assert _state(c) == mid and c.sampling == HG.SAMPLE_NEAREST
            again = c.to_host(d_w, total)
            for f, g in enumerate(gg):                                    # (the padding between frames is nobody's)
                assert np.array_equal(again[offs[f]:offs[f] + RF.n_px(g) * 4], alone[offs[f]:offs[f] + RF.n_px(g) * 4]) and again[offs[f]:offs[f] + RF.n_px(g) * 4].any(), f
            want = BM.bicubic_frames(gg, fields, [img.reshape(H, W, 4)], 1 / 3, 1 / 3)
            got = c.to_host(d_r, total)
            for f, g in enumerate(gg):
                assert np.array_equal(got[offs[f]:offs[f] + RF.n_px(g) * 4], want[f].ravel()), f
        finally:
            c.set_image(img)
            for p in (d_src, d_f, d_w, d_r):
                c.free(p)


def test_a_queued_redo_never_lands_on_a_later_bicubic_remap():
    """A piecewise warp whose rows carry 1100 spans is queued into buffer B (its frame is flagged, to be redone through the map at hg_sync);
    a bicubic remap then writes B.  After hg_sync B holds the remap.  (The redo needs the wide source and window of the anisotropic test of
    the same name: a row must carry more spans than the row kernel holds.)"""
    n, W2, H2 = 1100, 2400, 8
    img = WL.lcg_image(W2, H2, 10)
    xs = np.linspace(0, W2, n + 1)
    sp = np.stack([np.repeat(xs, 2), np.tile([0.0, H2], n + 1)], 1).astype(np.float32).ravel()
    tr = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(n)], np.uint32).ravel()
    dp = sp.copy()
    dp[1::2] *= 1.5
    mm, md = O.minmax_xy(sp), O.minmax_xy(dp)
    g = (int(md[0]), int(md[1]), int(md[2] - md[0]), int(md[3] - md[1]))
    npx = g[2] * g[3]
    i, j = np.meshgrid(np.arange(g[2]), np.arange(g[3]))
    co = np.stack([(i * 0.3) % W2, j * 0.6], -1).astype(F32).reshape(-1, 2)
    want = BM.bicubic_frames([g], [co], [img.reshape(H2, W2, 4)], 0.0, 0.5)[0]
    with HG.Context(0) as c:
        d_src, d_f, d_b = c.alloc(img.nbytes), c.alloc(npx * 8), c.alloc(npx * 4)
        try:
            c.to_device(d_src, img)
            c.to_device(d_f, co)
            c.set_image_device(d_src, W2, H2)
            c.piecewise_set_mesh(sp, tr, int(mm[0]), int(mm[1]))
            c.piecewise_set_frames(dp, [g], [0])
            r0 = c.redone_frames()
            c.warp_inverse_piecewise_frames_device(d_b)
            c.remap_bicubic_frames_device([g], d_f, d_src, W2, H2, 1, 0, U8E, 4, d_b)
            c.sync()
            assert c.redone_frames() > r0                      # the warp's frame WAS flagged and redone ...
            got = c.to_host(d_b, npx * 4).reshape(npx, 4)
            assert np.array_equal(got, want)                   # ... and the remap stands
        finally:
            c.set_image(img)
            for p in (d_src, d_f, d_b):
                c.free(p)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_bicubic_matches_the_ctypes_result(ctx):
    """tests/js/bicubic_gpu.mjs: remap(plane, {sampling: 'bicubic'}) of js/Homography.mjs on the real addon for an affine, a projective and
    a piecewise enlargement; it prints its coordinate fields and the SHA-256 of every result, and the same planes through the same fields
    by ctypes (Catmull-Rom by default for the u8 plane, [1/3, 1/3] for the f32 plane) must hash alike -- and equal the model."""
    node = shutil.which("node")
    addon = os.path.join(ROOT, "homography.js_amd", "lib", "hgwarp.node")
    assert node is not None and os.path.exists(addon), "node and the N-API addon are needed on a GPU box"
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "bicubic_gpu.mjs")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert p.returncode == 0 and res["ok"] and not res["fails"], (res["fails"], p.stderr[-2000:])
    W, H = res["W"], res["H"]
    idx = np.arange(W * H * 4, dtype=np.int64)
    u8 = ((idx * 7 + (idx >> 3) * 13) & 255).astype(np.uint8).reshape(H, W, 4)
    f32 = ((idx[:W * H] * 37 % 1001) * 0.25 - 100).astype(F32).reshape(H, W, 1)
    assert set(res["cases"]) == {"affine", "projective", "piecewise"}
    third = float(F32(1 / 3))
    for name, case in res["cases"].items():
        g = [(0, 0, case["width"], case["height"])]
        co = np.frombuffer(base64.b64decode(case["coords"]), F32).reshape(-1, 2)
        assert co.shape[0] == case["width"] * case["height"] and np.isfinite(co).any()
        assert _enlarges(g, [co]) < 0.6, name                             # the case does enlarge
        for key, plane, elem, ch, (B, C) in (("u8x4", u8, U8E, 4, (0.0, 0.5)), ("f32x1", f32, F32E, 1, (third, third)),
                                             ("u8x4_mitchell", u8, U8E, 4, (third, third)), ("f32x1_default", f32, F32E, 1, (0.0, 0.5))):
            raw, oo = _run(ctx, g, [co], (plane,), elem, ch, B, C)
            got = raw[:co.shape[0] * ch * _es(elem)]
            assert hashlib.sha256(got.tobytes()).hexdigest() == case[key], (name, key)
            assert np.array_equal(got, BM.bicubic_frames(g, [co], [plane], B, C)[0].view(np.uint8).ravel()), (name, key)
