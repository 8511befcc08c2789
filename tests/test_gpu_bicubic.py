"""The bicubic remap on the GPU (include/hgwarp.h: hg_remap_bicubic_frames_device) against the numpy model of tests/hgtest/bicubic.py --
frame by frame, byte for byte (bit for bit for f32) --, against hg_remap_bilinear_frames_device and hg_remap_index_frames_device where
they must agree, and the drop-in class on the real addon against the ctypes result.  tests/test_bicubic_cpu.py pins the model itself
against a scalar model written from the header.  Small shapes throughout: planes of 67 x 45 at most, frames of 48 x 32 at most."""
import base64
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import bicubic as BM             # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import CO, F32, F32E, FILL, INVALID, POISON, U8E      # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
SW, SH = 67, 45                              # the source
GRID = [(0, 0, 48, 32), (0, 0, 1, 7), (2, 1, 33, 5), (0, 0, 47, 1), (-1, 0, 17, 31)]
PARAMS = ((0.0, 0.5), (1 / 3, 1 / 3), (1.0, 0.0), (0.37, 0.81))


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ inputs, made once and never modified
@functools.lru_cache(maxsize=None)
def _planes(elem, ch, n=3, w=SW, h=SH):
    """n planes (h, w, ch); f32: normal-range values.  uint8 planes hold 1..159, so that no byte of a result equals POISON: the positive
    weights of an axis sum to at most P = 1.188 and the negative ones to at least -N = -0.188 for every pair of PARAMS (the largest lobes:
    (0.37, 0.81)), so a blend stays below 159 * (P * P + N * N) < 231 < POISON, while values near 1 beside larger ones still go below 0 and
    meet the lower clamp."""
    return GF.random_planes(5000 + 10 * ch + elem + 100 * w + 7 * h, elem, (h, w, ch), n)


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
            out["projective"] = (GRID, GF.split(c.to_host(d, total), offs, GRID, 8, F32, 2))
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
            out["piecewise"] = (PW_GEOMS, GF.split(c.to_host(d, total), offs, PW_GEOMS, 8, F32, 2))
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


def _run(ctx, geoms, fields, planes, elem, ch, B=0.0, C=0.5, foffs=None, ooffs=None, stride=None, front=256, call=None):
    """GF.run_frames; call (None: the bicubic remap) gets GF.Buffers.  Returns (output bytes, offsets)."""
    h, w = planes[0].shape[:2]
    if call is None:
        def call(b):
            ctx.remap_bicubic_frames_device(geoms, b.d_f, b.d_p, w, h, len(planes), b.stride, elem, ch, b.d_o, B, C, foffs, ooffs)
    ran = GF.run_frames(ctx, geoms, fields, 8, planes, ch * GF.es(elem), call, foffs, ooffs, stride, front)
    return ran.raw, ran.oo


# ------------------------------------------------------------------------------------------------ the remap against the model
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_bicubic_frames_of_the_librarys_projective_fields(ctx, elem, channels):
    px = channels * GF.es(elem)
    geoms, fields = _library_fields()["projective"]
    assert _enlarges(geoms, fields) < 0.6 and sum(int(np.isfinite(f).all(-1).sum()) for f in fields) > 1500      # on the CPU, before anything is compared
    first = (channels + 2 * elem) % 4
    for n_planes, (B, C) in ((3, PARAMS[first]), (1, PARAMS[(first + 1) % 4])):
        planes = _planes(elem, channels)[:n_planes]
        want = BM.bicubic_frames(geoms, fields, planes, B, C)
        raw, oo = _run(ctx, geoms, fields, planes, elem, channels, B, C)
        GF.check_frames(raw, oo, geoms, want, px, ("projective", elem, channels, n_planes, B, C))


@pytest.mark.parametrize("elem,channels,par", ((U8E, 4, 0), (F32E, 1, 1), (U8E, 3, 2), (F32E, 2, 3)))
def test_bicubic_frames_of_a_piecewise_field_with_uncovered_pixels(ctx, elem, channels, par):
    geoms, fields = _library_fields()["piecewise"]
    px = channels * GF.es(elem)
    nan = sum(int((~np.isfinite(f).all(-1)).sum()) for f in fields)
    assert nan > 50 and sum(int(np.isfinite(f).all(-1).sum()) for f in fields) > 300
    assert _enlarges(geoms, fields) < 0.6
    B, C = PARAMS[par]
    for n_planes in (1, 3):
        planes = _planes(elem, channels)[:n_planes]
        want = BM.bicubic_frames(geoms, fields, planes, B, C)
        assert any(not w_[~np.isfinite(f).all(-1)].any() and w_.any() for w_, f in zip(want, fields))
        raw, oo = _run(ctx, geoms, fields, planes, elem, channels, B, C)
        GF.check_frames(raw, oo, geoms, want, px, ("piecewise", elem, channels, n_planes, B, C))


@pytest.mark.parametrize("elem,channels,par", ((U8E, 1, 0), (U8E, 2, 1), (U8E, 4, 3), (F32E, 1, 2), (F32E, 3, 0), (F32E, 4, 1)))
def test_caller_made_fields_with_nan_infinite_and_huge_entries_beyond_every_edge(ctx, elem, channels, par):
    px = channels * GF.es(elem)
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
    GF.check_frames(raw, oo, GRID, want, px, ("caller-made", elem, channels, B, C))
    if elem == U8E:
        frames = np.concatenate([raw[o:o + RF.n_px(g) * px] for o, g in zip(oo, GRID)])
        assert not (frames == POISON).any()


def test_explicit_offsets_and_strides_that_break_every_wider_alignment(ctx):
    fields = _caller_fields()
    fo8 = [o + 8 * (2 * f + 1) + 512 * f for f, o in enumerate(RF.pack(GRID, 8)[0])]            # odd multiples of 8: no 16-byte alignment
    assert all(o % 8 == 0 and o % 16 != 0 for o in fo8)
    for elem in (U8E, F32E):
        es = GF.es(elem)
        for ch in (1, 2, 3, 4):
            planes = _planes(elem, ch)
            oo = [o + 640 * f + es * (2 * f + 1) for f, o in enumerate(RF.pack(GRID, ch * es)[0])]  # odd element offsets: no 2- or 4-byte store fits (u8)
            assert all(o % es == 0 and (o // es) % 2 == 1 for o in oo)
            stride = planes[0].nbytes + 256 + es * 3
            B, C = PARAMS[(ch + elem) % 4]
            want = BM.bicubic_frames(GRID, fields, planes, B, C)
            raw, used = _run(ctx, GRID, fields, planes, elem, ch, B, C, fo8, oo, stride, front=256 + es)
            GF.check_frames(raw, used, GRID, want, ch * es, ("explicit offsets", elem, ch))


@pytest.mark.parametrize("w,h", ((1, 5), (5, 1), (2, 2)))
def test_tiny_planes(ctx, w, h):
    fields = _caller_fields(w, h)
    for elem, ch, par in ((U8E, 2, 0), (F32E, 1, 1), (U8E, 3, 2), (F32E, 4, 3)):
        planes = _planes(elem, ch, 2, w, h)
        B, C = PARAMS[par]
        want = BM.bicubic_frames(GRID, fields, planes, B, C)
        raw, oo = _run(ctx, GRID, fields, planes, elem, ch, B, C, stride=planes[0].nbytes, front=16)
        GF.check_frames(raw, oo, GRID, want, ch * GF.es(elem), ("tiny", w, h, elem, ch))


# ------------------------------------------------------------------------------------------------ where it IS another remap
@pytest.mark.parametrize("elem,channels", ((U8E, 1), (U8E, 4), (F32E, 1), (F32E, 4), (U8E, 3), (F32E, 2)))
def test_catmull_rom_on_integer_coordinates_is_the_bilinear_and_the_index_remap(ctx, elem, channels):
    planes = _planes(elem, channels)
    px = channels * GF.es(elem)
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
                call=lambda b: ctx.remap_bilinear_frames_device(GRID, b.d_f, b.d_p, SW, SH, 3, b.stride, elem, channels, b.d_o))
    assert np.array_equal(a, b) and (a != FILL).any()
    GF.check_frames(a, oo, GRID, [planes[f % 3].reshape(-1, channels)[index[f]] for f in range(len(GRID))], px, ("integer coordinates", elem, channels))
    if px == 4:
        # the same gather through the matching index field (fields of 4 bytes per pixel at the packed offsets of that format)
        fo4 = RF.pack(GRID, 4)[0]
        d_i = ctx.alloc(fo4[-1] + RF.n_px(GRID[-1]) * 4 + 256)
        try:
            ctx.to_device(d_i, GF.place(index, fo4, fo4[-1] + RF.n_px(GRID[-1]) * 4 + 256, 0))
            c_, _ = _run(ctx, GRID, fields, planes, elem, channels,
                         call=lambda b: ctx.remap_index_frames_device(GRID, d_i, b.d_p, SW * SH, 3, b.stride, 4, b.d_o))
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
    GF.check_frames(got, oo, geoms, want, channels, ("step edge", channels))
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
def test_refusals():
    g = [(0, 0, 8, 2), (0, 0, 4, 1)]
    W, H = 8, 4
    with HG.Context(0) as c:
        d = c.alloc(16384)
        d_f, d_p, d_o = d, d + 4096, d + 8192
        co = (np.random.default_rng(2).random((20, 2)) * [9, 5] - 1).astype(F32)
        plane = np.arange(1, 33, dtype=np.float32).reshape(H, W, 1)
        c.to_device(d_f, GF.place([co[:16], co[16:]], [0, 256], 512, 0))
        c.to_device(d_p, plane)
        want = BM.bicubic_frames(g, [co[:16], co[16:]], [plane], 1 / 3, 1 / 3)

        def still_works():
            c.to_device(d_o, np.full(512, FILL, np.uint8))
            c.remap_bicubic_frames_device(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, 1 / 3, 1 / 3)
            c.sync()
            raw = c.to_host(d_o, 512)
            assert np.array_equal(raw[:64].view(F32), want[0].ravel()) and np.array_equal(raw[256:272].view(F32), want[1].ravel()) and (raw[64:256] == FILL).all()

        def refused(*a):
            assert GF.refusal_code(c.remap_bicubic_frames_device, *a) == INVALID, a
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
def test_state_is_untouched_and_a_queued_nearest_warp_keeps_its_bytes():
    W, H, F = 24, 16, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((1.9, 1.9), W=W, H=H, fit=((24, 16), (48, 32)))      # an enlargement: the inverse loop
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
            fields = GF.split(c.to_host(d_f, 2 * total), fo, gg, 8, F32, 2)
            assert _enlarges(gg, fields) < 0.7
            c.to_device(d_w, np.zeros(total, np.uint8))
            c.warp_inverse_geometric_frames_device(d_w)                   # queued ...
            mid = GF.tap_state(c)
            c.remap_bicubic_frames_device(gg, d_f, d_src, W, H, 1, 0, U8E, 4, d_r, 1 / 3, 1 / 3)      # ... in front of the remap of the picture itself
            assert GF.tap_state(c) == mid
            c.sync()
            assert GF.tap_state(c) == mid and c.sampling == HG.SAMPLE_NEAREST
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
    s = GF.strip_mesh_overflow()
    img, W2, H2, g = s.img, s.W, s.H, s.g
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
            c.piecewise_set_mesh(s.sp, s.tris, *s.min_src)
            c.piecewise_set_frames(s.dp, [g], [0])
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
    res = GF.run_node_case("bicubic_gpu.mjs")
    W, H = res["W"], res["H"]
    u8, f32 = GF.js_pattern_planes(W, H)
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
            got = raw[:co.shape[0] * ch * GF.es(elem)]
            assert hashlib.sha256(got.tobytes()).hexdigest() == case[key], (name, key)
            assert np.array_equal(got, BM.bicubic_frames(g, [co], [plane], B, C)[0].view(np.uint8).ravel()), (name, key)
