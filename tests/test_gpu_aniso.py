"""The anisotropic remap on the GPU (include/hgwarp.h: hg_remap_aniso_frames_device) against the numpy model of tests/hgtest/aniso.py --
frame by frame, byte for byte (bit for bit for f32) --, against hg_remap_trilinear_frames_device and hg_remap_bilinear_frames_device where
they must agree, and the drop-in class on the real addon against the ctypes result.  tests/test_aniso_cpu.py pins the model itself
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
from hgtest import aniso as AM               # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import CO, F32, F32E, FILL, INVALID, POISON, U8E      # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest import trilinear as TM           # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
SW, SH = 67, 45                              # the source: 8 levels, every level size odd somewhere
LMAX = 8
GRID = [(0, 0, 48, 32), (0, 0, 1, 7), (2, 1, 33, 5), (0, 0, 47, 1), (-1, 0, 17, 31)]
assert TM.n_levels(SW, SH) == LMAX


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ inputs, made once and never modified
@functools.lru_cache(maxsize=None)
def _planes(elem, ch, n=3):
    """n planes (SH, SW, ch); no byte of a uint8 plane (nor of a blend of its bytes) equals FILL or POISON; f32: normal-range values."""
    return GF.random_planes(3000 + 10 * ch + elem, elem, (SH, SW, ch), n)


@functools.lru_cache(maxsize=None)
def _pyrs(elem, ch, levels, n=3):
    return tuple(TM.pyramid(p, levels) for p in _planes(elem, ch, n))


PW_GEOMS = [(0, 0, 48, 8), (-2, -1, 40, 9), (1, 1, 20, 4)]


@functools.lru_cache(maxsize=None)
def _library_fields():
    """The HG_FIELD_COORDS fields the library makes over the SW x SH source, downloaded once: a projective set on GRID that looks along a
    floor (the vertical step grows much faster than the horizontal one), and a piecewise set (shrinks of 0.7 x 0.12 and 0.9 x 0.1, one magnifying frame) whose windows
    reach beyond the mesh (uncovered pixels are NaN)."""
    out = {}
    with HG.Context(0) as c:
        c.set_image(np.zeros((SH, SW, 4), np.uint8))             # (a field reads the source's SIZE only)
        pro = np.concatenate([[0.4 + 0.1 * f, 0.02 * f, 20 - 2 * f, 0.01, 0.45, 0.4 + 0.1 * f, -0.0005 * f, -0.0285] for f in range(len(GRID))])
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
               for f, (kx, ky) in enumerate(((0.7, 0.12), (1.4, 1.3), (0.9, 0.1)))]
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


@functools.lru_cache(maxsize=None)
def _caller_fields():
    """Caller-made fields on GRID: the horizontal step grows from below one pixel to beyond the source while the vertical one stays near
    one or two pixels, with NaN, +-Inf and 1e30 entries, and a neighbour 2e30 away whose squared step overflows."""
    rng = np.random.default_rng(41)
    out = []
    for f, (_, _, w, h) in enumerate(GRID):
        i, j = np.meshgrid(np.arange(w), np.arange(h))
        sx = 0.05 * (np.exp(i / 6.0) - 1) * (1 + 0.02 * j) + f
        co = np.stack([sx, (1.0 + 0.3 * f) * j * (1 + i / 200.0) + 0.3 * f], -1).astype(F32)
        if w >= 33:
            co[rng.random((h, w)) < 0.04] = np.nan
            co[0, 5:13] = [[np.nan, 3], [3, np.nan], [np.inf, 2], [2, -np.inf], [1e30, 5], [5, -1e30], [-1e30, 1e30], [3e38, -3e38]]
            co[h - 1, 20] = [1e30, 1e30]
            co[h - 1, w - 1] = np.inf
            co[0, 0] = np.nan
            co[h // 2, 25:27] = [[-1e30, 4], [1e30, 4]]         # neighbours 2e30 apart: the step is finite, its square is +Inf
        co = co.reshape(-1, 2)
        co.setflags(write=False)
        out.append(co)
    return out


def _run(ctx, geoms, fields, planes, elem, ch, levels, max_aniso=None, foffs=None, ooffs=None, stride=None, front=256, pyr_slack=256, call=None):
    """GF.run_frames over pyramids of `levels` built first; call (None: the anisotropic remap) gets GF.Buffers.  Returns (output bytes, offsets)."""
    h, w = planes[0].shape[:2]
    if call is None:
        def call(b):
            ctx.remap_aniso_frames_device(geoms, b.d_f, b.d_p, w, h, len(planes), b.stride, elem, ch, b.d_o, b.d_y, b.pyr_stride, levels, max_aniso, foffs, ooffs)
    ran = GF.run_frames(ctx, geoms, fields, 8, planes, ch * GF.es(elem), call, foffs, ooffs, stride, front, pyramid=(elem, ch, levels, pyr_slack))
    return ran.raw, ran.oo


def _premises(geoms, fields, levels, max_aniso):
    """What the fields of a comparison exercise: the probe counts and whether one level or two are read, over the finite pixels."""
    ns, twos = [], []
    for g, co in zip(geoms, fields):
        if RF.n_px(g) == 0:
            continue
        co = co.reshape(g[3], g[2], 2)
        ok = np.isfinite(co).all(-1)
        _, _, N, q = AM.probe_plan(co, max_aniso)
        _, two, _ = TM.level_choice(q, levels)
        ns.append(N[ok])
        twos.append(two[ok])
    return np.concatenate(ns), np.concatenate(twos)


def _assert_premises(geoms, fields, levels, max_aniso, what):
    N, two = _premises(geoms, fields, levels, max_aniso)
    assert (N == 1).any() and ((N > 1) & (N < max_aniso)).any() and (N == max_aniso).any(), (what, np.bincount(N).tolist())
    assert two.any() and (~two).any(), what


# ------------------------------------------------------------------------------------------------ the remap against the model
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_aniso_frames_of_the_librarys_projective_fields(ctx, elem, channels):
    px = channels * GF.es(elem)
    geoms, fields = _library_fields()["projective"]
    _assert_premises(geoms, fields, LMAX, 4, "projective")      # on the CPU, before anything is compared
    planes = _planes(elem, channels)
    for levels, max_aniso in ((LMAX, 4), (LMAX, 16), (2, 4)):
        want = AM.aniso_frames(geoms, fields, _pyrs(elem, channels, levels), max_aniso)
        raw, oo = _run(ctx, geoms, fields, planes, elem, channels, levels, max_aniso)
        GF.check_frames(raw, oo, geoms, want, px, ("projective", elem, channels, levels, max_aniso))


@pytest.mark.parametrize("elem,channels", ((U8E, 4), (F32E, 1), (U8E, 3), (F32E, 2)))
def test_aniso_frames_of_a_piecewise_field_with_uncovered_pixels(ctx, elem, channels):
    geoms, fields = _library_fields()["piecewise"]
    px = channels * GF.es(elem)
    _assert_premises(geoms, fields, LMAX, 8, "piecewise")
    nan = sum(int((~np.isfinite(f).all(-1)).sum()) for f in fields)
    assert nan > 50 and sum(int(np.isfinite(f).all(-1).sum()) for f in fields) > 300
    for n_planes in (1, 3):
        planes = _planes(elem, channels)[:n_planes]
        for max_aniso in (8, 16):
            want = AM.aniso_frames(geoms, fields, _pyrs(elem, channels, LMAX)[:n_planes], max_aniso)
            assert any(not w_[~np.isfinite(f).all(-1)].any() and w_.any() for w_, f in zip(want, fields))
            raw, oo = _run(ctx, geoms, fields, planes, elem, channels, LMAX, max_aniso)
            GF.check_frames(raw, oo, geoms, want, px, ("piecewise", elem, channels, n_planes, max_aniso))


@pytest.mark.parametrize("elem,channels", ((U8E, 1), (U8E, 2), (U8E, 4), (F32E, 1), (F32E, 3), (F32E, 4)))
def test_caller_made_fields_with_nan_infinite_huge_and_overflowing_steps(ctx, elem, channels):
    px = channels * GF.es(elem)
    fields = _caller_fields()
    planes = _planes(elem, channels)
    _assert_premises(GRID, fields, LMAX, 8, "caller-made")
    f0 = fields[0].reshape(32, 48, 2)
    assert np.isnan(f0).any() and np.isinf(f0).any() and (np.abs(f0[np.isfinite(f0)]) >= 1e30).any()
    with np.errstate(all="ignore"):
        plan = AM.probe_plan(f0, 8)
    assert np.isinf(plan[3][16, 25]) and plan[2][16, 25] == 1          # the 2e30 step: q' = +Inf, one probe from the last level
    for levels, max_aniso in ((2, 8), (LMAX, 8), (LMAX, 16)):
        want = AM.aniso_frames(GRID, fields, _pyrs(elem, channels, levels), max_aniso)
        w0 = want[0].reshape(32, 48, channels)
        assert not w0[0, 5:9].any() and w0[0, 9:13].any()               # NaN / Inf: zeros; 1e30: clamped taps
        raw, oo = _run(ctx, GRID, fields, planes, elem, channels, levels, max_aniso, stride=planes[0].nbytes, front=16)      # planes back to back
        GF.check_frames(raw, oo, GRID, want, px, ("caller-made", elem, channels, levels, max_aniso))
        if elem == U8E:
            assert not (raw == POISON).any()


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
            want = AM.aniso_frames(GRID, fields, _pyrs(elem, ch, LMAX), 8)
            raw, used = _run(ctx, GRID, fields, planes, elem, ch, LMAX, 8, fo8, oo, stride, front=256 + es, pyr_slack=256 + es * 3)
            GF.check_frames(raw, used, GRID, want, ch * es, ("explicit offsets", elem, ch))


# ------------------------------------------------------------------------------------------------ where it IS another remap
@pytest.mark.parametrize("elem,channels", ((U8E, 1), (U8E, 4), (F32E, 1), (F32E, 4), (U8E, 3), (F32E, 2)))
def test_max_aniso_1_is_the_trilinear_remap_and_one_level_the_bilinear_one(ctx, elem, channels):
    planes = _planes(elem, channels)

    def trilinear(levels):
        return lambda b: ctx.remap_trilinear_frames_device(GRID, b.d_f, b.d_p, SW, SH, 3, b.stride, elem, channels, b.d_o, b.d_y, b.pyr_stride, levels)

    def bilinear(b):
        ctx.remap_bilinear_frames_device(GRID, b.d_f, b.d_p, SW, SH, 3, b.stride, elem, channels, b.d_o)

    for name, fields in (("caller-made", _caller_fields()), ("projective", _library_fields()["projective"][1])):
        for levels in (LMAX, 2):
            a, _ = _run(ctx, GRID, fields, planes, elem, channels, levels, 1)
            b, _ = _run(ctx, GRID, fields, planes, elem, channels, levels, call=trilinear(levels))
            assert np.array_equal(a, b) and (a != FILL).any(), (name, levels, int((a != b).sum()))
        a, _ = _run(ctx, GRID, fields, planes, elem, channels, 1, 1)
        b, _ = _run(ctx, GRID, fields, planes, elem, channels, 1, call=bilinear)
        assert np.array_equal(a, b) and (a != FILL).any(), (name, "levels == 1")
    # a field that nowhere shrinks: the bilinear remap whatever max_aniso is
    mag = []
    for f, (_, _, w, h) in enumerate(GRID):
        i, j = np.meshgrid(np.arange(w), np.arange(h))
        co = np.stack([0.6 * i + 0.3 * j + 5 * f - 2, 0.7 * j - 0.2 * i + f], -1).astype(F32)
        if w >= 33:
            co[0, 7] = np.nan                                   # (a hole only removes neighbours)
        mag.append(co.reshape(-1, 2))
    assert (_premises(GRID, mag, LMAX, 16)[0] == 1).all()
    a, _ = _run(ctx, GRID, mag, planes, elem, channels, LMAX, 16)
    b, _ = _run(ctx, GRID, mag, planes, elem, channels, LMAX, call=bilinear)
    assert np.array_equal(a, b) and (a != FILL).any(), "magnifying"
    # levels == 1 needs no pyramid at all
    c, _ = _run(ctx, GRID, _caller_fields(), planes, elem, channels, 1,
                call=lambda b: ctx.remap_aniso_frames_device(GRID, b.d_f, b.d_p, SW, SH, 3, b.stride, elem, channels, b.d_o, 0, 0, 1, 1))
    d, _ = _run(ctx, GRID, _caller_fields(), planes, elem, channels, 1, call=bilinear)
    assert np.array_equal(c, d)


def test_the_stripes_stay_stripes_on_the_device_where_trilinear_gives_grey(ctx):
    plane = np.zeros((64, 64, 1), np.uint8)
    plane[:, 1::2] = 255
    i, j = np.meshgrid(np.arange(64), np.arange(8))
    co = [np.stack([1.0 * i, 8.0 * j + 3.5], -1).astype(F32).reshape(-1, 2)]
    g = [(0, 0, 64, 8)]
    levels = TM.n_levels(64, 64)
    for max_aniso in (8, 16):
        ani, _ = _run(ctx, g, co, (plane,), U8E, 1, levels, max_aniso)
        assert np.array_equal(ani[:512].reshape(8, 64), np.broadcast_to(plane[0, :, 0], (8, 64))), max_aniso
    tri, _ = _run(ctx, g, co, (plane,), U8E, 1, levels,
                  call=lambda b: ctx.remap_trilinear_frames_device(g, b.d_f, b.d_p, 64, 64, 1, b.stride, U8E, 1, b.d_o, b.d_y, b.pyr_stride, levels))
    assert (tri[:512] == 128).all()


def test_a_constant_u8_plane_stays_constant(ctx):
    geoms, fields = _library_fields()["projective"]
    for value in (1, 127, 255):
        planes = tuple(np.full((SH, SW, 3), value, np.uint8) for _ in range(2))
        raw, oo = _run(ctx, geoms, fields, planes, U8E, 3, LMAX, 16)
        for f, g in enumerate(geoms):
            got = raw[oo[f]:oo[f] + RF.n_px(g) * 3].reshape(-1, 3)
            fin = np.isfinite(fields[f]).all(-1)
            assert (got[fin] == value).all() and not got[~fin].any(), (value, f)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    g = [(0, 0, 8, 2), (0, 0, 4, 1)]
    W, H = 8, 4                                                  # 4 levels
    with HG.Context(0) as c:
        d = c.alloc(16384)
        d_f, d_p, d_o, d_y = d, d + 4096, d + 8192, d + 12288
        co = (np.random.default_rng(2).random((20, 2)) * [7, 3]).astype(F32)
        co[:, 1] *= F32(3)                                       # steps that ask for more than one probe
        plane = np.arange(1, 33, dtype=np.float32).reshape(H, W, 1)
        c.to_device(d_f, GF.place([co[:16], co[16:]], [0, 256], 512, 0))
        c.to_device(d_p, plane)
        want = AM.aniso_frames(g, [co[:16], co[16:]], [TM.pyramid(plane, 4)], 4)

        def still_works():
            c.to_device(d_o, np.full(512, FILL, np.uint8))
            c.pyramid_build_device(d_p, W, H, 1, 0, F32E, 1, 4, d_y, 1024)
            c.remap_aniso_frames_device(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, d_y, 1024, 4, 4)
            c.sync()
            raw = c.to_host(d_o, 512)
            assert np.array_equal(raw[:64].view(F32), want[0].ravel()) and np.array_equal(raw[256:272].view(F32), want[1].ravel()) and (raw[64:256] == FILL).all()

        def refused(*a):
            assert GF.refusal_code(c.remap_aniso_frames_device, *a) == INVALID, a
            still_works()

        try:
            still_works()
            # (geoms, d_coords, d_planes, w, h, n_planes, stride, elem, channels, d_out, d_pyr, pyr_stride, levels, max_aniso, field_offsets, out_offsets)
            for max_aniso in (0, 17, -1, 1 << 20):
                refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, d_y, 1024, 4, max_aniso)
            # ... and what the trilinear form refuses
            for levels in (0, 5):
                refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, d_y, 1024, levels, 4)
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, 0, 1024, 2, 4)          # d_pyr NULL with levels > 1
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, d_y + 2, 1024, 4, 4)    # a misaligned pyramid / stride
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, d_y, 1026, 4, 4)
            refused(g, d_f, d_p, W, H, 1, 0, 2, 1, d_o, d_y, 1024, 4, 4)           # elem
            for ch in (0, 5):
                refused(g, d_f, d_p, W, H, 1, 0, F32E, ch, d_o, d_y, 4096, 4, 4)
            refused(g, d_f, d_p, 0, H, 1, 0, F32E, 1, d_o, d_y, 1024, 1, 4)
            refused(g, d_f, d_p, W, H, 0, 0, F32E, 1, d_o, d_y, 1024, 4, 4)        # n_planes
            refused(g, 0, d_p, W, H, 1, 0, F32E, 1, d_o, d_y, 1024, 4, 4)          # NULL pointers
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, 0, d_y, 1024, 4, 4)
            refused(g, d_f + 4, d_p, W, H, 1, 0, F32E, 1, d_o, d_y, 1024, 4, 4)    # misaligned coordinates, planes, output, offsets
            refused(g, d_f, d_p + 2, W, H, 1, 0, F32E, 1, d_o, d_y, 1024, 4, 4)
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o + 1, d_y, 1024, 4, 4)
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, d_y, 1024, 4, 4, [0, 260])
            refused(g, d_f, d_p, W, H, 1, 0, F32E, 1, d_o, d_y, 1024, 4, 4, None, [0, 258])
            L = HG.lib()
            geoms = HG._geoms(g)
            vp = HG.C.c_void_p
            assert L.hg_remap_aniso_frames_device(c._h, geoms, -1, vp(d_f), None, vp(d_p), W, H, 1, 0, 0, 1, vp(d_o), None, vp(d_y), 1024, 4, 4) == INVALID
            assert L.hg_remap_aniso_frames_device(c._h, None, 2, vp(d_f), None, vp(d_p), W, H, 1, 0, 0, 1, vp(d_o), None, vp(d_y), 1024, 4, 4) == INVALID
            assert L.hg_remap_aniso_frames_device(c._h, None, 0, None, None, None, W, H, 1, 0, 0, 1, None, None, None, 0, 1, 4) == 0      # n_frames == 0
            assert L.hg_remap_aniso_frames_device(c._h, None, 0, None, None, None, W, H, 1, 0, 0, 1, None, None, None, 0, 1, 0) == INVALID
            assert b"max_aniso" in L.hg_last_error(c._h)
            still_works()
        finally:
            c.free(d)


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def test_state_is_untouched_and_a_queued_nearest_warp_keeps_its_bytes():
    W, H, F = 64, 40, 3
    img, s4, d4s, gg, offs, total = GF.oblique_projective_set((0.6, 0.15))      # an oblique shrink (the inverse loop); windows of 48 x 32 at most
    levels = HG.pyramid_levels(W, H)
    _, ptotal = HG.pyramid_layout(W, H, U8E, 4, levels)
    with HG.Context(0) as c:
        d_src, d_f, d_w, d_r, d_y = c.alloc(img.nbytes), c.alloc(2 * total), c.alloc(total), c.alloc(total), c.alloc(ptotal)
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
            assert (_premises(gg, fields, levels, 16)[0] > 1).any()
            c.to_device(d_w, np.zeros(total, np.uint8))
            c.warp_inverse_geometric_frames_device(d_w)                   # queued ...
            mid = GF.tap_state(c)
            c.pyramid_build_device(d_src, W, H, 1, 0, U8E, 4, levels, d_y, ptotal)
            c.remap_aniso_frames_device(gg, d_f, d_src, W, H, 1, 0, U8E, 4, d_r, d_y, ptotal, levels, 16)      # ... in front of the remap of the picture itself
            assert GF.tap_state(c) == mid
            c.sync()
            assert GF.tap_state(c) == mid and c.sampling == HG.SAMPLE_NEAREST
            again = c.to_host(d_w, total)
            for f, g in enumerate(gg):                                    # (the padding between frames is nobody's)
                assert np.array_equal(again[offs[f]:offs[f] + RF.n_px(g) * 4], alone[offs[f]:offs[f] + RF.n_px(g) * 4]) and again[offs[f]:offs[f] + RF.n_px(g) * 4].any(), f
            want = AM.aniso_frames(gg, fields, [TM.pyramid(img.reshape(H, W, 4), levels)], 16)
            got = c.to_host(d_r, total)
            for f, g in enumerate(gg):
                assert np.array_equal(got[offs[f]:offs[f] + RF.n_px(g) * 4], want[f].ravel()), f
        finally:
            c.set_image(img)
            for p in (d_src, d_f, d_w, d_r, d_y):
                c.free(p)


def test_a_queued_redo_never_lands_on_a_later_aniso_remap():
    """A piecewise warp whose rows carry 1100 spans is queued into buffer B (its frame is flagged, to be redone through the map at hg_sync);
    an anisotropic remap then writes B.  After hg_sync B holds the remap.  (The redo needs the wide source and window of the trilinear test of
    the same name: a row must carry more spans than the row kernel holds.)"""
    s = GF.strip_mesh_overflow()
    img, W2, H2, g = s.img, s.W, s.H, s.g
    npx = g[2] * g[3]
    i, j = np.meshgrid(np.arange(g[2]), np.arange(g[3]))
    co = np.stack([(i * 7.3) % W2, j * 0.6], -1).astype(F32).reshape(-1, 2)
    levels = 5
    want = AM.aniso_frames([g], [co], [TM.pyramid(img.reshape(H2, W2, 4), levels)], 8)[0]
    assert (AM.probe_plan(co.reshape(g[3], g[2], 2), 8)[2] == 8).any()
    _, ptotal = HG.pyramid_layout(W2, H2, U8E, 4, levels)
    with HG.Context(0) as c:
        d_src, d_f, d_b, d_y = c.alloc(img.nbytes), c.alloc(npx * 8), c.alloc(npx * 4), c.alloc(ptotal)
        try:
            c.to_device(d_src, img)
            c.to_device(d_f, co)
            c.set_image_device(d_src, W2, H2)
            c.piecewise_set_mesh(s.sp, s.tris, *s.min_src)
            c.piecewise_set_frames(s.dp, [g], [0])
            r0 = c.redone_frames()
            c.pyramid_build_device(d_src, W2, H2, 1, 0, U8E, 4, levels, d_y, ptotal)
            c.warp_inverse_piecewise_frames_device(d_b)
            c.remap_aniso_frames_device([g], d_f, d_src, W2, H2, 1, 0, U8E, 4, d_b, d_y, ptotal, levels, 8)
            c.sync()
            assert c.redone_frames() > r0                      # the warp's frame WAS flagged and redone ...
            got = c.to_host(d_b, npx * 4).reshape(npx, 4)
            assert np.array_equal(got, want)                   # ... and the remap stands
        finally:
            c.set_image(img)
            for p in (d_src, d_f, d_b, d_y):
                c.free(p)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_anisotropic_matches_the_ctypes_result(ctx):
    """tests/js/aniso_gpu.mjs: remap(plane, {sampling: 'anisotropic'}) of js/Homography.mjs on the real addon for an affine, a projective
    and a piecewise oblique shrink; it prints its coordinate fields and the SHA-256 of every result, and the same planes through the same
    fields by ctypes (all levels; maxAniso 8 by default, 3 for the f32 plane) must hash alike -- and equal the model."""
    res = GF.run_node_case("aniso_gpu.mjs")
    W, H = res["W"], res["H"]
    u8, f32 = GF.js_pattern_planes(W, H)
    levels = HG.pyramid_levels(W, H)
    assert set(res["cases"]) == {"affine", "projective", "piecewise"}
    for name, case in res["cases"].items():
        g = [(0, 0, case["width"], case["height"])]
        co = np.frombuffer(base64.b64decode(case["coords"]), F32).reshape(-1, 2)
        assert co.shape[0] == case["width"] * case["height"] and np.isfinite(co).any()
        assert (_premises(g, [co], levels, 8)[0] > 1).any(), name        # the case does ask for more than one probe
        for key, plane, elem, ch, max_aniso in (("u8x4", u8, U8E, 4, 8), ("f32x1", f32, F32E, 1, 3)):
            raw, oo = _run(ctx, g, [co], (plane,), elem, ch, levels, max_aniso)
            got = raw[:co.shape[0] * ch * GF.es(elem)]
            assert hashlib.sha256(got.tobytes()).hexdigest() == case[key], (name, key)
            assert np.array_equal(got, AM.aniso_frames(g, [co], [TM.pyramid(plane, levels)], max_aniso)[0].view(np.uint8).ravel()), (name, key)
