"""The remaps of whole frame sets and the 8-bit bilinear remap on the GPU (include/hgwarp.h: hg_remap_index_frames_device,
hg_remap_bilinear_frames_device, hg_remap_bilinear_u8_device) against the numpy model of tests/hgtest/remap_frames.py -- frame by frame,
bit for bit --, against the loop of single-list calls, and against the warps whose geometry the fields carry.  tests/test_remap_frames_cpu.py
pins the u8 model itself on hand-computed cases."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import field as FM               # noqa: E402
from hgtest import fwd_edges as FE           # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import CO, F32E, FILL, INVALID, POISON, U8E      # noqa: E402
from hgtest import moving as MV              # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest import workloads as WL           # noqa: E402

pytestmark = pytest.mark.gpu
IDX = HG.FIELD_INDEX
SW, SH = 97, 61                              # the small source
N_SRC = SW * SH
# pixel counts 1, 3, 4, 5, an empty frame in the middle, 255, 257, 1021 and one frame of several blocks
RAGGED = [(0, 0, 1, 1), (3, -2, 3, 1), (0, 0, 2, 2), (-1, 0, 5, 1), (4, 4, 0, 7), (0, 0, 255, 1), (0, 0, 257, 1), (0, 0, 1021, 1), (-5, -5, 300, 200)]
assert [RF.n_px(g) for g in RAGGED] == [1, 3, 4, 5, 0, 255, 257, 1021, 60000]


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ inputs, made once and never modified
@functools.lru_cache(maxsize=None)
def _index_fields():
    """One caller-made index field per ragged frame: mostly in range, some just outside, and the int32 extremes."""
    rng = np.random.default_rng(11)
    out = []
    for g in RAGGED:
        f = rng.integers(-2, N_SRC + 2, RF.n_px(g)).astype(np.int32)
        if f.size >= 255:
            f[:6] = [-1, N_SRC, -2 ** 31, 2 ** 31 - 1, 0, N_SRC - 1]
        f.setflags(write=False)
        out.append(f)
    return out


@functools.lru_cache(maxsize=None)
def _coord_fields():
    """One caller-made coordinate field per ragged frame: in and around the source, NaN / infinite / huge entries in the larger frames."""
    rng = np.random.default_rng(12)
    out = []
    for g in RAGGED:
        c = (rng.random((RF.n_px(g), 2)) * [SW + 3, SH + 3] - 1.5).astype(np.float32)
        if c.shape[0] >= 255:
            c[:8] = np.float32([[np.nan, 3], [3, np.nan], [np.inf, 2], [2, -np.inf], [1e30, 5], [5, -1e30], [-1e-30, 7.5], [SW - 0.5, SH - 0.5]])
            c[8::17] = np.floor(c[8::17])                    # integer coordinates: fx = fy = 0
        c.setflags(write=False)
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _planes(dtype, per_px, n=3):
    """n source planes of per_px elements per pixel; no byte of a uint8 plane equals FILL or POISON."""
    return GF.random_planes(1000 + per_px + (0 if dtype == "u8" else 50), U8E if dtype == "u8" else F32E, (N_SRC, per_px), n, f32_affine=None)


def _run(*a, **k):
    """GF.run_frames(ctx, geoms, fields, fld_px, planes, px_bytes, call, foffs, ooffs, stride, front): (output bytes, output offsets)."""
    ran = GF.run_frames(*a, **k)
    return ran.raw, ran.oo


def _index_call(ctx, geoms, pb, n_planes, foffs=None, ooffs=None):
    return lambda b: ctx.remap_index_frames_device(geoms, b.d_f, b.d_p, N_SRC, n_planes, b.stride, pb, b.d_o, foffs, ooffs)


def _bilinear_call(ctx, geoms, elem, ch, n_planes, foffs=None, ooffs=None):
    return lambda b: ctx.remap_bilinear_frames_device(geoms, b.d_f, b.d_p, SW, SH, n_planes, b.stride, elem, ch, b.d_o, foffs, ooffs)


def _hwc(planes, ch):
    return [p.reshape(SH, SW, ch) for p in planes]


# ------------------------------------------------------------------------------------------------ ragged sets against the model
def test_the_packed_layouts_are_the_librarys():
    for per in (1, 2, 3, 4, 8, 12, 16):
        assert HG.pack_plane_offsets(RAGGED, per) == RF.pack(RAGGED, per)
    assert HG.pack_field_offsets(RAGGED, IDX) == RF.pack(RAGGED, 4) and HG.pack_field_offsets(RAGGED, CO) == RF.pack(RAGGED, 8)


@pytest.mark.parametrize("n_planes", (1, 3))
@pytest.mark.parametrize("pixel_bytes", (1, 2, 4, 8, 16))
def test_index_frames_of_a_ragged_set(ctx, pixel_bytes, n_planes):
    planes = _planes("u8", pixel_bytes)[:n_planes]
    want = RF.index_frames(RAGGED, _index_fields(), planes)
    assert any(w.any() for w in want) and not want[5][:4].any()
    raw, oo = _run(ctx, RAGGED, _index_fields(), 4, planes, pixel_bytes, _index_call(ctx, RAGGED, pixel_bytes, n_planes))
    GF.check_frames(raw, oo, RAGGED, want, pixel_bytes, ("index", pixel_bytes, n_planes))
    assert not (raw == POISON).any()


@pytest.mark.parametrize("n_planes", (1, 3))
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_bilinear_frames_of_a_ragged_set(ctx, elem, channels, n_planes):
    planes = _planes("u8" if elem == U8E else "f32", channels)[:n_planes]
    px = channels * (1 if elem == U8E else 4)
    want = RF.bilinear_frames(RAGGED, _coord_fields(), _hwc(planes, channels))
    assert not want[8][:4].any() and want[8][4:8].any()       # NaN / infinite coordinates: zeros; 1e30, -1e30, -1e-30: clamped taps
    raw, oo = _run(ctx, RAGGED, _coord_fields(), 8, planes, px, _bilinear_call(ctx, RAGGED, elem, channels, n_planes))
    GF.check_frames(raw, oo, RAGGED, want, px, ("bilinear", elem, channels, n_planes))


# ------------------------------------------------------------------------------------------------ the frames form == the loop of single calls
def _loop_of_singles(ctx, single):
    """single(f, d_field_f, n_px, d_plane_f, d_out_f) for every non-empty frame, over the packed layouts."""
    def call(fo, oo, n_planes):
        def run(b):
            for f, g in enumerate(RAGGED):
                if RF.n_px(g):
                    single(b.d_f + fo[f], RF.n_px(g), b.d_p + (f % n_planes) * b.stride, b.d_o + oo[f])
        return run
    return call


@pytest.mark.parametrize("pixel_bytes", (1, 2, 4, 8, 16))
def test_index_frames_equal_the_loop_of_single_calls(ctx, pixel_bytes):
    planes = _planes("u8", pixel_bytes)
    fo, oo = RF.pack(RAGGED, 4)[0], RF.pack(RAGGED, pixel_bytes)[0]
    loop = _loop_of_singles(ctx, lambda d_f, n, d_p, d_o: ctx.remap_index_device(d_f, n, d_p, N_SRC, pixel_bytes, d_o))(fo, oo, 3)
    a, _ = _run(ctx, RAGGED, _index_fields(), 4, planes, pixel_bytes, _index_call(ctx, RAGGED, pixel_bytes, 3))
    b, _ = _run(ctx, RAGGED, _index_fields(), 4, planes, pixel_bytes, loop)
    assert np.array_equal(a, b) and (a != FILL).any()


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
def test_bilinear_frames_equal_the_loop_of_single_calls(ctx, elem, channels):
    planes = _planes("u8" if elem == U8E else "f32", channels)
    px = channels * (1 if elem == U8E else 4)
    fo, oo = RF.pack(RAGGED, 8)[0], RF.pack(RAGGED, px)[0]
    fn = ctx.remap_bilinear_u8_device if elem == U8E else ctx.remap_bilinear_f32_device
    loop = _loop_of_singles(ctx, lambda d_f, n, d_p, d_o: fn(d_f, n, d_p, SW, SH, channels, d_o))(fo, oo, 3)
    a, _ = _run(ctx, RAGGED, _coord_fields(), 8, planes, px, _bilinear_call(ctx, RAGGED, elem, channels, 3))
    b, _ = _run(ctx, RAGGED, _coord_fields(), 8, planes, px, loop)
    assert np.array_equal(a, b) and (a != FILL).any()


# ------------------------------------------------------------------------------------------------ explicit offsets that break the packed alignment
def test_offsets_and_strides_that_break_the_packed_alignment(ctx):
    n = len(RAGGED)
    fo4 = [o + 4 * (f % 3 + 1) + 768 * f for f, o in enumerate(RF.pack(RAGGED, 4)[0])]          # multiples of 4, not of 16 (frames 0, 1, 2, ...: +4, +8, +12)
    assert all(o % 4 == 0 and o % 16 != 0 for o in fo4)
    for pb in (1, 2, 4, 8, 16):
        planes = _planes("u8", pb)
        oo = [o + 1024 * f + pb * (2 * f + 1) for f, o in enumerate(RF.pack(RAGGED, pb)[0])]   # odd multiples of the pixel size
        assert all(o % pb == 0 and (o // pb) % 2 == 1 for o in oo)
        stride = planes[0].nbytes + 256
        while pb < 16 and stride % 16 == 0:                     # a multiple of pb, not of 16
            stride += pb
        assert stride % pb == 0 and (pb == 16 or stride % 16 != 0)
        want = RF.index_frames(RAGGED, _index_fields(), planes)
        for fo_, oo_ in ((fo4, oo), (None, oo), (fo4, None)):
            raw, used = _run(ctx, RAGGED, _index_fields(), 4, planes, pb, _index_call(ctx, RAGGED, pb, 3, fo_, oo_), fo_, oo_, stride, front=256 + pb)
            GF.check_frames(raw, used, RAGGED, want, pb, ("index, explicit offsets", pb, fo_ is None, oo_ is None))
    fo8 = [o + 8 * (2 * f + 1) + 512 * f for f, o in enumerate(RF.pack(RAGGED, 8)[0])]
    for elem, es in ((U8E, 1), (F32E, 4)):
        for ch in (1, 2, 3, 4):
            planes = _planes("u8" if elem == U8E else "f32", ch)
            oo = [o + 640 * f + es * (2 * f + 1) for f, o in enumerate(RF.pack(RAGGED, ch * es)[0])]      # odd element offsets: no 2- or 4-byte store fits
            stride = planes[0].nbytes + 256 + es * 3
            want = RF.bilinear_frames(RAGGED, _coord_fields(), _hwc(planes, ch))
            raw, used = _run(ctx, RAGGED, _coord_fields(), 8, planes, ch * es, _bilinear_call(ctx, RAGGED, elem, ch, 3, fo8, oo), fo8, oo, stride, front=256 + es)
            GF.check_frames(raw, used, RAGGED, want, ch * es, ("bilinear, explicit offsets", elem, ch))
    assert n == 9


# ------------------------------------------------------------------------------------------------ it IS the warp
def _frames_equal(ctx, d_a, d_b, geoms, offs, what):
    for f, g in enumerate(geoms):
        n = RF.n_px(g) * 4
        if n:
            a, b = ctx.to_host(d_a, n, offs[f]), ctx.to_host(d_b, n, offs[f])
            assert a.any(), (what, f, "an all-zero frame proves nothing")
            assert np.array_equal(a, b), (what, f, int((a != b).sum()))


def test_index_frames_of_the_rgba_sources_are_the_geometric_warp(ctx):
    W, H, F = 256, 160, 5
    img = WL.lcg_image(W, H, 81)
    s4 = WL.corners(W, H)
    d4s = [WL.projective_dst(W, H, 0.03 * k) for k in range(F)]
    gg = [tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W, H)) for d4 in d4s]
    gg = [(g[0] - 3 * f, g[1] + f - 2, g[2] - 11 * f, g[3] - 5 * f) for f, g in enumerate(gg)]
    gg[3] = (gg[3][0], gg[3][1], 0, gg[3][3])                # an empty frame in the middle
    offs, total = HG.pack_offsets(gg)
    assert (offs, total) == HG.pack_plane_offsets(gg, 4)
    ctx.set_sampling(HG.SAMPLE_NEAREST)
    d_src, d_f, d_w, d_r = ctx.alloc(img.nbytes), ctx.alloc(total), ctx.alloc(total), ctx.alloc(total)
    try:
        ctx.to_device(d_src, img)
        ctx.set_image_device(d_src, W, H)
        ctx.geometric_set_frames_points(1, np.concatenate(d4s), np.tile(s4, F), gg, offs)
        ctx.field_inverse_geometric_frames_device(IDX, d_f)
        ctx.remap_index_frames_device(gg, d_f, d_src, W * H, 1, 0, 4, d_r)
        ctx.warp_inverse_geometric_frames_device(d_w)
        ctx.sync()
        _frames_equal(ctx, d_r, d_w, gg, offs, "projective set")
    finally:
        ctx.set_image(img)
        for p in (d_src, d_f, d_w, d_r):
            ctx.free(p)


def test_index_frames_are_the_piecewise_warp_with_own_source_points_and_three_images(ctx):
    ms = MV.set_a(4, 5)
    NI, stride = 3, ms.W * ms.H * 4 + 256
    offs, total = HG.pack_offsets(ms.geoms)
    ctx.set_sampling(HG.SAMPLE_NEAREST)
    d_src, d_f, d_w, d_r = ctx.alloc(stride * NI), ctx.alloc(total), ctx.alloc(total), ctx.alloc(total)
    try:
        for k in range(NI):
            ctx.to_device(d_src, ms.imgs[k], k * stride)
        ctx.set_images_device(d_src, ms.W, ms.H, NI, stride)
        ctx.piecewise_set_mesh(ms.base, ms.tris, *WL.src_min(ms.base))
        ctx.piecewise_set_frames_src(ms.src_all, ms.min_all, ms.dst_all, ms.geoms, offs)
        ctx.field_inverse_piecewise_frames_device(IDX, d_f)
        ctx.remap_index_frames_device(ms.geoms, d_f, d_src, ms.W * ms.H, NI, stride, 4, d_r)
        ctx.warp_inverse_piecewise_frames_device(d_w)
        ctx.sync()
        _frames_equal(ctx, d_r, d_w, ms.geoms, offs, "piecewise set, 3 images, 5 frames")
    finally:
        ctx.set_image(ms.imgs[0])
        for p in (d_src, d_f, d_w, d_r):
            ctx.free(p)


def test_index_frames_are_the_forward_piecewise_warp():
    b = FE.piecewise_batch()
    W, H, box = b["W"], b["H"], b["box"]
    geoms = [g for _, g in b["frames"]]
    n = len(geoms)
    imgs = [O.lcg_image(W, H, s) for s in b["seeds"]]
    dps = np.concatenate([d for d, _ in b["frames"]])
    offs, total = HG.pack_offsets(geoms)
    stride = W * H * 4
    with HG.Context(0) as c:
        d_src, d_f, d_w, d_r = c.alloc(n * stride), c.alloc(total), c.alloc(total), c.alloc(total)
        try:
            for k in range(n):
                c.to_device(d_src, imgs[k], k * stride)
            c.set_images_device(d_src, W, H, n, stride)
            c.piecewise_set_mesh(b["sp"], b["tris"], box[0], box[1])
            c.to_device(d_r, np.full(total, FILL, np.uint8))
            c.to_device(d_w, np.full(total, FILL, np.uint8))
            c.field_forward_piecewise_batch_device(dps, box[2], box[3], geoms, None, d_f)
            c.remap_index_frames_device(geoms, d_f, d_src, W * H, n, stride, 4, d_r)
            c.warp_forward_piecewise_batch_device(dps, box[2], box[3], geoms, offs, d_w)
            c.sync()
            _frames_equal(c, d_r, d_w, geoms, offs, "forward piecewise batch")
        finally:
            c.set_image(imgs[0])
            for p in (d_src, d_f, d_w, d_r):
                c.free(p)


# ------------------------------------------------------------------------------------------------ caller-made fields
def test_caller_made_fields_never_read_outside_their_plane(ctx):
    geoms = [(0, 0, 16, 1), (0, 0, 9, 1), (0, 0, 16, 1)]
    special = np.array([-1, N_SRC, -2 ** 31, 2 ** 31 - 1, N_SRC + 1, -2, 2 ** 30, -2 ** 30, 0, N_SRC - 1, 1, 2, 3, 4, 5, 6], np.int32)
    fields = [special, special[:9], special[::-1].copy()]
    for pb in (1, 2, 4, 8, 16):
        planes = _planes("u8", pb)
        want = RF.index_frames(geoms, fields, planes)
        assert not want[0][:8].any() and want[0][8:].all()
        raw, oo = _run(ctx, geoms, fields, 4, planes, pb, lambda b: ctx.remap_index_frames_device(geoms, b.d_f, b.d_p, N_SRC, 3, b.stride, pb, b.d_o),
                       stride=planes[0].nbytes, front=16)          # planes back to back, poison right in front and behind
        GF.check_frames(raw, oo, geoms, want, pb, ("caller-made index field", pb))
        assert not (raw == POISON).any(), pb
    co = np.float32([[np.nan, 1], [1, np.nan], [np.inf, 1], [1, np.inf], [-np.inf, 1], [1, -np.inf], [np.nan, np.nan],
                     [1e30, 1e30], [-1e30, -1e30], [1e30, -1e30], [-1e30, 2.5], [SW - 1, SH - 1], [SW, SH], [-1, -1], [0, 0], [SW - 0.5, 0.25]])
    cgeoms = [(0, 0, 16, 1), (0, 0, 4, 4)]
    for elem in (U8E, F32E):
        for ch in (1, 4):
            planes = _planes("u8" if elem == U8E else "f32", ch)
            es = 1 if elem == U8E else 4
            hw = _hwc(planes, ch)
            want = RF.bilinear_frames(cgeoms, [co, co], hw)
            assert not want[0][:7].any()                                                     # NaN and +-inf: zeros
            assert np.array_equal(want[0][7], hw[0][SH - 1, SW - 1]) and np.array_equal(want[0][8], hw[0][0, 0]) and np.array_equal(want[0][9], hw[0][0, SW - 1])
            assert np.array_equal(want[1][12], hw[1][SH - 1, SW - 1]) and np.array_equal(want[1][13], hw[1][0, 0])      # clamped
            raw, oo = _run(ctx, cgeoms, [co, co], 8, planes, ch * es,
                           lambda b: ctx.remap_bilinear_frames_device(cgeoms, b.d_f, b.d_p, SW, SH, 3, b.stride, elem, ch, b.d_o),
                           stride=planes[0].nbytes, front=16)
            GF.check_frames(raw, oo, cgeoms, want, ch * es, ("caller-made coordinates", elem, ch))
            if elem == U8E:
                assert not (raw == POISON).any()


# ------------------------------------------------------------------------------------------------ frame count limits
def test_65535_one_pixel_frames_launch_and_65536_are_refused(ctx):
    F, NP = 65535, 3
    geoms = [(0, 0, 1, 1)] * F
    rng = np.random.default_rng(21)
    fld = rng.integers(-1, N_SRC + 1, F).astype(np.int32)
    co = (rng.random((F, 2)) * [SW, SH]).astype(np.float32)
    p4, pf = _planes("u8", 4), _planes("f32", 1)
    foffs4, foffs8, ooffs = [4 * f for f in range(F)], [8 * f for f in range(F)], [4 * f for f in range(F)]
    want_i = np.stack([p4[f % NP][fld[f]] if 0 <= fld[f] < N_SRC else np.zeros(4, np.uint8) for f in range(F)])
    want_b = np.concatenate([FM.remap_bilinear_f32(co[k::NP], pf[k].reshape(SH, SW, 1)) for k in range(NP)])
    order = np.concatenate([np.arange(k, F, NP) for k in range(NP)])
    stride = (N_SRC * 4 + 255) // 256 * 256
    d_f, d_p, d_o = ctx.alloc(F * 8), ctx.alloc(stride * NP), ctx.alloc(F * 4 + 256)
    try:
        ctx.to_device(d_f, fld)
        for k in range(NP):
            ctx.to_device(d_p, p4[k], k * stride)
        ctx.to_device(d_o, np.full(F * 4 + 256, FILL, np.uint8))
        ctx.remap_index_frames_device(geoms, d_f, d_p, N_SRC, NP, stride, 4, d_o, foffs4, ooffs)
        ctx.sync()
        raw = ctx.to_host(d_o, F * 4 + 256)
        assert np.array_equal(raw[:F * 4].reshape(F, 4), want_i) and (raw[F * 4:] == FILL).all()
        ctx.to_device(d_f, co)
        for k in range(NP):
            ctx.to_device(d_p, pf[k], k * stride)
        ctx.to_device(d_o, np.full(F * 4 + 256, FILL, np.uint8))
        ctx.remap_bilinear_frames_device(geoms, d_f, d_p, SW, SH, NP, stride, F32E, 1, d_o, foffs8, ooffs)
        ctx.sync()
        raw = ctx.to_host(d_o, F * 4 + 256)
        assert np.array_equal(raw[:F * 4].view(np.uint32)[order], want_b.view(np.uint32).ravel()) and (raw[F * 4:] == FILL).all()
        more = geoms + [(0, 0, 1, 1)]
        assert GF.refusal_code(ctx.remap_index_frames_device, more, d_f, d_p, N_SRC, NP, stride, 4, d_o, foffs4 + [0], ooffs + [0]) == INVALID
        assert GF.refusal_code(ctx.remap_bilinear_frames_device, more, d_f, d_p, SW, SH, NP, stride, F32E, 1, d_o, foffs8 + [0], ooffs + [0]) == INVALID
        assert (ctx.to_host(d_o, F * 4 + 256) == raw).all()
    finally:
        for p in (d_f, d_p, d_o):
            ctx.free(p)


# ------------------------------------------------------------------------------------------------ u8 specifics
def test_u8_through_an_integer_shift_is_the_index_remap_and_the_nearest_warp(ctx):
    W, H = 131, 77
    img = WL.lcg_image(W, H, 5)
    m = np.array([1, 0, 0, 1, -7, 5], np.float64)             # inverse matrix: source = output + (-7, 5)
    g = (-3, -9, 150, 95)
    n = g[2] * g[3]
    ctx.set_sampling(HG.SAMPLE_NEAREST)
    d_src, d_i, d_c, d_a, d_b, d_w = ctx.alloc(img.nbytes), ctx.alloc(n * 4), ctx.alloc(n * 8), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4)
    try:
        ctx.to_device(d_src, img)
        ctx.set_image_device(d_src, W, H)
        ctx.field_inverse_geometric_device(0, m, g, IDX, d_i)
        ctx.field_inverse_geometric_device(0, m, g, CO, d_c)
        ctx.remap_bilinear_frames_device([g], d_c, d_src, W, H, 1, 0, U8E, 4, d_a)
        ctx.remap_index_frames_device([g], d_i, d_src, W * H, 1, 0, 4, d_b)
        ctx.warp_inverse_geometric_device(0, m, g, d_w)
        ctx.sync()
        a, b, w = ctx.to_host(d_a, n * 4), ctx.to_host(d_b, n * 4), ctx.to_host(d_w, n * 4)
        co = ctx.to_host(d_c, n * 8).view(np.float32)
        fin = np.isfinite(co)
        assert fin.any() and not fin.all() and np.array_equal(co[fin], np.floor(co[fin]))      # an integer-valued field with uncovered pixels
        assert np.array_equal(a, b) and np.array_equal(b, w)
        assert np.array_equal(w.reshape(g[3], g[2], 4), O.warp_inverse_geometric(0, m, img, *g))
    finally:
        ctx.set_image(img)
        for p in (d_src, d_i, d_c, d_a, d_b, d_w):
            ctx.free(p)


def test_u8_ties_clamp_and_the_single_list_form(ctx):
    src = np.array([[[0, 255, 10, 1], [1, 255, 20, 2]], [[255, 255, 30, 3], [254, 255, 40, 5]]], np.uint8)      # 2 x 2, 4 channels
    co = np.float32([[0.5, 0], [0.5, 1], [0.5, 0.5], [0, 0.5], [0.25, 0.75], [1, 1], [0, 0], [0.3, 0.7], [1 / 3, 2 / 3], [0.999, 0.001], [-1e-30, 0], [np.nan, 0]])
    co = np.concatenate([co, (np.random.default_rng(4).random((500, 2)) * 2 - 0.5).astype(np.float32)])
    n = co.shape[0]
    g = [(0, 0, n, 1)]
    for ch in (1, 2, 3, 4):
        s = np.ascontiguousarray(src[:, :, :ch])
        want = RF.remap_bilinear_u8(co, s)
        assert want[0, 0] == 1                                  # the tie: (0 + 1) / 2 = 0.5 -> 1
        if ch >= 2:
            assert (want[:11, 1] == 255).all()                  # all-255 taps stay 255 at every fraction
        assert np.array_equal(want[6], s[0, 0]) and np.array_equal(want[5], s[1, 1]) and np.array_equal(want[10], s[0, 0]) and not want[11].any()
        d_c, d_s, d_a, d_b = ctx.alloc(n * 8), ctx.alloc(256), ctx.alloc(n * ch + 256), ctx.alloc(n * ch + 256)
        try:
            ctx.to_device(d_c, co)
            ctx.to_device(d_s, s)
            for d in (d_a, d_b):
                ctx.to_device(d, np.full(n * ch + 256, FILL, np.uint8))
            ctx.remap_bilinear_frames_device(g, d_c, d_s, 2, 2, 1, 0, U8E, ch, d_a)
            ctx.remap_bilinear_u8_device(d_c, n, d_s, 2, 2, ch, d_b)
            ctx.sync()
            a, b = ctx.to_host(d_a, n * ch + 256), ctx.to_host(d_b, n * ch + 256)
        finally:
            for p in (d_c, d_s, d_a, d_b):
                ctx.free(p)
        bad = np.flatnonzero((a[:n * ch].reshape(n, ch) != want).any(1))
        assert bad.size == 0, (ch, [(co[i].tolist(), a[:n * ch].reshape(n, ch)[i].tolist(), want[i].tolist()) for i in bad[:6]])
        assert np.array_equal(a, b) and (a[n * ch:] == FILL).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    g = [(0, 0, 8, 2), (0, 0, 4, 1)]
    with HG.Context(0) as c:
        d = c.alloc(16384)
        d_f, d_p, d_o = d, d + 4096, d + 8192
        fld = np.arange(20, dtype=np.int32)[::-1].copy()
        plane = (np.arange(1, 65, dtype=np.uint64) * 2654435761 % (2 ** 32)).astype(np.uint32)
        c.to_device(d_f, GF.place([fld[:16], fld[16:]], [0, 256], 512, 0))
        c.to_device(d_p, plane)

        def still_works():
            c.to_device(d_o, np.full(512, FILL, np.uint8))
            c.remap_index_frames_device(g, d_f, d_p, 64, 1, 256, 4, d_o)
            c.sync()
            raw = c.to_host(d_o, 512).view(np.uint32)
            assert np.array_equal(raw[:16], plane[fld[:16]]) and np.array_equal(raw[64:68], plane[fld[16:]]) and (raw[16:64] == 0xA5A5A5A5).all()

        def refused(fn, *a):
            assert GF.refusal_code(fn, *a) == INVALID, a
            still_works()

        ri, rb, ru = c.remap_index_frames_device, c.remap_bilinear_frames_device, c.remap_bilinear_u8_device
        try:
            still_works()
            # index: (geoms, d_field, d_planes, n_src_px, n_planes, stride, pixel_bytes, d_out, field_offsets, out_offsets)
            for pb in (0, 3, 5, 32, -4):
                refused(ri, g, d_f, d_p, 64, 1, 256, pb, d_o)
            refused(ri, g, d_f, d_p, 64, 0, 256, 4, d_o)                      # n_planes
            refused(ri, g, d_f, d_p, 64, -1, 256, 4, d_o)
            refused(ri, g, 0, d_p, 64, 1, 256, 4, d_o)                        # NULL pointers
            refused(ri, g, d_f, 0, 64, 1, 256, 4, d_o)
            refused(ri, g, d_f, d_p, 64, 1, 256, 4, 0)
            refused(ri, g, d_f + 2, d_p, 64, 1, 256, 4, d_o)                  # misaligned pointers
            refused(ri, g, d_f, d_p + 2, 64, 1, 256, 4, d_o)
            refused(ri, g, d_f, d_p, 64, 1, 256, 8, d_o + 4)
            refused(ri, g, d_f, d_p, 64, 2, 258, 4, d_o)                      # a misaligned stride
            refused(ri, g, d_f, d_p, 64, 1, 256, 4, d_o, [0, 258])            # misaligned offsets
            refused(ri, g, d_f, d_p, 64, 1, 256, 4, d_o, None, [0, 258])
            refused(ri, g, d_f, d_p, 64, 1, 256, 16, d_o, None, [0, 264])
            L = HG.lib()
            geoms = HG._geoms(g)
            vp = HG.C.c_void_p
            assert L.hg_remap_index_frames_device(c._h, geoms, -1, vp(d_f), None, vp(d_p), 64, 1, 256, 4, vp(d_o), None) == INVALID
            assert L.hg_remap_index_frames_device(c._h, None, 2, vp(d_f), None, vp(d_p), 64, 1, 256, 4, vp(d_o), None) == INVALID
            assert L.hg_remap_bilinear_frames_device(c._h, geoms, -1, vp(d_f), None, vp(d_p), 4, 4, 1, 256, 0, 1, vp(d_o), None) == INVALID
            assert L.hg_remap_bilinear_frames_device(c._h, None, 2, vp(d_f), None, vp(d_p), 4, 4, 1, 256, 0, 1, vp(d_o), None) == INVALID
            # n_frames == 0: HG_OK whatever the pointers
            assert L.hg_remap_index_frames_device(c._h, None, 0, None, None, None, 0, 1, 0, 4, None, None) == 0
            assert L.hg_remap_bilinear_frames_device(c._h, None, 0, None, None, None, 4, 4, 1, 0, 1, 1, None, None) == 0
            still_works()
            # bilinear: (geoms, d_coords, d_planes, W, H, n_planes, stride, elem, channels, d_out, field_offsets, out_offsets)
            for elem in (2, -1):
                refused(rb, g, d_f, d_p, 4, 4, 1, 256, elem, 1, d_o)
            for ch in (0, 5):
                refused(rb, g, d_f, d_p, 4, 4, 1, 256, F32E, ch, d_o)
                refused(rb, g, d_f, d_p, 4, 4, 1, 256, U8E, ch, d_o)
                refused(ru, d_f, 16, d_p, 4, 4, ch, d_o)
            for w, h in ((0, 4), (4, 0), (-1, 4)):
                refused(rb, g, d_f, d_p, w, h, 1, 256, U8E, 1, d_o)
                refused(ru, d_f, 16, d_p, w, h, 1, d_o)
            refused(rb, g, d_f, d_p, 4, 4, 0, 256, U8E, 1, d_o)               # n_planes
            refused(rb, g, 0, d_p, 4, 4, 1, 256, U8E, 1, d_o)                 # NULL pointers
            refused(rb, g, d_f, 0, 4, 4, 1, 256, U8E, 1, d_o)
            refused(rb, g, d_f, d_p, 4, 4, 1, 256, U8E, 1, 0)
            refused(ru, 0, 16, d_p, 4, 4, 1, d_o)
            refused(ru, d_f, 16, 0, 4, 4, 1, d_o)
            refused(ru, d_f, 16, d_p, 4, 4, 1, 0)
            refused(rb, g, d_f + 4, d_p, 4, 4, 1, 256, U8E, 1, d_o)           # misaligned coordinates
            refused(ru, d_f + 4, 16, d_p, 4, 4, 1, d_o)
            refused(rb, g, d_f, d_p + 2, 4, 4, 1, 256, F32E, 1, d_o)          # misaligned f32 planes / output / stride / offsets
            refused(rb, g, d_f, d_p, 4, 4, 1, 256, F32E, 1, d_o + 1)
            refused(rb, g, d_f, d_p, 4, 4, 2, 258, F32E, 1, d_o)
            refused(rb, g, d_f, d_p, 4, 4, 1, 256, F32E, 1, d_o, None, [0, 258])
            refused(rb, g, d_f, d_p, 4, 4, 1, 256, U8E, 1, d_o, [0, 260])
        finally:
            c.free(d)


# ------------------------------------------------------------------------------------------------ redo ordering
def test_a_queued_redo_never_lands_on_a_later_frames_remap():
    """A piecewise warp whose rows carry 1100 spans is queued into buffer B (its frame is flagged, to be redone through the map at hg_sync); a
    frames remap then writes B.  After hg_sync B holds the remap."""
    s = GF.strip_mesh_overflow()
    img, W2, H2, g = s.img, s.W, s.H, s.g
    npx = g[2] * g[3]
    fld = ((np.arange(npx, dtype=np.int64) * 7919) % (W2 * H2)).astype(np.int32)
    want = FM.remap_index(fld, img.reshape(-1, 4))
    with HG.Context(0) as c:
        d_src, d_f, d_b = c.alloc(img.nbytes), c.alloc(npx * 4), c.alloc(npx * 4)
        try:
            c.to_device(d_src, img)
            c.to_device(d_f, fld)
            c.set_image_device(d_src, W2, H2)
            c.piecewise_set_mesh(s.sp, s.tris, *s.min_src)
            c.piecewise_set_frames(s.dp, [g], [0])
            r0 = c.redone_frames()
            c.warp_inverse_piecewise_frames_device(d_b)
            c.remap_index_frames_device([g], d_f, d_src, W2 * H2, 1, 0, 4, d_b)
            c.sync()
            assert c.redone_frames() > r0                      # the warp's frame WAS flagged and redone ...
            got = c.to_host(d_b, npx * 4).reshape(npx, 4)
            assert np.array_equal(got, want)                   # ... and the remap stands
        finally:
            c.set_image(img)
            for p in (d_src, d_f, d_b):
                c.free(p)


# ------------------------------------------------------------------------------------------------ the drop-in class
def test_js_class_remap():
    """tests/js/remap_gpu.mjs: remap() of js/Homography.mjs on the real addon, for affine, projective and piecewise instances."""
    res = GF.run_node_case("remap_gpu.mjs")
    assert set(res["report"]) == {"affine", "projective", "piecewise"}
