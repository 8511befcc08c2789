"""tests/hgtest/gpu_frames.py on the CPU: the harness of the field-consuming GPU tests over a fake context (one bytearray arena), so that
its layouts are the documented ones and its checks fail when they should."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest import trilinear as TM           # noqa: E402
from hgtest import workloads as WL           # noqa: E402

FILL, POISON, F32 = GF.FILL, GF.POISON, GF.F32
# the first three frames of test_gpu_aniso's GRID around an empty frame, and a frame of one pixel
GEOMS = [(0, 0, 48, 32), (0, 0, 1, 7), (0, 0, 0, 5), (2, 1, 33, 5), (3, -2, 1, 1)]
PX = 3
SHAPE = (5, 7, PX)                           # the planes: 105 bytes each


class FakeContext:
    """Device memory is one arena; an address is an index into it."""

    def __init__(self):
        self.mem, self.top, self.live, self.log = bytearray(1 << 18), 256, {}, []

    def alloc(self, n):
        at, self.top = self.top, (self.top + n + 255) // 256 * 256 + 256
        assert self.top <= len(self.mem)
        self.live[at] = n
        return at

    def free(self, at):
        del self.live[at]

    def to_device(self, at, arr, offset=0):
        b = np.ascontiguousarray(arr).view(np.uint8).ravel()
        self.mem[at + offset:at + offset + b.size] = b.tobytes()

    def to_host(self, at, n, offset=0):
        return np.frombuffer(bytes(self.mem[at + offset:at + offset + n]), np.uint8).copy()

    def sync(self):
        self.log.append("sync")

    def pyramid_build_device(self, *a):
        self.log.append(("pyramid",) + a)


def _inputs():
    rng = np.random.default_rng(1)
    fields = [rng.random((RF.n_px(g), 2)).astype(F32) for g in GEOMS]
    planes = GF.random_planes(2, GF.U8E, SHAPE, 2)
    want = [rng.integers(1, 160, (RF.n_px(g), PX), dtype=np.uint8) for g in GEOMS]
    return fields, planes, want


def _writer(ctx, want, oo, seen):
    """A `call` that records what lies on the device and then writes the wanted frames itself."""
    def call(b):
        seen["b"] = b
        seen["sizes"] = [ctx.live[p] for p in sorted(ctx.live)]
        seen["fields"] = ctx.to_host(b.d_f, ctx.live[b.d_f])
        seen["out"] = ctx.to_host(b.d_o, ctx.live[b.d_o])
        seen["log"] = list(ctx.log)
        for w, o in zip(want, oo):
            ctx.to_device(b.d_o, w, o)
    return call


def _planes_allocation(ctx, b, front):
    return ctx.to_host(b.d_p - front, ctx.live[b.d_p - front])


# ------------------------------------------------------------------------------------------------ run_frames
def test_run_frames_packed_layout():
    fields, planes, want = _inputs()
    fo, oo = RF.pack(GEOMS, 8)[0], RF.pack(GEOMS, PX)[0]
    f_total, o_total = fo[-1] + 8 + 256, oo[-1] + PX + 512
    stride = 256 + 256                                            # 105 bytes rounded up to 256, and 256 more
    p_total = 256 + 2 * stride + 256
    ctx, seen = FakeContext(), {}
    planes_seen = []
    call = _writer(ctx, want, oo, seen)
    ran = GF.run_frames(ctx, GEOMS, fields, 8, planes, PX, lambda b: (planes_seen.append(_planes_allocation(ctx, b, 256)), call(b)))
    b = seen["b"]
    assert seen["sizes"] == [f_total, p_total, o_total] and (b.stride, b.d_y, b.pyr_stride) == (stride, 0, 0)
    assert b.d_f % 256 == 0 and b.d_f > 0
    assert np.array_equal(seen["fields"], GF.place(fields, fo, f_total, 0x11)) and (seen["fields"][-256:] == 0x11).all()
    assert np.array_equal(seen["fields"][fo[3]:fo[3] + 8 * 165].view(F32).reshape(-1, 2), fields[3])
    expect = np.full(p_total, POISON, np.uint8)
    for k, p in enumerate(planes):
        expect[256 + k * stride:256 + k * stride + p.nbytes] = p.ravel()
    assert np.array_equal(planes_seen[0], expect)
    assert seen["out"].size == o_total and (seen["out"] == FILL).all() and seen["log"] == []
    assert ctx.log == ["sync"] and not ctx.live                   # synchronised after the call, everything freed
    assert ran.oo == oo and ran.raw.size == o_total and ran.pyr is None
    GF.check_frames(ran.raw, ran.oo, GEOMS, want, PX, "packed")


def test_run_frames_explicit_offsets_stride_front_and_pyramid():
    fields, planes, want = _inputs()
    fo = [o + 8 * (2 * f + 1) + 512 * f for f, o in enumerate(RF.pack(GEOMS, 8)[0])]
    oo = [o + 640 * f + 7 for f, o in enumerate(RF.pack(GEOMS, PX)[0])]
    stride, front, levels, slack = planes[0].nbytes + 5, 17, 3, 256 + 9
    f_total, o_total, p_total = fo[-1] + 8 + 256, oo[-1] + PX + 512, front + 2 * stride + 256
    pyr_stride = TM.layout(SHAPE[1], SHAPE[0], PX, levels)[1] + slack
    y_total = 2 * pyr_stride + 256
    ctx, seen = FakeContext(), {}
    planes_seen, pyr_seen = [], []
    call = _writer(ctx, want, oo, seen)

    def both(b):
        planes_seen.append(_planes_allocation(ctx, b, front))
        pyr_seen.append(ctx.to_host(b.d_y, ctx.live[b.d_y]))
        call(b)
        ctx.to_device(b.d_y, np.uint8([1, 2, 3]), 5)

    ran = GF.run_frames(ctx, GEOMS, fields, 8, planes, PX, both, fo, oo, stride, front, pyramid=(GF.U8E, PX, levels, slack))
    b = seen["b"]
    assert seen["sizes"] == [f_total, p_total, o_total, y_total] and (b.stride, b.pyr_stride) == (stride, pyr_stride)
    assert np.array_equal(seen["fields"], GF.place(fields, fo, f_total, 0x11))
    expect = np.full(p_total, POISON, np.uint8)
    for k, p in enumerate(planes):
        expect[front + k * stride:front + k * stride + p.nbytes] = p.ravel()
    assert np.array_equal(planes_seen[0], expect)
    assert (seen["out"] == FILL).all() and pyr_seen[0].size == y_total and (pyr_seen[0] == FILL).all()
    assert seen["log"] == [("pyramid", b.d_p, SHAPE[1], SHAPE[0], 2, stride, GF.U8E, PX, levels, b.d_y, pyr_stride)]      # built before the call
    assert ctx.log[-1] == "sync" and not ctx.live
    assert ran.oo == oo and ran.pyr_stride == pyr_stride and ran.pyr.size == y_total and ran.pyr[5:8].tolist() == [1, 2, 3]
    GF.check_frames(ran.raw, ran.oo, GEOMS, want, PX, "explicit")


def test_run_frames_refuses_a_stride_below_the_plane():
    fields, planes, want = _inputs()
    ctx = FakeContext()
    with pytest.raises(AssertionError):
        GF.run_frames(ctx, GEOMS, fields, 8, planes, PX, lambda b: None, stride=planes[0].nbytes - 1)
    assert not ctx.live


# ------------------------------------------------------------------------------------------------ check_frames
def _exact(oo):
    want = _inputs()[2]
    total = oo[-1] + PX + 512
    return GF.place(want, oo, total, FILL), want


def test_check_frames_passes_on_an_exact_result_and_fails_on_every_single_wrong_byte():
    oo = RF.pack(GEOMS, PX)[0]
    raw, want = _exact(oo)
    GF.check_frames(raw, oo, GEOMS, want, PX, "exact")
    n = [RF.n_px(g) * PX for g in GEOMS]
    assert n == [4608, 21, 0, 495, 3] and oo[1] + n[1] < oo[2] == oo[3]      # padding behind frame 1; the empty frame takes no room
    spots = {"first byte of frame 0": oo[0], "last byte of frame 0": oo[0] + n[0] - 1, "inside frame 3": oo[3] + 100,
             "first byte of the one-pixel frame": oo[4], "last byte of the one-pixel frame": oo[4] + 2,
             "padding right behind frame 1": oo[1] + n[1], "padding right in front of frame 3": oo[3] - 1,
             "right behind the last frame": oo[4] + n[4], "the last byte of the tail": raw.size - 1}
    for what, at in spots.items():
        for flip in (1, 0x80):
            bad = raw.copy()
            bad[at] ^= flip
            with pytest.raises(AssertionError):
                GF.check_frames(bad, oo, GEOMS, want, PX, what)
    GF.check_frames(raw, oo, GEOMS, want, PX, "still exact")        # (the copies were changed, not the result)


def test_check_frames_guards_the_bytes_in_front_of_an_offset_first_frame_and_the_size_of_want():
    oo = [o + 640 * f + 7 for f, o in enumerate(RF.pack(GEOMS, PX)[0])]
    raw, want = _exact(oo)
    GF.check_frames(raw, oo, GEOMS, want, PX, "exact, explicit offsets")
    for at in (oo[0] - 1, 0, oo[1] - 1):
        bad = raw.copy()
        bad[at] = 0
        with pytest.raises(AssertionError):
            GF.check_frames(bad, oo, GEOMS, want, PX, at)
    for f, wrong in ((1, np.zeros((8, PX), np.uint8)), (1, want[1][:6]), (2, np.zeros((1, PX), np.uint8)), (4, want[4].view(np.uint8)[:, :2])):
        w = list(want)
        w[f] = wrong
        with pytest.raises(AssertionError):
            GF.check_frames(raw, oo, GEOMS, w, PX, ("size", f))
    other = np.where(raw == FILL, np.uint8(0), raw)                # another fill is another check
    GF.check_frames(other, oo, GEOMS, want, PX, "fill 0", fill=0)
    with pytest.raises(AssertionError):
        GF.check_frames(other, oo, GEOMS, want, PX, "fill 0 against FILL")


# ------------------------------------------------------------------------------------------------ check_canvas
def test_check_canvas_compares_canvas_bytes_and_weight_bits():
    rng = np.random.default_rng(3)
    wc, ww = rng.standard_normal((4, 6, 2)).astype(F32), rng.random((4, 6)).astype(F32)
    ww[0, 0] = 0.0
    got = (wc.view(np.uint8).ravel().copy(), ww.ravel().copy())
    GF.check_canvas(got, (wc, ww), "exact")
    GF.check_canvas((got[0], None), (wc, ww), "no weight plane asked for")
    for k in (0, ww.size - 1, 7):
        bits = got[1].view(np.uint32).copy()
        bits[k] ^= 1 if k else 0x80000000                          # one bit; at [0] the sign of a zero: equal as a number, not as bits
        with pytest.raises(AssertionError):
            GF.check_canvas((got[0], bits.view(F32)), (wc, ww), ("weight", k))
    for k in (0, got[0].size - 1):
        c = got[0].copy()
        c[k] ^= 1
        with pytest.raises(AssertionError):
            GF.check_canvas((c, got[1]), (wc, ww), ("canvas", k))


# ------------------------------------------------------------------------------------------------ the small helpers
def test_split_returns_read_only_copies_and_place_overlays_in_order():
    raw = np.arange(4096, dtype=np.uint32).view(np.uint8)
    geoms = [(0, 0, 3, 2), (0, 0, 0, 4), (5, 5, 2, 1)]
    parts = GF.split(raw, [0, 256, 256], geoms, 8, F32, 2)
    assert [p.shape for p in parts] == [(6, 2), (0, 2), (2, 2)] and all(p.dtype == F32 and not p.flags.writeable for p in parts)
    assert np.array_equal(parts[2].view(np.uint32).ravel(), np.arange(64, 68))
    assert not any(np.shares_memory(p, raw) for p in parts)
    rgba = GF.split(raw, [16], [(0, 0, 2, 2)], 4, np.uint8, 4)[0]
    assert rgba.shape == (4, 4) and rgba.dtype == np.uint8 and rgba[1].tolist() == [5, 0, 0, 0]
    with pytest.raises(ValueError):
        parts[0][0, 0] = 1
    buf = GF.place([np.uint8([1, 2, 3, 4]), np.uint16([0x0605]), np.zeros(0, F32)], [2, 4, 9], 12, 0xEE)
    assert buf.tolist() == [0xEE, 0xEE, 1, 2, 5, 6, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE] and buf.dtype == np.uint8      # the later part lies on top
    assert GF.place([], [], 3, 7).tolist() == [7, 7, 7]
    assert (GF.es(GF.U8E), GF.es(GF.F32E)) == (1, 4) and GF.u32(np.float32([1.0])).tolist() == [0x3F800000]


# ------------------------------------------------------------------------------------------------ the scenario builders
def test_strip_mesh_overflow_is_the_inline_scenario():
    n, W2, H2 = 1100, 2400, 8
    img = WL.lcg_image(W2, H2, 10)
    xs = np.linspace(0, W2, n + 1)
    sp = np.stack([np.repeat(xs, 2), np.tile([0.0, H2], n + 1)], 1).astype(np.float32).ravel()
    tr = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(n)], np.uint32).ravel()
    dp = sp.copy()
    dp[1::2] *= 1.5
    mm, md = O.minmax_xy(sp), O.minmax_xy(dp)
    g = (int(md[0]), int(md[1]), int(md[2] - md[0]), int(md[3] - md[1]))
    s = GF.strip_mesh_overflow()
    for got, want in ((s.img, img), (s.sp, sp), (s.tris, tr), (s.dp, dp)):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    assert (s.W, s.H, s.min_src, s.g) == (W2, H2, (int(mm[0]), int(mm[1])), g) and g == (0, 0, 2400, 12) and tr.size == 3 * 1100


@pytest.mark.parametrize("name", ("aniso", "mosaic", "trilinear", "bicubic"))
def test_oblique_projective_set_is_the_inline_scenario(name):
    W, H, F = {"trilinear": (256, 160, 3), "bicubic": (24, 16, 3)}.get(name, (64, 40, 3))
    img = WL.lcg_image(W, H, 81)
    s4 = WL.corners(W, H)
    if name == "aniso":
        d4s = [WL.projective_dst(W, H, 0.03 * k) * np.tile([0.6, 0.15], 4) for k in range(F)]
        got = GF.oblique_projective_set((0.6, 0.15))
    elif name == "mosaic":
        d4s = [WL.projective_dst(W, H, 0.03 * k) * np.tile([0.6, 0.45], 4) + np.tile([7.0 * k, 3.0 * k], 4) for k in range(F)]
        got = GF.oblique_projective_set((0.6, 0.45), (7.0, 3.0))
    elif name == "trilinear":
        d4s = [WL.projective_dst(W, H, 0.03 * k) * 0.3 for k in range(F)]
        got = GF.oblique_projective_set(0.3, W=256, H=160, fit=None)
    else:
        d4s = [WL.projective_dst(W, H, 0.03 * k) * np.tile([1.9, 1.9], 4) for k in range(F)]
        got = GF.oblique_projective_set((1.9, 1.9), W=24, H=16, fit=((24, 16), (48, 32)))
    gg = [tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W, H)) for d4 in d4s]
    offs, total = HG.pack_offsets(gg)
    assert np.array_equal(got[0], img) and np.array_equal(got[1], s4) and got[1].dtype == s4.dtype
    assert len(got[2]) == F and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got[2], d4s))
    assert got[3:] == (gg, offs, total)
    if name == "trilinear":
        assert max(g[2] for g in gg) > 48
        with pytest.raises(AssertionError):
            GF.oblique_projective_set(0.3, W=256, H=160)             # the windows must fit 48 x 32 unless told otherwise
