"""The device-side harness the field-consuming GPU tests share (tests/test_gpu_remap_frames.py, _trilinear, _aniso, _bicubic, _mosaic,
_mosaic_gain; refusal_code, u32 and run_node_case also serve the other test_gpu_*.py files): the poisoned upload / fill / call / download
routines, the checks that every frame equals its model and that no other byte was written, and the inputs of the two scenarios every
consumer repeats.  No fixtures and no assertions about a kernel live here: each test file keeps its geometry, its models and its tests.
tests/test_gpu_harness_cpu.py pins this module on the CPU over a fake context."""
import collections
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
import hgwarp as HG                          # noqa: E402
from hgtest import oracle as O               # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest import trilinear as TM           # noqa: E402
from hgtest import workloads as WL           # noqa: E402

CO = HG.FIELD_COORDS
F32E, U8E = HG.ELEM_F32, HG.ELEM_U8
F32 = np.float32
INVALID = 1
FILL, POISON = 0xA5, 0xEE                    # the outputs and the pyramids before a call; the bytes around the source planes


def es(elem):
    return 1 if elem == U8E else 4


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def place(parts, offs, total, fill):
    buf = np.full(total, fill, np.uint8)
    for p, o in zip(parts, offs):
        b = np.ascontiguousarray(p).view(np.uint8).ravel()
        buf[o:o + b.size] = b
    return buf


def split(raw, offs, geoms, px_bytes, dtype, cols):
    """Read-only copies of the frames of a packed download; a coordinate field is split(raw, offs, geoms, 8, F32, 2)."""
    out = []
    for o, g in zip(offs, geoms):
        a = raw[o:o + RF.n_px(g) * px_bytes].view(dtype).reshape(-1, cols).copy()
        a.setflags(write=False)
        out.append(a)
    return out


def random_planes(seed, elem, shape, n, f32_affine=(40, 3)):
    """n read-only planes: uint8 values 1..159 (no byte equals FILL or POISON), or normal float32 values times f32_affine[0] plus
    f32_affine[1] (None: as drawn)."""
    rng = np.random.default_rng(seed)
    if elem == U8E:
        ps = [rng.integers(1, 160, shape, dtype=np.uint8) for _ in range(n)]
    elif f32_affine is None:
        ps = [rng.standard_normal(shape).astype(F32) for _ in range(n)]
    else:
        ps = [(rng.standard_normal(shape) * f32_affine[0] + f32_affine[1]).astype(F32) for _ in range(n)]
    for p in ps:
        p.setflags(write=False)
    return tuple(ps)


# ------------------------------------------------------------------------------------------------ frames remaps: run and check
Buffers = collections.namedtuple("Buffers", "d_f d_p stride d_o d_y pyr_stride")      # what `call` gets; d_p is the first plane
Ran = collections.namedtuple("Ran", "raw oo pyr pyr_stride")                          # pyr is None without a pyramid


def run_frames(ctx, geoms, fields, fld_px, planes, px_bytes, call, foffs=None, ooffs=None, stride=None, front=256, pyramid=None):
    """Upload the fields (at foffs, or packed; over 0x11) and the planes (inside an allocation full of POISON, `front` bytes in, `stride`
    apart), fill the output with FILL, run call(Buffers), sync, and return Ran(output bytes, output offsets, ...).  With
    pyramid=(elem, channels, levels, slack) the pyramids (one per plane, `slack` bytes between them) are filled with FILL and built before
    `call`, and come back too."""
    fo = list(foffs) if foffs is not None else RF.pack(geoms, fld_px)[0]
    oo = list(ooffs) if ooffs is not None else RF.pack(geoms, px_bytes)[0]
    plane_bytes = planes[0].nbytes
    stride = stride if stride is not None else (plane_bytes + 255) // 256 * 256 + 256
    assert stride >= plane_bytes
    f_total = max([o + RF.n_px(g) * fld_px for o, g in zip(fo, geoms)] + [0]) + 256
    o_total = max([o + RF.n_px(g) * px_bytes for o, g in zip(oo, geoms)] + [0]) + 512
    p_total = front + stride * len(planes) + 256
    pyr_stride = y_total = 0
    if pyramid is not None:
        elem, ch, levels, slack = pyramid
        h, w = planes[0].shape[:2]
        pyr_stride = TM.layout(w, h, px_bytes, levels)[1] + slack
        y_total = pyr_stride * len(planes) + 256
    d_f, d_p, d_o = ctx.alloc(f_total), ctx.alloc(p_total), ctx.alloc(o_total)
    d_y = ctx.alloc(y_total) if pyramid is not None else 0
    try:
        ctx.to_device(d_f, place(fields, fo, f_total, 0x11))
        ctx.to_device(d_p, place(planes, [front + k * stride for k in range(len(planes))], p_total, POISON))
        ctx.to_device(d_o, np.full(o_total, FILL, np.uint8))
        if pyramid is not None:
            ctx.to_device(d_y, np.full(y_total, FILL, np.uint8))
            ctx.pyramid_build_device(d_p + front, w, h, len(planes), stride, elem, ch, levels, d_y, pyr_stride)
        call(Buffers(d_f, d_p + front, stride, d_o, d_y, pyr_stride))
        ctx.sync()
        return Ran(ctx.to_host(d_o, o_total), oo, ctx.to_host(d_y, y_total) if pyramid is not None else None, pyr_stride)
    finally:
        for p in (d_f, d_p, d_o) + ((d_y,) if pyramid is not None else ()):
            ctx.free(p)


def check_frames(raw, oo, geoms, want, px_bytes, what, fill=FILL):
    """Every frame equals the model, bit for bit, and every byte outside the frames is still `fill`."""
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
    assert (raw[untouched] == fill).all(), (what, "bytes between the frames, the padding and the tail must not be written")


# ------------------------------------------------------------------------------------------------ the mosaic: run and check
def run_mosaic(ctx, geoms, fields, frames, elem, ch, src_w, src_h, mode, feather, canvas, gains=None, weight=True, foffs=None, poffs=None,
               front=0, cfront=0):
    """Upload the fields (at foffs, or packed) and the frames (inside an allocation full of POISON, `front` bytes in; at poffs, or packed),
    fill the canvas and the weight plane with FILL, run the mosaic (with gains, if any), check that no byte outside the canvas extent
    (cfront bytes in) and the weight extent changed, and return (canvas bytes, weights or None)."""
    px = ch * es(elem)
    fo = list(foffs) if foffs is not None else RF.pack(geoms, 8)[0]
    po = list(poffs) if poffs is not None else RF.pack(geoms, px)[0]
    f_total = max([o + RF.n_px(g) * 8 for o, g in zip(fo, geoms)] + [0]) + 256
    p_total = front + max([o + RF.n_px(g) * px for o, g in zip(po, geoms)] + [0]) + 256
    n = max(canvas[2], 0) * max(canvas[3], 0)
    c_total, w_total = cfront + n * px + 512, n * 4 + 512
    d_f, d_p, d_c, d_w = ctx.alloc(f_total), ctx.alloc(p_total), ctx.alloc(c_total), ctx.alloc(w_total)
    try:
        ctx.to_device(d_f, place(fields, fo, f_total, 0x11))
        ctx.to_device(d_p, place(frames, [front + o for o in po], p_total, POISON))
        ctx.to_device(d_c, np.full(c_total, FILL, np.uint8))
        ctx.to_device(d_w, np.full(w_total, FILL, np.uint8))
        ctx.mosaic_frames_device(geoms, d_f, d_p + front, elem, ch, src_w, src_h, mode, feather, canvas, d_c + cfront, d_w if weight else 0, foffs, poffs,
                                 gains=gains)
        ctx.sync()
        raw, wraw = ctx.to_host(d_c, c_total), ctx.to_host(d_w, w_total)
    finally:
        for p in (d_f, d_p, d_c, d_w):
            ctx.free(p)
    assert (raw[:cfront] == FILL).all() and (raw[cfront + n * px:] == FILL).all(), "bytes outside the canvas must not be written"
    assert (wraw[n * 4 if weight else 0:] == FILL).all(), "bytes outside the weight plane must not be written"
    return raw[cfront:cfront + n * px], (wraw[:n * 4].view(F32) if weight else None)


def check_canvas(got, want, what):
    """(canvas bytes, weights or None) of run_mosaic against the model's (canvas, weight plane), bit for bit."""
    canvas, weight = got
    wc, ww = want
    w = np.ascontiguousarray(wc).view(np.uint8).ravel()
    if not np.array_equal(canvas, w):
        bad = np.flatnonzero(canvas != w)
        px = wc.dtype.itemsize * wc.shape[2]
        raise AssertionError(f"{what}: {bad.size} of {w.size} bytes differ, first at pixel {int(bad[0]) // px} (row width {wc.shape[1]}): "
                             f"got {canvas[bad[:8]].tolist()}, want {w[bad[:8]].tolist()}")
    if weight is not None:
        assert np.array_equal(weight.view(np.uint32), ww.ravel().view(np.uint32)), (what, "weight plane")


# ------------------------------------------------------------------------------------------------ refusals and what a call leaves alone
def refusal_code(fn, *a, **k):
    with pytest.raises(HG.HgError) as e:
        fn(*a, **k)
    return e.value.code


def tap_state(c):
    return (c.last_piecewise_kernel(), c.last_piecewise_variant(), c.last_piecewise_self(), c.last_piecewise_flag(), c.last_geometric_kernel(),
            c.last_forward_kernel(), c.last_forward_field_kernel(), c.sampling, c.redone_frames(), c.layout_walks())


# ------------------------------------------------------------------------------------------------ the inputs of the two repeated scenarios
Strip = collections.namedtuple("Strip", "img W H sp tris dp min_src g")


def strip_mesh_overflow():
    """A 2400 x 8 source under a strip of 1100 triangles, stretched 1.5 x downwards: every row of the window g carries more spans than the
    row kernel holds, so a queued piecewise warp of it is flagged and redone at hg_sync."""
    n, W2, H2 = 1100, 2400, 8
    img = WL.lcg_image(W2, H2, 10)
    xs = np.linspace(0, W2, n + 1)
    sp = np.stack([np.repeat(xs, 2), np.tile([0.0, H2], n + 1)], 1).astype(np.float32).ravel()
    tr = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(n)], np.uint32).ravel()
    dp = sp.copy()
    dp[1::2] *= 1.5
    mm, md = O.minmax_xy(sp), O.minmax_xy(dp)
    g = (int(md[0]), int(md[1]), int(md[2] - md[0]), int(md[3] - md[1]))
    return Strip(img, W2, H2, sp, tr, dp, (int(mm[0]), int(mm[1])), g)


def oblique_projective_set(scale, shift=None, W=64, H=40, fit=((0, 0), (48, 32))):
    """Three projective frames of a W x H picture: its corners sent to projective_dst(W, H, 0.03 k) times `scale` (a number, or one per
    axis), plus k times `shift`.  Returns (img, s4, d4s, windows, packed RGBA offsets, total); every window is larger than fit[0] and at most
    fit[1] (fit=None: any)."""
    F = 3
    img = WL.lcg_image(W, H, 81)
    s4 = WL.corners(W, H)
    by = scale if np.isscalar(scale) else np.tile(scale, 4)
    d4s = [WL.projective_dst(W, H, 0.03 * k) * by for k in range(F)]
    if shift is not None:
        d4s = [d4 + np.tile([shift[0] * k, shift[1] * k], 4) for k, d4 in enumerate(d4s)]
    gg = [tuple(int(v) for v in O.transform_limits(1, O.projective_from_squares(s4, d4), W, H)) for d4 in d4s]
    if fit is not None:
        assert all(fit[0][0] < g[2] <= fit[1][0] and fit[0][1] < g[3] <= fit[1][1] for g in gg), gg
    offs, total = HG.pack_offsets(gg)
    return img, s4, d4s, gg, offs, total


# ------------------------------------------------------------------------------------------------ the drop-in class on the real addon
def run_node_case(script, *args, timeout=300, verdict=True):
    """Run tests/js/<script> under node from the repository root and return the record of its last JSON line; verdict: the record carries
    `ok` and `fails`, and both must be clean."""
    node = shutil.which("node")
    addon = os.path.join(ROOT, "homography.js_amd", "lib", "hgwarp.node")
    assert node is not None and os.path.exists(addon), "node and the N-API addon are needed on a GPU box"
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", script), *args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    if verdict:
        assert p.returncode == 0 and res["ok"] and not res["fails"], (res["fails"], p.stderr[-2000:])
    else:
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return res


def js_pattern_planes(W, H):
    """The planes the tests/js/*_gpu.mjs scripts build: (H, W, 4) uint8 and (H, W, 1) float32."""
    idx = np.arange(W * H * 4, dtype=np.int64)
    u8 = ((idx * 7 + (idx >> 3) * 13) & 255).astype(np.uint8).reshape(H, W, 4)
    f32 = ((idx[:W * H] * 37 % 1001) * 0.25 - 100).astype(F32).reshape(H, W, 1)
    return u8, f32
