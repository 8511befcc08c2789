"""Numpy model of the mip pyramids and the trilinear remap (include/hgwarp.h, hg_pyramid_* / hg_remap_trilinear_frames_device).  Test
infrastructure only.  One np.float32 operation per step the header writes (numpy does not fuse); the bilinear rule on a level is
tests/hgtest/field.py's remap_bilinear_f32 itself.

    n_levels, level_sizes, layout   the host-only geometry of a pyramid
    down, pyramid                   level k from level k - 1; [plane, level 1, ..., level levels-1]
    footprint, level_choice         q of every pixel of a frame; (k, two, t) from q
    remap_trilinear                 one frame; trilinear_frames: frame f reads pyramid f % n_planes"""
import numpy as np

from . import field as FM

F32 = np.float32


def n_levels(w, h):
    if w < 1 or h < 1:
        return 0
    n = 1
    while w > 1 or h > 1:
        w, h, n = (w + 1) >> 1, (h + 1) >> 1, n + 1
    return n


def level_sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(1, levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        out.append((w, h))
    return out


def layout(w, h, px_bytes, levels):
    """(offsets, total) of one pyramid buffer: offsets[0] = 0 unused, levels 1.. packed at 256-byte aligned starts."""
    offs, off = [0], 0
    for wk, hk in level_sizes(w, h, levels)[1:]:
        offs.append(off)
        off += (wk * hk * px_bytes + 255) // 256 * 256
    return offs, off


def down(a):
    """(H, W, C) uint8 or float32 -> ((H + 1) >> 1, (W + 1) >> 1, C)."""
    a = np.asarray(a)
    H, W, _ = a.shape
    ys, xs = np.arange((H + 1) >> 1), np.arange((W + 1) >> 1)
    r0, r1 = np.minimum(2 * ys, H - 1), np.minimum(2 * ys + 1, H - 1)
    c0, c1 = np.minimum(2 * xs, W - 1), np.minimum(2 * xs + 1, W - 1)
    pa, pb, pc, pd = a[r0][:, c0], a[r0][:, c1], a[r1][:, c0], a[r1][:, c1]
    if a.dtype == np.uint8:
        pa, pb, pc, pd = (p.astype(np.int32) for p in (pa, pb, pc, pd))
        return ((((pa + pb) + (pc + pd)) + 2) >> 2).astype(np.uint8)
    assert a.dtype == F32
    top = pa + pb
    bot = pc + pd
    out = (top + bot) * F32(0.25)
    assert out.dtype == F32
    return out


def pyramid(plane, levels):
    out = [np.asarray(plane)]
    for _ in range(1, levels):
        out.append(down(out[-1]))
    return out


def _step2(co, fin, axis):
    """Squared step to the neighbour along axis (1: horizontal, 0: vertical): the next pixel if it exists and is finite, else the previous."""
    h, w, _ = co.shape
    nxt, prv = np.roll(co, -1, axis), np.roll(co, 1, axis)
    idx = np.arange(w)[None, :] if axis == 1 else np.arange(h)[:, None]
    n = co.shape[axis]
    a_ok = (idx + 1 < n) & np.roll(fin, -1, axis)
    b_ok = (idx >= 1) & np.roll(fin, 1, axis)
    nb = np.where(a_ok[..., None], nxt, prv)
    with np.errstate(all="ignore"):
        dx = nb[..., 0] - co[..., 0]
        dy = nb[..., 1] - co[..., 1]
        xx = dx * dx
        yy = dy * dy
        q = xx + yy
    assert q.dtype == F32
    return np.where(a_ok | b_ok, q, F32(0))


def footprint(co):
    """co: (h, w, 2) float32.  q (h, w) float32 of every pixel (meaningless where the pixel itself is not finite)."""
    co = np.asarray(co, F32)
    fin = np.isfinite(co[..., 0]) & np.isfinite(co[..., 1])
    return np.maximum(_step2(co, fin, 1), _step2(co, fin, 0))


def level_choice(q, levels):
    """(k, two, t): the level (the lower one of two), whether level k + 1 is blended in, and its weight."""
    q = np.asarray(q, F32)
    shrink = q > F32(1)
    e = (q.view(np.uint32) >> 23).astype(np.int64) - 127          # the unbiased exponent (q >= 1 is normal; +Inf: 128)
    k = np.where(shrink, e >> 1, 0)
    two = shrink & (k < levels - 1)
    k = np.minimum(k, levels - 1)
    with np.errstate(all="ignore"):
        s = np.ldexp(np.where(two, q, F32(1)), (-2 * np.where(two, k, 0)).astype(np.int32))
        assert s.dtype == F32
        t = (s - F32(1)) * F32(0.33333334)
    return k.astype(np.int32), two, np.where(two, t, F32(0)).astype(F32)


def _sample(co, level, k):
    """The bilinear rule on level k for the finite coordinates co (n, 2): unrounded float32 (n, C)."""
    if k > 0:
        inv = F32(2.0 ** -k)
        co = ((co + F32(0.5)) * inv) - F32(0.5)
        assert co.dtype == F32
    return FM.remap_bilinear_f32(co, level.astype(F32))


def remap_trilinear(co, pyr):
    """co: (h, w, 2) float32; pyr: pyramid() of the (H, W, C) plane.  Returns (h * w, C) of the plane's type."""
    co = np.asarray(co, F32)
    h, w, _ = co.shape
    levels, C = len(pyr), pyr[0].shape[2]
    flat = co.reshape(-1, 2)
    fin = np.isfinite(flat[:, 0]) & np.isfinite(flat[:, 1])
    k, two, t = (a.reshape(-1) for a in level_choice(footprint(co), levels))
    r = np.zeros((h * w, C), F32)
    for L in range(levels):
        m = fin & (k == L)
        if m.any():
            r[m] = _sample(flat[m], pyr[L], L)
        m = fin & two & (k == L - 1)
        if m.any():
            hi = _sample(flat[m], pyr[L], L)
            d = hi - r[m]
            r[m] = r[m] + d * t[m][:, None]
    assert r.dtype == F32
    if pyr[0].dtype == np.uint8:
        return np.minimum(F32(255), np.floor(r + F32(0.5))).astype(np.uint8)
    return r


def trilinear_frames(geoms, coords, pyrs):
    """coords[f]: (n_px, 2) float32 of frame f = (x_off, y_off, obj_w, obj_h); pyrs: one pyramid per plane.  Per frame (n_px, C)."""
    out = []
    for f, g in enumerate(geoms):
        w, h = max(g[2], 0), max(g[3], 0)
        pyr = pyrs[f % len(pyrs)]
        if w * h == 0:
            out.append(np.zeros((0, pyr[0].shape[2]), pyr[0].dtype))
        else:
            out.append(remap_trilinear(np.asarray(coords[f], F32).reshape(h, w, 2), pyr))
    return out
