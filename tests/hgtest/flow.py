"""numpy model of the dense flow and of the chained field (include/hgwarp.h, "dense optical flow"), written from the header alone: the u8
pyramids, the walk from the coarsest level down, the integer window sums, the f64 solve and the f32 flow, operation by operation.  Window sums
are integers, so the model's order of summation is free and the device is compared with it byte for byte (tests/test_gpu_flow.py)."""
import collections

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
NAN_WORD = 0x7fc00000
NAN = np.array([NAN_WORD], np.uint32).view(F32)[0]
TILE_W, TILE_H = 32, 16                      # the output tile of the iteration kernel (the GPU test picks its sizes around it)
MAX_LEVELS, MAX_ITER, MAX_RADIUS = 12, 32, 7

Flow = collections.namedtuple("Flow", "field flow residual good")      # (H, W, 2) f32, (H, W, 2) f32, (H, W) u8, (H, W) u8


def luma(rgba):
    p = np.asarray(rgba).astype(np.uint32)
    return ((77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8).astype(np.uint8)


def n_levels(w, h):
    n = 1
    while w > 1 or h > 1:
        w, h, n = (w + 1) >> 1, (h + 1) >> 1, n + 1
    return n


def max_levels(w, h):
    return min(n_levels(w, h), MAX_LEVELS)


def default_levels(w, h):
    n, s = 1, min(w, h)
    while n < MAX_LEVELS and ((s + 1) >> 1) >= 16:
        s, n = (s + 1) >> 1, n + 1
    return n


def down(a):
    """(H, W) uint8 -> ((H + 1) >> 1, (W + 1) >> 1): ((a + b) + (c + d) + 2) >> 2 over columns min(2x, W-1), min(2x+1, W-1), rows alike."""
    H, W = a.shape
    ys, xs = np.arange((H + 1) >> 1), np.arange((W + 1) >> 1)
    r0, r1 = np.minimum(2 * ys, H - 1), np.minimum(2 * ys + 1, H - 1)
    c0, c1 = np.minimum(2 * xs, W - 1), np.minimum(2 * xs + 1, W - 1)
    pa, pb, pc, pd = (a[r][:, c].astype(np.int32) for r, c in ((r0, c0), (r0, c1), (r1, c0), (r1, c1)))
    return ((((pa + pb) + (pc + pd)) + 2) >> 2).astype(np.uint8)


def pyramid(plane, levels):
    out = [np.ascontiguousarray(plane, np.uint8)]
    for _ in range(1, levels):
        out.append(down(out[-1]))
    return out


def _tap(v, n):
    return np.minimum(np.minimum(np.maximum(v, F32(0)), F32(2147483520.0)).astype(np.int64), n - 1)


def bilinear(src, u, v):
    """The rule of hg_remap_bilinear_f32_device: src (H, W, C) of any dtype (taps converted to f32), u / v finite f32 arrays of one shape.
    Returns (..., C) f32."""
    H, W = src.shape[:2]
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    x0, y0 = np.floor(u), np.floor(v)
    fx, fy = u - x0, v - y0
    gx, gy = F32(1) - fx, F32(1) - fy
    c0, c1 = _tap(x0, W), _tap(x0 + F32(1), W)
    r0, r1 = _tap(y0, H), _tap(y0 + F32(1), H)
    p00, p01, p10, p11 = (src[r, c].astype(F32) for r, c in ((r0, c0), (r0, c1), (r1, c0), (r1, c1)))
    fx, fy, gx, gy = (a[..., None] for a in (fx, fy, gx, gy))
    with np.errstate(invalid="ignore", over="ignore"):
        out = (p00 * gx + p01 * fx) * gy + (p10 * gx + p11 * fx) * fy
    assert out.dtype == F32
    return out


def box(a, R):
    """Sums of the int64 plane a over the window |dx|, |dy| <= R clipped to the plane."""
    H, W = a.shape
    p = np.zeros((H + 2 * R, W + 2 * R), I64)
    p[R:R + H, R:R + W] = a
    rows = sum(p[:, k:k + W] for k in range(2 * R + 1))
    return sum(rows[k:k + H] for k in range(2 * R + 1))


def gradients(T):
    t = T.astype(I64)
    H, W = t.shape
    xs, ys = np.arange(W), np.arange(H)
    gx = t[:, np.minimum(xs + 1, W - 1)] - t[:, np.maximum(xs - 1, 0)]
    gy = t[np.minimum(ys + 1, H - 1)] - t[np.maximum(ys - 1, 0)]
    return gx, gy


def structure(T, R, min_eig):
    """(gx, gy, Gxx, Gxy, Gyy, det as f64, good) of one level."""
    gx, gy = gradients(T)
    H, W = T.shape
    gxx, gxy, gyy = box(gx * gx, R), box(gx * gy, R), box(gy * gy, R)
    xs, ys = np.arange(W), np.arange(H)
    n = ((np.minimum(ys + R, H - 1) - np.maximum(ys - R, 0) + 1)[:, None] * (np.minimum(xs + R, W - 1) - np.maximum(xs - R, 0) + 1)[None, :])
    trace, det = gxx + gyy, gxx * gyy - gxy * gxy
    good = (trace > 0) & (det > 0) & (det.astype(F64) >= ((4.0 * n.astype(F64)) * F64(min_eig)) * trace.astype(F64))
    return gx, gy, gxx, gxy, gyy, det.astype(F64), good


def grid(W, H):
    return np.arange(W, dtype=F32)[None, :].repeat(H, 0), np.arange(H, dtype=F32)[:, None].repeat(W, 1)


def sample(Fp, u, v):
    """s of every pixel: F at ((float)x + u, (float)y + v)."""
    H, W = Fp.shape
    xs, ys = grid(W, H)
    return bilinear(Fp[..., None], xs + u, ys + v)[..., 0]


def iterate(T, Fp, st, u, v, R, max_update):
    gx, gy, gxx, gxy, gyy, det, good = st
    e = sample(Fp, u, v) - T.astype(F32)
    e0 = e.astype(F64) - ((gx.astype(F64) * u.astype(F64)) + (gy.astype(F64) * v.astype(F64))) / 2.0
    eq = np.rint(16.0 * e0).astype(I64)
    bx, by = box(gx * eq, R), box(gy * eq, R)
    a, b, c, p, q = (z.astype(F64) for z in (gyy, gxy, gxx, bx, by))
    with np.errstate(divide="ignore", invalid="ignore"):
        U = -(((a * p) - (b * q)) / det) / 8.0
        V = -(((c * q) - (b * p)) / det) / 8.0
    m = F64(max_update)
    un, vn = u.copy(), v.copy()
    for new, old, tgt in ((un, u, U), (vn, v, V)):
        d = np.where(good, tgt, 0.0) - old.astype(F64)
        d = np.where(d < -m, -m, np.where(d > m, m, d))
        new[good] = (old.astype(F64) + d).astype(F32)[good]
    return un, vn


def upsample(u, v, W, H):
    """The start of a level of W x H from the flow of the level below it."""
    xs, ys = grid(W, H)
    cx, cy = (xs + F32(0.5)) * F32(0.5) - F32(0.5), (ys + F32(0.5)) * F32(0.5) - F32(0.5)
    r = bilinear(np.stack([u, v], -1), cx, cy) * F32(2.0)
    return np.ascontiguousarray(r[..., 0]), np.ascontiguousarray(r[..., 1])


def flow(frm, to, levels, n_iter=4, radius=3, min_eig=1.0, max_update=1.0):
    """One pair of one-byte planes (H, W)."""
    assert frm.shape == to.shape and frm.dtype == np.uint8 and to.dtype == np.uint8
    H, W = to.shape
    assert 1 <= levels <= max_levels(W, H) and 1 <= n_iter <= MAX_ITER and 1 <= radius <= MAX_RADIUS and min_eig >= 0 and 0 < max_update <= 4
    pf, pt = pyramid(frm, levels), pyramid(to, levels)
    u = v = None
    st = None
    for k in range(levels - 1, -1, -1):
        T, Fp = pt[k], pf[k]
        hk, wk = T.shape
        if u is None:
            u, v = np.zeros((hk, wk), F32), np.zeros((hk, wk), F32)
        else:
            u, v = upsample(u, v, wk, hk)
        st = structure(T, radius, min_eig)
        for _ in range(n_iter):
            u, v = iterate(T, Fp, st, u, v, radius, max_update)
    xs, ys = grid(W, H)
    sx, sy = xs + u, ys + v
    covered = (sx >= 0) & (sx < F32(W)) & (sy >= 0) & (sy < F32(H))
    field = np.stack([np.where(covered, sx, NAN), np.where(covered, sy, NAN)], -1).astype(F32)
    field.view(np.uint32)[~covered] = NAN_WORD
    e = bilinear(frm[..., None], sx, sy)[..., 0] - to.astype(F32)
    residual = np.minimum(F32(255), np.floor(np.abs(e) + F32(0.5))).astype(np.uint8)
    return Flow(field, np.stack([u, v], -1), residual, st[6].astype(np.uint8))


def flow_frames(frms, tos, channels, levels, **kw):
    """The frames of a call: FROM plane f onto TO plane f % len(tos); planes (H, W) or (H, W, 4)."""
    lu = (lambda p: luma(p)) if channels == 4 else (lambda p: p)
    return [flow(lu(f), lu(tos[k % len(tos)]), levels, **kw) for k, f in enumerate(frms)]


def compose(outer, inner):
    """outer (n, 2) f32 coordinates, inner (Hi, Wi, 2) f32: the bilinear remap where the coordinate and both results are finite, else NaN."""
    outer = np.asarray(outer, F32).reshape(-1, 2)
    fin = np.isfinite(outer).all(1)
    out = np.empty((outer.shape[0], 2), F32)
    out.view(np.uint32)[:] = NAN_WORD
    if fin.any():
        r = bilinear(inner, outer[fin, 0], outer[fin, 1])
        ok = np.isfinite(r).all(1)
        idx = np.flatnonzero(fin)[ok]
        out[idx] = r[ok]
    return out


def layout(W, H, channels, n_frames, n_to_sets, levels):
    """hg_flow_layout's bytes, part by part at the 256-byte grain."""
    pad = lambda b: (b + 255) // 256 * 256
    off = 0
    if channels == 4:
        off += pad(n_frames * W * H) + pad(n_to_sets * W * H)
    w, h, pyr = W, H, 0
    sizes = [(W, H)]
    for _ in range(1, levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        sizes.append((w, h))
        pyr += pad(w * h)
    off += (n_frames + n_to_sets) * pyr
    for w, h in sizes:
        off += 2 * pad(n_frames * w * h * 8)
    return off


# ------------------------------------------------------------------------------------------------ fixtures
def texture(W, H, seed, cutoff=0.12):
    """A band-limited random texture, quantised to u8: white noise low-passed in the frequency domain at `cutoff` cycles per pixel."""
    rng = np.random.default_rng(seed)
    spec = np.fft.fft2(rng.standard_normal((H, W)))
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    spec *= np.exp(-(fx * fx + fy * fy) / (2 * (cutoff / 2) ** 2))
    t = np.real(np.fft.ifft2(spec))
    t = (t - t.mean()) / t.std()
    return np.clip(np.rint(128 + 48 * t), 0, 255).astype(np.uint8)


def smooth_flow(W, H, amp=1.0):
    """The fixture's true flow: sinusoids of amplitude 5 px horizontally and 3 px vertically plus a 1.5 px offset, times amp."""
    xs, ys = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    u = amp * (5.0 * np.sin(2 * np.pi * ys / H) * np.cos(np.pi * xs / W) + 1.5)
    v = amp * (3.0 * np.cos(2 * np.pi * xs / W) * np.sin(np.pi * ys / H))
    return u.astype(F32), v.astype(F32)


def fixture(W=160, H=224, seed=7, amp=1.0):
    """(FROM, TO, u, v): TO is FROM sampled bilinearly through the true flow, rounded to u8."""
    frm = texture(W, H, seed)
    u, v = smooth_flow(W, H, amp)
    to = np.minimum(F32(255), np.floor(sample(frm, u, v) + F32(0.5))).astype(np.uint8)
    return frm, to, u, v


def epe(fl, u, v, margin=0):
    d = np.hypot(fl[..., 0].astype(F64) - u, fl[..., 1].astype(F64) - v)
    if margin:
        d = d[margin:-margin, margin:-margin]
    return float(d.mean())
