"""Numpy model of the bicubic remap (include/hgwarp.h, hg_remap_bicubic_frames_device).  Test infrastructure only.  One np.float32
operation per step the header writes (numpy does not fuse); taps and fractions are those of tests/hgtest/field.py.

    coefficients           (p3, p2, p0, q3, q2, q1, q0) of the (B, C) cubic: in double, each rounded once to float32
    weights                (w0, w1, w2, w3) of a fraction t
    remap_bicubic          one frame's flat list; unrounded=True returns the float32 blend of a uint8 plane before the store
    bicubic_frames         frame f reads plane f % n_planes"""
import numpy as np

from . import field as FM

F32 = np.float32
CATMULL_ROM, MITCHELL, BSPLINE = (0.0, 0.5), (1 / 3, 1 / 3), (1.0, 0.0)


def coefficients(B, C):
    """The seven coefficients, from (double)(float)B and (double)(float)C as the C ABI receives them."""
    B, C = float(F32(B)), float(F32(C))
    p3 = ((12.0 - 9.0 * B) - 6.0 * C) / 6.0
    p2 = ((-18.0 + 12.0 * B) + 6.0 * C) / 6.0
    p0 = (6.0 - 2.0 * B) / 6.0
    q3 = (-B - 6.0 * C) / 6.0
    q2 = (6.0 * B + 30.0 * C) / 6.0
    q1 = (-12.0 * B - 48.0 * C) / 6.0
    q0 = (8.0 * B + 24.0 * C) / 6.0
    return tuple(F32(v) for v in (p3, p2, p0, q3, q2, q1, q0))


def _near(x, k):
    p3, p2, p0 = k[0], k[1], k[2]
    r = (((p3 * x) + p2) * x) * x + p0
    assert r.dtype == F32
    return r


def _far(x, k):
    q3, q2, q1, q0 = k[3], k[4], k[5], k[6]
    r = ((((q3 * x) + q2) * x) + q1) * x + q0
    assert r.dtype == F32
    return r


def weights(t, k):
    """t: float32 array of fractions in [0, 1); k: coefficients().  Four float32 arrays."""
    t = np.asarray(t, F32)
    return _far(F32(1) + t, k), _near(t, k), _near(F32(1) - t, k), _far(F32(2) - t, k)


def remap_bicubic(co, plane, B, C, unrounded=False):
    """co: (n, 2) float32 (sx, sy); plane: (H, W, Cn) float32 or uint8.  Returns (n, Cn) of the plane's type."""
    co = np.asarray(co, F32).reshape(-1, 2)
    plane = np.asarray(plane)
    assert plane.dtype in (np.uint8, F32)
    src = plane.astype(F32)
    H, W, Cn = src.shape
    k = coefficients(B, C)
    out = np.zeros((co.shape[0], Cn), F32)
    fin = np.isfinite(co[:, 0]) & np.isfinite(co[:, 1])
    sx, sy = co[fin, 0], co[fin, 1]
    x0, y0 = np.floor(sx), np.floor(sy)
    wx = [w[:, None] for w in weights(sx - x0, k)]
    wy = [w[:, None] for w in weights(sy - y0, k)]
    cols = [FM._tap(x0 - F32(1), W), FM._tap(x0, W), FM._tap(x0 + F32(1), W), FM._tap(x0 + F32(2), W)]
    rows = [FM._tap(y0 - F32(1), H), FM._tap(y0, H), FM._tap(y0 + F32(1), H), FM._tap(y0 + F32(2), H)]
    with np.errstate(all="ignore"):
        r = None
        for n in range(4):
            p = [src[rows[n], c] for c in cols]
            h = ((p[0] * wx[0] + p[1] * wx[1]) + p[2] * wx[2]) + p[3] * wx[3]
            r = h * wy[0] if n == 0 else r + h * wy[n]
        assert r.dtype == F32
        out[fin] = r
    if plane.dtype == np.uint8 and not unrounded:
        q = np.minimum(F32(255), np.maximum(F32(0), np.floor(out + F32(0.5))))
        assert q.dtype == F32
        return q.astype(np.uint8)
    return out


def bicubic_frames(geoms, fields, planes, B, C):
    """fields[f]: (n_px, 2) float32 of frame f; planes: list of (H, W, Cn) float32 or uint8.  Per frame (n_px, Cn) of the planes' type."""
    return [remap_bicubic(fields[f], planes[f % len(planes)], B, C) for f in range(len(geoms))]
