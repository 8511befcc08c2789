"""Numpy model of the source fields of the inverse warps and of the remaps through them (include/hgwarp.h, HG_FIELD_*).  Test
infrastructure only.  Everything starts from (sx, sy, valid) in f64 -- bilinear.geometric_coords / bilinear.piecewise_coords, the
latter over the CPU oracle's map and inverse matrices, never the library's.

    index field   Math.round(sy) * W + Math.round(sx) where `valid`, the unrounded coordinate is inside [minSrc, W or H + minSrc) (:1001,
                  :1047) and the index lies in [0, W*H); else -1
    coords field  (float32(sx), float32(sy)) where `valid` and inside the bounds; both words 0x7fc00000 elsewhere
    remap_index   out[i] = src[field[i]] where 0 <= field[i] < n, else zeros
    remap_bilinear_f32   f32 taps and blend, one operation per step, in the order of the library's blend"""
import numpy as np

from . import edges as E

F32 = np.float32
NAN_BITS = np.uint32(0x7FC00000)


def covered(sx, sy, valid, W, H, msx=0, msy=0):
    with np.errstate(invalid="ignore"):
        return valid & (sx >= msx) & (sx < W + msx) & (sy >= msy) & (sy < H + msy)


def index_field(sx, sy, valid, W, H, msx=0, msy=0):
    cov = covered(sx, sy, valid, W, H, msx, msy)
    out = np.full(sx.shape, -1, np.int32)
    idx = E.js_round(sy[cov]).astype(np.int64) * W + E.js_round(sx[cov]).astype(np.int64)
    out[cov] = np.where((idx >= 0) & (idx < W * H), idx, -1).astype(np.int32)
    return out


def coords_field(sx, sy, valid, W, H, msx=0, msy=0):
    cov = covered(sx, sy, valid, W, H, msx, msy)
    out = np.full(sx.shape + (2,), NAN_BITS, np.uint32).view(F32)
    out[cov, 0] = sx[cov].astype(F32)
    out[cov, 1] = sy[cov].astype(F32)
    return out


def remap_index(field, src):
    """src: (n, ...) array of pixels; field: any integer array.  Zeros where the index is outside [0, n)."""
    f = np.asarray(field).astype(np.int64).ravel()
    ok = (f >= 0) & (f < src.shape[0])
    out = np.zeros((f.size,) + src.shape[1:], src.dtype)
    out[ok] = src[f[ok]]
    return out


def _tap(v, n):
    """clamp(v, 0, n - 1) of integer-valued finite f32 values: in float first (to [0, 2147483520]), then as integers."""
    return np.minimum(np.clip(v, F32(0), F32(2147483520.0)).astype(np.int64), n - 1)


def remap_bilinear_f32(coords, src):
    """coords: (n, 2) float32 (sx, sy); src: (H, W, C) float32.  Returns (n, C) float32."""
    coords = np.asarray(coords, F32).reshape(-1, 2)
    src = np.asarray(src, F32)
    H, W, C = src.shape
    out = np.zeros((coords.shape[0], C), F32)
    fin = np.isfinite(coords[:, 0]) & np.isfinite(coords[:, 1])
    sx, sy = coords[fin, 0], coords[fin, 1]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0)[:, None], (sy - y0)[:, None]
    gx, gy = F32(1) - fx, F32(1) - fy
    c0, c1 = _tap(x0, W), _tap(x0 + F32(1), W)
    r0, r1 = _tap(y0, H), _tap(y0 + F32(1), H)
    p00, p01, p10, p11 = src[r0, c0], src[r0, c1], src[r1, c0], src[r1, c1]
    with np.errstate(all="ignore"):
        a = p00 * gx
        b = p01 * fx
        top = (a + b) * gy
        c = p10 * gx
        d = p11 * fx
        bot = (c + d) * fy
        out[fin] = top + bot
    assert out.dtype == F32
    return out
