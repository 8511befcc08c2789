"""Numpy model of the bilinear sampling mode of the inverse warps (include/hgwarp.h, HG_SAMPLE_BILINEAR).  Test infrastructure only.
Source coordinates in f64 in the reference's operation order (numpy never fuses a*b+c), the coverage test of the nearest loops,
four clamped taps, straight RGBA blended per channel in f32:
    v = (p00*(1-fx) + p01*fx)*(1-fy) + (p10*(1-fx) + p11*fx)*fy,   out = min(255, floor(v + 0.5f))."""
import numpy as np

F32 = np.float32


def sample(img, sx, sy, covered):
    """RGBA8 of every position of sx / sy (f64 arrays of one shape); positions where `covered` is False stay all-zero.  Only the four
    taps of the covered positions are converted to f32 (a source of 2 GiB or more is never copied)."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    out = np.zeros(sx.shape + (4,), np.uint8)
    x, y = sx[covered], sy[covered]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0).astype(F32)[:, None], (y - y0).astype(F32)[:, None]
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    c0, c1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
    r0, r1 = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
    p00, p01 = img[r0, c0].astype(F32), img[r0, c1].astype(F32)
    p10, p11 = img[r1, c0].astype(F32), img[r1, c1].astype(F32)
    gx, gy = F32(1) - fx, F32(1) - fy
    v = (p00 * gx + p01 * fx) * gy + (p10 * gx + p11 * fx) * fy
    out[covered] = np.minimum(F32(255), np.floor(v + F32(0.5))).astype(np.uint8)
    return out


def geometric_coords(kind, m, xoff, yoff, objw, objh):
    """(sx, sy) of the inverse geometric loop :999 for an output window: kind 0 affine (m[0..5]), 1 projective (m[0..7])."""
    m = np.asarray(m, np.float64)
    x = (np.arange(objw, dtype=np.float64) + xoff)[None, :]
    y = (np.arange(objh, dtype=np.float64) + yoff)[:, None]
    with np.errstate(all="ignore"):
        if kind == 0:
            sx = (m[0] * x + m[2] * y) + m[4]
            sy = (m[1] * x + m[3] * y) + m[5]
        else:
            den = (m[6] * x + m[7] * y) + 1.0
            sx = ((m[0] * x + m[1] * y) + m[2]) / den
            sy = ((m[3] * x + m[4] * y) + m[5]) / den
    return np.broadcast_to(sx, (objh, objw)).copy(), np.broadcast_to(sy, (objh, objw)).copy()


def warp_geometric(kind, m, img, xoff, yoff, objw, objh):
    """Bilinear _inverseGeometricWarp; returns (rgba, covered mask)."""
    H, W = img.shape[:2]
    sx, sy = geometric_coords(kind, m, xoff, yoff, objw, objh)
    with np.errstate(invalid="ignore"):
        cov = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)                     # :1001 (NaN fails)
    return sample(img, sx, sy, cov), cov


def piecewise_coords(map16, inv, xoff, yoff, objw, objh):
    """(sx, sy, valid) of the inverse piecewise loop :1044-1046 given the Int16 map and the (T, 6) float32 inverse matrices."""
    ids = np.asarray(map16).reshape(objh, objw).astype(np.int64)
    valid = ids >= 0
    m = np.asarray(inv, np.float32).reshape(-1, 6).astype(np.float64)
    sx = np.zeros((objh, objw)); sy = np.zeros((objh, objw))
    x = np.arange(objw, dtype=np.float64) + xoff
    for r0 in range(0, objh, 256):                          # (row blocks: a 4K frame's per-pixel matrices would take 400 MB)
        r1 = min(objh, r0 + 256)
        y = (np.arange(r0, r1, dtype=np.float64) + yoff)[:, None]
        mm = m[np.where(valid[r0:r1], ids[r0:r1], 0)]
        sx[r0:r1] = (mm[..., 0] * x + mm[..., 2] * y) + mm[..., 4]
        sy[r0:r1] = (mm[..., 1] * x + mm[..., 3] * y) + mm[..., 5]
    return sx, sy, valid


def warp_piecewise(map16, inv, img, min_src_x, min_src_y, xoff, yoff, objw, objh):
    """Bilinear _inversePiecewiseAffineWarp over a given map; the taps index the source without the minSrc shift. (rgba, covered)."""
    H, W = img.shape[:2]
    sx, sy, valid = piecewise_coords(map16, inv, xoff, yoff, objw, objh)
    with np.errstate(invalid="ignore"):
        cov = valid & (sx >= min_src_x) & (sx < W + min_src_x) & (sy >= min_src_y) & (sy < H + min_src_y)   # :1047
    return sample(img, sx, sy, cov), cov
