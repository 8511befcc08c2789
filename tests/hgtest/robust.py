"""Numpy models of the robust mosaic (include/hgwarp.h, hg_mosaic_robust_device).  Test infrastructure only; both sort, which the kernel
never does.

    gained                 step 2's byte of a gained value
    result                 step 4 of one channel's contributor values (a Python list), by `sorted`
    mosaic_scalar          the header's steps pixel by pixel, a Python loop
    mosaic                 (canvas pixels (h, w, C) uint8, weight plane (h, w) float32): the contributors stacked with a mask, np.sort"""
import math

import numpy as np

F32 = np.float32
MEDIAN, TRIMMED, MIN, MAX = 0, 1, 2, 3
MODES = (MEDIAN, TRIMMED, MIN, MAX)


def stat_channels(C):
    return 3 if C == 4 else C


def gained(g, p):
    """min(255, floor(g * (float)p + 0.5f)) in float32, for a scalar or an array of bytes."""
    q = F32(g) * np.asarray(p).astype(F32)
    assert q.dtype == F32
    return np.minimum(F32(255), np.floor(q + F32(0.5))).astype(np.uint8)


def trim_count(trim, n):
    """t = min((int)(trim * (float)n), (n - 1) / 2) with one f32 multiply, for n >= 1."""
    return min(int(F32(trim) * F32(n)), (n - 1) // 2)


def result(values, mode, trim=0.0):
    n = len(values)
    if n == 0:
        return 0
    s = sorted(int(v) for v in values)
    if mode == MIN:
        return s[0]
    if mode == MAX:
        return s[-1]
    if mode == MEDIAN:
        return s[(n - 1) // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2] + 1) >> 1
    assert mode == TRIMMED
    t = trim_count(trim, n)
    m = n - 2 * t
    return (2 * sum(s[t:n - t]) + m) // (2 * m)


def mosaic_scalar(geoms, fields, frames, C, mode, trim, canvas, gains=None):
    cx, cy, cw, ch = canvas
    out = np.zeros((ch, cw, C), np.uint8)
    weight = np.zeros((ch, cw), F32)
    for j in range(ch):
        for i in range(cw):
            X, Y = cx + i, cy + j
            vals = [[] for _ in range(C)]
            for f, (x, y, w, h) in enumerate(geoms):
                u, v = X - x, Y - y
                if w <= 0 or h <= 0 or not (0 <= u < w and 0 <= v < h):
                    continue
                sx, sy = np.asarray(fields[f]).reshape(-1, 2)[v * w + u]
                if not (math.isfinite(sx) and math.isfinite(sy)):
                    continue
                p = np.asarray(frames[f]).reshape(-1, C)[v * w + u]
                for c in range(C):
                    vals[c].append(int(gained(gains[f], p[c])) if gains is not None and c < stat_channels(C) else int(p[c]))
            out[j, i] = [result(vals[c], mode, trim) for c in range(C)]
            weight[j, i] = len(vals[0])
    return out, weight


def mosaic(geoms, fields, frames, C, mode, trim, canvas, gains=None):
    """geoms[f] = (x_off, y_off, obj_w, obj_h); fields[f]: obj_w * obj_h float32 coordinate pairs; frames[f]: obj_w * obj_h pixels of C
    uint8 channels; canvas = (x, y, width, height), not empty; gains: None or one factor per frame."""
    cx, cy, cw, ch = (int(v) for v in canvas)
    assert cw > 0 and ch > 0
    F = len(geoms)
    val = np.full((max(F, 1), ch, cw, C), 256, np.int32)           # 256: not a contributor, sorts behind every byte
    for f, (x, y, w, h) in enumerate(geoms):
        x, y, w, h = int(x), int(y), int(w), int(h)
        x0, x1, y0, y1 = max(x, cx), min(x + w, cx + cw), max(y, cy), min(y + h, cy + ch)
        if w <= 0 or h <= 0 or x0 >= x1 or y0 >= y1:
            continue
        co = np.asarray(fields[f], F32).reshape(h, w, 2)[y0 - y:y1 - y, x0 - x:x1 - x]
        px = np.asarray(frames[f]).reshape(h, w, C)[y0 - y:y1 - y, x0 - x:x1 - x]
        assert px.dtype == np.uint8
        if gains is not None:
            k = stat_channels(C)
            px = np.concatenate([gained(gains[f], px[..., :k]), px[..., k:]], -1)
        cover = np.isfinite(co).all(-1)
        val[f, y0 - cy:y1 - cy, x0 - cx:x1 - cx] = np.where(cover[..., None], px.astype(np.int32), 256)
    n = (val[..., 0] < 256).sum(0)                                 # (h, w)
    s = np.sort(val, axis=0)
    some = np.maximum(n, 1)
    if mode in (MIN, MAX):
        lo = hi = np.zeros_like(n) if mode == MIN else some - 1
    elif mode == MEDIAN:
        lo, hi = (some - 1) // 2, some // 2
    else:
        assert mode == TRIMMED
        prod = F32(trim) * some.astype(F32)
        assert prod.dtype == F32
        t = np.minimum(prod.astype(np.int64), (some - 1) // 2)
        lo, hi = t, some - 1 - t
    pick = lambda k: np.take_along_axis(s, np.broadcast_to(k[None, ..., None], (1, ch, cw, C)), 0)[0]
    if mode == TRIMMED:
        cs = np.concatenate([np.zeros((1, ch, cw, C), np.int64), np.cumsum(np.where(s < 256, s, 0), 0, dtype=np.int64)], 0)
        at = lambda k: np.take_along_axis(cs, np.broadcast_to(k[None, ..., None], (1, ch, cw, C)), 0)[0]
        S, m = at(hi + 1) - at(lo), (hi - lo + 1)[..., None]
        r = (2 * S + m) // (2 * m)
    else:
        r = (pick(lo) + pick(hi) + 1) >> 1
    out = np.where((n > 0)[..., None], r, 0).astype(np.uint8)
    return out, n.astype(F32)
