"""Numpy model of the mosaic (include/hgwarp.h, hg_mosaic_frames_device).  Test infrastructure only.  One np.float32 operation per step
the header writes (numpy does not fuse).  Per frame, in ascending order, the model works over the rectangle window ∩ canvas.

    feather_weight         step 6's w_f of a coordinate array
    mosaic                 (canvas pixels (h, w, C), weight plane (h, w) float32) of a frame list"""
import numpy as np

F32 = np.float32
LAST, MEAN, FEATHER = 0, 1, 2
FLOOR = F32(2.0 ** -10)


def feather_weight(co, W, H, feather):
    """w_f = fmaxf(fminf(fminf(dx, dy), feather), 0x1p-10f) for finite coordinates co (..., 2)."""
    co = np.asarray(co, F32)
    sx, sy = co[..., 0], co[..., 1]
    with np.errstate(all="ignore"):
        dx = np.minimum(sx + F32(1), F32(W) - sx)
        dy = np.minimum(sy + F32(1), F32(H) - sy)
        w = np.maximum(np.minimum(np.minimum(dx, dy), F32(feather)), FLOOR)
    assert w.dtype == F32
    return w


def mosaic(geoms, fields, frames, W, H, mode, feather, canvas):
    """geoms[f] = (x_off, y_off, obj_w, obj_h); fields[f]: obj_w * obj_h float32 coordinate pairs; frames[f]: obj_w * obj_h pixels of C
    channels, float32 or uint8 (any shape that reshapes to (obj_h, obj_w, ...)); canvas = (x, y, width, height), not empty."""
    cx, cy, cw, ch = (int(v) for v in canvas)
    assert cw > 0 and ch > 0
    live = [f for f, g in enumerate(geoms) if g[2] > 0 and g[3] > 0]
    dtype = np.asarray(frames[live[0]]).dtype if live else np.uint8
    C = np.asarray(frames[live[0]]).size // (geoms[live[0]][2] * geoms[live[0]][3]) if live else 1
    out = np.zeros((ch, cw, C), dtype)                            # LAST: the picture; MEAN / FEATHER: the first contributor's pixel
    acc = np.zeros((ch, cw, C), F32)
    wsum = np.zeros((ch, cw), F32)
    count = np.zeros((ch, cw), np.int64)
    for f in live:
        x, y, w, h = (int(v) for v in geoms[f])
        x0, x1, y0, y1 = max(x, cx), min(x + w, cx + cw), max(y, cy), min(y + h, cy + ch)
        if x0 >= x1 or y0 >= y1:
            continue
        co = np.asarray(fields[f], F32).reshape(h, w, 2)[y0 - y:y1 - y, x0 - x:x1 - x]
        px = np.asarray(frames[f]).reshape(h, w, C)[y0 - y:y1 - y, x0 - x:x1 - x]
        assert px.dtype == dtype
        cover = np.isfinite(co).all(-1)
        rect = (slice(y0 - cy, y1 - cy), slice(x0 - cx, x1 - cx))
        if mode == LAST:
            out[rect] = np.where(cover[..., None], px, out[rect])
            wsum[rect] = np.where(cover, F32(1), wsum[rect])
            continue
        wf = feather_weight(np.where(cover[..., None], co, F32(0)), W, H, feather) if mode == FEATHER else np.ones(cover.shape, F32)
        with np.errstate(all="ignore"):
            prod = wf[..., None] * px.astype(F32)
            nacc = acc[rect] + prod
            nsum = wsum[rect] + wf
        assert nacc.dtype == F32 and nsum.dtype == F32
        out[rect] = np.where((cover & (count[rect] == 0))[..., None], px, out[rect])
        acc[rect] = np.where(cover[..., None], nacc, acc[rect])
        wsum[rect] = np.where(cover, nsum, wsum[rect])
        count[rect] += cover
    if mode != LAST:
        with np.errstate(all="ignore"):
            r = acc / wsum[..., None]
            if dtype == np.uint8:
                r = np.minimum(F32(255), np.floor(r + F32(0.5)))
        assert r.dtype == F32
        many = (count > 1)[..., None]
        out = np.where(many, np.where(many, r, F32(0)).astype(dtype), out)
    return out, wsum
