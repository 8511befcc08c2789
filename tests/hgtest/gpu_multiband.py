"""The device-side routine of the multi-band mosaic's GPU tests (tests/test_gpu_multiband.py), beside hgtest.gpu_frames.run_mosaic: the
poisoned upload / fill / call / download, and the check that no byte outside the canvas, the weight plane, the labels and the first
work_bytes of the work area changed.  No assertions about the blend itself live here."""
import numpy as np

from . import gpu_frames as GF
from . import remap_frames as RF
from .gpu_frames import F32, FILL, POISON, HG


def run_multiband(ctx, geoms, fields, frames, elem, ch, src_w, src_h, feather, bands, canvas, gains=None, weight=True, labels=True, foffs=None,
                  poffs=None, front=0, cfront=0, work_bytes=None):
    """Upload the fields (at foffs, or packed) and the frames (inside an allocation full of POISON, `front` bytes in; at poffs, or packed),
    fill the canvas, the weight plane, the labels and the work area with FILL, run the multi-band mosaic with a work area of work_bytes
    (None: what the layout call returns), check every byte that must not change, and return (canvas bytes, weights or None, labels or
    None)."""
    px = ch * GF.es(elem)
    fo = list(foffs) if foffs is not None else RF.pack(geoms, 8)[0]
    po = list(poffs) if poffs is not None else RF.pack(geoms, px)[0]
    f_total = max([o + RF.n_px(g) * 8 for o, g in zip(fo, geoms)] + [0]) + 256
    p_total = front + max([o + RF.n_px(g) * px for o, g in zip(po, geoms)] + [0]) + 256
    n = max(canvas[2], 0) * max(canvas[3], 0)
    need = HG.mosaic_multiband_layout(geoms, canvas, ch, bands)
    wb = need if work_bytes is None else work_bytes
    c_total, w_total, l_total, k_total = cfront + n * px + 512, n * 4 + 512, n * 4 + 512, max(wb, need) + 512
    bufs = [ctx.alloc(t) for t in (f_total, p_total, c_total, w_total, l_total, k_total)]
    d_f, d_p, d_c, d_w, d_l, d_k = bufs
    try:
        ctx.to_device(d_f, GF.place(fields, fo, f_total, 0x11))
        ctx.to_device(d_p, GF.place(frames, [front + o for o in po], p_total, POISON))
        for d, t in ((d_c, c_total), (d_w, w_total), (d_l, l_total), (d_k, k_total)):
            ctx.to_device(d, np.full(t, FILL, np.uint8))
        ctx.mosaic_multiband_device(geoms, d_f, d_p + front, elem, ch, src_w, src_h, feather, bands, canvas, d_c + cfront, d_k, wb,
                                    d_weight=d_w if weight else 0, d_labels=d_l if labels else 0, field_offsets=foffs, frame_offsets=poffs, gains=gains)
        ctx.sync()
        raw, wraw, lraw, kraw = ctx.to_host(d_c, c_total), ctx.to_host(d_w, w_total), ctx.to_host(d_l, l_total), ctx.to_host(d_k, k_total)
    finally:
        for p in bufs:
            ctx.free(p)
    assert (raw[:cfront] == FILL).all() and (raw[cfront + n * px:] == FILL).all(), "bytes outside the canvas must not be written"
    assert (wraw[n * 4 if weight else 0:] == FILL).all(), "bytes outside the weight plane must not be written"
    assert (lraw[n * 4 if labels else 0:] == FILL).all(), "bytes outside the labels must not be written"
    assert (kraw[need:] == FILL).all(), "bytes beyond work_bytes must not be written"
    own = lraw[:n * 4].view(np.int32) if labels else (kraw[:n * 4].view(np.int32) if n else None)      # (without d_labels: the work area's first part)
    return raw[cfront:cfront + n * px], (wraw[:n * 4].view(F32) if weight else None), own


def check(got, want, what):
    """(canvas bytes, weights or None, labels) of run_multiband against the model's (canvas, weight plane, labels), bit for bit."""
    GF.check_canvas(got[:2], want[:2], what)
    if got[2] is not None:
        assert np.array_equal(got[2], want[2].ravel()), (what, "labels")
