#!/usr/bin/env python3
"""bench_multiband.py -- what blending a frame set in frequency bands costs: hg_mosaic_multiband_device at 1, 3 and 5 bands beside
hg_mosaic_frames_device in HG_MOSAIC_FEATHER mode on the same frames and fields, same box, one process, back to back.

The two panorama sets of tools/bench_mosaic.py, u8 x 4 frames made by the library itself (an affine frame set warped out of a random
source; its HG_FIELD_COORDS fields):
    overlap   64 frames with identical 3840x2160 windows (frame f looks f/8 of a pixel further right)
    strip     16 frames of 1920x1080, each shifted by 60 % of its width, on their bounding canvas (19200x1080)
    feather                  one hg_mosaic_frames_device, HG_MOSAIC_FEATHER uncapped, with the weight plane
    bands1 / bands3 / bands5 one hg_mosaic_multiband_device with the weight plane and d_labels (feather uncapped)
    work_bytes               what hg_mosaic_multiband_layout returns for that band count
    floor_ms                 the work-area traffic over 8 TB/s: every part of the work area but the unused labels written once and read once,
                             the coordinates (8 B) of every candidate read twice (labels, flags) and its pixel (4 B) once, labels, canvas
                             and weight plane (4 B each) written once
The variants run in turn inside every round (alternating, so that drift hits all alike); a region is one variant's whole work between two
events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed
ones.  Before anything is timed the one-band blend of one frame is compared with that frame byte for byte.  One JSON line per set.
    python tools/bench_multiband.py [--regions N] [--warmup W] [--sets overlap,strip]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "homography.js_amd")
BANDS = (1, 3, 5)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


HG = _load("hgwarp", os.path.join(PKG, "hgwarp.py"))


def _bytes(n, dev):
    return torch.empty(int(n), dtype=torch.uint8, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", default="overlap,strip")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_multiband.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    sets = {
        "overlap": (3840, 2160, [(0, 0, 3840, 2160)] * 64, [[1, 0, 0, 1, f / 8.0, 0, 0, 0] for f in range(64)]),
        "strip": (1920, 1080, [(1152 * f, 0, 1920, 1080) for f in range(16)], [[1, 0, 0, 1, -1152.0 * f, 0, 0, 0] for f in range(16)]),
    }
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        try:
            for name in args.sets.split(","):
                W, H, geoms, mats = sets[name]
                F = len(geoms)
                x0, y0 = min(g[0] for g in geoms), min(g[1] for g in geoms)
                canvas = (x0, y0, max(g[0] + g[2] for g in geoms) - x0, max(g[1] + g[3] for g in geoms) - y0)
                n_canvas = canvas[2] * canvas[3]
                n_cand = sum(g[2] * g[3] for g in geoms)             # (every window lies inside the bounding canvas)
                gen = torch.Generator(device=dev)
                gen.manual_seed(7)
                src = torch.randint(0, 256, (W * H * 4,), dtype=torch.uint8, device=dev, generator=gen)
                ctx.set_image_device(src.data_ptr(), W, H)
                ctx.geometric_set_frames(0, np.array(mats, np.float64).ravel(), geoms)
                fo, ftotal = HG.pack_field_offsets(geoms, HG.FIELD_COORDS)
                po, ptotal = HG.pack_plane_offsets(geoms, 4)
                work = {b: HG.mosaic_multiband_layout(geoms, canvas, 4, b) for b in BANDS}
                d_co, d_px = _bytes(ftotal, dev), _bytes(ptotal, dev)
                d_cv, d_wt, d_lb, d_wk = _bytes(n_canvas * 4, dev), _bytes(n_canvas * 4, dev), _bytes(n_canvas * 4, dev), _bytes(max(work.values()), dev)
                assert d_wk.data_ptr() % 256 == 0
                ctx.field_inverse_geometric_frames_device(HG.FIELD_COORDS, d_co.data_ptr())
                ctx.warp_inverse_geometric_frames_device(d_px.data_ptr())
                ctx.sync()
                # one frame, blended alone over its own window in one band, is itself
                g0 = geoms[-1]
                ctx.mosaic_multiband_device([g0], d_co.data_ptr() + fo[-1], d_px.data_ptr() + po[-1], HG.ELEM_U8, 4, W, H, float("inf"), 1, g0, d_cv.data_ptr(),
                                            d_wk.data_ptr(), HG.mosaic_multiband_layout([g0], g0, 4, 1))
                ctx.sync()
                n0 = g0[2] * g0[3] * 4
                co = d_co[fo[-1]:fo[-1] + n0 * 2].view(torch.float32).reshape(-1, 2)
                cover = torch.isfinite(co).all(-1)
                if not torch.equal(d_cv[:n0].reshape(-1, 4)[cover], d_px[po[-1]:po[-1] + n0].reshape(-1, 4)[cover]) or d_cv[:n0].reshape(-1, 4)[~cover].any():
                    sys.exit(f"{name}: the one-band blend of one frame differs from the frame")
                del co, cover

                def feather():
                    ctx.mosaic_frames_device(geoms, d_co.data_ptr(), d_px.data_ptr(), HG.ELEM_U8, 4, W, H, HG.MOSAIC_FEATHER, float("inf"), canvas,
                                             d_cv.data_ptr(), d_wt.data_ptr())

                def multiband(b):
                    return lambda: ctx.mosaic_multiband_device(geoms, d_co.data_ptr(), d_px.data_ptr(), HG.ELEM_U8, 4, W, H, float("inf"), b, canvas, d_cv.data_ptr(),
                                                               d_wk.data_ptr(), work[b], d_weight=d_wt.data_ptr(), d_labels=d_lb.data_ptr())

                variants = [("feather", feather)] + [(f"bands{b}", multiband(b)) for b in BANDS]
                times = {label: [] for label, _ in variants}
                for r in range(args.warmup + args.regions):
                    for label, run in variants:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        run()
                        e1.record(stream)
                        e1.synchronize()
                        if r >= args.warmup:
                            times[label].append(e0.elapsed_time(e1))
                res = {}
                for label, t in times.items():
                    res[label] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4)}
                for b in BANDS:
                    part = work[b] - (n_canvas * 4 + 255) // 256 * 256                  # (d_labels is given: the work area's own labels stay unused)
                    floor_ms = (2 * part + n_cand * (2 * 8 + 4) + n_canvas * 12) / 8e12 * 1e3
                    r_ = res[f"bands{b}"]
                    r_.update(work_bytes=work[b], floor_ms=round(floor_ms, 4), vs_feather=round(r_["median_ms"] / res["feather"]["median_ms"], 3),
                              vs_floor=round(r_["median_ms"] / floor_ms, 2))
                print(json.dumps({"set": name, "n_frames": F, "frame": [geoms[0][2], geoms[0][3]], "canvas": list(canvas), "candidate_px": n_cand, **res,
                                  "regions": args.regions, "warmup": args.warmup}), flush=True)
                ctx.sync()
                ctx.set_image(np.zeros((1, 1, 4), np.uint8))     # drop the alias before the buffer goes away
                del src, d_co, d_px, d_cv, d_wt, d_lb, d_wk
        finally:
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))


if __name__ == "__main__":
    main()
