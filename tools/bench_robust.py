#!/usr/bin/env python3
"""bench_robust.py -- what an order statistic costs where a mean would do: hg_mosaic_robust_device beside hg_mosaic_frames_device
(HG_MOSAIC_MEAN, the yardstick) on the same frames and fields, and beside the byte floor; same box, one process, back to back.

Three sets of u8 x 4 frames, all made by the library itself (an affine frame set warped out of a random source; its HG_FIELD_COORDS
fields), the shapes of tools/bench_mosaic.py:
    overlap   64 frames with identical 3840x2160 windows: 64 contributors per canvas pixel (a tripod burst)
    strip     16 frames of 1920x1080, each shifted by 60 % of its width, on their bounding canvas (19200x1080): 1 or 2 contributors, and
              2-3 frames out of 16 hit a tile
    scatter   256 frames of 128x128 thrown over a 3840x2160 area: a few contributors out of 256 records
    mean                            one hg_mosaic_frames_device(HG_MOSAIC_MEAN), with the weight plane
    median / trimmed / min / max    one hg_mosaic_robust_device in that mode (trimmed: trim 0.25), with the weight plane
    floor_ms                        coords (8 B) plus pixel bytes (4 B) of every candidate read once, plus canvas and weights (8 B) written, over 8 TB/s
The variants run in turn inside every round (alternating, so that drift hits all alike); a region is one variant's whole work between two
events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed
ones, and the median as a ratio to `mean`'s and to the floor.  Before anything is timed, HG_ROBUST_TRIMMED at trim 0 is compared with the
mean mosaic byte for byte, weight plane included, and min <= median <= max is checked on the whole canvas.  One JSON line per set; `cap`
is the staging cap of the binding (the library under test may be built with another: HGWARP_LIB selects it, --cap labels it).
    python tools/bench_robust.py [--regions N] [--warmup W] [--sets overlap,strip,scatter] [--cap L]
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
    ap.add_argument("--sets", default="overlap,strip,scatter")
    ap.add_argument("--cap", type=int, default=HG.ROBUST_LMAX)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_robust.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    scatter = [((f * 1543) % (3840 - 128), (f * 977) % (2160 - 128)) for f in range(256)]
    sets = {
        "overlap": (3840, 2160, [(0, 0, 3840, 2160)] * 64, [[1, 0, 0, 1, f / 8.0, 0, 0, 0] for f in range(64)], None),
        "strip": (1920, 1080, [(1152 * f, 0, 1920, 1080) for f in range(16)], [[1, 0, 0, 1, -1152.0 * f, 0, 0, 0] for f in range(16)], None),
        "scatter": (128, 128, [(x, y, 128, 128) for x, y in scatter], [[1, 0, 0, 1, -float(x), -float(y), 0, 0] for x, y in scatter], (0, 0, 3840, 2160)),
    }
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        try:
            for name in args.sets.split(","):
                W, H, geoms, mats, canvas = sets[name]
                F = len(geoms)
                if canvas is None:
                    x0, y0 = min(g[0] for g in geoms), min(g[1] for g in geoms)
                    canvas = (x0, y0, max(g[0] + g[2] for g in geoms) - x0, max(g[1] + g[3] for g in geoms) - y0)
                n_canvas = canvas[2] * canvas[3]
                n_cand = sum(g[2] * g[3] for g in geoms)             # (every window lies inside the canvas)
                gen = torch.Generator(device=dev)
                gen.manual_seed(7)
                src = torch.randint(0, 256, (W * H * 4,), dtype=torch.uint8, device=dev, generator=gen)
                ctx.set_image_device(src.data_ptr(), W, H)
                ctx.geometric_set_frames(0, np.array(mats, np.float64).ravel(), geoms)
                fo, ftotal = HG.pack_field_offsets(geoms, HG.FIELD_COORDS)
                po, ptotal = HG.pack_plane_offsets(geoms, 4)
                d_co, d_px = _bytes(ftotal, dev), _bytes(ptotal, dev)
                d_cv, d_wt, d_c2, d_w2 = (_bytes(n_canvas * 4, dev) for _ in range(4))
                ctx.field_inverse_geometric_frames_device(HG.FIELD_COORDS, d_co.data_ptr())
                ctx.warp_inverse_geometric_frames_device(d_px.data_ptr())
                ctx.sync()

                def mean(cv=d_cv, wt=d_wt):
                    ctx.mosaic_frames_device(geoms, d_co.data_ptr(), d_px.data_ptr(), HG.ELEM_U8, 4, W, H, HG.MOSAIC_MEAN, 1.0, canvas, cv.data_ptr(), wt.data_ptr())

                def robust(mode, trim=0.0, cv=d_cv, wt=d_wt):
                    return lambda: ctx.mosaic_robust_device(geoms, d_co.data_ptr(), d_px.data_ptr(), 4, mode, canvas, cv.data_ptr(), wt.data_ptr(), trim)

                # the trimmed mean at 0 is the mean mosaic, byte for byte; min <= median <= max
                mean(d_c2, d_w2)
                robust(HG.ROBUST_TRIMMED, 0.0)()
                ctx.sync()
                if not torch.equal(d_cv, d_c2) or not torch.equal(d_wt, d_w2):
                    sys.exit(f"{name}: HG_ROBUST_TRIMMED at trim 0 differs from HG_MOSAIC_MEAN")
                most = int(d_wt.view(torch.float32).max().item())
                robust(HG.ROBUST_MIN, 0.0, d_c2, d_w2)()
                robust(HG.ROBUST_MEDIAN)()
                ctx.sync()
                low = bool((d_c2 <= d_cv).all().item())
                robust(HG.ROBUST_MAX, 0.0, d_c2, d_w2)()
                ctx.sync()
                if not low or not bool((d_cv <= d_c2).all().item()):
                    sys.exit(f"{name}: min <= median <= max does not hold")

                variants = [("mean", mean), ("median", robust(HG.ROBUST_MEDIAN)), ("trimmed", robust(HG.ROBUST_TRIMMED, 0.25)),
                            ("min", robust(HG.ROBUST_MIN)), ("max", robust(HG.ROBUST_MAX))]
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
                floor_ms = (n_cand * 12 + n_canvas * 8) / 8e12 * 1e3
                res = {}
                for label, t in times.items():
                    res[label] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4)}
                    res[label]["vs_floor"] = round(res[label]["median_ms"] / floor_ms, 2)
                for label in ("median", "trimmed", "min", "max"):
                    res[label]["vs_mean"] = round(res[label]["median_ms"] / res["mean"]["median_ms"], 3)
                print(json.dumps({"set": name, "cap": args.cap, "n_frames": F, "frame": [geoms[0][2], geoms[0][3]], "canvas": list(canvas), "candidate_px": n_cand,
                                  "most_contributors": most, "floor_ms": round(floor_ms, 4), **res, "regions": args.regions, "warmup": args.warmup}), flush=True)
                ctx.sync()
                ctx.set_image(np.zeros((1, 1, 4), np.uint8))     # drop the alias before the buffer goes away
                del src, d_co, d_px, d_cv, d_wt, d_c2, d_w2
        finally:
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))


if __name__ == "__main__":
    main()
