#!/usr/bin/env python3
"""bench_mosaic_gain.py -- what equalising the exposures of a frame set costs: hg_mosaic_overlap_stats_device and
hg_mosaic_frames_gain_device beside hg_mosaic_frames_device on the same frames and fields, same box, one process, back to back.

The three sets of tools/bench_mosaic.py, u8 x 4 frames made by the library itself (the statistics take at most 256 frames, so `scatter`
keeps the first 256 of its 4096):
    overlap   64 frames with identical 3840x2160 windows: 64 contributors per canvas pixel, 4096 overlapping pairs
    strip     16 frames of 1920x1080, each shifted by 60 % of its width: 1 or 2 contributors, 46 pairs
    scatter   256 frames of 128x128 thrown over a 3840x2160 area
    (a) stats                  one hg_mosaic_overlap_stats_device; it reads what the MEAN mosaic reads and writes almost nothing, so
        mean                   one ungained HG_MOSAIC_MEAN mosaic (with the weight plane) is its yardstick
    (b) mean_gain, feather_gain   the gained mosaics beside `mean` and `feather`, the ungained ones
    (c) sequence               exposure 'gain' as a caller runs it: statistics, 16 F^2 bytes down (this waits for the GPU), the host solve,
                               the gained MEAN mosaic -- wall time from the first call to the end of the mosaic, beside `mean_wall`, one
                               ungained mosaic timed the same way
The event-timed variants run in turn inside every round (alternating, so that drift hits all alike); a region is one variant's whole work
between two events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup`
untimed ones.  Before anything is timed, gains of 1 are compared with the ungained mosaic byte for byte and the statistics' diagonal with
the covered pixels of every frame.  One JSON line per set.
    python tools/bench_mosaic_gain.py [--regions N] [--warmup W] [--sets overlap,strip,scatter]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mosaic_gain.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    scatter = [((f * 1543) % (3840 - 128), (f * 977) % (2160 - 128)) for f in range(256)]
    sets = {
        "overlap": (3840, 2160, [(0, 0, 3840, 2160)] * 64, [[1, 0, 0, 1, f / 8.0, 0, 0, 0] for f in range(64)]),
        "strip": (1920, 1080, [(1152 * f, 0, 1920, 1080) for f in range(16)], [[1, 0, 0, 1, -1152.0 * f, 0, 0, 0] for f in range(16)]),
        "scatter": (128, 128, [(x, y, 128, 128) for x, y in scatter], [[1, 0, 0, 1, -float(x), -float(y), 0, 0] for x, y in scatter]),
    }
    INF = float("inf")
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        try:
            for name in args.sets.split(","):
                W, H, geoms, mats = sets[name]
                F = len(geoms)
                x0, y0 = min(g[0] for g in geoms), min(g[1] for g in geoms)
                canvas = (x0, y0, max(g[0] + g[2] for g in geoms) - x0, max(g[1] + g[3] for g in geoms) - y0)
                n_canvas = canvas[2] * canvas[3]
                gen = torch.Generator(device=dev)
                gen.manual_seed(7)
                src = torch.randint(0, 256, (W * H * 4,), dtype=torch.uint8, device=dev, generator=gen)
                ctx.set_image_device(src.data_ptr(), W, H)
                ctx.geometric_set_frames(0, np.array(mats, np.float64).ravel(), geoms)
                fo, ftotal = HG.pack_field_offsets(geoms, HG.FIELD_COORDS)
                po, ptotal = HG.pack_plane_offsets(geoms, 4)
                d_co, d_px = _bytes(ftotal, dev), _bytes(ptotal, dev)
                d_cv, d_wt, d_c2 = _bytes(n_canvas * 4, dev), _bytes(n_canvas * 4, dev), _bytes(n_canvas * 4, dev)
                d_st = torch.empty(F * F * 2, dtype=torch.int64, device=dev)
                ctx.field_inverse_geometric_frames_device(HG.FIELD_COORDS, d_co.data_ptr())
                ctx.warp_inverse_geometric_frames_device(d_px.data_ptr())
                ctx.sync()

                def mosaic(mode, gains=None, out=d_cv):
                    return lambda: ctx.mosaic_frames_device(geoms, d_co.data_ptr(), d_px.data_ptr(), HG.ELEM_U8, 4, W, H, mode, INF, canvas,
                                                            out.data_ptr(), d_wt.data_ptr(), gains=gains)

                def stats():
                    ctx.mosaic_overlap_stats_device(geoms, d_co.data_ptr(), d_px.data_ptr(), 4, canvas, d_st.data_ptr())

                # gains of 1 are the ungained mosaic; the diagonal of N is every frame's covered area
                mosaic(HG.MOSAIC_FEATHER)()
                mosaic(HG.MOSAIC_FEATHER, np.ones(F, np.float32), d_c2)()
                stats()
                ctx.sync()
                if not torch.equal(d_cv, d_c2):
                    sys.exit(f"{name}: gains of 1 differ from the ungained mosaic")
                st = d_st.cpu().numpy().astype(np.uint64).reshape(F, F, 2)
                for f in (0, F - 1):
                    co = d_co[fo[f]:fo[f] + geoms[f][2] * geoms[f][3] * 8].view(torch.float32).reshape(-1, 2)
                    if int(torch.isfinite(co).all(-1).sum().item()) != int(st[f, f, 0]):
                        sys.exit(f"{name}: N[{f}][{f}] is not the covered area of frame {f}")
                if not np.array_equal(st[..., 0], st[..., 0].T):
                    sys.exit(f"{name}: N is not symmetric")
                pairs = int((st[..., 0][np.triu_indices(F, 1)] > 0).sum())
                gains = HG.mosaic_solve_gains(st, 4)

                variants = [("mean", mosaic(HG.MOSAIC_MEAN)), ("stats", stats), ("mean_gain", mosaic(HG.MOSAIC_MEAN, gains)),
                            ("feather", mosaic(HG.MOSAIC_FEATHER)), ("feather_gain", mosaic(HG.MOSAIC_FEATHER, gains))]
                times = {label: [] for label, _ in variants}
                wall = {"mean_wall": [], "sequence": []}
                host = np.empty(F * F * 2, np.uint64)

                def sequence():
                    stats()
                    ctx.sync()
                    host[:] = d_st.cpu().numpy().view(np.uint64)
                    mosaic(HG.MOSAIC_MEAN, HG.mosaic_solve_gains(host, 4))()
                    ctx.sync()

                def mean_wall():
                    mosaic(HG.MOSAIC_MEAN)()
                    ctx.sync()

                for r in range(args.warmup + args.regions):
                    for label, run in variants:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        run()
                        e1.record(stream)
                        e1.synchronize()
                        if r >= args.warmup:
                            times[label].append(e0.elapsed_time(e1))
                    for label, run in (("mean_wall", mean_wall), ("sequence", sequence)):
                        t0 = time.perf_counter()
                        run()
                        if r >= args.warmup:
                            wall[label].append((time.perf_counter() - t0) * 1e3)
                res = {}
                for label, t in list(times.items()) + list(wall.items()):
                    res[label] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4)}
                res["stats"]["vs_mean"] = round(res["stats"]["median_ms"] / res["mean"]["median_ms"], 3)
                res["mean_gain"]["vs_mean"] = round(res["mean_gain"]["median_ms"] / res["mean"]["median_ms"], 3)
                res["feather_gain"]["vs_feather"] = round(res["feather_gain"]["median_ms"] / res["feather"]["median_ms"], 3)
                res["sequence"]["vs_mean_wall"] = round(res["sequence"]["median_ms"] / res["mean_wall"]["median_ms"], 3)
                print(json.dumps({"set": name, "n_frames": F, "frame": [geoms[0][2], geoms[0][3]], "canvas": list(canvas), "overlapping_pairs": pairs,
                                  "gains_min_max": [round(float(gains.min()), 4), round(float(gains.max()), 4)], **res,
                                  "regions": args.regions, "warmup": args.warmup}), flush=True)
                ctx.sync()
                ctx.set_image(np.zeros((1, 1, 4), np.uint8))     # drop the alias before the buffer goes away
                del src, d_co, d_px, d_cv, d_wt, d_c2, d_st
        finally:
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))


if __name__ == "__main__":
    main()
