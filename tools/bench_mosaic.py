#!/usr/bin/env python3
"""bench_mosaic.py -- what blending a frame set into one canvas costs: hg_mosaic_frames_device beside hg_remap_bilinear_frames_device on the
same frames and fields (the parent's kernel, unchanged: the yardstick) and beside the byte floor, same box, one process, back to back.

Three sets of u8 x 4 frames, all made by the library itself (an affine frame set warped out of a random source; its HG_FIELD_COORDS fields):
    overlap   64 frames with identical 3840x2160 windows (frame f looks f/8 of a pixel further right): 64 contributors per canvas pixel
    strip     16 frames of 1920x1080, each shifted by 60 % of its width, on their bounding canvas (19200x1080): 1 or 2 contributors
    scatter   4096 frames of 128x128 thrown over a 3840x2160 area (not asked for by a panorama; it prices the kernel's walk over the frame
              table, which every block makes in full: about 8 contributors per pixel out of 4096 records)
    last / mean / feather    one hg_mosaic_frames_device in that mode, with the weight plane (feather uncapped)
    bilinear                 one hg_remap_bilinear_frames_device of the source through the same fields: every frame's pixels once
    floor_ms                 coords (8 B) plus pixel bytes (4 B) of every candidate read once, plus the canvas (4 B) written, over 8 TB/s
The variants run in turn inside every round (alternating, so that drift hits all alike); a region is one variant's whole work between two
events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed
ones.  Before anything is timed the `last` mosaic of one frame is compared with that frame byte for byte.  One JSON line per set.
    python tools/bench_mosaic.py [--regions N] [--warmup W] [--sets overlap,strip,scatter]
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mosaic.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    scatter = [((f * 1543) % (3840 - 128), (f * 977) % (2160 - 128)) for f in range(4096)]
    sets = {
        "overlap": (3840, 2160, [(0, 0, 3840, 2160)] * 64, [[1, 0, 0, 1, f / 8.0, 0, 0, 0] for f in range(64)]),
        "strip": (1920, 1080, [(1152 * f, 0, 1920, 1080) for f in range(16)], [[1, 0, 0, 1, -1152.0 * f, 0, 0, 0] for f in range(16)]),
        "scatter": (128, 128, [(x, y, 128, 128) for x, y in scatter], [[1, 0, 0, 1, -float(x), -float(y), 0, 0] for x, y in scatter]),
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
                d_co, d_px, d_rm = _bytes(ftotal, dev), _bytes(ptotal, dev), _bytes(ptotal, dev)
                d_cv, d_wt = _bytes(n_canvas * 4, dev), _bytes(n_canvas * 4, dev)
                ctx.field_inverse_geometric_frames_device(HG.FIELD_COORDS, d_co.data_ptr())
                ctx.warp_inverse_geometric_frames_device(d_px.data_ptr())
                ctx.sync()
                # one frame, painted alone over its own window, is itself
                g0 = geoms[-1]
                ctx.mosaic_frames_device([g0], d_co.data_ptr() + fo[-1], d_px.data_ptr() + po[-1], HG.ELEM_U8, 4, W, H, HG.MOSAIC_LAST, 1.0, g0, d_cv.data_ptr())
                ctx.sync()
                n0 = g0[2] * g0[3] * 4
                co = d_co[fo[-1]:fo[-1] + n0 * 2].view(torch.float32).reshape(-1, 2)
                cover = torch.isfinite(co).all(-1)
                if not torch.equal(d_cv[:n0].reshape(-1, 4)[cover], d_px[po[-1]:po[-1] + n0].reshape(-1, 4)[cover]) or d_cv[:n0].reshape(-1, 4)[~cover].any():
                    sys.exit(f"{name}: the mosaic of one frame differs from the frame")
                covered = float(cover.float().mean().item())
                del co, cover

                def mosaic(mode):
                    return lambda: ctx.mosaic_frames_device(geoms, d_co.data_ptr(), d_px.data_ptr(), HG.ELEM_U8, 4, W, H, mode, float("inf"), canvas,
                                                            d_cv.data_ptr(), d_wt.data_ptr())

                def bilinear():
                    ctx.remap_bilinear_frames_device(geoms, d_co.data_ptr(), src.data_ptr(), W, H, 1, 0, HG.ELEM_U8, 4, d_rm.data_ptr())

                variants = [("bilinear", bilinear), ("last", mosaic(HG.MOSAIC_LAST)), ("mean", mosaic(HG.MOSAIC_MEAN)), ("feather", mosaic(HG.MOSAIC_FEATHER))]
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
                floor_ms = (n_cand * 12 + n_canvas * 4) / 8e12 * 1e3
                res = {}
                for label, t in times.items():
                    res[label] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4)}
                for label in ("last", "mean", "feather"):
                    res[label]["vs_bilinear"] = round(res[label]["median_ms"] / res["bilinear"]["median_ms"], 3)
                    res[label]["vs_floor"] = round(res[label]["median_ms"] / floor_ms, 2)
                print(json.dumps({"set": name, "n_frames": F, "frame": [geoms[0][2], geoms[0][3]], "canvas": list(canvas), "candidate_px": n_cand,
                                  "covered_share_of_last_frame": round(covered, 4), "floor_ms": round(floor_ms, 4), **res,
                                  "regions": args.regions, "warmup": args.warmup}), flush=True)
                ctx.sync()
                ctx.set_image(np.zeros((1, 1, 4), np.uint8))     # drop the alias before the buffer goes away
                del src, d_co, d_px, d_rm, d_cv, d_wt
        finally:
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))


if __name__ == "__main__":
    main()
