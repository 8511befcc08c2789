#!/usr/bin/env python3
"""bench_moving.py -- what frame sets with their own source points (hg_piecewise_set_frames_src) buy, same box, one process.

C4's 68-landmark face mesh on 4K, 64 frames, one source image per frame.  Three ways to warp the same 64 destination point sets:
    static   hg_piecewise_set_frames + frames_device: one source side for all frames (the mesh's), as before;
    moving   hg_piecewise_set_frames_src + frames_device: the same frames, every frame with its own (jittered) source points and minima;
    single   what a caller had to do for moving source points without it: hg_piecewise_set_mesh + hg_piecewise_prepare +
             hg_warp_inverse_piecewise_device for every frame (set_mesh settles the stream).
The cases alternate for `--rounds` rounds of `--warmup` + `--steps` steps.  kernel_ms_per_frame = hipEvents around the warp kernel
(hg_set_timing), wall_ms_per_frame = host time of the whole step including the frame-set upload, hg_sync at the end of the timed region.
One JSON line per case with every round's figures, then one line with the ratios of the medians.
    python tools/bench_moving.py [--steps K] [--warmup W] [--rounds R] [--frames F]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "homography.js_amd")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


HG = _load("hgwarp", os.path.join(PKG, "hgwarp.py"))
WL = _load("hg_workloads", os.path.join(PKG, "workloads.py"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    args = ap.parse_args()
    cfg = WL.CONFIGS["C4"]
    W, H, F = cfg["W"], cfg["H"], args.frames
    sp = WL.face_mesh(W, H, cfg["landmarks"])
    tris = HG.triangulate(sp)
    dsts = WL.face_frames(sp, W, F)
    geoms = [WL.piecewise_geom(d) for d in dsts]
    offs, total = HG.pack_offsets(geoms)
    rng = np.random.default_rng(4)
    srcs = [(sp.astype(np.float64) + rng.uniform(-6.0, 6.0, sp.size)).astype(np.float32) for _ in range(F)]   # landmarks tracked per frame
    mins = np.asarray([WL.src_min(s) for s in srcs], np.int32).ravel()
    msx, msy = WL.src_min(sp)
    dst_all, src_all = np.concatenate(dsts), np.concatenate(srcs)
    stride = W * H * 4
    with HG.Context(0) as ctx:
        d_src, d_out = ctx.alloc(stride * F), ctx.alloc(total)
        try:
            for k in range(F):
                ctx.to_device(d_src, WL.lcg_image(W, H, 1 + k), k * stride)
            ctx.set_images_device(d_src, W, H, F, stride)
            ctx.piecewise_set_mesh(sp, tris, msx, msy)

            def static():
                ctx.piecewise_set_frames(dst_all, geoms, offs)
                ctx.warp_inverse_piecewise_frames_device(d_out)

            def moving():
                ctx.piecewise_set_frames_src(src_all, mins, dst_all, geoms, offs)
                ctx.warp_inverse_piecewise_frames_device(d_out)

            def single():
                for f in range(F):
                    ctx.set_images_device(d_src + f * stride, W, H, 1, stride)
                    ctx.piecewise_set_mesh(srcs[f], tris, int(mins[2 * f]), int(mins[2 * f + 1]))
                    ctx.piecewise_prepare(dsts[f], geoms[f])
                    ctx.warp_inverse_piecewise_frames_device(d_out + offs[f])

            def restore():
                ctx.set_images_device(d_src, W, H, F, stride)
                ctx.piecewise_set_mesh(sp, tris, msx, msy)

            cases = {"static": static, "moving": moving, "single": single}
            series = {k: {"kernel_ms_per_frame": [], "wall_ms_per_frame": [], "variant": None} for k in cases}
            for _ in range(args.rounds):
                for name, step in cases.items():
                    restore()
                    for _ in range(args.warmup):
                        step()
                    ctx.sync()
                    ctx.set_timing(True)
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    ctx.sync()
                    el = time.perf_counter() - t0
                    k_ms, n = ctx.kernel_ms_stats()
                    ctx.set_timing(False)
                    series[name]["kernel_ms_per_frame"].append(round(k_ms / (args.steps * F), 6))
                    series[name]["wall_ms_per_frame"].append(round(el * 1e3 / (args.steps * F), 6))
                    series[name]["variant"] = ctx.last_piecewise_variant()
            assert ctx.redone_frames() == 0, "a frame went through the map path: the figures are not those of the fast kernels"
            med = {}
            for name in cases:
                s = series[name]
                med[name] = (statistics.median(s["kernel_ms_per_frame"]), statistics.median(s["wall_ms_per_frame"]))
                print(json.dumps({"case": name, "frames": F, "steps": args.steps, **s}))
            print(json.dumps({"moving_over_static_kernel": round(med["moving"][0] / med["static"][0], 4),
                              "moving_over_static_wall": round(med["moving"][1] / med["static"][1], 4),
                              "single_over_moving_kernel": round(med["single"][0] / med["moving"][0], 4),
                              "single_over_moving_wall": round(med["single"][1] / med["moving"][1], 4),
                              "static_kernel_spread": round(max(series["static"]["kernel_ms_per_frame"]) - min(series["static"]["kernel_ms_per_frame"]), 6)}))
        finally:
            ctx.free(d_out); ctx.free(d_src)


if __name__ == "__main__":
    main()
