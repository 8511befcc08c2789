#!/usr/bin/env python3
"""bench_camera.py -- what a source field from a camera model costs: hg_field_camera_frames_device (k_camera_field) for 64 windows of
3840 x 2160, HG_FIELD_COORDS, on the plane, the cylinder and the sphere, with and without lens terms; 64 cameras fanned over a full turn
of yaw, each window the 3840 x 2160 canvas pixels around its own optical axis (so nearly every pixel is covered and stored as a value).

    beside    hg_field_inverse_geometric_frames_device (projective) on the same windows, from the same build: the cheapest field there is,
              eight multiply-adds and one division per pixel;
              the byte floor: 8 bytes per pixel at 8 TB/s.

A region is one whole call between two events on the context's stream; the calls run in turn inside every round (alternating, so that drift
hits all alike); per call the median and the minimum over `--regions` regions after `--warmup` untimed ones.  One JSON line.
    python tools/bench_camera.py [--regions N] [--warmup W] [--frames 64] [--width 3840] [--height 2160]
"""
import argparse
import importlib.util
import json
import math
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
SURFACES = (("plane", HG.SURFACE_PLANE), ("cylinder", HG.SURFACE_CYLINDER), ("sphere", HG.SURFACE_SPHERE))


def timed(stream, calls, regions, warmup):
    times = {k: [] for k in calls}
    for r in range(warmup + regions):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4)} for k, t in times.items()}


def yaw_pitch(yaw, pitch):
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    world_from_cam = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return world_from_cam.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_camera.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    F, W, H = args.frames, args.width, args.height
    f = 0.8 * W                                              # a 64 degree lens
    scale = f
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        res, covered = {}, {}
        calls = {}
        keep = []
        d_field = None
        for lens, dist in (("plain", None), ("lens", (-0.12, 0.03, 0.001, -0.0015, 0.002))):
            yaws = [2 * math.pi * k / F + 0.013 for k in range(F)]
            recs = np.stack([HG.camera_pack_record(yaw_pitch(y, 0.02), (f, 1.01 * f), (W / 2 + 0.3, H / 2 - 0.2), W, H, dist) for y in yaws])
            d_rec = torch.from_numpy(recs).to(dev)
            keep.append(d_rec)
            for name, surface in SURFACES:
                # the window around each camera's own axis: on the plane every camera gets the plane of its own axis (a plane holds no full turn)
                if surface == HG.SURFACE_PLANE:
                    recs_s = np.stack([HG.camera_pack_record(yaw_pitch(0.013, 0.02), (f, 1.01 * f), (W / 2 + 0.3, H / 2 - 0.2), W, H, dist)] * F)
                    d_rec_s = torch.from_numpy(recs_s).to(dev)
                    keep.append(d_rec_s)
                    geoms = [(int(round(scale * math.tan(0.013))) - W // 2, -H // 2, W, H)] * F
                else:
                    d_rec_s = d_rec
                    geoms = [(int(round(scale * y)) - W // 2, -H // 2, W, H) for y in yaws]
                if d_field is None:
                    total = HG.pack_field_offsets(geoms, HG.FIELD_COORDS)[1]
                    d_field = torch.empty(total, dtype=torch.uint8, device=dev)
                fn = (lambda r=d_rec_s, g=geoms, s=surface: ctx.field_camera_frames_device(r.data_ptr(), g, W, H, s, scale, 0.0, 0.0, HG.FIELD_COORDS, d_field.data_ptr()))
                fn()
                ctx.sync()
                v = d_field[:W * H * 8].view(torch.float32).view(-1, 2)
                covered[f"{name}_{lens}"] = round(float((~torch.isnan(v[:, 0])).float().mean().item()), 4)
                calls[f"{name}_{lens}"] = fn
        # the projective field of the same windows
        geoms = [(-W // 2, -H // 2, W, H)] * F
        mats = np.stack([[1.0 + 0.001 * k, 0.02, W / 2.0, -0.015, 1.0 - 0.001 * k, H / 2.0, 1e-5, -2e-5] for k in range(F)])
        d_src = torch.zeros(W * H * 4, dtype=torch.uint8, device=dev)
        ctx.set_image_device(d_src.data_ptr(), W, H)
        ctx.geometric_set_frames(HG.HG_PROJECTIVE, mats, geoms, HG.pack_offsets(geoms)[0])
        calls["projective"] = lambda: ctx.field_inverse_geometric_frames_device(HG.FIELD_COORDS, d_field.data_ptr())
        calls["projective"]()
        ctx.sync()
        v = d_field[:W * H * 8].view(torch.float32).view(-1, 2)
        covered["projective"] = round(float((~torch.isnan(v[:, 0])).float().mean().item()), 4)
        res = timed(stream, calls, args.regions, args.warmup)
        ctx.sync()
        ctx.set_image(np.zeros((1, 1, 4), np.uint8))         # drop the alias before the buffer goes away
        floor_ms = F * W * H * 8 / 8e12 * 1e3
        for k in res:
            res[k]["x_byte_floor"] = round(res[k]["median_ms"] / floor_ms, 2)
            res[k]["covered_share_frame0"] = covered[k]
        print(json.dumps({"frames": F, "width": W, "height": H, "byte_floor_ms": round(floor_ms, 4), **res,
                          "sphere_over_plane": round(res["sphere_plain"]["median_ms"] / res["plane_plain"]["median_ms"], 3),
                          "regions": args.regions, "warmup": args.warmup}), flush=True)


if __name__ == "__main__":
    main()
