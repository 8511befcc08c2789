#!/usr/bin/env python3
"""bench_trilinear.py -- what minification filtering costs: hg_pyramid_build_device against the bytes of the planes it reads, and
hg_remap_trilinear_frames_device beside hg_remap_bilinear_frames_device (the parent's kernel, unchanged: the yardstick), same box, one
process, same fields and planes.

The set: 64 frames out of 3840x2160 source planes (`--planes` of them, frame f reads plane f % planes), through two frame sets
    shrink4      an affine 4x shrink: 960x540 per frame
    projective   the C2-like projective pattern onto half the size: about 1730x1080 per frame, shrinking 2x and more towards one edge
and two kinds of plane: u8 x 4 channels (a picture) and f32 x 1 channel.
    build        hg_pyramid_build_device, all levels of all planes; gbs = plane bytes read per second of the median
    bilinear     one hg_remap_bilinear_frames_device
    trilinear    one hg_remap_trilinear_frames_device over the built pyramids (the build is not inside the region)
The variants run in turn inside every round (alternating, so that drift hits all alike); a region is one variant's whole work between two
events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed
ones.  Before anything is timed the trilinear remap with levels = 1 is compared with the bilinear remap byte for byte.  One JSON line per case.
    python tools/bench_trilinear.py [--regions N] [--warmup W] [--frames F] [--planes P] [--cases shrink4:u8x4,shrink4:f32x1,projective:u8x4,projective:f32x1]
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
WL = _load("hg_workloads", os.path.join(PKG, "workloads.py"))


def _bytes(n, dev):
    return torch.empty(int(n), dtype=torch.uint8, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--cases", default="shrink4:u8x4,shrink4:f32x1,projective:u8x4,projective:f32x1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_trilinear.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    W, H, F, NP = 3840, 2160, args.frames, args.planes
    levels = HG.pyramid_levels(W, H)
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        size_only = _bytes(W * H * 4, dev)                       # the field calls read the source's size only
        ctx.set_image_device(size_only.data_ptr(), W, H)
        s4 = WL.corners(W, H)
        sets = {}
        g4 = [(0, 0, W // 4, H // 4)] * F
        sets["shrink4"] = (g4, lambda: ctx.geometric_set_frames(0, np.tile(np.array([4, 0, 0, 4, 1.5, 1.5, 0, 0], np.float64), F), g4))
        d4 = [WL.projective_dst(W, H, 0.01 * (f % 4)) * 0.5 for f in range(F)]
        gp = [tuple(int(v) for v in HG.transform_limits(1, HG.solve_projective(s4, d), W, H)) for d in d4]
        sets["projective"] = (gp, lambda: ctx.geometric_set_frames_points(1, np.concatenate(d4), np.tile(s4, F), gp, HG.pack_offsets(gp)[0]))
        fields = {}
        try:
            for case in args.cases.split(","):
                which, kind = case.split(":")
                geoms, stage = sets[which]
                n_px = sum(max(g[2], 0) * max(g[3], 0) for g in geoms)
                if which not in fields:
                    stage()
                    d_co = _bytes(HG.pack_field_offsets(geoms, HG.FIELD_COORDS)[1], dev)
                    ctx.field_inverse_geometric_frames_device(HG.FIELD_COORDS, d_co.data_ptr())
                    ctx.sync()
                    fields[which] = d_co
                d_co = fields[which]
                elem = HG.ELEM_U8 if kind.startswith("u8") else HG.ELEM_F32
                ch = int(kind.split("x")[1])
                px = ch * (1 if elem == HG.ELEM_U8 else 4)
                stride = (W * H * px + 255) // 256 * 256
                _, ptotal = HG.pyramid_layout(W, H, elem, ch, levels)
                ototal = HG.pack_plane_offsets(geoms, px)[1]
                g = torch.Generator(device=dev)
                g.manual_seed(7)
                if elem == HG.ELEM_U8:
                    planes = torch.randint(0, 256, (NP * stride,), dtype=torch.uint8, device=dev, generator=g)
                else:
                    planes = torch.rand(NP * stride // 4, dtype=torch.float32, device=dev, generator=g)
                pyr = _bytes(NP * ptotal, dev)
                P, Y, C = planes.data_ptr(), pyr.data_ptr(), d_co.data_ptr()

                def build(_):
                    ctx.pyramid_build_device(P, W, H, NP, stride, elem, ch, levels, Y, ptotal)

                def bilinear(d_out):
                    ctx.remap_bilinear_frames_device(geoms, C, P, W, H, NP, stride, elem, ch, d_out)

                def trilinear(d_out, lv=levels):
                    ctx.remap_trilinear_frames_device(geoms, C, P, W, H, NP, stride, elem, ch, d_out, Y, ptotal, lv)

                a = torch.full((ototal,), 0xA5, dtype=torch.uint8, device=dev)
                b = torch.full((ototal,), 0xA5, dtype=torch.uint8, device=dev)
                build(None)
                bilinear(a.data_ptr())
                trilinear(b.data_ptr(), 1)
                ctx.sync()
                if not torch.equal(a, b):
                    sys.exit(f"{case}: the trilinear remap with one level differs from the bilinear remap")
                trilinear(b.data_ptr())
                ctx.sync()
                differs = int((a != b).sum().item())
                d_out = a.data_ptr()
                del b
                variants = [("build", build), ("bilinear", bilinear), ("trilinear", trilinear)]
                times = {label: [] for label, _ in variants}
                for r in range(args.warmup + args.regions):
                    for label, run in variants:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        run(d_out)
                        e1.record(stream)
                        e1.synchronize()
                        if r >= args.warmup:
                            times[label].append(e0.elapsed_time(e1))
                res = {}
                for label, t in times.items():
                    res[label] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4)}
                res["build"]["gbs"] = round(NP * W * H * px / (res["build"]["median_ms"] * 1e-3) / 1e9, 1)
                res["trilinear"]["vs_bilinear"] = round(res["trilinear"]["median_ms"] / res["bilinear"]["median_ms"], 3)
                print(json.dumps({"case": case, "n_frames": F, "n_planes": NP, "output_px": n_px, "pixel_bytes": px, "levels": levels,
                                  "plane_bytes": NP * W * H * px, "pyramid_bytes": NP * ptotal, "bytes_changed_by_the_filter": differs, **res,
                                  "regions": args.regions, "warmup": args.warmup}), flush=True)
                del planes, pyr, a
        finally:
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))         # drop the alias before the buffer goes away


if __name__ == "__main__":
    main()
