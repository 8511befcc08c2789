#!/usr/bin/env python3
"""bench_bicubic.py -- what the bicubic remap costs: hg_remap_bicubic_frames_device beside hg_remap_bilinear_frames_device (the parent's
kernel, unchanged: the yardstick), same box, one process, same fields and planes, back to back.

The set: 64 frames enlarged out of 960x540 source planes (`--planes` of them, frame f reads plane f % planes), through two frame sets
    enlarge4     an affine 4x enlargement, 3840x2160 per frame: neighbouring lanes share their taps
    projective   bench_aniso.py's projective pattern turned into an enlargement (the destination corners times 4): about 3460x2160 per frame
and two kinds of plane: u8 x 4 channels (a picture) and f32 x 1 channel.
    bilinear     one hg_remap_bilinear_frames_device
    catmull_rom / mitchell / bspline    one hg_remap_bicubic_frames_device with that (B, C); vs_bilinear = its median over bilinear's
The variants run in turn inside every round (alternating, so that drift hits all alike); a region is one variant's whole work between two
events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed
ones, and out_GBps = the bytes of output written per second of the median.  Before anything is timed, Catmull-Rom through a field of
integer coordinates is compared with the bilinear remap byte for byte.  One JSON line per case.
    python tools/bench_bicubic.py [--regions N] [--warmup W] [--frames F] [--planes P] [--cases enlarge4:u8x4,...]
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
CUBICS = (("catmull_rom", HG.CUBIC_CATMULL_ROM), ("mitchell", HG.CUBIC_MITCHELL), ("bspline", HG.CUBIC_BSPLINE))


def _bytes(n, dev):
    return torch.empty(int(n), dtype=torch.uint8, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--cases", default="enlarge4:u8x4,enlarge4:f32x1,projective:u8x4,projective:f32x1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bicubic.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    W, H, F, NP = 960, 540, args.frames, args.planes
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        size_only = _bytes(W * H * 4, dev)                       # the field calls read the source's size only
        ctx.set_image_device(size_only.data_ptr(), W, H)
        s4 = WL.corners(W, H)
        sets = {}
        g4 = [(0, 0, W * 4, H * 4)] * F
        sets["enlarge4"] = (g4, lambda: ctx.geometric_set_frames(0, np.tile(np.array([0.25, 0, 0, 0.25, 0.0, 0.0, 0, 0], np.float64), F), g4))
        d4 = [WL.projective_dst(W, H, 0.01 * (f % 4)) * 4.0 for f in range(F)]
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
                    covered = 0
                    for g, o in zip(geoms[:4], HG.pack_field_offsets(geoms, HG.FIELD_COORDS)[0][:4]):      # (the sets repeat every four frames)
                        n = max(g[2], 0) * max(g[3], 0)
                        covered += int(torch.isfinite(d_co[o:o + n * 8].view(torch.float32).reshape(-1, 2)).all(-1).sum().item())
                    fields[which] = (d_co, covered * (F // 4) if F % 4 == 0 else None)
                d_co, covered = fields[which]
                elem = HG.ELEM_U8 if kind.startswith("u8") else HG.ELEM_F32
                ch = int(kind.split("x")[1])
                px = ch * (1 if elem == HG.ELEM_U8 else 4)
                stride = (W * H * px + 255) // 256 * 256
                ototal = HG.pack_plane_offsets(geoms, px)[1]
                g = torch.Generator(device=dev)
                g.manual_seed(7)
                if elem == HG.ELEM_U8:
                    planes = torch.randint(0, 256, (NP * stride,), dtype=torch.uint8, device=dev, generator=g)
                else:
                    planes = torch.rand(NP * stride // 4, dtype=torch.float32, device=dev, generator=g)
                P, C = planes.data_ptr(), d_co.data_ptr()

                def bilinear(d_out):
                    ctx.remap_bilinear_frames_device(geoms, C, P, W, H, NP, stride, elem, ch, d_out)

                def bicubic(bc):
                    return lambda d_out: ctx.remap_bicubic_frames_device(geoms, C, P, W, H, NP, stride, elem, ch, d_out, bc[0], bc[1])

                # the check: integer coordinates, where Catmull-Rom IS the bilinear remap
                gi = [(0, 0, 1024, 64)] * 3
                ico = torch.stack([torch.randint(0, W, (3 * 65536,), device=dev, generator=g), torch.randint(0, H, (3 * 65536,), device=dev, generator=g)], -1).to(torch.float32).contiguous()
                ia = torch.full((HG.pack_plane_offsets(gi, px)[1],), 0xA5, dtype=torch.uint8, device=dev)
                ib = ia.clone()
                ctx.remap_bilinear_frames_device(gi, ico.data_ptr(), P, W, H, NP, stride, elem, ch, ia.data_ptr())
                ctx.remap_bicubic_frames_device(gi, ico.data_ptr(), P, W, H, NP, stride, elem, ch, ib.data_ptr())
                ctx.sync()
                if not torch.equal(ia, ib):
                    sys.exit(f"{case}: Catmull-Rom on integer coordinates differs from the bilinear remap")
                del ia, ib, ico

                a = torch.full((ototal,), 0xA5, dtype=torch.uint8, device=dev)
                d_out = a.data_ptr()
                variants = [("bilinear", bilinear)] + [(label, bicubic(bc)) for label, bc in CUBICS]
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
                    med = statistics.median(t)
                    res[label] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "out_GBps": round(n_px * px / med / 1e6, 1)}
                for label, _ in CUBICS:
                    res[label]["vs_bilinear"] = round(res[label]["median_ms"] / res["bilinear"]["median_ms"], 3)
                print(json.dumps({"case": case, "n_frames": F, "n_planes": NP, "source": [W, H], "frame": list(geoms[0][2:]), "output_px": n_px,
                                  "covered_px": covered, "pixel_bytes": px, **res, "regions": args.regions, "warmup": args.warmup}), flush=True)
                del planes, a
        finally:
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))         # drop the alias before the buffer goes away


if __name__ == "__main__":
    main()
