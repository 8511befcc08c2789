#!/usr/bin/env python3
"""bench_remap_frames.py -- the remaps of a whole frame set (hg_remap_*_frames_device) beside the loop of single-list calls, same box, one
process, same fields and planes.

The set: 64 frames of 1920x1080 through the fields of the C2-like projective set of tools/bench_field.py, one source plane per frame.
    index     pixels of 1, 2, 4, 8 and 16 bytes through the HG_FIELD_INDEX field:
                  loop           64 x hg_remap_index_device (k_remap_index: one pixel per lane)
                  frames_1px     one hg_remap_index_frames_device, option "remap_pack" 0 (one pixel per lane)
                  frames_packed  one hg_remap_index_frames_device, option "remap_pack" 1 (4 pixels per lane, one packed store)
    bilinear  u8 and f32 planes of 1 and 4 channels through the HG_FIELD_COORDS field:
                  loop           64 x hg_remap_bilinear_u8_device / _f32_device
                  frames         one hg_remap_bilinear_frames_device
Every variant of a case runs in turn inside every round (alternating, so that drift hits all alike); a region is one variant's whole work
between two events on the context's stream -- for the loop that includes the gaps between its 64 launches, which is what the caller waits
for --; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed ones.  gbs = bytes the
remap must move (field read + one source pixel or four taps' worth counted once + output written) per second of the median.  The outputs
of all variants of a case are compared byte for byte before anything is timed.  One JSON line per case.
    python tools/bench_remap_frames.py [--regions N] [--warmup W] [--frames F] [--cases index1,index2,index4,index8,index16,u8x1,u8x4,f32x1,f32x4]
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
    ap.add_argument("--cases", default="index1,index2,index4,index8,index16,u8x1,u8x4,f32x1,f32x4")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_remap_frames.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    W, H, F = 1920, 1080, args.frames
    n_src = W * H
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        s4 = WL.corners(W, H)
        d4 = [WL.projective_dst(W, H, 0.01 * (f % 4)) for f in range(F)]
        geoms = [tuple(int(v) for v in HG.transform_limits(1, HG.solve_projective(s4, d), W, H)) for d in d4]
        n_px = [max(g[2], 0) * max(g[3], 0) for g in geoms]
        ioffs, itotal = HG.pack_field_offsets(geoms, HG.FIELD_INDEX)
        coffs, ctotal = HG.pack_field_offsets(geoms, HG.FIELD_COORDS)
        size_only = _bytes(n_src * 4, dev)                   # the field calls read the source's size only
        ctx.set_image_device(size_only.data_ptr(), W, H)
        ctx.geometric_set_frames_points(1, np.concatenate(d4), np.tile(s4, F), geoms, HG.pack_offsets(geoms)[0])
        d_idx, d_co = _bytes(itotal, dev), _bytes(ctotal, dev)
        ctx.field_inverse_geometric_frames_device(HG.FIELD_INDEX, d_idx.data_ptr())
        ctx.field_inverse_geometric_frames_device(HG.FIELD_COORDS, d_co.data_ptr())
        ctx.sync()
        try:
            for case in args.cases.split(","):
                index = case.startswith("index")
                if index:
                    px = int(case[5:])
                    fld, foffs, fld_px = d_idx, ioffs, 4
                else:
                    elem = HG.ELEM_U8 if case.startswith("u8") else HG.ELEM_F32
                    ch = int(case.split("x")[1])
                    px = ch * (1 if elem == HG.ELEM_U8 else 4)
                    fld, foffs, fld_px = d_co, coffs, 8
                stride = (n_src * px + 255) // 256 * 256
                ooffs, ototal = HG.pack_plane_offsets(geoms, px)
                g = torch.Generator(device=dev)
                g.manual_seed(7)
                planes = torch.randint(0, 256, (F * stride,), dtype=torch.uint8, device=dev, generator=g)
                if not index and elem == HG.ELEM_F32:            # finite floats
                    planes = torch.rand(F * stride // 4, dtype=torch.float32, device=dev, generator=g)
                outs = {}
                P, FP = planes.data_ptr(), fld.data_ptr()

                def loop(d_out):
                    for f in range(F):
                        if not n_px[f]:
                            continue
                        if index:
                            ctx.remap_index_device(FP + foffs[f], n_px[f], P + f * stride, n_src, px, d_out + ooffs[f])
                        elif elem == HG.ELEM_U8:
                            ctx.remap_bilinear_u8_device(FP + foffs[f], n_px[f], P + f * stride, W, H, ch, d_out + ooffs[f])
                        else:
                            ctx.remap_bilinear_f32_device(FP + foffs[f], n_px[f], P + f * stride, W, H, ch, d_out + ooffs[f])

                def frames(pack):
                    def run(d_out):
                        if index:
                            ctx.set_option("remap_pack", pack)
                            ctx.remap_index_frames_device(geoms, FP, P, n_src, F, stride, px, d_out)
                            ctx.set_option("remap_pack", -1)
                        else:
                            ctx.remap_bilinear_frames_device(geoms, FP, P, W, H, F, stride, elem, ch, d_out)
                    return run
                variants = [("loop", loop)] + ([("frames_1px", frames(0)), ("frames_packed", frames(1))] if index else [("frames", frames(-1))])
                # the same bytes from every variant, before anything is timed
                for label, run in variants:
                    outs[label] = torch.full((ototal,), 0xA5, dtype=torch.uint8, device=dev)
                    run(outs[label].data_ptr())
                ctx.sync()
                for label, _ in variants[1:]:
                    if not torch.equal(outs[label], outs["loop"]):
                        sys.exit(f"{case}: variant {label} differs from the loop of single calls")
                d_out = outs["loop"].data_ptr()
                for label, _ in variants[1:]:
                    del outs[label]
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
                moved = sum(n_px) * (fld_px + 2 * px)
                res = {}
                for label, t in times.items():
                    med = statistics.median(t)
                    res[label] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "gbs": round(moved / (med * 1e-3) / 1e9, 1)}
                for label in list(res)[1:]:
                    res[label]["vs_loop"] = round(res[label]["median_ms"] / res["loop"]["median_ms"], 3)
                print(json.dumps({"case": case, "n_frames": F, "output_px": sum(n_px), "pixel_bytes": px, **res,
                                  "regions": args.regions, "warmup": args.warmup}), flush=True)
                del planes, outs
        finally:
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))         # drop the alias before the buffer goes away


if __name__ == "__main__":
    main()
