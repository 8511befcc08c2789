#!/usr/bin/env python3
"""bench_field.py -- the source field of an inverse warp (hg_field_*) beside the warp itself, same box, one process, same frames.

Per case, alternating for `--rounds` rounds, `--warmup` untimed then `--steps` timed steps of
    warp          warp_*_frames_device                               (nearest; the direct path)
    index/coords  field_inverse_*_frames_device in that format       (the field kernel alone)
    pair          the index field + remap_index_device of 4-byte pixels over all frames (frame by frame: one source offset each)
kernel_ms = hipEvents around the dominant kernel (hg_set_timing: the warp kernel, or the field kernel), per launch; step_ms = wall time
per step with one hg_sync at the end of the timed region (piecewise field calls settle themselves inside every call).  field_gbs = field
bytes written per second of kernel time, and its share of the 8 TB/s the README measures bandwidth against.  One JSON line per case:
    C2   1080p projective, 64 frames, device-side solves, shared source
    C3   4K piecewise, 200 triangles, 64 frames, shared source
    python tools/bench_field.py [--steps K] [--warmup W] [--rounds R] [--cases C2,C3]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "homography.js_amd")
PEAK_GBS = 8000.0


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


HG = _load("hgwarp", os.path.join(PKG, "hgwarp.py"))
WL = _load("hg_workloads", os.path.join(PKG, "workloads.py"))


def _case(ctx, name):
    """(W, H, geoms, stage(), warp(d_out), field(fmt, d_field))"""
    if name == "C2":
        W, H, F = 1920, 1080, 64
        s4 = WL.corners(W, H)
        d4 = [WL.projective_dst(W, H, 0.01 * (f % 4)) for f in range(F)]
        geoms = [tuple(int(v) for v in HG.transform_limits(1, HG.solve_projective(s4, d), W, H)) for d in d4]
        offs, _ = HG.pack_offsets(geoms)

        def stage():
            ctx.geometric_set_frames_points(1, np.concatenate(d4), np.tile(s4, F), geoms, offs)
        return W, H, geoms, stage, ctx.warp_inverse_geometric_frames_device, ctx.field_inverse_geometric_frames_device
    cfg = WL.CONFIGS[name]
    sp, tris, frames, geoms = WL.piecewise_frames(cfg, 64)
    msx, msy = WL.src_min(sp)
    offs, _ = HG.pack_offsets(geoms)

    def stage():
        ctx.piecewise_set_mesh(sp, tris, msx, msy)
        ctx.piecewise_set_frames(np.concatenate(frames), geoms, offs)
    return cfg["W"], cfg["H"], geoms, stage, ctx.warp_inverse_piecewise_frames_device, ctx.field_inverse_piecewise_frames_device


def _timed(ctx, step, steps, warmup):
    for _ in range(warmup):
        step()
    ctx.sync()
    ctx.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.sync()
    el = time.perf_counter() - t0
    k_ms, n = ctx.kernel_ms_stats()
    ctx.set_timing(False)
    return k_ms / max(n, 1), el / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="alternations per case (the best kernel time of each variant is reported)")
    ap.add_argument("--cases", default="C2,C3")
    args = ap.parse_args()
    with HG.Context(0) as ctx:
        for name in args.cases.split(","):
            W, H, geoms, stage, warp, field = _case(ctx, name)
            n_px = [max(g[2], 0) * max(g[3], 0) for g in geoms]
            roffs, rtotal = HG.pack_offsets(geoms)
            ioffs, itotal = HG.pack_field_offsets(geoms, HG.FIELD_INDEX)
            _, ctotal = HG.pack_field_offsets(geoms, HG.FIELD_COORDS)
            d_src, d_out, d_field = ctx.alloc(W * H * 4), ctx.alloc(rtotal), ctx.alloc(ctotal)
            try:
                ctx.to_device(d_src, WL.lcg_image(W, H, 1))
                ctx.set_image_device(d_src, W, H)
                stage()

                def pair():
                    field(HG.FIELD_INDEX, d_field)
                    for f, n in enumerate(n_px):
                        if n:
                            ctx.remap_index_device(d_field + ioffs[f], n, d_src, W * H, 4, d_out + roffs[f])
                variants = (("warp", lambda: warp(d_out)), ("index", lambda: field(HG.FIELD_INDEX, d_field)),
                            ("coords", lambda: field(HG.FIELD_COORDS, d_field)), ("pair", pair))
                res = {}
                for _ in range(args.rounds):
                    for label, step in variants:
                        k_ms, s_ms = _timed(ctx, step, args.steps, args.warmup)
                        if label not in res or k_ms < res[label]["kernel_ms"]:
                            res[label] = {"kernel_ms": round(k_ms, 5), "step_ms": round(s_ms, 5)}
                for label, per in (("index", 4), ("coords", 8)):
                    gbs = per * sum(n_px) / (res[label]["kernel_ms"] * 1e-3) / 1e9 if res[label]["kernel_ms"] > 0 else None
                    res[label]["field_bytes"] = per * sum(n_px)
                    res[label]["field_gbs"] = round(gbs, 1) if gbs else None
                    res[label]["share_of_8TBs"] = round(gbs / PEAK_GBS, 3) if gbs else None
                    res[label]["kernel_vs_warp"] = round(res[label]["kernel_ms"] / res["warp"]["kernel_ms"], 3) if res["warp"]["kernel_ms"] > 0 else None
                line = {"case": name, "frames": len(geoms), "output_px": sum(n_px), **res,
                        "pair_step_vs_warp_step": round(res["pair"]["step_ms"] / res["warp"]["step_ms"], 3),
                        "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
                print(json.dumps(line), flush=True)
            finally:
                ctx.set_image(np.zeros((1, 1, 4), np.uint8))                       # drop the alias before the buffer goes away
                for p in (d_field, d_out, d_src):
                    ctx.free(p)


if __name__ == "__main__":
    main()
