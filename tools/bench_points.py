#!/usr/bin/env python3
"""bench_points.py -- point lists through a frame set's geometry (hg_points_*) beside the only route a caller had before them: the
full-frame HG_FIELD_COORDS call of the same set.  Same box, one process, same frames.

Per case and list length, `--warmup` untimed then `--steps` timed calls of
    to_source   points_to_source_*_frames_device           (the staged set; piecewise: settled inside the call)
    to_output   points_to_output_*_batch_device            (stages its frames itself, as the forward entry points do)
    field       field_inverse_*_frames_device(COORDS)      (the whole window of every frame)
call_ms = hipEvents on the context's stream around the WHOLE call (everything it queues: uploads, k_tri_setup, the kernel), mean over the
timed calls.  One JSON line per (case, N):
    GEO    1080p projective, 64 frames, matrices on the host
    T200   4K piecewise, 200 triangles (10 x 10 cells), 64 frames
    T5000  4K piecewise, 5000 triangles (50 x 50 cells), 64 frames
    python tools/bench_points.py [--steps K] [--warmup W] [--cases GEO,T200,T5000] [--points 68,65536]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "homography.js_amd")
F = 64


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


HG = _load("hgwarp", os.path.join(PKG, "hgwarp.py"))
WL = _load("hg_workloads", os.path.join(PKG, "workloads.py"))
MESHES = {"T200": dict(W=3840, H=2160, nx=10, ny=10, A=40.0), "T5000": dict(W=3840, H=2160, nx=50, ny=50, A=10.0)}


def _case(ctx, name):
    """(W, H, geoms, triangles, stage(), to_source(p, n, s, o), to_output(p, n, s, o), field(fmt, d_field))"""
    if name == "GEO":
        W, H = 1920, 1080
        s4 = WL.corners(W, H)
        d4 = [WL.projective_dst(W, H, 0.01 * (f % 4)) for f in range(F)]
        fwd = np.array([HG.solve_projective(s4, d) for d in d4])
        inv = np.array([HG.solve_projective(d, s4) for d in d4])
        geoms = [tuple(int(v) for v in HG.transform_limits(1, m, W, H)) for m in fwd]

        def stage():
            ctx.geometric_set_frames(1, inv, geoms)
        return (W, H, geoms, 0, stage, ctx.points_to_source_geometric_frames_device,
                lambda p, n, s, o: ctx.points_to_output_geometric_batch_device(1, fwd, geoms, p, n, s, o), ctx.field_inverse_geometric_frames_device)
    cfg = MESHES[name]
    sp, tris, frames, geoms = WL.piecewise_frames(cfg, F)
    msx, msy = WL.src_min(sp)
    mm = HG.minmax_xy(sp)
    dst = np.concatenate(frames)

    def stage():
        ctx.piecewise_set_mesh(sp, tris, msx, msy)
        ctx.piecewise_set_frames(dst, geoms)
    return (cfg["W"], cfg["H"], geoms, tris.size // 3, stage, ctx.points_to_source_piecewise_frames_device,
            lambda p, n, s, o: ctx.points_to_output_piecewise_batch_device(dst, int(mm[2]), int(mm[3]), geoms, p, n, s, o),
            ctx.field_inverse_piecewise_frames_device)


def _timed(ctx, stream, step, steps, warmup):
    for _ in range(warmup):
        step()
    ctx.sync()
    total = 0.0
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        step()
        e1.record(stream)
        e1.synchronize()
        total += e0.elapsed_time(e1)
    ctx.sync()
    return total / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="GEO,T200,T5000")
    ap.add_argument("--points", default="68,65536")
    args = ap.parse_args()
    stream = torch.cuda.Stream(device=0)
    box = torch.cuda.get_device_name(0)
    with HG.Context(0, stream.cuda_stream) as ctx:
        for name in args.cases.split(","):
            W, H, geoms, T, stage, to_source, to_output, field = _case(ctx, name)
            mw, mh = max(g[2] for g in geoms), max(g[3] for g in geoms)
            _, ctotal = HG.pack_field_offsets(geoms, HG.FIELD_COORDS)
            d_src, d_field = ctx.alloc(W * H * 4), ctx.alloc(ctotal)
            try:
                ctx.to_device(d_src, WL.lcg_image(W, H, 1))
                ctx.set_image_device(d_src, W, H)
                stage()
                field_ms = _timed(ctx, stream, lambda: field(HG.FIELD_COORDS, d_field), args.steps, args.warmup)
                for N in (int(v) for v in args.points.split(",")):
                    rng = np.random.default_rng(N)
                    src_side = np.stack([rng.uniform(0, W, N), rng.uniform(0, H, N)], 1).astype(np.float32)
                    out_side = np.stack([rng.uniform(0, mw, N), rng.uniform(0, mh, N)], 1).astype(np.float32)
                    d_p, d_q, d_o = ctx.alloc(N * 8), ctx.alloc(N * 8), ctx.alloc(F * N * 8)
                    try:
                        ctx.to_device(d_p, out_side)
                        ctx.to_device(d_q, src_side)
                        stage()
                        src_ms = _timed(ctx, stream, lambda: to_source(d_p, N, 1, d_o), args.steps, args.warmup)
                        mapped = float((~np.isnan(ctx.to_host(d_o, F * N * 8).view(np.float32)[::2])).mean())
                        out_ms = _timed(ctx, stream, lambda: to_output(d_q, N, 1, d_o), args.steps, args.warmup)
                    finally:
                        for p in (d_p, d_q, d_o):
                            ctx.free(p)
                    print(json.dumps({"case": name, "box": box, "frames": F, "triangles": T, "points": N, "to_source_call_ms": round(src_ms, 4),
                                      "to_output_call_ms": round(out_ms, 4), "coords_field_call_ms": round(field_ms, 4),
                                      "field_px": sum(g[2] * g[3] for g in geoms), "to_source_vs_field": round(src_ms / field_ms, 4),
                                      "to_source_mapped_share": round(mapped, 3), "steps": args.steps, "warmup": args.warmup}), flush=True)
            finally:
                ctx.set_image(np.zeros((1, 1, 4), np.uint8))                       # drop the alias before the buffer goes away
                for p in (d_field, d_src):
                    ctx.free(p)


if __name__ == "__main__":
    main()
