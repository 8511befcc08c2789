#!/usr/bin/env python3
"""bench_sampling.py -- nearest vs bilinear sampling of the inverse warps (hg_set_sampling), same box, one process.

Per case both modes run the same frame set on the same context, alternating: `--warmup` steps, then `--steps` timed steps of
`warp_*_frames_device` (the whole step: per-frame solves / set-up + the warp kernel, then hg_sync at the end of the timed region).
kernel_ms = hipEvents around the dominant kernel (hg_set_timing: k_geo_fast / the piecewise warp kernel), per launch; step_ms = wall
time per step.  Algorithmic bytes per launch are the same for both modes, the nearest loop's: 4 bytes written per output pixel + 4
bytes read per covered pixel (the covered count comes from one untimed warp of an all-255 source).  One JSON line per case:
    C2_shared / C2_distinct   1080p projective, 64 frames, device-side solves, one shared source / one source per frame
    C3                        4K piecewise, 200 triangles, 64 frames, shared source
    C5                        8K piecewise, 5 000 triangles, 8 frames, shared source
    python tools/bench_sampling.py [--steps K] [--warmup W] [--cases C2_shared,C2_distinct,C3,C5]
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


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


HG = _load("hgwarp", os.path.join(PKG, "hgwarp.py"))
WL = _load("hg_workloads", os.path.join(PKG, "workloads.py"))


def _case(ctx, name):
    """Stages the case's frame set on ctx; returns (W, H, geoms, offsets, total bytes, n_sources, run(d_out), covered(d_out) -> count)."""
    if name.startswith("C2"):
        W, H, F = 1920, 1080, 64
        s4 = WL.corners(W, H)
        d4 = [WL.projective_dst(W, H, 0.01 * (f % 4)) for f in range(F)]
        fwd = [HG.solve_projective(s4, d) for d in d4]
        geoms = [tuple(int(v) for v in HG.transform_limits(1, m, W, H)) for m in fwd]
        offs, total = HG.pack_offsets(geoms)
        n_src = F if name == "C2_distinct" else 1

        def stage():
            ctx.geometric_set_frames_points(1, np.concatenate(d4), np.tile(s4, F), geoms, offs)

        def run(d_out):
            ctx.warp_inverse_geometric_frames_device(d_out)
        return W, H, geoms, offs, total, n_src, stage, run
    cfg = WL.CONFIGS[name]
    F = 64 if name == "C3" else 8
    sp, tris, frames, geoms = WL.piecewise_frames(cfg, F)
    msx, msy = WL.src_min(sp)
    offs, total = HG.pack_offsets(geoms)

    def stage():
        ctx.piecewise_set_mesh(sp, tris, msx, msy)
        ctx.piecewise_set_frames(np.concatenate(frames), geoms, offs)

    def run(d_out):
        ctx.warp_inverse_piecewise_frames_device(d_out)
    return cfg["W"], cfg["H"], geoms, offs, total, 1, stage, run


def _timed(ctx, run, d_out, steps, warmup):
    for _ in range(warmup):
        run(d_out)
    ctx.sync()
    ctx.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        run(d_out)
    ctx.sync()
    el = time.perf_counter() - t0
    k_ms, n = ctx.kernel_ms_stats()
    ctx.set_timing(False)
    return k_ms / max(n, 1), el / steps * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="nearest / bilinear alternations per case (the best of each mode is reported)")
    ap.add_argument("--cases", default="C2_shared,C2_distinct,C3,C5")
    args = ap.parse_args()
    with HG.Context(0) as ctx:
        for name in args.cases.split(","):
            W, H, geoms, offs, total, n_src, stage, run = _case(ctx, name)
            stride = W * H * 4
            d_src = ctx.alloc(stride * n_src)
            d_out = ctx.alloc(total)
            try:
                ctx.to_device(d_src, np.full((H, W, 4), 255, np.uint8))            # all-255 source: covered pixels = non-zero alpha
                ctx.set_images_device(d_src, W, H, 1, stride)
                stage()
                run(d_out)
                ctx.sync()
                out = np.empty(total, np.uint8)
                for f, g in enumerate(geoms):
                    out[offs[f]:offs[f] + g[2] * g[3] * 4] = ctx.to_host(d_out, g[2] * g[3] * 4, offs[f])
                n_out = sum(max(g[2], 0) * max(g[3], 0) for g in geoms)
                n_hit = int(sum(int(np.count_nonzero(out[offs[f] + 3:offs[f] + g[2] * g[3] * 4:4])) for f, g in enumerate(geoms)))
                algo = 4.0 * n_out + 4.0 * n_hit
                for k in range(n_src):
                    ctx.to_device(d_src, WL.lcg_image(W, H, 1 + k), k * stride)
                ctx.set_images_device(d_src, W, H, n_src, stride)
                stage()
                res = {}
                for _ in range(args.rounds):
                    for mode, label in ((HG.SAMPLE_NEAREST, "nearest"), (HG.SAMPLE_BILINEAR, "bilinear")):
                        ctx.set_sampling(mode)
                        k_ms, s_ms, n = _timed(ctx, run, d_out, args.steps, args.warmup)
                        kind = ctx.last_piecewise_kernel() if not name.startswith("C2") else None
                        best = res.get(label)
                        if best is None or k_ms < best["kernel_ms"]:
                            res[label] = {"kernel_ms": round(k_ms, 5), "step_ms": round(s_ms, 5), "launches": n,
                                          "kernel_gbs": round(algo / (k_ms * 1e-3) / 1e9, 1) if k_ms > 0 else None,
                                          "step_gbs": round(algo / (s_ms * 1e-3) / 1e9, 1) if s_ms > 0 else None,
                                          "piecewise_kernel": kind}
                ctx.set_sampling(HG.SAMPLE_NEAREST)
                line = {"case": name, "frames": len(geoms), "sources": n_src, "output_px": n_out, "covered_px": n_hit,
                        "algorithmic_bytes_per_launch": int(algo), **res,
                        "ratio_kernel": round(res["bilinear"]["kernel_ms"] / res["nearest"]["kernel_ms"], 3),
                        "ratio_step": round(res["bilinear"]["step_ms"] / res["nearest"]["step_ms"], 3),
                        "steps": args.steps, "warmup": args.warmup}
                print(json.dumps(line), flush=True)
            finally:
                ctx.set_image(np.zeros((1, 1, 4), np.uint8))                       # drop the alias before the buffer goes away
                ctx.free(d_out)
                ctx.free(d_src)


if __name__ == "__main__":
    main()
