#!/usr/bin/env python3
"""bench_forward_field.py -- the source field of a FORWARD warp (hg_field_forward_*) beside the forward warp itself, same box, one process,
same frames: a 4K source, batches of 8 resident frames, both paths (option fwd_tiles 1: the tile-binned kernels; 0: scatter + winner buffer).

Per case and path, alternating for `--rounds` rounds, `--warmup` untimed then `--steps` timed steps of
    warp    warp_forward_*_batch_device   (8 frames; queued, one hg_sync at the end of the timed region)
    field   field_forward_*_batch_device  (8 frames; the piecewise form settles itself inside every call, the geometric form is queued like the warp)
    pair    the field + remap_index_device of 4-byte pixels, frame by frame (what a second plane costs)
The forward paths have no event taps, so the figure is WALL time per frame (step / 8), best round; `field_vs_warp` is their ratio.  The
expectation is only that a field costs no more than the warp of the same frames: it issues one store and no gather.  One JSON line per case:
    affine       4K, same-size window, a slight rotation about the centre (what warp() sends through _geometricWarp)
    projective   4K, same-size window, a mild perspective (the forward loop of a projective matrix; warp() itself never takes it)
    piecewise    4K, 200 triangles (10 x 10 cells), the sinusoidal destination sets of the benchmark, their own windows
    python tools/bench_forward_field.py [--steps K] [--warmup W] [--rounds R] [--cases affine,projective,piecewise]
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
W, H, FRAMES = 3840, 2160, 8


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


HG = _load("hgwarp", os.path.join(PKG, "hgwarp.py"))
WL = _load("hg_workloads", os.path.join(PKG, "workloads.py"))


def _case(ctx, name):
    """(geoms, warp(offs, d_out), field(offs, d_field))"""
    if name in ("affine", "projective"):
        kind = 0 if name == "affine" else 1
        mats = np.zeros((FRAMES, 8))
        cx, cy = W / 2, H / 2
        for f in range(FRAMES):
            a = 0.004 * (1 + f % 4)
            c, s = np.cos(a), np.sin(a)
            tx, ty = cx - c * cx + s * cy, cy - s * cx - c * cy              # rotation by a about the centre
            if kind == 0:
                mats[f, :6] = [c, s, -s, c, tx, ty]
            else:
                g = 2.0e-6 * (1 + f % 4)
                mats[f] = [c, -s, tx, s, c, ty, g, -g]
        geoms = [(0, 0, W, H)] * FRAMES
        for f in range(FRAMES):
            assert HG.forward_tiles_admissible(kind, mats[f], W, H, geoms[f]) == 2, (name, f)
        return (geoms, lambda offs, d: ctx.warp_forward_geometric_batch_device(kind, mats, geoms, offs, d),
                lambda offs, d: ctx.field_forward_geometric_batch_device(kind, mats, geoms, offs, d))
    cfg = WL.CONFIGS["C3"]
    sp, tris, frames, geoms = WL.piecewise_frames(cfg, FRAMES)
    msx, msy = WL.src_min(sp)
    mm = HG.minmax_xy(sp)
    Mx, My = int(mm[2]), int(mm[3])
    dps = np.concatenate(frames)
    ctx.piecewise_set_mesh(sp, tris, msx, msy)
    return (geoms, lambda offs, d: ctx.warp_forward_piecewise_batch_device(dps, Mx, My, geoms, offs, d),
            lambda offs, d: ctx.field_forward_piecewise_batch_device(dps, Mx, My, geoms, offs, d))


def _timed(ctx, step, steps, warmup):
    for _ in range(warmup):
        step()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternations per case and path (the best time of each variant is reported)")
    ap.add_argument("--cases", default="affine,projective,piecewise")
    args = ap.parse_args()
    with HG.Context(0) as ctx:
        d_src = ctx.alloc(W * H * 4)
        ctx.to_device(d_src, WL.lcg_image(W, H, 1))
        ctx.set_image_device(d_src, W, H)
        try:
            for name in args.cases.split(","):
                geoms, warp, field = _case(ctx, name)
                n_px = [max(g[2], 0) * max(g[3], 0) for g in geoms]
                offs, total = HG.pack_offsets(geoms)
                assert HG.pack_field_offsets(geoms, HG.FIELD_INDEX) == (offs, total)
                d_out, d_field = ctx.alloc(total), ctx.alloc(total)
                try:
                    def pair():
                        field(offs, d_field)
                        for f, n in enumerate(n_px):
                            if n:
                                ctx.remap_index_device(d_field + offs[f], n, d_src, W * H, 4, d_out + offs[f])
                    line = {"case": name, "frames": FRAMES, "output_px": sum(n_px)}
                    for tiles, path in ((1, "tiles"), (0, "scatter")):
                        ctx.set_option("fwd_tiles", tiles)
                        res = {}
                        for _ in range(args.rounds):
                            for label, step in (("warp", lambda: warp(offs, d_out)), ("field", lambda: field(offs, d_field)), ("pair", pair)):
                                ms = _timed(ctx, step, args.steps, args.warmup) / FRAMES
                                res[label] = min(res.get(label, ms), ms)
                        assert ctx.last_forward_kernel() == (2 if tiles else 1) and ctx.last_forward_field_kernel() == (2 if tiles else 1)
                        line[path] = {"warp_ms_per_frame": round(res["warp"], 5), "field_ms_per_frame": round(res["field"], 5),
                                      "pair_ms_per_frame": round(res["pair"], 5), "field_vs_warp": round(res["field"] / res["warp"], 3)}
                    line.update(redone_frames=ctx.redone_frames(), steps=args.steps, warmup=args.warmup, rounds=args.rounds)
                    print(json.dumps(line), flush=True)
                finally:
                    ctx.free(d_field); ctx.free(d_out)
        finally:
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))                       # drop the alias before the buffer goes away
            ctx.free(d_src)


if __name__ == "__main__":
    main()
