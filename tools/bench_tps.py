#!/usr/bin/env python3
"""bench_tps.py -- what warping through thin-plate splines costs: hg_tps_solve_frames_device (k_tps_solve) and hg_field_tps_frames_device
(k_tps_field; above step 1 the lattice and k_tps_blend) on the landmarks of configuration C4 (workloads.py: a seeded face mesh, every frame
moving every landmark by 0.02 W), the destiny points as FROM and the mesh as TO, the whole 3840 x 2160 frame as every window.

    cases     64 frames of 3840 x 2160 at N = 68, 200 and 1024 landmarks: the coords field at steps 1, 4, 8 and 16, and the solve alone
    beside    the piecewise coords field of the same landmarks (Delaunay triangles of the mesh) over the same windows: the price of smoothness;
              scipy's RBFInterpolator (thin_plate_spline) for ONE frame on the CPU; the lattice's error against step 1 (max and mean, px, over
              the pixels both cover) on the first frame

A region is one whole call between two events on the context's stream; the calls of a case run in turn inside every round (alternating, so
that drift hits all alike); per call the median and the minimum over `--regions` regions after `--warmup` untimed ones.  One JSON line per N.
    python tools/bench_tps.py [--regions N] [--warmup W] [--points 68,200,1024] [--frames 64] [--no-scipy]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

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
W, H = WL.CONFIGS["C4"]["W"], WL.CONFIGS["C4"]["H"]
STEPS = (1, 4, 8, 16)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", default="68,200,1024")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tps.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    F = args.frames
    geoms = [(0, 0, W, H)] * F
    offs, total = HG.pack_field_offsets(geoms, HG.FIELD_COORDS)
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        d_field = torch.empty(total, dtype=torch.uint8, device=dev)
        d_one = torch.empty(W * H * 8, dtype=torch.uint8, device=dev)            # frame 0 at step 1, for the lattice's error
        for n in (int(v) for v in args.points.split(",")):
            sp = WL.face_mesh(W, H, n, seed=68)
            dst = np.concatenate(WL.face_frames(sp, W, F)).astype(np.float32)
            rec_b, scr_b = HG.tps_layout(n, F)
            d_from, d_to = torch.from_numpy(dst).to(dev), torch.from_numpy(np.asarray(sp, np.float32)).to(dev)
            d_rec = torch.empty(rec_b * F, dtype=torch.uint8, device=dev)
            d_st = torch.empty(F, dtype=torch.int32, device=dev)
            d_scr = torch.empty(max(scr_b, 8), dtype=torch.uint8, device=dev)
            node_b = max(HG.tps_field_layout(geoms, s) for s in STEPS)
            d_nodes = torch.empty(max(node_b, 16), dtype=torch.uint8, device=dev)
            solve = lambda: ctx.tps_solve_frames_device(d_from.data_ptr(), F, d_to.data_ptr(), 1, n, F, d_rec.data_ptr(), d_st.data_ptr(),
                                                        d_scratch=d_scr.data_ptr() if scr_b else 0)
            field = lambda step: (lambda: ctx.field_tps_frames_device(d_rec.data_ptr(), n, geoms, W, H, HG.FIELD_COORDS, d_field.data_ptr(), step=step,
                                                                      d_scratch=d_nodes.data_ptr() if step > 1 else 0))
            solve()
            ctx.sync()
            status = d_st.cpu().numpy()
            if (status != HG.TPS_OK).any():
                sys.exit(f"N = {n}: a frame did not solve: {status.tolist()}")
            extra = {}
            field(1)()
            ctx.sync()
            d_one.copy_(d_field[:W * H * 8])
            ref = d_one.view(torch.float32).view(-1, 2)
            extra["covered_share_frame0"] = round(float((~torch.isnan(ref[:, 0])).float().mean().item()), 4)
            for step in STEPS[1:]:
                field(step)()
                ctx.sync()
                got = d_field[:W * H * 8].view(torch.float32).view(-1, 2)
                both = ~torch.isnan(ref[:, 0]) & ~torch.isnan(got[:, 0])
                err = torch.linalg.vector_norm((got[both] - ref[both]).double(), dim=1)
                extra[f"step{step}_error_px"] = {"max": float(f"{err.max().item():.3g}"), "mean": float(f"{err.mean().item():.3g}")}
            calls = {"solve": solve}
            calls.update({f"step{s}": field(s) for s in STEPS})
            res = timed(stream, calls, args.regions, args.warmup)
            res["step1"]["terms_per_s"] = float(f"{F * W * H * n / (res['step1']['median_ms'] * 1e-3):.4g}")
            # the piecewise coords field of the same landmarks over the same windows
            tris = HG.triangulate(sp)
            msx, msy = WL.src_min(sp)
            d_src = torch.zeros(W * H * 4, dtype=torch.uint8, device=dev)
            ctx.set_image_device(d_src.data_ptr(), W, H)
            ctx.piecewise_set_mesh(sp, tris, msx, msy)
            ctx.piecewise_set_frames(dst, geoms, HG.pack_offsets(geoms)[0])
            res.update({"piecewise_coords": timed(stream, {"pw": lambda: ctx.field_inverse_piecewise_frames_device(HG.FIELD_COORDS, d_field.data_ptr())},
                                                  args.regions, args.warmup)["pw"]})
            extra["triangles"] = int(len(tris) // 3)
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))                       # drop the alias before the buffer goes away
            if not args.no_scipy and n <= 200:
                try:
                    from scipy.interpolate import RBFInterpolator
                    t0 = time.perf_counter()
                    rbf = RBFInterpolator(dst[:2 * n].reshape(n, 2).astype(np.float64), np.asarray(sp, np.float64).reshape(n, 2), kernel="thin_plate_spline", degree=1)
                    rows = 135                                                   # 1/16 of the frame, scaled up: the whole frame would need 16 x the memory at once
                    yy, xx = np.mgrid[0:rows, 0:W]
                    rbf(np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64))
                    extra["scipy_one_frame_s"] = round((time.perf_counter() - t0) * H / rows, 2)
                except ImportError:
                    extra["scipy_one_frame_s"] = None
            print(json.dumps({"points": n, "frames": F, "width": W, "height": H, **res, **extra, "regions": args.regions, "warmup": args.warmup}), flush=True)
            del d_from, d_to, d_rec, d_st, d_scr, d_nodes, d_src


if __name__ == "__main__":
    main()
