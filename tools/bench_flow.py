#!/usr/bin/env python3
"""bench_flow.py -- what dense optical flow costs: hg_flow_dense_frames_device (luma copies, both pyramids, per level k_flow_up and n_iter
launches of k_flow_iter, then k_flow_finish) on RGBA frames cut from one smooth seeded picture, every frame moved a few pixels.

    cases     64 pairs of 1920 x 1080 x 4 against one keyframe;  8 pairs of 3840 x 2160 x 4
    call      the default parameters (levels down to 16 pixels on the shorter side, 4 iterations, radius 3, min_eig 1, max_update 1), and
              the same at radius 7; field only

The two radii run in turn inside every round (alternating, so that drift hits both alike); a region is one whole call between two events on
the context's stream; per radius the median and the minimum over `--regions` regions after `--warmup` untimed ones.  Beside each: the time to
read both planes and write the field once at 8 TB/s (the floor no flow can beat), the share of good pixels at level 0, and the time of a
plain torch formulation of ONE iteration of ONE frame at level 0 on the same GPU (grid_sample for the taps of F, avg_pool2d for the five
window sums, the 2 x 2 solve in float64).  One JSON line per case.  Without a GPU the script reports the numpy model's endpoint error on
the fixture of tests/hgtest/flow.py and says that nothing was timed.
    python tools/bench_flow.py [--regions N] [--warmup W] [--cases 64x1920x1080,8x3840x2160]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hgtest import flow as FM                # noqa: E402  (the model: the CPU figure)

N_ITER, MIN_EIG, MAX_UPDATE = 4, 1.0, 1.0
RADII = (3, 7)


def picture(W, H, seed, dev):
    """A smooth picture (seeded noise of 1/8 the size, enlarged) as RGBA u8 on the device: (H, W, 4)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    low = torch.rand(1, 3, H // 8 + 2, W // 8 + 2, generator=g)
    big = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    rgba = torch.cat([big[0] * 255, torch.full((1, H, W), 255.0)]).permute(1, 2, 0).round().to(torch.uint8)
    return rgba.contiguous().to(dev)


def torch_iteration(T, F, u, v, R):
    """One iteration of one frame in plain torch (float32 planes on the GPU, the solve in float64): -> (u, v)."""
    H, W = T.shape
    pad = torch.nn.functional.pad
    Tp = pad(T[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]
    gx, gy = Tp[1:-1, 2:] - Tp[1:-1, :-2], Tp[2:, 1:-1] - Tp[:-2, 1:-1]
    ys, xs = torch.meshgrid(torch.arange(H, device=T.device, dtype=torch.float32), torch.arange(W, device=T.device, dtype=torch.float32), indexing="ij")
    grid = torch.stack([(xs + u + 0.5) * 2 / W - 1, (ys + v + 0.5) * 2 / H - 1], -1)[None]
    s = torch.nn.functional.grid_sample(F[None, None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0, 0]
    e0 = (s - T) - (gx * u + gy * v) / 2
    k = 2 * R + 1
    planes = torch.stack([gx * gx, gx * gy, gy * gy, gx * e0, gy * e0])[None]
    sums = torch.nn.functional.avg_pool2d(planes, k, 1, R, count_include_pad=True)[0].to(torch.float64) * (k * k)
    gxx, gxy, gyy, bx, by = sums
    det = gxx * gyy - gxy * gxy
    good = (gxx + gyy > 0) & (det >= 4 * k * k * MIN_EIG * (gxx + gyy)) & (det > 0)
    U, V = -((gyy * bx - gxy * by) / det) / 0.5, -((gxx * by - gxy * bx) / det) / 0.5
    un = torch.where(good, u + (U - u).clamp(-MAX_UPDATE, MAX_UPDATE), u.to(torch.float64)).to(torch.float32)
    vn = torch.where(good, v + (V - v).clamp(-MAX_UPDATE, MAX_UPDATE), v.to(torch.float64)).to(torch.float32)
    return un, vn


def model_figures():
    frm, to, u, v = FM.fixture()
    zero = float(np.hypot(u, v).mean())
    out = {"fixture": "160x224", "zero_flow_epe_px": round(zero, 3)}
    for levels, it, R in ((4, 2, 3), (4, 4, 3), (4, 8, 4), (4, 16, 4), (1, 8, 4)):
        out[f"model_epe_px_L{levels}_I{it}_R{R}"] = round(FM.epe(FM.flow(frm, to, levels, it, R).flow, u, v), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="64x1920x1080,8x3840x2160")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"timed": False, "note": "no GPU: nothing was timed", **model_figures()}), flush=True)
        return
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        for case in args.cases.split(","):
            F, W, H = (int(v) for v in case.split("x"))
            levels = HG.flow_default_levels(W, H)
            key = picture(W, H, 3, dev)
            frames = torch.stack([torch.roll(key, (1 + f % 3, f % 5 - 2), (1, 0)) for f in range(F)]).contiguous()
            scratch = torch.empty(HG.flow_layout(W, H, 4, F, 1, levels), dtype=torch.uint8, device=dev)
            field = torch.empty(F * ((W * H * 8 + 255) // 256 * 256), dtype=torch.uint8, device=dev)
            good = torch.empty(F * W * H, dtype=torch.uint8, device=dev)

            def call(R, want_good=False):
                return lambda: ctx.flow_dense_frames_device(frames.data_ptr(), F, key.data_ptr(), 1, W, H, 4, field.data_ptr(), scratch.data_ptr(), levels=levels,
                                                            n_iter=N_ITER, radius=R, min_eig=MIN_EIG, max_update=MAX_UPDATE,
                                                            d_good=good.data_ptr() if want_good else 0)

            res, extra = {}, {}
            for R in RADII:
                call(R, True)()
                ctx.sync()
                extra[f"radius{R}_good_share"] = round(float(good.to(torch.float32).mean().item()), 4)
                fl = field.view(torch.float32).reshape(F, -1)[:, :W * H * 2].reshape(F, H, W, 2)[0, H // 4:-H // 4, W // 4:-W // 4]
                xs = torch.arange(W, device=dev, dtype=torch.float32)[W // 4:-W // 4]
                extra[f"radius{R}_frame0_median_u_px"] = round(float((fl[..., 0] - xs[None, :]).median().item()), 3)      # (frame 0 is rolled by 1 column)
            times = {R: [] for R in RADII}
            for r in range(args.warmup + args.regions):
                for R in RADII:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call(R)()
                    e1.record(stream)
                    e1.synchronize()
                    if r >= args.warmup:
                        times[R].append(e0.elapsed_time(e1))
            px_iters = F * N_ITER * sum(w * h for w, h in [(-(-W // 2 ** k), -(-H // 2 ** k)) for k in range(levels)])
            for R, t in times.items():
                med = statistics.median(t)
                res[f"radius{R}"] = {"median_ms": round(med, 3), "min_ms": round(min(t), 3), "pixel_iterations_per_s": float(f"{px_iters / (med * 1e-3):.4g}")}
            extra["floor_ms_at_8TBs"] = round((F * W * H * (4 + 8) + W * H * 4) / 8e12 * 1e3, 3)      # read every RGBA pair once, write the field once
            lum = lambda p: ((77 * p[..., 0].long() + 150 * p[..., 1].long() + 29 * p[..., 2].long() + 128) >> 8).to(torch.float32)
            T, Fp = lum(key), lum(frames[0])
            z = torch.zeros_like(T)
            for R in RADII:
                tt = []
                for _ in range(7):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    torch_iteration(T, Fp, z, z, R)
                    e1.record(stream)
                    e1.synchronize()
                    tt.append(e0.elapsed_time(e1))
                extra[f"radius{R}_torch_one_frame_one_iteration_ms"] = round(statistics.median(tt), 3)
            print(json.dumps({"timed": True, "case": case, "frames": F, "width": W, "height": H, "levels": levels, "iterations": N_ITER, **res, **extra,
                              "regions": args.regions, "warmup": args.warmup}), flush=True)
            ctx.sync()
            del frames, key, scratch, field, good


if __name__ == "__main__":
    main()
