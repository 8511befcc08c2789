#!/usr/bin/env python3
"""bench_align.py -- what refining frame transforms on the pixels costs: hg_align_refine_frames_device (k_align_luma, then per pass
k_align_accumulate and k_align_update) on RGBA frames cut from one smooth seeded picture, every frame started 0.7 px off.

    cases     64 frames of 1920 x 1080 x 4 against one keyframe at step 1, 2 and 4;  8 frames of 3840 x 2160;  1 frame of 1920 x 1080
    call      projective, photometric, 8 updates (eps 0: every frame runs them all, 9 passes), the whole frame as the rectangle

The steps of a case run in turn inside every round (alternating, so that drift hits all alike); a region is one whole call between two
events on the context's stream; per step the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed ones,
and the samples per second the median stands for (frames x samples x passes / time).  Beside them, for ONE frame and ONE pass: a plain torch
formulation on the same GPU (grid_sample for I and its central differences, the Jacobian rows as an N x 10 float64 matrix, J^T J by
matmul) and the numpy model (tests/hgtest/align.py), the CPU yardstick, whose pass-0 count the device's must equal.  One JSON line per case.
    python tools/bench_align.py [--regions N] [--warmup W] [--cases 64x1920x1080,8x3840x2160,1x1920x1080] [--no-model]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hgtest import align as AM               # noqa: E402  (the model: the yardstick and the check)

UPDATES = 8
START = np.array([1.0, 0.0, 0.5, 0.0, 1.0, -0.5, 0.0, 0.0])      # 0.7 px off the truth, which is the identity


def picture(W, H, seed, dev):
    """A smooth picture (seeded noise of 1/16 the size, enlarged) as RGBA u8 on the device: (H, W, 4)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    low = torch.rand(1, 3, H // 16 + 2, W // 16 + 2, generator=g)
    big = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    rgba = torch.cat([big[0] * 255, torch.full((1, H, W), 255.0)]).permute(1, 2, 0).round().to(torch.uint8)
    return rgba.contiguous().to(dev)


def torch_pass(luma_from, luma_to, m, step):
    """One pass, P = 10, in plain torch on the GPU: -> (n_valid, J^T J (10 x 10), J^T r (10))."""
    H, W = luma_from.shape
    dev = luma_from.device
    ys, xs = torch.arange(0, H, step, device=dev, dtype=torch.float64), torch.arange(0, W, step, device=dev, dtype=torch.float64)
    y, x = torch.meshgrid(ys, xs, indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    c, s = ((W - 1) / 2, (H - 1) / 2), 2 / max(W, H)
    xn, yn = (x - c[0]) * s, (y - c[1]) * s
    h = torch.tensor(AM.normalise(1, m, AM.geom(W, H, W, H)), device=dev)
    D = h[6] * xn + h[7] * yn + 1
    un, vn = (h[0] * xn + h[1] * yn + h[2]) / D, (h[3] * xn + h[4] * yn + h[5]) / D
    u, v = un / s + c[0], vn / s + c[1]
    ok = (u >= 1) & (u < W - 2) & (v >= 1) & (v < H - 2) & (D > 0)
    img = luma_to.to(torch.float32)[None, None]

    def sample(uu, vv):
        grid = torch.stack([(uu + 0.5) * 2 / W - 1, (vv + 0.5) * 2 / H - 1], -1).to(torch.float32)[None, None]
        return torch.nn.functional.grid_sample(img, grid, mode="bilinear", align_corners=False)[0, 0, 0].to(torch.float64)

    I = sample(u, v)
    gx, gy = (sample(u + 1, v) - sample(u - 1, v)) / 2 / s / D, (sample(u, v + 1) - sample(u, v - 1)) / 2 / s / D
    a = luma_from[(y.long()), (x.long())].to(torch.float64)
    w = -(gx * un + gy * vn)
    J = torch.stack([gx * xn, gx * yn, gx, gy * xn, gy * yn, gy, w * xn, w * yn, -a, -torch.ones_like(a)], 1) * ok[:, None]
    r = (a - I) * ok
    return int(ok.sum().item()), J.T @ J, J.T @ r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="64x1920x1080,8x3840x2160,1x1920x1080")
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_align.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        for case in args.cases.split(","):
            F, W, H = (int(v) for v in case.split("x"))
            key = picture(W, H, 3, dev)
            frames = key[None].expand(F, H, W, 4).contiguous()      # every frame shows the keyframe: the truth is the identity
            d_in = torch.from_numpy(np.tile(START, (F, 1))).to(dev)
            d_out = torch.empty(F * 8, dtype=torch.float64, device=dev)
            d_info = torch.empty(F * 48, dtype=torch.uint8, device=dev)

            def call(step):
                return lambda: ctx.align_refine_frames_device(HG.HG_PROJECTIVE, frames.data_ptr(), W, H, F, key.data_ptr(), W, H, 1, 4, (0, 0, W, H), d_in.data_ptr(),
                                                              d_out.data_ptr(), d_info.data_ptr(), step=step, photometric=True, n_iter=UPDATES, eps=0.0)

            steps = (1, 2, 4)
            res, extra = {}, {}
            for step in steps:
                call(step)()
                ctx.sync()
                info = d_info.cpu().numpy().view(HG.ALIGN_INFO)
                if not ((info["status"] == HG.ALIGN_MAX_ITER) & (info["updates"] == UPDATES)).all():
                    sys.exit(f"{case} step {step}: a frame did not run its {UPDATES} updates: {info['status'].tolist()}")
                err = max(AM.corner_displacement(1, m, [1, 0, 0, 0, 1, 0, 0, 0], (0, 0, W, H)) for m in d_out.cpu().numpy().reshape(F, 8))
                extra[f"step{step}_corner_error_px"] = float(f"{err:.3g}")
                extra[f"step{step}_n_valid"] = int(info["n_valid_first"][0])
            times = {s: [] for s in steps}
            for r in range(args.warmup + args.regions):
                for step in steps:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call(step)()
                    e1.record(stream)
                    e1.synchronize()
                    if r >= args.warmup:
                        times[step].append(e0.elapsed_time(e1))
            for step, t in times.items():
                med = statistics.median(t)
                n = -(-W // step) * -(-H // step)
                res[f"step{step}"] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "samples_per_s": float(f"{F * n * (UPDATES + 1) / (med * 1e-3):.4g}")}
            # one frame, one pass: plain torch on the same GPU, and the numpy model
            lum = lambda p: ((77 * p[..., 0].long() + 150 * p[..., 1].long() + 29 * p[..., 2].long() + 128) >> 8).to(torch.uint8)
            lf = lt = lum(key)
            for step in steps:
                n_t, _, _ = torch_pass(lf, lt, START, step)
                tt = []
                for _ in range(7):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    torch_pass(lf, lt, START, step)
                    e1.record(stream)
                    e1.synchronize()
                    tt.append(e0.elapsed_time(e1))
                extra[f"step{step}_torch_one_frame_one_pass_ms"] = round(statistics.median(tt), 3)
                if n_t != extra[f"step{step}_n_valid"]:
                    sys.exit(f"{case} step {step}: torch counts {n_t} valid samples, the device {extra[f'step{step}_n_valid']}")
            if not args.no_model:
                host = lf.cpu().numpy().astype(np.int64)
                step = 2
                t0 = time.perf_counter()
                n_m, _, _ = AM.one_pass(1, 1, AM.normalise(1, START, AM.geom(W, H, W, H)), 1.0, 0.0, host, host, AM.geom(W, H, W, H), (0, 0, W, H), step)
                extra["step2_numpy_one_frame_one_pass_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                if n_m != extra["step2_n_valid"]:
                    sys.exit(f"{case}: the model counts {n_m} valid samples at step 2, the device {extra['step2_n_valid']}")
            print(json.dumps({"case": case, "frames": F, "width": W, "height": H, "updates": UPDATES, **res, **extra, "regions": args.regions, "warmup": args.warmup}), flush=True)
            ctx.sync()
            del frames, key, d_in, d_out, d_info


if __name__ == "__main__":
    main()
