#!/usr/bin/env python3
"""bench_fit.py -- what fitting frame transforms to point matches costs: hg_fit_matches_frames_device (k_fit_hypotheses, k_fit_score,
k_fit_finish) on planted matches, 60 % following a fixed map and the rest uniform in a 1920 x 1080 picture.

    cases     64 frames x 2048 matches x 2048 hypotheses;  64 x 512 x 512;  1 x 4096 x 4096
    variants  affine and projective, each with and without the least-squares refit, device-drawn samples, threshold 3

The variants of a case run in turn inside every round (alternating, so that drift hits all alike); a region is one whole call between two
events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed
ones, and the reprojections per second the median stands for (frames x hypotheses x matches / time).  Beside them the time of the numpy
model (tests/hgtest/fit.py) on ONE frame of the case, the CPU yardstick, and its frame's result compared with the device's (best, count,
mask, minimal matrix: exact).  One JSON line per case.
    python tools/bench_fit.py [--regions N] [--warmup W] [--cases 64x2048x2048,64x512x512,1x4096x4096] [--no-model]
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
from hgtest import fit as FM                 # noqa: E402  (the model: the yardstick and the check)

MAPS = {0: np.array([0.9, 0.1, -0.2, 1.05, 12.0, -7.0, 0.0, 0.0]), 1: np.array([1.1, 0.05, 3.0, -0.04, 0.95, -2.0, 1e-5, -2e-5])}


def matches_of(kind, F, N, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, [1920.0, 1080.0], (F, N, 2))
    px, py = FM.project(kind, MAPS[kind].reshape(1, 8), xy[..., 0].ravel(), xy[..., 1].ravel())
    uv = np.stack([px[0], py[0]], 1).reshape(F, N, 2) + rng.normal(0, 0.5, (F, N, 2))
    out = rng.random((F, N)) >= 0.6
    uv[out] = rng.uniform(0, [1920.0, 1080.0], (int(out.sum()), 2))
    return np.concatenate([xy, uv], 2).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="64x2048x2048,64x512x512,1x4096x4096")
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fit.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    thr, seed = 3.0, 11
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        for case in args.cases.split(","):
            F, N, H = (int(v) for v in case.split("x"))
            host = {k: matches_of(k, F, N, 5 + k) for k in (0, 1)}
            d_m = {k: torch.from_numpy(host[k]).to(dev) for k in (0, 1)}
            d_mats, d_min = torch.empty(F * 8, dtype=torch.float64, device=dev), torch.empty(F * 8, dtype=torch.float64, device=dev)
            d_cnt, d_best = torch.empty(F, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev)
            d_mask = torch.empty(F * N, dtype=torch.uint8, device=dev)

            def call(kind, refit):
                return lambda: ctx.fit_matches_frames_device(kind, d_m[kind].data_ptr(), N, None, F, thr, H, seed, d_mats.data_ptr(), d_cnt.data_ptr(),
                                                             refit=refit, d_min_mats=d_min.data_ptr(), d_best=d_best.data_ptr(), d_mask=d_mask.data_ptr())

            model = {}
            for kind, name in ((0, "affine"), (1, "projective")):
                call(kind, True)()
                ctx.sync()
                got = (int(d_best[0].item()), int(d_cnt[0].item()), d_mask[:N].cpu().numpy(), d_min[:8].cpu().numpy())
                if not args.no_model:
                    t0 = time.perf_counter()
                    w = FM.fit(kind, host[kind][:1], None, thr, H, seed=seed, refit_on=True)
                    model[name + "_numpy_one_frame_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    same = (got[0] == int(w.best[0]) and got[1] == int(w.counts[0]) and np.array_equal(got[2], w.mask[0])
                            and np.array_equal(got[3].view(np.uint64), w.min_mats[0].view(np.uint64)))
                    if not same:
                        sys.exit(f"{case} {name}: the device's frame 0 differs from the model")
                model[name + "_inliers_frame0"] = got[1]
            variants = [(f"{name}{'_refit' if refit else ''}", call(kind, refit)) for kind, name in ((0, "affine"), (1, "projective")) for refit in (False, True)]
            times = {label: [] for label, _ in variants}
            for r in range(args.warmup + args.regions):
                for label, run in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    run()
                    e1.record(stream)
                    e1.synchronize()
                    if r >= args.warmup:
                        times[label].append(e0.elapsed_time(e1))
            res = {}
            for label, t in times.items():
                med = statistics.median(t)
                res[label] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "reprojections_per_s": float(f"{F * N * H / (med * 1e-3):.4g}")}
            print(json.dumps({"case": case, "frames": F, "matches": N, "hypotheses": H, **res, **model, "regions": args.regions, "warmup": args.warmup}), flush=True)
            ctx.sync()
            del d_m, d_mats, d_min, d_cnt, d_best, d_mask


if __name__ == "__main__":
    main()
