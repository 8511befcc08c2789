#!/usr/bin/env python3
"""bench_bundle.py -- what adjusting a frame set over all pairs costs: hg_bundle_adjust_frames_device on planted frames (a strip whose
neighbours and next-but-one neighbours are paired, matches with 0.5 px of noise, every frame started about a pixel off).

    cases     64 projective frames x 126 pairs x 2048 matches;  16 frames x 30 pairs x 2048 (the one-workgroup solve);  256 frames x ~1000
              pairs x 256 matches
    call      10 rounds (eps 0: every round runs), lambda0 1e-3, huber off; and the same call with n_iter = 0, which is one pass

A region is one whole call between two synchronisations of the context; per case the median and the minimum over `--regions` regions after
`--warmup` untimed ones.  The per-stage split comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python
tools/bench_bundle.py --regions 3), which names k_bundle_pass, _assemble, _chol_* and _back_large.  Beside them, for the 64-frame case, ONE
round of the numpy model (tests/hgtest/bundle.py) on the CPU.  One JSON line per case.
    python tools/bench_bundle.py [--regions N] [--warmup W] [--cases 64x2x2048,16x2x2048,256x4x256] [--no-model]
"""
import argparse
import importlib.util
import json
import os
import statistics
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hgtest import bundle as BM              # noqa: E402  (the case builder and the CPU yardstick)

ROUNDS = 10


def build(F, reach, n):
    """F projective frames in a strip of 16 columns; frame f is paired with f + 1 .. f + reach."""
    rng = np.random.default_rng(F * 1000 + n)
    truth = BM.true_mats(BM.PROJECTIVE, F, 96, 64, rng, cols=16)
    pairs = [(f, f + d) for f in range(F) for d in range(1, reach + 1) if f + d < F]
    M = BM.make_matches(BM.PROJECTIVE, truth, pairs, n, 96, 64, rng, 0.5)
    return BM.case(BM.PROJECTIVE, 96, 64, BM.perturb(BM.PROJECTIVE, truth, 96, 64, rng, 1.0), (0,), pairs, M, n_iter=ROUNDS, eps=0.0)


def timed(ctx, c, bufs, n_iter, regions, warmup):
    ts = []
    for r in range(warmup + regions):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.bundle_adjust_frames_device(c.kind, c.W, c.H, c.F, c.fixed, c.pairs, bufs["m"], c.n_points, None, bufs["in"], bufs["out"], bufs["info"],
                                        bufs["scratch"], bufs["bytes"], n_iter=n_iter, eps=c.eps, lambda0=c.lambda0, huber=c.huber)
        ctx.sync()
        if r >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="64x2x2048,16x2x2048,256x4x256")
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    with HG.Context(0) as ctx:
        for spec in a.cases.split(","):
            F, reach, n = [int(v) for v in spec.split("x")]
            c = build(F, reach, n)
            NP = len(c.pairs)
            scratch = HG.bundle_layout(c.kind, F, NP, n)
            bufs = {"m": ctx.alloc(c.matches.nbytes), "in": ctx.alloc(F * 64), "out": ctx.alloc(F * 64), "info": ctx.alloc(HG.bundle_info_bytes(F, NP)),
                    "scratch": ctx.alloc(scratch), "bytes": scratch}
            try:
                ctx.to_device(bufs["m"], c.matches)
                ctx.to_device(bufs["in"], c.mats)
                full = timed(ctx, c, bufs, ROUNDS, a.regions, a.warmup)
                one = timed(ctx, c, bufs, 0, a.regions, a.warmup)
                info = HG.bundle_split_info(ctx.to_host(bufs["info"], HG.bundle_info_bytes(F, NP)), F, NP)[0]
                timed(ctx, c, bufs, ROUNDS, 1, 0)
                info = HG.bundle_split_info(ctx.to_host(bufs["info"], HG.bundle_info_bytes(F, NP)), F, NP)[0]
            finally:
                for k in ("m", "in", "out", "info", "scratch"):
                    ctx.free(bufs[k])
            rec = {"frames": F, "pairs": NP, "matches": n, "unknowns": 8 * (F - 1), "rounds": int(info["rounds"]), "accepted": int(info["accepted"]),
                   "rms_first": float(info["rms_first"]), "rms_last": float(info["rms_last"]), "call_ms_median": round(full[0], 4), "call_ms_min": round(full[1], 4),
                   "pass_only_ms_median": round(one[0], 4), "per_round_ms": round((full[0] - one[0]) / max(int(info["rounds"]), 1), 4), "scratch_mb": round(scratch / 2 ** 20, 1)}
            if not a.no_model and F == 64:
                d = BM.case(c.kind, c.W, c.H, c.mats, (0,), c.pairs, c.matches, n_iter=1, eps=0.0)
                t0 = time.perf_counter()
                BM.adjust(d)
                rec["numpy_one_round_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
