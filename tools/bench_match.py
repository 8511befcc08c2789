#!/usr/bin/env python3
"""bench_match.py -- what matching feature descriptors costs: hg_match_descriptors_frames_device (k_match_bits resp. k_match_u8, then
k_match_finish) on random descriptors of which every train row is a noisy copy of a query row.

    cases     64 frames x 2048 queries x 2048 train rows;  1 x 4096 x 4096
    kinds     bits: 32-byte binary rows (ORB), Hamming;  u8: 128-byte vectors (SIFT), squared L2 on the i8 matrix cores
    variants  plain (ratio 0.8, no cap); the same with the cross-check (the best query of a train row by atomicMin on (d << 32) | i); and
              the cross-check's other form, option "match_cross" 0: a second launch of the search with the sides swapped

The variants of a case run in turn inside every round (alternating, so that drift hits all alike); a region is one whole call between two
events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed
ones, the descriptor pairs per second the median stands for (frames x queries x train rows / time; the cross-check's extra work is
NOT counted as pairs) and the share of the machine's bound:
    u8    2 * 128 integer operations per pair against the i8 matrix-core peak, 2 x the BF16 rate = 5.0e15 / s
    bits  8 words x (XOR + popcount + add) = 24 lane operations per pair against 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 3.93e13 / s
          (v_bcnt_u32_b32 adds while it counts, so 16 is what the kernel can reach; both shares are printed)
Beside them, on the same box: a plain torch formulation on `--torch-frames` frames (u8: float32 matmul of the shifted bytes, norms,
topk(2); bits: byte XOR, a 256-entry popcount table, sum, topk(2)), scaled to the case's frames; and the numpy model
(tests/hgtest/match.py) on ONE frame, the CPU yardstick, whose frame is compared with the device's (counts and pairs: exact).  One JSON
line per case and kind.
    python tools/bench_match.py [--regions N] [--warmup W] [--cases 64x2048x2048,1x4096x4096] [--kinds bits,u8] [--no-model]
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
from hgtest import match as MM               # noqa: E402  (the model: the yardstick and the check)

I8_PEAK = 5.0e15                              # integer operations / s: twice the ~2.5e15 dense BF16 rate
VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9          # 32-bit lane operations / s


def descriptors(kind, F, nq, nt, nb, seed):
    """Query rows uniform; train row j of frame f a noisy copy of query row perm[j] (bits: each bit flipped with p = 0.1; bytes: +-20)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (F, nq, nb), dtype=np.uint8)
    src = np.stack([q[f][rng.integers(0, nq, nt)] for f in range(F)])
    if kind == MM.BITS:
        t = src ^ np.packbits(rng.random((F, nt, nb * 8)) < 0.1, axis=2)
    else:
        t = np.clip(src.astype(np.int16) + rng.integers(-20, 21, src.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    return q, t


def torch_two_nearest(kind, q, t, table):
    """(d, j) of the two nearest train rows of every query of ONE frame, the plain way."""
    if kind == MM.U8:
        a, b = q.to(torch.float32) - 128.0, t.to(torch.float32) - 128.0
        d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    else:
        d = table[(q[:, None, :] ^ t[None, :, :]).long()].sum(2)
    return torch.topk(d, 2, dim=1, largest=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="64x2048x2048,1x4096x4096")
    ap.add_argument("--kinds", default="bits,u8")
    ap.add_argument("--torch-frames", type=int, default=2)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_match.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    table = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int16, device=dev)
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        for case in args.cases.split(","):
            F, nq, nt = (int(v) for v in case.split("x"))
            for name in args.kinds.split(","):
                kind, nb = (MM.BITS, 32) if name == "bits" else (MM.U8, 128)
                q, t = descriptors(kind, F, nq, nt, nb, 7)
                d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
                d_cnt = torch.empty(F, dtype=torch.int32, device=dev)
                d_pairs = torch.empty(F * nq * 2, dtype=torch.int32, device=dev)

                def call(cross):
                    return lambda: ctx.match_descriptors_frames_device(kind, nb, nb, d_q.data_ptr(), nq, None, F, d_t.data_ptr(), nt, None, F, d_cnt.data_ptr(),
                                                                       ratio=0.8, cross_check=cross, d_pairs=d_pairs.data_ptr())

                extra = {}
                call(True)()
                ctx.sync()
                got = (int(d_cnt[0].item()), d_pairs[:nq * 2].cpu().numpy().reshape(nq, 2))
                extra["accepted_frame0_cross"] = got[0]
                if not args.no_model:
                    t0 = time.perf_counter()
                    w = MM.match(kind, nb, q[:1], t[:1], ratio=0.8, cross_check=True)
                    extra["numpy_one_frame_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    if got[0] != int(w.counts[0]) or not np.array_equal(got[1], w.pairs[0]):
                        sys.exit(f"{case} {name}: the device's frame 0 differs from the model")
                def swapped():
                    ctx.set_option("match_cross", 0)
                    call(True)()
                    ctx.set_option("match_cross", -1)

                variants = [("plain", call(False)), ("cross_check", call(True)), ("cross_check_swapped_launch", swapped)]
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
                for label, tm in times.items():
                    med = statistics.median(tm)
                    pairs = F * nq * nt / (med * 1e-3)
                    res[label] = {"median_ms": round(med, 4), "min_ms": round(min(tm), 4), "pairs_per_s": float(f"{pairs:.4g}")}
                    if kind == MM.U8:
                        res[label]["share_of_i8_peak"] = round(pairs * 2 * nb / I8_PEAK, 4)
                    else:
                        res[label]["share_of_valu_bound_24_ops"] = round(pairs * 24 / VALU_LANE_OPS, 4)
                        res[label]["share_of_valu_bound_16_ops"] = round(pairs * 16 / VALU_LANE_OPS, 4)
                # the plain torch formulation, frame by frame (its temporaries for all frames at once would not fit)
                nf = min(F, max(args.torch_frames, 1))
                tt = []
                for r in range(2 + 5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for f in range(nf):
                        torch_two_nearest(kind, d_q[f], d_t[f], table)
                    e1.record(stream)
                    e1.synchronize()
                    if r >= 2:
                        tt.append(e0.elapsed_time(e1) / nf)
                extra["torch_ms_per_frame"] = round(statistics.median(tt), 4)
                extra["torch_ms_scaled_to_case"] = round(statistics.median(tt) * F, 3)
                print(json.dumps({"case": case, "kind": name, "desc_bytes": nb, "frames": F, "queries": nq, "train": nt, **res, **extra,
                                  "regions": args.regions, "warmup": args.warmup}), flush=True)
                ctx.sync()
                del d_q, d_t, d_cnt, d_pairs


if __name__ == "__main__":
    main()
