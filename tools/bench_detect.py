#!/usr/bin/env python3
"""bench_detect.py -- what detecting and describing keypoints costs: hg_detect_describe_frames_device (k_detect_cells, k_detect_compact,
k_detect_describe) on planes cut from one seeded scene of blurred rectangles (`--content scene`) or on uniform noise (`--content noise`: a
candidate in nearly every neighbourhood, the worst case of the per-cell selection).

    cases     64 planes of 1920 x 1080 x 4;  8 planes of 3840 x 2160 x 4;  1 plane of 3840 x 2160 x 4;  the same with 1 channel
    settings  cell 16, 32, 64 x per_cell 1, 2, 4 (a setting whose n_slots exceeds 65536 is refused by the call and reported as such)

A region is one whole call between two events on the context's stream.  Two variants alternate inside every round (so that drift hits both
alike): `full` (counts, points, descriptors, info: all three kernels) and `no_describe` (counts and points only: k_detect_cells and
k_detect_compact); their difference is k_detect_describe's share.  The split between the first two kernels needs a kernel trace (rocprofv3
--kernel-trace --stats over `--regions 25 --no-torch --no-model`).  Per variant the median and the minimum over `--regions` regions (at least
25) after `--warmup` untimed ones, and beside the median:
    floor_ms   the time of reading the planes once at 8 TB/s, the figure the other features quote against
    torch      the same response in a plain torch formulation on `--torch-planes` planes (float32: conv2d for Sobel, avg_pool2d for the 7 x 7
               sums, max_pool2d for the 3 x 3 test; no selection, no descriptors), scaled to the case's planes
    numpy      the model of tests/hgtest/detect.py on ONE plane, the CPU yardstick, whose plane is compared with the device's (exact)
One JSON line per case and setting.
    python tools/bench_detect.py [--regions N] [--warmup W] [--cases 64x1920x1080x4,...] [--cells 16,32,64] [--per-cell 1,2,4] [--content scene|noise]
                                 [--no-torch] [--no-model]
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
from hgtest import detect as DM              # noqa: E402  (the model: the yardstick and the check)

HBM_BYTES_PER_S = 8.0e12


def planes_on_device(content, P, W, H, channels, dev):
    """P planes of W x H x channels u8 on the device: plane p is the base picture rolled by (37 p, 11 p), so the planes differ; with 4 channels
    R = the picture, G = its inverse, B = a darker copy, A = 255."""
    if content == "noise":
        base = DM.noise(5, W, H)
    else:
        tile = DM.scene(5, 960, 540, rects=9000, side=28)
        base = np.tile(tile, ((H + 539) // 540, (W + 959) // 960))[:H, :W]
    b = torch.from_numpy(np.ascontiguousarray(base)).to(dev)
    grey = torch.stack([torch.roll(b, shifts=(11 * p, 37 * p), dims=(0, 1)) for p in range(P)])
    if channels == 1:
        return grey.contiguous()
    return torch.stack([grey, 255 - grey, (grey.to(torch.int32) * 3 // 4 + 17).to(torch.uint8), torch.full_like(grey, 255)], dim=-1).contiguous()


def torch_response(planes, channels):
    """The candidates of the planes the plain way, float32: (P, H - 8, W - 8) bool."""
    p = planes.to(torch.float32)
    L = p if channels == 1 else torch.floor((77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) / 256)
    L = L[:, None]
    kx = torch.tensor([[-1.0, 0, 1], [-2, 0, 2], [-1, 0, 1]], device=planes.device)[None, None]
    ix, iy = torch.nn.functional.conv2d(L, kx), torch.nn.functional.conv2d(L, kx.transpose(2, 3))
    box = lambda v: torch.nn.functional.avg_pool2d(v, 7, stride=1) * 49.0
    A, C, B = box(ix * ix), box(iy * iy), box(ix * iy)
    R = 16.0 * (A * C - B * B) - (A + C) * (A + C)
    return (R >= 1e10) & (R == torch.nn.functional.max_pool2d(R, 3, stride=1, padding=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="64x1920x1080x4,8x3840x2160x4,1x3840x2160x4,64x1920x1080x1,8x3840x2160x1,1x3840x2160x1")
    ap.add_argument("--cells", default="16,32,64")
    ap.add_argument("--per-cell", default="1,2,4")
    ap.add_argument("--content", default="scene", choices=("scene", "noise"))
    ap.add_argument("--min-response", type=int, default=10 ** 10)
    ap.add_argument("--torch-planes", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_detect.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        for case in args.cases.split(","):
            P, W, H, ch = (int(v) for v in case.split("x"))
            d_planes = planes_on_device(args.content, P, W, H, ch, dev)
            stream.synchronize()
            extra = {"floor_ms": round(P * W * H * ch / HBM_BYTES_PER_S * 1e3, 4)}
            if not args.no_torch:
                nf = min(P, max(args.torch_planes, 1))
                tt = []
                for r in range(2 + 5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    torch_response(d_planes[:nf], ch)
                    e1.record(stream)
                    e1.synchronize()
                    if r >= 2:
                        tt.append(e0.elapsed_time(e1) / nf)
                extra["torch_ms_per_plane"] = round(statistics.median(tt), 4)
                extra["torch_ms_scaled_to_case"] = round(statistics.median(tt) * P, 3)
            model_plane = None if args.no_model else d_planes[0].cpu().numpy()
            for cell in (int(v) for v in args.cells.split(",")):
                for per_cell in (int(v) for v in args.per_cell.split(",")):
                    head = {"case": case, "content": args.content, "planes": P, "W": W, "H": H, "channels": ch, "cell": cell, "per_cell": per_cell}
                    try:
                        n_slots = HG.detect_layout(W, H, cell, per_cell)[2]
                    except HG.HgError:
                        print(json.dumps({**head, "refused": "n_slots > 65536"}), flush=True)
                        continue
                    d_cnt = torch.empty(P, dtype=torch.int32, device=dev)
                    d_pts = torch.empty(P * n_slots * 2, dtype=torch.float32, device=dev)
                    d_desc = torch.empty(P * n_slots * 32, dtype=torch.uint8, device=dev)
                    d_info = torch.empty(P * n_slots * 2, dtype=torch.int64, device=dev)
                    kw = dict(cell=cell, per_cell=per_cell, min_response=args.min_response)
                    full = lambda: ctx.detect_describe_frames_device(d_planes.data_ptr(), W, H, P, ch, d_cnt.data_ptr(), d_points=d_pts.data_ptr(),
                                                                     d_desc=d_desc.data_ptr(), d_info=d_info.data_ptr(), **kw)
                    lean = lambda: ctx.detect_describe_frames_device(d_planes.data_ptr(), W, H, P, ch, d_cnt.data_ptr(), d_points=d_pts.data_ptr(), **kw)
                    full()
                    ctx.sync()
                    counts = d_cnt.cpu().numpy()
                    res = {"n_slots": n_slots, "keypoints_per_plane": round(float(counts.mean()), 1)}
                    if model_plane is not None and (cell, per_cell) == (32, 2):
                        t0 = time.perf_counter()
                        w = DM.model(model_plane[None], ch, cell, per_cell, args.min_response)
                        res["numpy_one_plane_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                        if int(counts[0]) != int(w.counts[0]) or not np.array_equal(d_desc[:n_slots * 32].cpu().numpy().reshape(n_slots, 32), w.desc[0]):
                            sys.exit(f"{case} cell {cell} per_cell {per_cell}: the device's plane 0 differs from the model")
                    variants = [("full", full), ("no_describe", lean)]
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
                    for label, tm in times.items():
                        res[label] = {"median_ms": round(statistics.median(tm), 4), "min_ms": round(min(tm), 4)}
                    res["describe_share"] = round(1.0 - res["no_describe"]["median_ms"] / res["full"]["median_ms"], 3)
                    res["times_the_floor"] = round(res["full"]["median_ms"] / extra["floor_ms"], 1)
                    print(json.dumps({**head, **res, **extra, "regions": args.regions, "warmup": args.warmup}), flush=True)
                    ctx.sync()
                    del d_cnt, d_pts, d_desc, d_info
            del d_planes


if __name__ == "__main__":
    main()
