#!/usr/bin/env python3
"""bench_aniso.py -- what anisotropic filtering costs: hg_remap_aniso_frames_device beside hg_remap_trilinear_frames_device (the parent's
kernel, unchanged: the yardstick), same box, one process, same fields, planes and pyramids, back to back.

The set: 64 frames out of 3840x2160 source planes (`--planes` of them, frame f reads plane f % planes), through three frame sets
    shrink4      an isotropic affine 4x shrink, 960x540 per frame: N = 1 nearly everywhere
    projective   bench_trilinear.py's projective pattern onto half the size: about 1730x1080 per frame
    shrink8x1    an affine shrink of 8x vertically and 1x horizontally, 3840x270 per frame: N = 8 where max_aniso allows it
and two kinds of plane: u8 x 4 channels (a picture) and f32 x 1 channel.
    trilinear    one hg_remap_trilinear_frames_device over the built pyramids
    aniso1/4/8/16    one hg_remap_aniso_frames_device with that max_aniso; vs_trilinear = its median over trilinear's
The variants run in turn inside every round (alternating, so that drift hits all alike); a region is one variant's whole work between two
events on the context's stream; per variant the median and the minimum over `--regions` regions (at least 25) after `--warmup` untimed
ones.  Before anything is timed the anisotropic remap with max_aniso = 1 is compared with the trilinear remap byte for byte.  n_hist is
the histogram of the probe count N (index = N, max_aniso = 16) over the finite pixels of the set, from the field itself by the header's
steps 2-4 in f32 torch operations.  One JSON line per case.
    python tools/bench_aniso.py [--regions N] [--warmup W] [--frames F] [--planes P] [--cases shrink4:u8x4,...]
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
WL = _load("hg_workloads", os.path.join(PKG, "workloads.py"))


def _bytes(n, dev):
    return torch.empty(int(n), dtype=torch.uint8, device=dev)


def _step(co, fin, axis):
    """Steps 2 of the header for one frame (h, w, 2) on the device: (dx, dy, q) to the next neighbour along axis if it exists and is finite,
    else to the previous one, else zeros."""
    nxt, prv = torch.roll(co, -1, axis), torch.roll(co, 1, axis)
    n = co.shape[axis]
    idx = torch.arange(n, device=co.device).reshape((-1, 1) if axis == 0 else (1, -1))
    a_ok = (idx + 1 < n) & torch.roll(fin, -1, axis)
    b_ok = (idx >= 1) & torch.roll(fin, 1, axis)
    nb = torch.where(a_ok[..., None], nxt, prv)
    dx, dy = nb[..., 0] - co[..., 0], nb[..., 1] - co[..., 1]
    q = dx * dx + dy * dy
    return torch.where(a_ok | b_ok, q, torch.zeros_like(q))


def n_histogram(d_co, geoms, offs, max_aniso=16):
    """The probe count N of every finite pixel of the set (steps 2-4 of hg_remap_aniso_frames_device's rule), as a histogram over 0..max_aniso."""
    hist = torch.zeros(max_aniso + 1, dtype=torch.int64, device=d_co.device)
    for g, o in zip(geoms, offs):
        w, h = max(g[2], 0), max(g[3], 0)
        if w * h == 0:
            continue
        co = d_co[o:o + w * h * 8].view(torch.float32).reshape(h, w, 2)
        fin = torch.isfinite(co).all(-1)
        qh, qv = _step(co, fin, 1), _step(co, fin, 0)
        qM, qm = torch.maximum(qh, qv), torch.minimum(qh, qv)
        qmc = torch.clamp(qm, min=1.0)
        N = torch.full(qM.shape, max_aniso, dtype=torch.int64, device=co.device)
        for n in range(max_aniso, 0, -1):
            N = torch.where(float(n * n) * qmc >= qM, n, N)
        N = torch.where((qM > 1.0) & torch.isfinite(qM), N, 1)
        hist += torch.bincount(N[fin], minlength=max_aniso + 1)
    return hist.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--cases", default="shrink4:u8x4,shrink4:f32x1,projective:u8x4,projective:f32x1,shrink8x1:u8x4,shrink8x1:f32x1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_aniso.py needs a GPU: a timing taken elsewhere says nothing")
    if args.regions < 25:
        sys.exit("--regions must be at least 25")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    W, H, F, NP = 3840, 2160, args.frames, args.planes
    levels = HG.pyramid_levels(W, H)
    with torch.cuda.stream(stream), HG.Context(0, stream=stream.cuda_stream) as ctx:
        size_only = _bytes(W * H * 4, dev)                       # the field calls read the source's size only
        ctx.set_image_device(size_only.data_ptr(), W, H)
        s4 = WL.corners(W, H)
        sets = {}
        g4 = [(0, 0, W // 4, H // 4)] * F
        sets["shrink4"] = (g4, lambda: ctx.geometric_set_frames(0, np.tile(np.array([4, 0, 0, 4, 1.5, 1.5, 0, 0], np.float64), F), g4))
        d4 = [WL.projective_dst(W, H, 0.01 * (f % 4)) * 0.5 for f in range(F)]
        gp = [tuple(int(v) for v in HG.transform_limits(1, HG.solve_projective(s4, d), W, H)) for d in d4]
        sets["projective"] = (gp, lambda: ctx.geometric_set_frames_points(1, np.concatenate(d4), np.tile(s4, F), gp, HG.pack_offsets(gp)[0]))
        g81 = [(0, 0, W, H // 8)] * F
        sets["shrink8x1"] = (g81, lambda: ctx.geometric_set_frames(0, np.tile(np.array([1, 0, 0, 8, 0.0, 3.5, 0, 0], np.float64), F), g81))
        fields, hists = {}, {}
        try:
            for case in args.cases.split(","):
                which, kind = case.split(":")
                geoms, stage = sets[which]
                n_px = sum(max(g[2], 0) * max(g[3], 0) for g in geoms)
                if which not in fields:
                    stage()
                    d_co = _bytes(HG.pack_field_offsets(geoms, HG.FIELD_COORDS)[1], dev)
                    ctx.field_inverse_geometric_frames_device(HG.FIELD_COORDS, d_co.data_ptr())
                    ctx.sync()
                    fields[which] = d_co
                    hists[which] = n_histogram(d_co, geoms, HG.pack_field_offsets(geoms, HG.FIELD_COORDS)[0])
                d_co = fields[which]
                elem = HG.ELEM_U8 if kind.startswith("u8") else HG.ELEM_F32
                ch = int(kind.split("x")[1])
                px = ch * (1 if elem == HG.ELEM_U8 else 4)
                stride = (W * H * px + 255) // 256 * 256
                _, ptotal = HG.pyramid_layout(W, H, elem, ch, levels)
                ototal = HG.pack_plane_offsets(geoms, px)[1]
                g = torch.Generator(device=dev)
                g.manual_seed(7)
                if elem == HG.ELEM_U8:
                    planes = torch.randint(0, 256, (NP * stride,), dtype=torch.uint8, device=dev, generator=g)
                else:
                    planes = torch.rand(NP * stride // 4, dtype=torch.float32, device=dev, generator=g)
                pyr = _bytes(NP * ptotal, dev)
                P, Y, C = planes.data_ptr(), pyr.data_ptr(), d_co.data_ptr()

                def trilinear(d_out):
                    ctx.remap_trilinear_frames_device(geoms, C, P, W, H, NP, stride, elem, ch, d_out, Y, ptotal, levels)

                def aniso(n):
                    return lambda d_out: ctx.remap_aniso_frames_device(geoms, C, P, W, H, NP, stride, elem, ch, d_out, Y, ptotal, levels, n)

                a = torch.full((ototal,), 0xA5, dtype=torch.uint8, device=dev)
                b = torch.full((ototal,), 0xA5, dtype=torch.uint8, device=dev)
                ctx.pyramid_build_device(P, W, H, NP, stride, elem, ch, levels, Y, ptotal)
                trilinear(a.data_ptr())
                aniso(1)(b.data_ptr())
                ctx.sync()
                if not torch.equal(a, b):
                    sys.exit(f"{case}: the anisotropic remap with max_aniso = 1 differs from the trilinear remap")
                aniso(16)(b.data_ptr())
                ctx.sync()
                differs = int((a != b).sum().item())
                d_out = a.data_ptr()
                del b
                variants = [("trilinear", trilinear)] + [(f"aniso{n}", aniso(n)) for n in (1, 4, 8, 16)]
                times = {label: [] for label, _ in variants}
                for r in range(args.warmup + args.regions):
                    for label, run in variants:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        run(d_out)
                        e1.record(stream)
                        e1.synchronize()
                        if r >= args.warmup:
                            times[label].append(e0.elapsed_time(e1))
                res = {}
                for label, t in times.items():
                    res[label] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4)}
                for n in (1, 4, 8, 16):
                    res[f"aniso{n}"]["vs_trilinear"] = round(res[f"aniso{n}"]["median_ms"] / res["trilinear"]["median_ms"], 3)
                print(json.dumps({"case": case, "n_frames": F, "n_planes": NP, "output_px": n_px, "pixel_bytes": px, "levels": levels,
                                  "bytes_changed_by_max_aniso_16": differs, "n_hist": hists[which], **res,
                                  "regions": args.regions, "warmup": args.warmup}), flush=True)
                del planes, pyr, a
        finally:
            ctx.sync()
            ctx.set_image(np.zeros((1, 1, 4), np.uint8))         # drop the alias before the buffer goes away


if __name__ == "__main__":
    main()
