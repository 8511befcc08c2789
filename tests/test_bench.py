"""bench.py's plain run and --dump-outputs: the plain command measures the headline alone, and the sample it writes of the last
timed step is the same from run to run (fixed inputs, fixed seeded pixel choice) and small enough to keep beside a result line."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("hg_bench", os.path.join(ROOT, "bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    return B


def test_output_sample_is_fixed_and_exact():
    """output_sample on a CPU tensor laid out like the library's packed frames: the sampled RGBA are the bytes at the sampled pixels,
    the sums cover every pixel, the pixel choice does not depend on the data, and 64 4K frames stay far below 64 MB."""
    B = _bench_module()
    geoms = [(3, -2, 17, 9), (0, 0, 5, 1), (1, 1, 40, 30)]
    n_out = [g[2] * g[3] for g in geoms]
    offs, pos = [], 0
    for n in n_out:
        offs.append(pos)
        pos += n * 4 + 12                                    # gaps between frames, as padded packing leaves them
    rng = np.random.default_rng(7)
    buf = rng.integers(0, 256, pos, dtype=np.uint8)
    a = B.output_sample(torch, torch.from_numpy(buf), offs, n_out, geoms, torch.device("cpu"))
    b = B.output_sample(torch, torch.from_numpy(buf ^ 0x5A), offs, n_out, geoms, torch.device("cpu"))
    assert a["frames_rgba_sample"].dtype == np.float32 and a["frames_pixel_index"].dtype == np.float64
    assert a["frames_window"].dtype == np.float64 and a["frames_channel_sum"].dtype == np.float64
    assert np.array_equal(a["frames_pixel_index"], b["frames_pixel_index"]) and not np.array_equal(a["frames_rgba_sample"], b["frames_rgba_sample"])
    S = a["frames_pixel_index"].shape[1]
    assert a["frames_rgba_sample"].shape == (3, S, 4) and a["frames_window"].tolist() == [list(g) for g in geoms]
    for f, n in enumerate(n_out):
        frame = buf[offs[f]: offs[f] + n * 4].reshape(-1, 4)
        idx = a["frames_pixel_index"][f].astype(np.int64)
        assert idx.min() >= 0 and idx.max() < n
        assert np.array_equal(a["frames_rgba_sample"][f], frame[idx].astype(np.float32))
        assert np.array_equal(a["frames_channel_sum"][f], frame.sum(0, dtype=np.int64).astype(np.float64))
    F = 64
    S64 = max(1, min(16384, B.DUMP_BYTES // (F * 24)))
    assert F * S64 * (4 * 4 + 8) + F * 8 * 8 < 64 << 20


def _plain_bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "4",
           "--dump-outputs", out_dir, *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_same_outputs(tmp_path):
    """Two plain runs with the same arguments: headline fields only, `steps` as asked, and byte-identical dumps; a --full run of the
    same workload verifies its timed bytes and dumps the same sample (the headline region is the same)."""
    line = _plain_bench(str(tmp_path / "a"))
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert line["verified"] is None and line["checks"] == [] and line["cpu_baseline"] is None and "also" not in line
    assert line["roofline"] is None and line["roofline_fresh"] is None and line["roofline_distinct"] is None
    _plain_bench(str(tmp_path / "b"))
    full = _plain_bench(str(tmp_path / "c"), "--full", "--no-cpu-baseline")
    assert full["verified"] is True and full["roofline"] is not None and full["roofline_distinct"] is not None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["frames_channel_sum.npy", "frames_pixel_index.npy", "frames_rgba_sample.npy", "frames_window.npy"]
    total = 0
    for n in names:
        a = np.load(tmp_path / "a" / n)
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == 4
        assert np.array_equal(a, np.load(tmp_path / "b" / n)) and np.array_equal(a, np.load(tmp_path / "c" / n)), n
    assert total < 64 << 20
    assert np.load(tmp_path / "a" / "frames_channel_sum.npy")[:, 3].min() > 0          # the frames hold warped pixels
