"""Frame sets whose frames bring their own source points (hg_piecewise_set_frames_src): shared inputs of tests/test_moving_cpu.py and
tests/test_gpu_moving.py.  Test infrastructure only; expected bytes come from the CPU oracle, one call per frame with that frame's
source points and minima (nearest), or from its taps fed into the numpy model (bilinear) -- never from the library.

"Set A": W x H = 320 x 200, grid_points / grid_triangles(6, 4), F frames, images lcg_image(W, H, 40 + f); for vertex k
    src_f = (1.1 x + 9 f + s + 3 sin(0.7 k + f),  1.1 y + 6 f + s + 3 cos(1.1 k + 2 f))   stored as float32
    dst_f = sin_dst(base, 6 + f, 8 + f),   geom = piecewise_geom(dst_f),   min_src = src_min(src_f)
The source mesh is wider than the image: the upper bound W + minSrcX clips, and where it clips depends on the frame's minimum.
s = 4: every minimum >= 0;  s = -12: minima of both signs in one set."""
import functools
import hashlib

import numpy as np

from hgtest import bilinear as B
from hgtest import oracle as O
from hgtest import workloads as WL


class MovingSet:
    def __init__(self, W, H, nx, ny, F, s, seed0=40):
        self.W, self.H, self.F, self.s = W, H, F, s
        self.base = WL.grid_points(W, H, nx, ny)
        self.tris = WL.grid_triangles(nx, ny)
        p = self.base.reshape(-1, 2).astype(np.float64)
        k = np.arange(p.shape[0], dtype=np.float64)
        self.srcs, self.dsts = [], []
        for f in range(F):
            sx = 1.1 * p[:, 0] + 9 * f + s + 3 * np.sin(0.7 * k + f)
            sy = 1.1 * p[:, 1] + 6 * f + s + 3 * np.cos(1.1 * k + 2 * f)
            self.srcs.append(np.stack([sx, sy], 1).astype(np.float32).ravel())
            self.dsts.append(WL.sin_dst(self.base, 6 + f, 8 + f))
        self.geoms = [WL.piecewise_geom(d) for d in self.dsts]
        self.mins = [WL.src_min(sp) for sp in self.srcs]
        self.imgs = [WL.lcg_image(W, H, seed0 + f) for f in range(F)]
        self._want = {}

    @property
    def src_all(self):
        return np.concatenate(self.srcs)

    @property
    def dst_all(self):
        return np.concatenate(self.dsts)

    @property
    def min_all(self):
        return np.asarray(self.mins, np.int32).ravel()

    def frame(self, f, src=None, mins=None, img=None):
        """(nearest rgba, bilinear rgba, covered mask, map, fwd, inv) of frame f on the oracle; src / mins / img override the frame's own."""
        src = self.srcs[f] if src is None else src
        mins = self.mins[f] if mins is None else mins
        img = self.imgs[f] if img is None else img
        near, wmap, fwd, inv = O.warp_inverse_piecewise(src, self.dsts[f], self.tris, img, mins[0], mins[1], *self.geoms[f], taps=True)
        bil, cov = B.warp_piecewise(wmap, inv, img, mins[0], mins[1], *self.geoms[f])
        return near, bil, cov, wmap, fwd, inv

    def want(self, f, n_images=None):
        """Frame f with its own source side over image f % n_images (default: its own image); computed once, never modified."""
        key = (f, n_images)
        if key not in self._want:
            img = self.imgs[f if n_images is None else f % n_images]
            r = self.frame(f, img=img)
            for a in r:
                a.setflags(write=False)
            self._want[key] = r
        return self._want[key]


@functools.lru_cache(maxsize=None)
def set_a(s=4, F=4):
    return MovingSet(320, 200, 6, 4, F, s)


@functools.lru_cache(maxsize=None)
def wide_set(s=4):
    """Wide, short: k_pw_tile / k_pw_patch cross their 2048-column split, k_pw_rows several 256-pixel windows with a ragged tail."""
    return MovingSet(2100, 48, 12, 2, 3, s)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
