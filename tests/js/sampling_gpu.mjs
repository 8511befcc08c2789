// GPU: the drop-in class with {sampling: 'bilinear'} on the real addon.  Prints one JSON line with, per case, the inputs the C ABI needs
// to reproduce it (points, triangles, window, inverse matrix) and the sha256 of the class's output; tests/test_gpu_sampling.py warps the
// same inputs through ctypes and compares.
import crypto from 'crypto';
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';

const sha = (t) => crypto.createHash('sha256').update(Buffer.from(t.buffer, t.byteOffset, t.byteLength)).digest('hex');
const f32 = (p) => Array.from(p instanceof Float32Array ? p : Float32Array.from(p.flat ? p.flat() : p));
function lcgImage(w, h, seed) {
    const data = new Uint8ClampedArray(w * h * 4);
    let s = seed >>> 0;
    for (let i = 0; i < data.length; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; data[i] = s >>> 24; }
    return { data, width: w, height: h };
}
const W = 320, H = 200, nx = 8, ny = 5, seed = 41;
const img = lcgImage(W, H, seed);
Homography.triangulate = () => gridTriangles(nx, ny);
const grid = [];
for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
const sets = [0, 1, 2].map((f) => grid.map(([x, y]) => [x / (1.05 + 0.1 * f), 3 + y / 1.07 + Math.sin(((8 + f) * x) / Math.PI) * 4]));
const out = { W, H, seed, cases: [] };

const h = new Homography('piecewiseaffine', W, H, { sampling: 'bilinear' });
h.setSourcePoints(grid, img, W, H, false);
for (const d of sets) {                                          // warp() (1.05x shrink: forward in nearest mode)
    h.setDestinyPoints(d, false);
    const r = h.warp();
    out.cases.push({ kind: 'piecewise', src: f32(h._srcPoints), dst: f32(h._dstPoints), tris: Array.from(h._triangles), min: [h._minSrcX, h._minSrcY],
                     win: h._window(), sha: sha(r.data), w: r.width, h: r.height });
}
const batch = h.warpBatch(sets);
out.batch = batch.map((r) => ({ sha: sha(r.data), w: r.width, h: r.height }));

for (const [transform, dst] of [['affine', [[5, 3], [W + 5, 3], [0, H]]], ['affine', [[0.5, 10], [W * 0.9, 2.25], [3, H * 1.1]]],
                                ['projective', [[W / 10, 0], [W, H / 4], [W / 10, H], [W, H * 0.8]]]]) {
    const g = new Homography(transform, W, H, { sampling: 'bilinear' });
    const src = transform === 'affine' ? [[0, 0], [W, 0], [0, H]] : [[0, 0], [W, 0], [0, H], [W, H]];
    g.setSourcePoints(src, img, W, H, false);
    g.setDestinyPoints(dst, false);
    const r = g.warp();
    out.cases.push({ kind: transform, inv: Array.from(g._solve(g._dstPoints, g._srcPoints)), win: g._window(), sha: sha(r.data), w: r.width, h: r.height });
    const b = g.warpBatch([dst]);
    out.cases[out.cases.length - 1].batchSha = sha(b[0].data);
    g.close();
}
h.close();
console.log(JSON.stringify(out));
