// GPU: h.mosaic(dstPointSets, { blend: 'multiband', ... }) of the drop-in class on the real addon, for an affine, a projective (bilinear
// sampling) and a piecewise set of overlapping frames of a 64 x 40 source.  Prints one JSON line: per case the windows, the point sets the
// batch entry gets (base64), the canvas, and per run its bands, feather and exposure with the SHA-256 of the canvas, the weight plane and the
// labels (and the fitted gains, base64) -- tests/test_gpu_multiband.py runs the same loop through ctypes (stage the set, warp, export the
// coords fields, fit the gains, blend) and compares.  Checked here: classes and shapes, the defaults, that one band is a paste of the
// frames and that the bands differ.  Exit code 1 on a failure.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';
import { createHash } from 'crypto';

const W = 64, H = 40, nx = 4, ny = 4;
const data = new Uint8ClampedArray(W * H * 4);
for (let i = 0; i < data.length; i++) data[i] = (i * 7 + (i >> 3) * 13) & 255;
const img = { data, width: W, height: H };
const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const bytesOf = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength);
const b64 = (t) => bytesOf(t).toString('base64');
const sha = (t) => createHash('sha256').update(bytesOf(t)).digest('hex');
const copy = (sets) => sets.map((s) => s.map((p) => p.slice()));
const cases = {};
// key: [bands, feather (null: Infinity), fitted gains?]
const runs = { five: [5, null, false], one: [1, null, false], capped: [3, 3, false], gain: [5, null, true] };
const optsOf = { five: {}, one: { bands: 1 }, capped: { bands: 3, feather: 3 }, gain: { exposure: 'gain' } };

function through(h, name, sets, geometric) {
    const hashes = {};
    let canvas = null;
    const F = sets.length;
    for (const key of Object.keys(runs)) {
        const r = h.mosaic(copy(sets), Object.assign({ blend: 'multiband', weight: true, labels: true, pointsAreNormalized: false }, optsOf[key]));
        const n = r.width * r.height;
        check(r.data instanceof Uint8ClampedArray && r.weight instanceof Float32Array && r.labels instanceof Int32Array && r.data.length === n * 4 && r.weight.length === n && r.labels.length === n, `${name} ${key}: shapes`);
        check(canvas === null || JSON.stringify(canvas) === JSON.stringify([r.x, r.y, r.width, r.height]), `${name} ${key}: the canvas moved`);
        canvas = [r.x, r.y, r.width, r.height];
        check(r.labels.every((l, i) => l >= -1 && l < F && r.weight[i] === (l < 0 ? 0 : 1)) && new Set(r.labels).size === F + 1, `${name} ${key}: every frame owns pixels, some pixels are nobody's, the weight is 1 where owned`);
        check(r.data.every((v, i) => r.labels[i >> 2] >= 0 || v === 0) && r.data.some((v) => v !== 0), `${name} ${key}: zeros where nobody owns the pixel`);
        hashes[key] = { data: sha(r.data), weight: sha(r.weight), labels: sha(r.labels) };
        if (runs[key][2]) { check(r.gains instanceof Float32Array && r.gains.length === F && r.gains.every((g) => g > 0.5 && g < 2), `${name} ${key}: gains`); hashes[key].gains = b64(r.gains); }
        else check(r.gains === undefined, `${name} ${key}: no gains`);
    }
    check(hashes.five.labels === hashes.one.labels && hashes.five.labels === hashes.gain.labels && hashes.five.weight === hashes.one.weight, `${name}: labels and weights do not depend on the bands or the gains`);
    check(new Set(Object.values(hashes).map((x) => x.data)).size === 4, `${name}: the four runs must differ on overlapping frames`);
    const d = h.mosaic(copy(sets), { blend: 'multiband', pointsAreNormalized: false });
    check(d.weight === undefined && d.labels === undefined && sha(d.data) === hashes.five.data, `${name}: the defaults are 5 bands, uncapped, no weight plane, no labels`);
    // one band is a paste: every owned pixel is its owner's warped pixel
    const one = h.mosaic(copy(sets), { blend: 'multiband', bands: 1, labels: true, pointsAreNormalized: false });
    const frames = h.warpBatch(copy(sets), { inverse: true, pointsAreNormalized: false });
    const geoms = [], from = [], to = [];
    for (const s of copy(sets)) {
        h.setDestinyPoints(s, false);
        geoms.push(h._window());
        if (geometric) { h._alignRanges(); from.push(...Array.from(h._dstPoints).slice(0, geometric)); to.push(...Array.from(h._srcPoints).slice(0, geometric)); } else from.push(...Array.from(h._dstPoints));
    }
    let paste = true;
    for (let j = 0; j < one.height && paste; j++) for (let i = 0; i < one.width && paste; i++) {
        const l = one.labels[j * one.width + i];
        if (l < 0) continue;
        const [gx, gy, gw] = geoms[l], u = one.x + i - gx, v = one.y + j - gy;
        for (let c = 0; c < 4; c++) paste = paste && one.data[(j * one.width + i) * 4 + c] === frames[l].data[(v * gw + u) * 4 + c];
    }
    check(paste, `${name}: one band is a paste of the owners' pixels`);
    cases[name] = { geoms, canvas, runs, hashes, sampling: h.sampling === 'bilinear' ? 1 : 0 };
    if (geometric) { cases[name].from = b64(Float32Array.from(from)); cases[name].to = b64(Float32Array.from(to)); } else {
        cases[name].dst = b64(Float32Array.from(from)); cases[name].src = b64(Float32Array.from(h._srcPoints));
        cases[name].tris = b64(Uint32Array.from(h._triangles)); cases[name].minSrc = [h._minSrcX, h._minSrcY];
    }
}

{
    const g = new Homography('affine', W, H);
    g.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    through(g, 'affine', [0, 1, 2, 3].map((k) => [[1.5 + 17 * k, 2 + k], [W * 0.6 + 1.5 + 17 * k, 3 + k], [0.5 + 17 * k, H * 0.5 + 2 + k]]), 6);
    g.close();
}
{
    const p = new Homography('projective', W, H);
    p.sampling = 'bilinear';
    p.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    through(p, 'projective', [0, 1, 2].map((k) => [[8 + 21 * k, k], [W * 0.5 + 21 * k, 0], [21 * k, H * 0.6], [W * 0.7 + 21 * k, H * 0.6 + 2 * k]]), 8);
    p.close();
}
{
    Homography.triangulate = () => gridTriangles(nx, ny);
    const grid = [];
    for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
    const h = new Homography('piecewiseaffine', W, H);
    h.setSourcePoints(grid, img, W, H, false);
    through(h, 'piecewise', [0, 1, 2, 3].map((k) => grid.map(([x, y]) => [x * 0.6 + 2 * Math.sin(y / 17 + k) + 19 * k, y * 0.55 + 1.0 * Math.cos(x / 23) + 2 + k])), 0);
    h.close();
}
console.log(JSON.stringify({ ok: fails.length === 0, fails, W, H, cases }));
process.exit(fails.length === 0 ? 0 : 1);
