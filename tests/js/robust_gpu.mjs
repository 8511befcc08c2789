// GPU: h.mosaic(dstPointSets, { blend: 'median' | 'trimmed' | 'min' | 'max' }) of the drop-in class on the real addon, for a projective
// (bilinear sampling) and a piecewise stack of overlapping frames of a 64 x 40 source.  Prints one JSON line: per case the windows, the
// point sets the batch entry gets (base64), the canvas, and the SHA-256 of the canvas and of the weight plane for every blend --
// tests/test_gpu_robust.py runs the same loop through ctypes (stage the set, warp, export the coords fields, robust mosaic) and compares
// the hashes.  Checked here: classes and shapes, the default trim, min <= median <= max, gains composing.  Exit code 1 on a failure.
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
const runs = { median: [0, 0, null], trimmed: [1, 0.25, null], trimmed10: [1, 0.1, null], min: [2, 0, null], max: [3, 0, null], gained: [0, 0, [1.5, 0.75, 1.25, 0.5]] };     // [mode, trim, gains]
const optsOf = { median: { blend: 'median' }, trimmed: { blend: 'trimmed' }, trimmed10: { blend: 'trimmed', trim: 0.1 }, min: { blend: 'min' }, max: { blend: 'max' },
                 gained: { blend: 'median', exposure: runs.gained[2] } };

function through(h, name, sets, geometric) {
    const hashes = {}, out = {};
    let canvas = null;
    for (const key of Object.keys(runs)) {
        const r = h.mosaic(copy(sets), Object.assign({ weight: true, pointsAreNormalized: false }, optsOf[key]));
        check(r.data instanceof Uint8ClampedArray && r.weight instanceof Float32Array && r.data.length === r.width * r.height * 4 && r.weight.length === r.width * r.height, `${name} ${key}: shapes`);
        check(canvas === null || JSON.stringify(canvas) === JSON.stringify([r.x, r.y, r.width, r.height]), `${name} ${key}: the canvas moved`);
        canvas = [r.x, r.y, r.width, r.height];
        check(r.data.some((v) => v !== 0) && r.weight.some((v) => v >= 3) && r.weight.some((v) => v === 0) && r.weight.every((v) => Number.isInteger(v)), `${name} ${key}: the weight counts the frames; three and more, and none`);
        hashes[key] = { data: sha(r.data), weight: sha(r.weight) };
        out[key] = r;
    }
    check(new Set(Object.values(hashes).map((x) => x.data)).size === 6 && new Set(Object.values(hashes).map((x) => x.weight)).size === 1, `${name}: the blends must differ on overlapping frames, the counts must not`);
    check(out.median.data.every((v, k) => out.min.data[k] <= v && v <= out.max.data[k]), `${name}: min <= median <= max`);
    check(out.gained.gains instanceof Float32Array && JSON.stringify(Array.from(out.gained.gains)) === JSON.stringify(runs.gained[2]), `${name}: the gains come back`);
    const d = h.mosaic(copy(sets), { blend: 'trimmed', trim: 0.25, feather: -1, bands: 0, pointsAreNormalized: false });
    check(d.weight === undefined && sha(d.data) === hashes.trimmed.data, `${name}: the default trim is 0.25; feather and bands are ignored`);
    const geoms = [], from = [], to = [];
    for (const s of copy(sets)) {
        h.setDestinyPoints(s, false);
        geoms.push(h._window());
        if (geometric) { h._alignRanges(); from.push(...Array.from(h._dstPoints).slice(0, geometric)); to.push(...Array.from(h._srcPoints).slice(0, geometric)); } else from.push(...Array.from(h._dstPoints));
    }
    cases[name] = { geoms, canvas, runs, hashes, sampling: h.sampling === 'bilinear' ? 1 : 0 };
    if (geometric) { cases[name].from = b64(Float32Array.from(from)); cases[name].to = b64(Float32Array.from(to)); } else {
        cases[name].dst = b64(Float32Array.from(from)); cases[name].src = b64(Float32Array.from(h._srcPoints));
        cases[name].tris = b64(Uint32Array.from(h._triangles)); cases[name].minSrc = [h._minSrcX, h._minSrcY];
    }
}

{
    const p = new Homography('projective', W, H);
    p.sampling = 'bilinear';
    p.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    through(p, 'projective', [0, 1, 2, 3].map((k) => [[8 + 9 * k, k], [W * 0.5 + 9 * k, 0], [9 * k, H * 0.6], [W * 0.7 + 9 * k, H * 0.6 + 2 * k]]), 8);
    p.close();
}
{
    Homography.triangulate = () => gridTriangles(nx, ny);
    const grid = [];
    for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
    const h = new Homography('piecewiseaffine', W, H);
    h.setSourcePoints(grid, img, W, H, false);
    through(h, 'piecewise', [0, 1, 2, 3].map((k) => grid.map(([x, y]) => [x * 0.6 + 2 * Math.sin(y / 17 + k) + 8 * k, y * 0.55 + 1.0 * Math.cos(x / 23) + 2 + k])), 0);
    h.close();
}
console.log(JSON.stringify({ ok: fails.length === 0, fails, W, H, cases }));
process.exit(fails.length === 0 ? 0 : 1);
