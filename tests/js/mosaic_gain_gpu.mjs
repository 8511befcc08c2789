// GPU: h.mosaic(dstPointSets, { exposure }) of the drop-in class on the real addon, for a projective (bilinear sampling) and a piecewise
// set of overlapping frames of a 64 x 40 source.  Prints one JSON line: per case the windows, the point sets the batch entry gets (base64),
// the canvas, and the SHA-256 of the canvas, of the weight plane and of the gains for every run -- tests/test_gpu_mosaic_gain.py runs the
// same loop through ctypes (stage the set, warp, export the coords fields, statistics, solve, gained mosaic) and compares the hashes.
// Checked here: classes and shapes, 'none' against an absent option, given gains of 1 against no gains, the gains handed back into the
// array form, and more than 256 frames.  Exit code 1 on a failure.
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
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const cases = {};
// key: [mode, feather, sigmaN, sigmaG]
const runs = { gain: [2, null, 10, 0.1], sigmas: [1, null, 5, 0.3], last: [0, null, 10, 0.1] };
const optsOf = { gain: { exposure: 'gain' }, sigmas: { blend: 'mean', exposure: { sigmaN: 5, sigmaG: 0.3 } }, last: { blend: 'last', exposure: 'gain' } };

function through(h, name, sets, geometric) {
    const hashes = {};
    const base = { weight: true, pointsAreNormalized: false };
    const plain = h.mosaic(copy(sets), base);
    const canvas = [plain.x, plain.y, plain.width, plain.height];
    check(plain.gains === undefined, `${name}: no exposure, no gains`);
    const none = h.mosaic(copy(sets), Object.assign({ exposure: 'none' }, base));
    check(none.gains === undefined && sha(none.data) === sha(plain.data) && sha(none.weight) === sha(plain.weight), `${name}: 'none' is an absent option`);
    const ones = h.mosaic(copy(sets), Object.assign({ exposure: sets.map(() => 1) }, base));
    check(ones.gains instanceof Float32Array && ones.gains.every((g) => g === 1) && sha(ones.data) === sha(plain.data) && sha(ones.weight) === sha(plain.weight), `${name}: gains of 1 reproduce the plain mosaic`);
    for (const key of Object.keys(runs)) {
        const r = h.mosaic(copy(sets), Object.assign({}, base, optsOf[key]));
        check(r.data instanceof Uint8ClampedArray && r.weight instanceof Float32Array && r.gains instanceof Float32Array && r.gains.length === sets.length && r.data.length === r.width * r.height * 4, `${name} ${key}: shapes`);
        check(JSON.stringify(canvas) === JSON.stringify([r.x, r.y, r.width, r.height]), `${name} ${key}: the canvas moved`);
        check(r.gains.every((g) => Number.isFinite(g) && g > 0) && r.gains.some((g) => Math.abs(g - 1) > 1e-4), `${name} ${key}: gains ${Array.from(r.gains)}`);
        hashes[key] = { data: sha(r.data), weight: sha(r.weight), gains: sha(r.gains) };
        const again = h.mosaic(copy(sets), Object.assign({}, base, optsOf[key], { exposure: r.gains }));      // the fitted gains, given back as an array
        check(sha(again.data) === hashes[key].data && sha(again.gains) === hashes[key].gains, `${name} ${key}: the array form with the fitted gains`);
    }
    check(hashes.gain.weight === sha(plain.weight) && hashes.gain.data !== sha(plain.data), `${name}: gains change the picture, not the weights`);
    check(hashes.gain.gains === hashes.last.gains && hashes.gain.gains !== hashes.sigmas.gains, `${name}: the gains depend on the sigmas, not on the blend`);
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
    const sets = [0, 1, 2].map((k) => [[8 + 21 * k, k], [W * 0.5 + 21 * k, 0], [21 * k, H * 0.6], [W * 0.7 + 21 * k, H * 0.6 + 2 * k]]);
    through(p, 'projective', sets, 8);
    // more than 256 frames: the library's own refusal, as a string; 256 are fine
    const many = (n) => Array.from({ length: n }, (_, k) => [[k % 9, 0], [6 + k % 9, 0], [k % 9, 5], [6 + k % 9, 5]]);
    const e = thrown(() => p.mosaic(many(257), { exposure: 'gain', pointsAreNormalized: false }));
    check(typeof e === 'string' && e.includes('n_frames must be 0..256'), `257 frames with 'gain': ${e}`);
    const r = p.mosaic(many(256), { exposure: 'gain', pointsAreNormalized: false });
    check(r.gains.length === 256 && r.gains.every((g) => g > 0), '256 frames with gain');
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
