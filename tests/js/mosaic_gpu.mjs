// GPU: h.mosaic(dstPointSets, options) of the drop-in class on the real addon, for an affine, a projective (bilinear sampling) and a
// piecewise set of overlapping frames of a 64 x 40 source.  Prints one JSON line: per case the windows, the point sets the batch entry
// gets (base64), the canvas, and the SHA-256 of the canvas and of the weight plane for every blend -- tests/test_gpu_mosaic.py runs the
// same loop through ctypes (stage the set, warp, export the coords fields, mosaic) and compares the hashes.  Checked here: classes and
// shapes, the defaults, an explicit canvas against a crop of the default one, and the state the call leaves.  Exit code 1 on a failure.
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
const runs = { feather: [2, null], capped: [2, 3], mean: [1, null], last: [0, null] };
const optsOf = { feather: {}, capped: { feather: 3 }, mean: { blend: 'mean' }, last: { blend: 'last' } };

function through(h, name, sets, geometric) {
    const hashes = {};
    let canvas = null, first = null;
    for (const key of Object.keys(runs)) {
        const r = h.mosaic(copy(sets), Object.assign({ weight: true, pointsAreNormalized: false }, optsOf[key]));
        check(r.data instanceof Uint8ClampedArray && r.weight instanceof Float32Array && r.data.length === r.width * r.height * 4 && r.weight.length === r.width * r.height, `${name} ${key}: shapes`);
        check(canvas === null || JSON.stringify(canvas) === JSON.stringify([r.x, r.y, r.width, r.height]), `${name} ${key}: the canvas moved`);
        canvas = [r.x, r.y, r.width, r.height];
        check(r.data.some((v) => v !== 0) && (key === 'last' ? r.weight.every((v) => v === 0 || v === 1) && r.weight.some((v) => v === 1) : r.weight.some((v) => v > 1)) && r.weight.some((v) => v === 0), `${name} ${key}: covered, overlapping and uncovered pixels`);
        hashes[key] = { data: sha(r.data), weight: sha(r.weight) };
        if (key === 'feather') first = r;
    }
    check(new Set(Object.values(hashes).map((x) => x.data)).size === 4, `${name}: the four blends must differ on overlapping frames`);
    const d = h.mosaic(copy(sets), { pointsAreNormalized: false });
    check(d.weight === undefined && sha(d.data) === hashes.feather.data, `${name}: the defaults are 'feather', uncapped, no weight plane`);
    // an explicit canvas is a crop of the default one
    const cx = canvas[0] + 3, cy = canvas[1] + 2, cw = canvas[2] - 7, ch = canvas[3] - 3;
    const c = h.mosaic(copy(sets), { canvas: { x: cx, y: cy, width: cw, height: ch }, pointsAreNormalized: false });
    let same = c.width === cw && c.height === ch && c.x === cx && c.y === cy;
    for (let j = 0; j < ch && same; j++) for (let i = 0; i < cw * 4 && same; i++) same = c.data[j * cw * 4 + i] === first.data[((j + 2) * canvas[2] + 3) * 4 + i];
    check(same, `${name}: an explicit canvas must be a crop of the default one`);
    const path = h._lastPath, map = h._mapState;
    const frames = h.warpBatch(copy(sets), { inverse: true, pointsAreNormalized: false });
    check(h._lastPath === path && h._mapState === map, `${name}: mosaic() leaves the path and map state of warpBatch(..., {inverse: true})`);
    // what the ctypes side needs
    const geoms = [], from = [], to = [];
    for (const s of copy(sets)) {
        h.setDestinyPoints(s, false);
        geoms.push(h._window());
        if (geometric) { h._alignRanges(); from.push(...Array.from(h._dstPoints).slice(0, geometric)); to.push(...Array.from(h._srcPoints).slice(0, geometric)); } else from.push(...Array.from(h._dstPoints));
    }
    check(frames.every((f, k) => f.width === geoms[k][2] && f.height === geoms[k][3]), `${name}: the windows are warpBatch's`);
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
