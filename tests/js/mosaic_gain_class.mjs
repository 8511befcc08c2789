// CPU: h.mosaic(dstPointSets, { exposure }) of the drop-in class over tests/js/mock_mosaic_gain_addon.cjs (run with HGWARP_ADDON pointing at
// it): the exposure argument follows the mosaic's own, in their order, as a Float64Array [sigmaN, sigmaG] ('gain': 10, 0.1) or a Float32Array
// of one gain per NON-BLANK frame; 'none' and an absent option make the call the class made before; the array form is validated (length,
// finite, > 0) before anything changes; the result carries `gains`, one per destiny point set.  Prints one JSON line {failures, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const trace = addon.trace, calls = addon.calls, exposures = addon.exposures;
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const take = () => { calls.splice(0, calls.length); trace.splice(0, trace.length); return exposures.splice(0, exposures.length); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const W = 96, H = 64, nx = 4, ny = 4;
const img = { data: new Uint8ClampedArray(W * H * 4).fill(9), width: W, height: H };
Homography.triangulate = () => gridTriangles(nx, ny);
const grid = [];
for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
const families = {
    projective: { make: () => { const h = new Homography('projective', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false); return h; },
                  sets: [0, 1, 2].map((k) => [[1 + 11 * k, k], [W / 4 + 11 * k, 2 + k], [11 * k, H / 4 + k], [W / 4 - 1 + 11 * k, H / 4 + 1 + k]]), blank: [[5, 5], [5.2, 5], [5, 5.2], [5.2, 5.2]], entry: 'mosaicInverseGeometric', n: 11 },
    piecewise: { make: () => { const h = new Homography('piecewiseaffine', W, H); h.setSourcePoints(grid, img, W, H, false); return h; },
                 sets: [0, 1, 2].map((k) => grid.map(([x, y]) => [x * 0.25 + 2 + 13 * k, y * 0.25 + 1 + 2 * k])), blank: grid.map(([x, y]) => [5 + x * 0.002, 5 + y * 0.002]), entry: 'mosaicInversePiecewise', n: 9 },
};
const copy = (sets) => sets.map((s) => s.map((p) => p.slice()));
const opt = { pointsAreNormalized: false };

for (const [name, fam] of Object.entries(families)) {
    const h = fam.make();
    // ---- absent and 'none': the call the class made before, no gains in the result
    for (const ex of [undefined, null, 'none']) {
        take();
        const r = h.mosaic(copy(fam.sets), Object.assign({ exposure: ex }, opt));
        const t = take();
        ok(t.length === 1 && t[0].entry === fam.entry && t[0].exposure === null && t[0].n === fam.n - 1 && r.gains === undefined, `${name} exposure ${ex}: today's call (${JSON.stringify(t)})`);
    }
    // ---- 'gain' and { sigmaN, sigmaG }: one more argument behind the mosaic's own
    for (const [ex, want] of [['gain', [10, 0.1]], [{ sigmaN: 4, sigmaG: 0.25 }, [4, 0.25]], [{ sigmaG: 0.5 }, [10, 0.5]], [{}, [10, 0.1]]]) {
        take();
        const r = h.mosaic(copy(fam.sets), Object.assign({ exposure: ex, blend: 'mean', weight: true }, opt));
        const t = take();
        ok(t.length === 1 && t[0].n === fam.n && same(t[0].exposure, { sigmas: want }), `${name} exposure ${JSON.stringify(ex)}: reaches the addon last, as ${JSON.stringify(t[0] && t[0].exposure)}`);
        ok(r.gains instanceof Float32Array && same(Array.from(r.gains), [1, 1.125, 1.25]) && r.weight instanceof Float32Array && r.data.length === r.width * r.height * 4, `${name} exposure ${JSON.stringify(ex)}: the result carries the gains`);
    }
    // ---- given gains: an array or a Float32Array, as they are
    for (const ex of [[0.5, 1, 2], Float32Array.of(0.5, 1, 2)]) {
        take();
        const r = h.mosaic(copy(fam.sets), Object.assign({ exposure: ex }, opt));
        const t = take();
        ok(t.length === 1 && t[0].n === fam.n && same(t[0].exposure, { gains: [0.5, 1, 2] }) && r.gains instanceof Float32Array && same(Array.from(r.gains), [0.5, 1, 2]), `${name}: given gains ${JSON.stringify(t[0] && t[0].exposure)}`);
    }
    // ---- a blank frame is left out of the call and of its gains; the result has one gain per destiny point set, 1 for the blank one
    {
        const sets = copy(fam.sets);
        sets.splice(1, 0, fam.blank.map((p) => p.slice()));
        take();
        const r = h.mosaic(copy(sets), Object.assign({ exposure: [0.5, 7, 1.5, 2] }, opt));
        const t = take();
        ok(t.length === 1 && same(t[0].exposure, { gains: [0.5, 1.5, 2] }) && same(Array.from(r.gains), [0.5, 1, 1.5, 2]), `${name}: a blank frame: ${JSON.stringify(t[0] && t[0].exposure)} -> ${Array.from(r.gains || [])}`);
        const r2 = h.mosaic(copy(sets), Object.assign({ exposure: 'gain' }, opt));
        ok(same(Array.from(r2.gains), [1, 1, 1.125, 1.25]), `${name}: fitted gains around a blank frame: ${Array.from(r2.gains || [])}`);
        take();
        const r0 = h.mosaic([fam.blank.map((p) => p.slice())], Object.assign({ exposure: 'gain' }, opt)), r1 = h.mosaic([], { exposure: [] });
        ok(take().length === 0 && same(Array.from(r0.gains), [1]) && r1.gains instanceof Float32Array && r1.gains.length === 0, `${name}: nothing to blend: no call, gains of 1`);
    }
    // ---- refusals: bare strings, before anything reaches the addon
    {
        take();
        const bad = ['gains', 'GAIN', 1, true, [1, 1], [1, 1, 1, 1], [1, 0, 1], [1, -2, 1], [1, NaN, 1], [1, Infinity, 1], [1, '2', 1], [1, 1e39, 1], Float32Array.of(1, 1), Float64Array.of(1, 1, 1),
                     { sigmaN: 0 }, { sigmaN: -1 }, { sigmaG: NaN }, { sigmaN: Infinity }, { sigmaG: '0.1' }, { sigmaN: null }];
        for (const ex of bad) {
            const e = thrown(() => h.mosaic(copy(fam.sets), Object.assign({ exposure: ex }, opt)));
            ok(typeof e === 'string' && e.startsWith('mosaic: options.exposure'), `${name} exposure ${JSON.stringify(ex)}: must throw a string (${e})`);
        }
        ok(take().length === 0, `${name}: a refused exposure reaches no native entry`);
    }
    h.close();
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length === 0 ? 0 : 1);
