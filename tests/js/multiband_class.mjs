// CPU: h.mosaic(dstPointSets, { blend: 'multiband', ... }) of the drop-in class over tests/js/mock_multiband_addon.cjs (run with HGWARP_ADDON
// pointing at it): one native 'mosaicMultibandInverse' + family call with the windows and points of the plain mosaic, the band count in the
// place of the mode (default 5), the feather, the canvas, the weight and label flags, the exposure behind them; labels come back as indices
// into dstPointSets, blank frames skipped; the other blends still take their own entries, unchanged; bad `bands` and `labels` without
// 'multiband' throw bare strings before anything changes.  Prints one JSON line {failures, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const { trace, calls, bandCalls } = addon;
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const take = () => { calls.splice(0, calls.length); trace.splice(0, trace.length); return bandCalls.splice(0, bandCalls.length); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const W = 96, H = 64, nx = 4, ny = 4;
const img = { data: new Uint8ClampedArray(W * H * 4).fill(9), width: W, height: H };
Homography.triangulate = () => gridTriangles(nx, ny);
const grid = [];
for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
const families = {
    affine: { make: () => { const h = new Homography('affine', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false); return h; },
              sets: [0, 1, 2, 3].map((k) => [[2 + 9 * k, 1 - k], [W / 4 + 2 + 9 * k, 1 - k], [2 + 9 * k, H / 4 + 1 - k]]), blank: [[5, 5], [5.2, 5], [5, 5.2]], entry: 'mosaicMultibandInverseGeometric', plain: 'mosaicInverseGeometric' },
    projective: { make: () => { const h = new Homography('projective', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false); return h; },
                  sets: [0, 1, 2].map((k) => [[1 + 11 * k, k], [W / 4 + 11 * k, 2 + k], [11 * k, H / 4 + k], [W / 4 - 1 + 11 * k, H / 4 + 1 + k]]), blank: [[5, 5], [5.2, 5], [5, 5.2], [5.2, 5.2]], entry: 'mosaicMultibandInverseGeometric', plain: 'mosaicInverseGeometric' },
    piecewise: { make: () => { const h = new Homography('piecewiseaffine', W, H); h.setSourcePoints(grid, img, W, H, false); return h; },
                 sets: [0, 1, 2].map((k) => grid.map(([x, y]) => [x * 0.25 + 2 + 13 * k, y * 0.25 + 1 + 2 * k])), blank: grid.map(([x, y]) => [5 + x * 0.002, 5 + y * 0.002]), entry: 'mosaicMultibandInversePiecewise', plain: 'mosaicInversePiecewise' },
};
const copy = (sets) => sets.map((s) => s.map((p) => p.slice()));
const stateOf = (h) => JSON.stringify([h._lastPath, h._mapState, h._window(), Array.from(h._dstPoints), Array.from(h._srcPoints), h._uploadedImage === h._image, h.sampling]);

for (const [name, fam] of Object.entries(families)) {
    // ---- the plain feathered mosaic, for the windows and the canvas; it still takes its own entry with its own arguments
    take();
    const p = fam.make();
    const plainRes = p.mosaic(copy(fam.sets));
    ok(bandCalls.length === 0 && trace.length === 1 && trace[0].entry === fam.plain && trace[0].mode === 2, `${name}: 'feather' still takes ${fam.plain}`);
    const plainCall = trace[0] || {};
    const plainState = stateOf(p);
    take();

    // ---- the defaults of 'multiband': 5 bands, uncapped feather, the bounding box, no weight plane, no labels, no exposure
    const h = fam.make();
    const r = h.mosaic(copy(fam.sets), { blend: 'multiband' });
    ok(trace.length === 0, `${name}: no plain mosaic call`);
    let t = take();
    ok(t.length === 1 && t[0].entry === fam.entry, `${name}: one native multiband call (${t.map((x) => x.entry)})`);
    const c0 = t[0] || {};
    ok(c0.bands === 5 && c0.feather === Infinity && c0.wantWeight === false && c0.wantLabels === false && c0.exposure === null && c0.W === W && c0.H === H,
       `${name}: defaults ${JSON.stringify([c0.bands, c0.feather, c0.wantWeight, c0.wantLabels, c0.exposure])}`);
    ok(same(c0.canvas, plainCall.canvas) && same(c0.head, plainCall.head), `${name}: the windows, points and canvas of the plain mosaic`);
    ok(same([r.x, r.y, r.width, r.height], [plainRes.x, plainRes.y, plainRes.width, plainRes.height]) && r.data instanceof Uint8ClampedArray &&
       r.data.length === plainRes.data.length && r.weight === undefined && r.labels === undefined && r.gains === undefined, `${name}: result shape`);
    ok(stateOf(h) === plainState, `${name}: the instance ends in the plain mosaic's state`);

    // ---- every option handed down; labels: Int32Array, one per canvas pixel
    const cv = { x: -3, y: -2, width: 40, height: 21 };
    const r2 = h.mosaic(copy(fam.sets), { blend: 'multiband', bands: 3, feather: 6.5, canvas: cv, weight: true, labels: true });
    t = take();
    const c1 = t[0] || {};
    ok(t.length === 1 && c1.bands === 3 && c1.feather === 6.5 && same(c1.canvas, [-3, -2, 40, 21]) && c1.wantWeight === true && c1.wantLabels === true && c1.exposure === null,
       `${name}: options ${JSON.stringify(c1)}`);
    ok(r2.labels instanceof Int32Array && r2.labels.length === 40 * 21 && r2.weight instanceof Float32Array && r2.weight.length === 40 * 21 && r2.labels[0] === -1, `${name}: labels and weight`);
    for (const bands of [1, 8]) { h.mosaic(copy(fam.sets), { blend: 'multiband', bands }); ok(take()[0].bands === bands, `${name}: bands ${bands}`); }

    // ---- exposure composes as it does for the other blends
    const r3 = h.mosaic(copy(fam.sets), { blend: 'multiband', exposure: 'gain', labels: true });
    t = take();
    ok(t.length === 1 && same(t[0].exposure, { sigmas: [10, 0.1] }) && t[0].wantLabels === true && t[0].bands === 5, `${name}: exposure 'gain' ${JSON.stringify(t[0] && t[0].exposure)}`);
    ok(r3.gains instanceof Float32Array && r3.gains.length === fam.sets.length && r3.gains[1] === 1.125, `${name}: the fitted gains come back`);
    const given = fam.sets.map((_, k) => 0.5 + k / 4);
    const r4 = h.mosaic(copy(fam.sets), { blend: 'multiband', bands: 2, exposure: given });
    t = take();
    ok(t.length === 1 && same(t[0].exposure, { gains: given }) && same(Array.from(r4.gains), given), `${name}: given gains`);

    // ---- a blank frame is skipped; labels and gains are indices into / one per dstPointSets
    const withBlank = [fam.sets[0], fam.blank, ...fam.sets.slice(1)];
    const r5 = h.mosaic(copy(withBlank), { blend: 'multiband', labels: true, exposure: 'gain', pointsAreNormalized: false });      // (the auto-detect would scale the blank set up)
    t = take();
    const F = fam.sets.length;
    ok(t.length === 1 && t[0].head[t[0].head.length - 1].length === 4 * F, `${name}: the blank frame is not part of the call`);
    const want = Array.from({ length: r5.labels.length }, (_, i) => { if (i === 0) return -1; const l = i % F; return l === 0 ? 0 : l + 1; });
    ok(same(Array.from(r5.labels), want), `${name}: labels name destiny point sets`);
    ok(r5.gains.length === F + 1 && r5.gains[1] === 1 && r5.gains[2] === 1.125, `${name}: gains per destiny point set`);
    const r6 = h.mosaic([fam.blank.map((q) => q.slice())], { blend: 'multiband', labels: true, weight: true, canvas: cv, pointsAreNormalized: false });
    ok(take().length === 0 && r6.labels instanceof Int32Array && r6.labels.length === 40 * 21 && r6.labels.every((l) => l === -1) && !r6.data.some((v) => v), `${name}: only blank frames: no call, labels -1`);

    // ---- refusals: bare strings, before anything changes
    const before = stateOf(h);
    for (const bands of [0, 9, 2.5, '5', NaN, null, -1]) {
        const e = thrown(() => h.mosaic(copy(fam.sets), { blend: 'multiband', bands }));
        ok(typeof e === 'string' && e.includes('bands'), `${name}: bands ${String(bands)} throws a string (${String(e)})`);
    }
    let e = thrown(() => h.mosaic(copy(fam.sets), { blend: 'feather', labels: true }));
    ok(typeof e === 'string' && e.includes('labels'), `${name}: labels without multiband (${String(e)})`);
    e = thrown(() => h.mosaic(copy(fam.sets), { blend: 'bands' }));
    ok(typeof e === 'string' && e.includes("'multiband'"), `${name}: an unknown blend names the four (${String(e)})`);
    e = thrown(() => h.mosaic(copy(fam.sets), { blend: 'multiband', feather: 0 }));
    ok(typeof e === 'string' && e.includes('feather'), `${name}: a bad feather`);
    ok(take().length === 0 && calls.length === 0 && stateOf(h) === before, `${name}: a refusal makes no native call and changes nothing`);
    h.mosaic(copy(fam.sets), { blend: 'mean', bands: 99 });                       // `bands` is ignored by the other blends
    ok(trace.length === 1 && trace[0].mode === 1 && bandCalls.length === 0, `${name}: 'mean' with a stray bands`);
    take();
    h.close(); p.close();
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length ? 1 : 0);
