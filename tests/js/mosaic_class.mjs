// CPU: h.mosaic(dstPointSets, options) of the drop-in class over tests/js/mock_mosaic_addon.cjs (run with HGWARP_ADDON pointing at it): one
// native 'mosaicInverse' + family call with the windows and points warpBatch(dstPointSets, {inverse: true}) hands to its batch entry, the
// blend, the feather, the canvas (default: the bounding box of the non-blank windows), the weight flag and the source's size; the refusals
// throw bare strings before anything changes; and the instance ends in the state warpBatch(..., {inverse: true}) leaves.  Prints one JSON
// line {failures, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const trace = addon.trace, calls = addon.calls;
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const take = () => { calls.splice(0, calls.length); return trace.splice(0, trace.length); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const W = 96, H = 64, nx = 4, ny = 4;
const image = (v) => ({ data: new Uint8ClampedArray(W * H * 4).fill(v), width: W, height: H });
const img = image(9);
Homography.triangulate = () => gridTriangles(nx, ny);
const grid = [];
for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
const families = {
    affine: { make: () => { const h = new Homography('affine', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false); return h; },
              sets: [0, 1, 2, 3].map((k) => [[2 + 9 * k, 1 - k], [W / 4 + 2 + 9 * k, 1 - k], [2 + 9 * k, H / 4 + 1 - k]]), blank: [[5, 5], [5.2, 5], [5, 5.2]], entry: 'mosaicInverseGeometric', per: 6 },
    projective: { make: () => { const h = new Homography('projective', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false); return h; },
                  sets: [0, 1, 2].map((k) => [[1 + 11 * k, k], [W / 4 + 11 * k, 2 + k], [11 * k, H / 4 + k], [W / 4 - 1 + 11 * k, H / 4 + 1 + k]]), blank: [[5, 5], [5.2, 5], [5, 5.2], [5.2, 5.2]], entry: 'mosaicInverseGeometric', per: 8 },
    piecewise: { make: () => { const h = new Homography('piecewiseaffine', W, H); h.setSourcePoints(grid, img, W, H, false); return h; },
                 sets: [0, 1, 2].map((k) => grid.map(([x, y]) => [x * 0.25 + 2 + 13 * k, y * 0.25 + 1 + 2 * k])), blank: grid.map(([x, y]) => [5 + x * 0.002, 5 + y * 0.002]), entry: 'mosaicInversePiecewise', per: 2 * grid.length },
};
const copy = (sets) => sets.map((s) => s.map((p) => p.slice()));
const stateOf = (h) => JSON.stringify([h._lastPath, h._mapState, h._map && [h._map.kind, Array.from(h._map.pts), h._map.width, h._map.height, h._map.yOff], h._window(),
                                       Array.from(h._dstPoints), Array.from(h._srcPoints), h._dstPointsAreNormalized, h._srcPointsAreNormalized, h._transformMatrix && Array.from(h._transformMatrix),
                                       h._uploadedImage === h._image, h.sampling]);

for (const [name, fam] of Object.entries(families)) {
    // ---- the windows the loop derives, for the expectations below
    const probe = fam.make(), wins = [];
    for (const s of copy(fam.sets)) { probe.setDestinyPoints(s, false); wins.push(probe._window()); }
    probe.close();
    const bbox = [Math.min(...wins.map((w) => w[0])), Math.min(...wins.map((w) => w[1]))];
    bbox.push(Math.max(...wins.map((w) => w[0] + w[2])) - bbox[0], Math.max(...wins.map((w) => w[1] + w[3])) - bbox[1]);
    ok(wins.every((w) => w[2] > 1 && w[3] > 1) && bbox[2] > wins[0][2], `${name}: the premise: windows side by side (${JSON.stringify(wins)})`);

    // ---- the defaults: feather, uncapped, the bounding box, no weight plane; the state of warpBatch(..., {inverse: true})
    take();
    const a = fam.make(), b = fam.make();
    const frames = a.warpBatch(copy(fam.sets), { inverse: true });
    const batchCalls = calls.slice();
    take();
    const r = b.mosaic(copy(fam.sets));
    const t = take();
    ok(t.length === 1 && t[0].entry === fam.entry, `${name}: one native mosaic call (${t.map((x) => x.entry)})`);
    const c0 = t[0] || {};
    ok(c0.mode === 2 && c0.feather === Infinity && c0.wantWeight === false && c0.W === W && c0.H === H, `${name}: defaults ${JSON.stringify([c0.mode, c0.feather, c0.wantWeight, c0.W, c0.H])}`);
    ok(same(c0.canvas, bbox), `${name}: the default canvas is the bounding box: ${JSON.stringify(c0.canvas)} / ${JSON.stringify(bbox)}`);
    ok(same(c0.head[c0.head.length - 1], wins.flat()), `${name}: the windows of the call ${JSON.stringify(c0.head && c0.head[c0.head.length - 1])}`);
    ok(same([r.x, r.y, r.width, r.height], bbox) && r.data instanceof Uint8ClampedArray && r.data.length === bbox[2] * bbox[3] * 4 && r.weight === undefined, `${name}: result shape`);
    ok(stateOf(a) === stateOf(b), `${name}: the state after mosaic() must be warpBatch(..., {inverse: true})'s:\n${stateOf(a)}\n${stateOf(b)}`);
    ok(frames.length === fam.sets.length && batchCalls.length === 1, `${name}: the batch it is compared with ran as one inverse batch (${batchCalls})`);
    // the points: what the batch entry of warpBatch gets
    {
        take();
        const seen = [];
        const key = fam.entry === 'mosaicInversePiecewise' ? 'warpInversePiecewiseBatch' : 'warpInverseGeometricBatch', orig = addon[key];
        const a2 = fam.make();
        a2._native = Object.assign({}, a2._native, { [key]: (c, ...args) => { seen.push(args.slice(0, fam.entry === 'mosaicInversePiecewise' ? 2 : 4).map((x) => (ArrayBuffer.isView(x) ? Array.from(x) : x))); return orig(c, ...args); } });
        a2.warpBatch(copy(fam.sets), { inverse: true });
        ok(seen.length === 1 && same(seen[0], c0.head), `${name}: the points and windows are those of warpBatch's batch call`);
        a2.close();
    }
    a.close(); b.close();

    // ---- every option reaches the addon
    for (const [opts, want] of [[{ blend: 'mean' }, [1, Infinity, false]], [{ blend: 'last', weight: true }, [0, Infinity, true]], [{ blend: 'feather', feather: 12.5, weight: true }, [2, 12.5, true]],
                                [{ feather: 3 }, [2, 3, false]], [{ blend: 'mean', feather: 7, weight: false }, [1, 7, false]]]) {
        take();
        const h = fam.make();
        const res = h.mosaic(copy(fam.sets), opts);
        const tt = take();
        ok(tt.length === 1 && same([tt[0].mode, tt[0].feather, tt[0].wantWeight], want), `${name} ${JSON.stringify(opts)}: reaches the addon as ${JSON.stringify(tt[0] && [tt[0].mode, tt[0].feather, tt[0].wantWeight])}`);
        ok((res.weight instanceof Float32Array && res.weight.length === res.width * res.height) === (opts.weight === true) && (opts.weight === true || res.weight === undefined), `${name} ${JSON.stringify(opts)}: the weight plane`);
        h.close();
    }
    // ---- an explicit canvas, a blank frame in the middle (left out of the call, painter's order kept), per-frame images, the sampling mode,
    //      pointsAreNormalized handed to every setDestinyPoints (the auto-detect would scale the blank set up)
    {
        take();
        const h = fam.make();
        h.sampling = 'bilinear';
        const sets = copy(fam.sets);
        sets.splice(1, 0, fam.blank.map((p) => p.slice()));
        const imgs = [image(1), image(2), image(3)];
        const res = h.mosaic(sets, { canvas: { x: -3, y: 2, width: 50, height: 7 }, images: imgs, weight: true, pointsAreNormalized: false });
        const tt = take();
        ok(tt.length === 1 && same(tt[0].canvas, [-3, 2, 50, 7]) && same([res.x, res.y, res.width, res.height], [-3, 2, 50, 7]) && res.data.length === 1400 && res.weight.length === 350, `${name}: an explicit canvas`);
        ok(tt.length === 1 && same(tt[0].head[tt[0].head.length - 1], wins.flat()), `${name}: a blank frame is left out of the call`);
        ok(tt.length === 1 && same(tt[0].image, [1, 3, 1, 2].slice(0, fam.sets.length)), `${name}: frame f reads images[f % n], the blank frame's turn included (${JSON.stringify(tt[0] && tt[0].image)})`);
        ok(tt.length === 1 && tt[0].sampling === 1 && h.sampling === 'bilinear', `${name}: the instance's sampling mode governs the frames`);
        const g = fam.make();
        g.sampling = 'bilinear';
        g.warpBatch(copy(sets), { inverse: true, images: imgs, pointsAreNormalized: false });
        ok(stateOf(g) === stateOf(h), `${name}: state with a blank frame and {images}`);
        g.close(); h.close();
    }
    // ---- nothing to blend: no addon call, the zero canvas
    {
        take();
        const h = fam.make();
        const r0 = h.mosaic([]), r1 = h.mosaic([fam.blank.map((p) => p.slice())], { weight: true, pointsAreNormalized: false }), r2 = h.mosaic(copy(fam.sets), { canvas: { x: 0, y: 0, width: 0, height: 5 } });
        const r3 = h.mosaic([], { canvas: { x: 1, y: 2, width: 3, height: 2 }, weight: true });
        ok(take().length === 0, `${name}: nothing to blend makes no native mosaic call`);
        ok(r0.width === 0 && r0.height === 0 && r0.data.length === 0 && r1.data.length === 0 && r1.weight.length === 0 && r2.data.length === 0 && r2.width === 0, `${name}: empty results`);
        ok(r3.data.length === 24 && r3.weight.length === 6 && !r3.data.some((v) => v) && same([r3.x, r3.y, r3.width, r3.height], [1, 2, 3, 2]), `${name}: no frames over an explicit canvas: zeros`);
        h.close();
    }
    // ---- refusals: bare strings, before anything changes
    {
        const h = fam.make();
        h.setDestinyPoints(copy(fam.sets)[0], false);
        const before = stateOf(h);
        take();
        const bad = [{ blend: 'max' }, { blend: 2 }, { blend: null }, { feather: 0 }, { feather: -1 }, { feather: NaN }, { feather: '3' }, { feather: null },
                     { canvas: { x: 0, y: 0, width: 10 } }, { canvas: { x: 0.5, y: 0, width: 10, height: 10 } }, { canvas: [0, 0, 10, 10] }, { canvas: { x: 0, y: 0, width: Infinity, height: 1 } },
                     { canvas: { x: 0, y: 0, width: 2 ** 31, height: 1 } }, { devices: [0] }, { devices: [] }, { sourcePoints: fam.sets.map(() => grid) }];
        for (const opts of bad) {
            const e = thrown(() => h.mosaic(copy(fam.sets), opts));
            ok(typeof e === 'string' && e.startsWith('mosaic:'), `${name} ${JSON.stringify(opts)}: must throw a string (${e})`);
        }
        ok(typeof thrown(() => h.mosaic('nope')) === 'string', `${name}: the point sets must be an array`);
        ok(take().length === 0 && stateOf(h) === before, `${name}: a refused call reaches no native entry and changes nothing`);
        h.close();
    }
}
{
    const h = new Homography();
    const e = thrown(() => h.mosaic([[[0, 0], [1, 0], [0, 1]]]));
    ok(typeof e === 'string' && e.includes('needs a transform'), `no transform: ${e}`);
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length === 0 ? 0 : 1);
