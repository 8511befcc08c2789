// CPU: h.mosaic(dstPointSets, { blend: 'median' | 'trimmed' | 'min' | 'max' }) of the drop-in class over tests/js/mock_robust_addon.cjs (run
// with HGWARP_ADDON pointing at it): one native 'mosaicRobustInverse' + family call with the windows of the plain mosaic's call, then the
// mode (HG_ROBUST_*), the trim (default 0.25, 0 for the blends that have none), the canvas, the weight flag, the source's size and the
// exposure, in that order; feather and bands are ignored; a bad trim throws a bare string and an f32 image a TypeError, before anything
// changes; an addon without the robust entries is refused by name.  Prints one JSON line {failures, checks}.
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
    projective: { make: () => { const h = new Homography('projective', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false); return h; },
                  sets: [0, 1, 2].map((k) => [[1 + 11 * k, k], [W / 4 + 11 * k, 2 + k], [11 * k, H / 4 + k], [W / 4 - 1 + 11 * k, H / 4 + 1 + k]]), entry: 'mosaicRobustInverseGeometric', plain: 'mosaicInverseGeometric' },
    piecewise: { make: () => { const h = new Homography('piecewiseaffine', W, H); h.setSourcePoints(grid, img, W, H, false); return h; },
                 sets: [0, 1, 2].map((k) => grid.map(([x, y]) => [x * 0.25 + 2 + 13 * k, y * 0.25 + 1 + 2 * k])), entry: 'mosaicRobustInversePiecewise', plain: 'mosaicInversePiecewise' },
};
const copy = (sets) => sets.map((s) => s.map((p) => p.slice()));
const stateOf = (h) => JSON.stringify([h._lastPath, h._mapState, h._window(), Array.from(h._dstPoints), Array.from(h._srcPoints), h.sampling]);

for (const [name, fam] of Object.entries(families)) {
    // ---- the plain mosaic's call, for the head and the canvas
    take();
    const p = fam.make();
    p.mosaic(copy(fam.sets), { blend: 'mean' });
    const plain = take()[0];
    ok(plain && plain.entry === fam.plain, `${name}: the plain call (${plain && plain.entry})`);
    const after = stateOf(p);
    p.close();

    // ---- blends, defaults and the argument order
    for (const [opts, want] of [[{ blend: 'median' }, [0, 0, false, 6]], [{ blend: 'trimmed' }, [1, 0.25, false, 6]], [{ blend: 'trimmed', trim: 0.1, weight: true }, [1, 0.1, true, 6]],
                                [{ blend: 'trimmed', trim: 0 }, [1, 0, false, 6]], [{ blend: 'min', trim: 0.4 }, [2, 0, false, 6]], [{ blend: 'max', weight: true }, [3, 0, true, 6]],
                                [{ blend: 'median', feather: -3, bands: 99, trim: 'x' }, [0, 0, false, 6]]]) {      // feather, bands and (off 'trimmed') trim are ignored
        take();
        const h = fam.make();
        const res = h.mosaic(copy(fam.sets), opts);
        const tt = take(), t0 = tt[0] || {};
        ok(tt.length === 1 && t0.entry === fam.entry, `${name} ${JSON.stringify(opts)}: one native call to ${fam.entry} (${tt.map((x) => x.entry)})`);
        ok(same([t0.mode, t0.trim, t0.wantWeight, t0.nArgs], want), `${name} ${JSON.stringify(opts)}: reaches the addon as ${JSON.stringify([t0.mode, t0.trim, t0.wantWeight, t0.nArgs])}`);
        ok(same(t0.head, plain.head) && same(t0.canvas, plain.canvas) && t0.W === W && t0.H === H && t0.exposure === null, `${name} ${JSON.stringify(opts)}: the head, canvas and source size of the plain call`);
        ok(res.data instanceof Uint8ClampedArray && res.data.length === res.width * res.height * 4 && (res.weight instanceof Float32Array) === (opts.weight === true) && res.gains === undefined, `${name} ${JSON.stringify(opts)}: result shape`);
        ok(stateOf(h) === after, `${name} ${JSON.stringify(opts)}: the state the plain mosaic leaves`);
        h.close();
    }
    // ---- exposure composes: the seventh argument, as the plain mosaic sends it; an explicit canvas
    for (const [ex, want] of [[[1.5, 0.75, 1], ['Float32Array', [1.5, 0.75, 1]]], ['gain', ['Float64Array', [10, 0.1]]], [{ sigmaN: 4, sigmaG: 0.5 }, ['Float64Array', [4, 0.5]]]]) {
        take();
        const h = fam.make();
        const res = h.mosaic(copy(fam.sets), { blend: 'median', exposure: ex, canvas: { x: -3, y: 2, width: 50, height: 7 } });
        const tt = take(), t0 = tt[0] || {};
        ok(tt.length === 1 && t0.entry === fam.entry && t0.nArgs === 7 && same(t0.exposure, want), `${name} exposure ${JSON.stringify(ex)}: ${JSON.stringify(t0.exposure)}`);
        ok(same(t0.canvas, [-3, 2, 50, 7]) && res.data.length === 1400 && res.gains instanceof Float32Array && res.gains.length === 3, `${name} exposure ${JSON.stringify(ex)}: canvas and gains`);
        h.close();
    }
    ok(take().length === 0 && thrown(() => { const h = fam.make(); h.mosaic(copy(fam.sets), { blend: 'max', exposure: 'none' }); h.close(); }) === undefined && take()[0].exposure === null, `${name}: exposure 'none' sends no seventh argument`);
    // ---- refusals, before anything changes
    {
        const h = fam.make();
        h.setDestinyPoints(copy(fam.sets)[0], false);
        const before = stateOf(h);
        take();
        for (const trim of [0.5, -0.1, NaN, '0.2', null, Infinity]) {
            const e = thrown(() => h.mosaic(copy(fam.sets), { blend: 'trimmed', trim }));
            ok(typeof e === 'string' && e.startsWith('mosaic:') && e.includes('trim'), `${name} trim ${trim}: must throw a string (${e})`);
        }
        const f32 = { data: new Float32Array(W * H * 4), width: W, height: H };
        for (const blend of ['median', 'trimmed', 'min', 'max']) {
            const e = thrown(() => h.mosaic(copy(fam.sets), { blend, images: [img, f32] }));
            ok(e instanceof TypeError && e.message.includes(blend), `${name} ${blend}: an f32 image set must be a TypeError (${e})`);
        }
        ok(thrown(() => h.mosaic(copy(fam.sets), { blend: 'median', images: [new Float32Array(W * H * 4)] })) instanceof TypeError, `${name}: a bare Float32Array is one too`);
        const e = thrown(() => h.mosaic(copy(fam.sets), { blend: 'median', labels: true }));
        ok(typeof e === 'string' && e.includes('labels'), `${name}: labels need 'multiband' (${e})`);
        ok(typeof thrown(() => h.mosaic(copy(fam.sets), { blend: 'mode' })) === 'string', `${name}: an unknown blend`);
        ok(take().length === 0 && stateOf(h) === before, `${name}: a refused call reaches no native entry and changes nothing`);
        // an addon from before the robust entries: refused by name, a bare string
        const old = fam.make();
        old._native = Object.assign({}, old._native, { mosaicRobustInverseGeometric: undefined, mosaicRobustInversePiecewise: undefined });
        const eo = thrown(() => old.mosaic(copy(fam.sets), { blend: 'max' }));
        ok(typeof eo === 'string' && eo.startsWith('mosaic:') && eo.includes("'max'") && take().length === 0, `${name}: an addon without the entries (${eo})`);
        old.close(); h.close();
    }
    // ---- nothing to blend: no addon call, the zero canvas
    {
        take();
        const h = fam.make();
        const r0 = h.mosaic([], { blend: 'median' }), r3 = h.mosaic([], { blend: 'max', canvas: { x: 1, y: 2, width: 3, height: 2 }, weight: true });
        ok(take().length === 0 && r0.data.length === 0 && r3.data.length === 24 && r3.weight.length === 6 && !r3.data.some((v) => v), `${name}: nothing to blend`);
        h.close();
    }
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length === 0 ? 0 : 1);
