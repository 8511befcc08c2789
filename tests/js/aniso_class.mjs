// CPU: remap(plane, {sampling: 'anisotropic'}) of the drop-in class over tests/js/mock_aniso_addon.cjs (run with HGWARP_ADDON pointing at it):
// it makes the native calls {sampling: 'trilinear'} makes, with the same arguments, except that the last one goes to 'remapAniso' + entry
// with maxAniso appended (default 8); a bad maxAniso and everything 'trilinear' refuses throw bare strings, forward loops included; the
// calls of 'nearest', 'bilinear' and 'trilinear' are what they were.  Prints one JSON line {failures, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const trace = addon.trace;
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const take = () => trace.splice(0, trace.length);
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const W = 96, H = 64, nx = 4, ny = 4;
const img = { data: new Uint8ClampedArray(W * H * 4).fill(9), width: W, height: H };
Homography.triangulate = () => gridTriangles(nx, ny);
const grid = [];
for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
const small = grid.map(([x, y]) => [x * 0.25 + 2, y * 0.25 + 1]);          // a 4x shrink: every warp of it takes the inverse loop
const makers = {
    affine: () => { const h = new Homography('affine', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false); h.setDestinyPoints([[2, 1], [W / 4 + 2, 1], [2, H / 4 + 1]], false); return h; },
    projective: () => { const h = new Homography('projective', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false); h.setDestinyPoints([[1, 0], [W / 4, 2], [0, H / 4], [W / 4 - 1, H / 4 + 1]], false); return h; },
    piecewise: () => { const h = new Homography('piecewiseaffine', W, H); h.setSourcePoints(grid, img, W, H, false); h.setDestinyPoints(small, false); return h; },
};
const entryOf = { affine: 'InverseGeometric', projective: 'InverseGeometric', piecewise: 'InversePiecewise' };

// ---- the entry chosen and its arguments: those of 'trilinear', the name apart, then maxAniso
for (const [name, make] of Object.entries(makers)) {
    for (const loop of ['inverse', 'warp']) {
        for (const [Cls, channels, maxAniso, want] of [[Float32Array, 1, undefined, 8], [Uint8Array, 4, 1, 1], [Uint8ClampedArray, 3, 16, 16], [Float32Array, 2, 5, 5]]) {
            const what = `${name} ${loop} ${Cls.name} x ${channels} maxAniso ${maxAniso}`;
            take();
            const a = make(), b = make();
            const rt = a.remap(new Cls(W * H * channels), { channels, sampling: 'trilinear', loop });
            const tt = take();
            const ra = b.remap(new Cls(W * H * channels), maxAniso === undefined ? { channels, sampling: 'anisotropic', loop } : { channels, sampling: 'anisotropic', loop, maxAniso });
            const ta = take();
            ok(tt.length === ta.length && ta.length >= 2, `${what}: call counts ${tt.map((t) => t[0])} / ${ta.map((t) => t[0])}`);
            tt.slice(0, -1).forEach((t, i) => ok(JSON.stringify(t) === JSON.stringify(ta[i]), `${what}: call ${i} differs: ${t[0]} / ${(ta[i] || [])[0]}`));
            const lt = tt[tt.length - 1], la = ta[ta.length - 1];
            ok(lt[0] === 'remapTrilinear' + entryOf[name] && la[0] === 'remapAniso' + entryOf[name], `${what}: entries ${lt[0]} / ${la[0]}`);
            ok(JSON.stringify(lt.slice(1)) === JSON.stringify(la.slice(1, 6)), `${what}: the arguments behind the entry differ`);
            ok(la.length === 7 && la[6] === want, `${what}: maxAniso reaches the addon as ${la[6]}`);
            ok(la[2] === Cls.name && la[3] === channels && la[4] === W && la[5] === H, `${what}: the plane's part of the call ${la.slice(2)}`);
            ok(ta.filter((t) => t[0].startsWith('remap') || t[0].startsWith('field')).length === 1, `${what}: one native field-side entry`);
            ok(ra.data instanceof Cls && ra.channels === channels && ra.width === rt.width && ra.height === rt.height && ra.data.length === ra.width * ra.height * channels && ra.data.length > 0, `${what}: result shape`);
            ok(b._lastPath === null, `${what}: remap() must not record a path`);
            a.close(); b.close();
        }
    }
}

// ---- a bad maxAniso, the refusals of 'trilinear', forward loops included
{
    const h = makers.projective();
    const good = new Uint8Array(W * H);
    const bad = {};
    for (const v of [0, 17, -1, 1.5, '8', null, NaN, Infinity, [4], true]) bad[`maxAniso ${JSON.stringify(v)} (${typeof v})`] = () => h.remap(good, { sampling: 'anisotropic', maxAniso: v });
    Object.assign(bad, {
        'an Array': () => h.remap(Array.from(good), { sampling: 'anisotropic' }),
        'a DataView': () => h.remap(new DataView(good.buffer), { sampling: 'anisotropic' }),
        'a short plane': () => h.remap(good.subarray(1), { sampling: 'anisotropic' }),
        'a plane of another channel count': () => h.remap(good, { channels: 2, sampling: 'anisotropic' }),
        'channels 0': () => h.remap(good, { channels: 0, sampling: 'anisotropic' }),
        'Int16Array': () => h.remap(new Int16Array(W * H), { sampling: 'anisotropic' }),
        'Float64Array': () => h.remap(new Float64Array(W * H), { sampling: 'anisotropic' }),
        '5 channels': () => h.remap(new Float32Array(W * H * 5), { channels: 5, sampling: 'anisotropic' }),
        'a forward loop': () => h.remap(good, { sampling: 'anisotropic', loop: 'forward' }),
        "loop 'scatter'": () => h.remap(good, { sampling: 'anisotropic', loop: 'scatter' }),
        "sampling 'Anisotropic'": () => h.remap(good, { sampling: 'Anisotropic' }),
        "sampling 'aniso'": () => h.remap(good, { sampling: 'aniso' }),
    });
    take();
    for (const [what, fn] of Object.entries(bad)) {
        const e = thrown(fn);
        ok(typeof e === 'string' && e.startsWith('remap'), `${what} must throw a bare string (${e})`);
    }
    ok(String(thrown(() => h.remap(good, { sampling: 'anisotropic', maxAniso: 0 }))).includes('maxAniso'), 'the maxAniso refusal names the option');
    ok(!take().some((t) => t[0].startsWith('remap') || t[0].startsWith('field')), 'a refused remap reaches no field-side entry point');
    // the other samplings do not look at maxAniso
    for (const sampling of ['nearest', 'bilinear', 'trilinear']) ok(thrown(() => h.remap(good, { sampling, maxAniso: 99 })) === undefined, `'${sampling}' ignores maxAniso`);
    take();
    // a same-size affine frame dispatches forward: {loop: 'warp'} refuses 'anisotropic' as it refuses 'trilinear'
    const s = new Homography('affine', W, H);
    s.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    s.setDestinyPoints([[5, 3], [W + 5, 3], [5, H + 3]], false);
    const et = thrown(() => s.remap(good, { sampling: 'trilinear', loop: 'warp' })), ea = thrown(() => s.remap(good, { sampling: 'anisotropic', loop: 'warp' }));
    ok(typeof et === 'string' && et === ea, `a forward dispatch refuses both alike (${et} / ${ea})`);
    const ef = thrown(() => h.remap(good, { sampling: 'trilinear', loop: 'forward' })), eg = thrown(() => h.remap(good, { sampling: 'anisotropic', loop: 'forward' }));
    ok(typeof ef === 'string' && ef === eg, `a forward loop refuses both alike (${ef} / ${eg})`);
    ok(typeof thrown(() => new Homography('projective').remap(good, { sampling: 'anisotropic' })) === 'string', 'no image: a bare string');
    const none = new Homography('affine', W, H);
    none.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    none.setDestinyPoints([[0, 5], [10, 5], [20, 5]], false);
    take();
    const r = none.remap(new Float32Array(W * H * 3), { channels: 3, sampling: 'anisotropic' });
    ok(r.data instanceof Float32Array && r.data.length === 0 && r.width === 0 && r.height === 0 && r.channels === 3, `empty window: ${JSON.stringify(r)}`);
    ok(!take().some((t) => t[0].startsWith('remap')), 'an empty window reaches no remap entry point');
}

// ---- 'nearest', 'bilinear' and 'trilinear' call what they called: the entry behind sourceField()'s own calls, six-element records
for (const [name, make] of Object.entries(makers)) {
    for (const [sampling, fmt, fmtName, prefix] of [['nearest', 0, 'index', 'remap'], ['bilinear', 1, 'coords', 'remap'], [undefined, 0, 'index', 'remap'], ['trilinear', 1, 'coords', 'remapTrilinear']]) {
        const what = `${name} ${sampling}`;
        take();
        const a = make();
        a.sourceField(fmtName);
        const tf = take();
        const b = make();
        b.remap(new Uint8Array(W * H * 2), sampling === undefined ? { channels: 2 } : { channels: 2, sampling });
        const tr = take();
        ok(tf.length === tr.length, `${what}: call counts`);
        tf.forEach((t, i) => ok(t[0].replace(/^field/, prefix) === String((tr[i] || [])[0]) && t[1] === (tr[i] || [])[1], `${what}: call ${i}: ${t[0]} / ${(tr[i] || [])[0]}`));
        const last = tr[tr.length - 1], args = JSON.parse(last[1]);
        ok(last[0] === prefix + entryOf[name] && !tr.some((t) => t[0].includes('Aniso')), `${what}: the entry ${last[0]}`);
        ok(args.length === (name === 'piecewise' ? 1 : 7) && args[args.length - 1] === fmt, `${what}: the field arguments ${last[1].slice(0, 80)}`);
        ok(last[2] === 'Uint8Array' && last[3] === 2 && last[4] === W && last[5] === H && last.length === 6, `${what}: the plane's part ${last.slice(2)}`);
        a.close(); b.close();
    }
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length ? 1 : 0);
