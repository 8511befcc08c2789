// CPU: remap(plane, {sampling: 'trilinear'}) of the drop-in class over tests/js/mock_trilinear_addon.cjs (run with HGWARP_ADDON pointing at
// it): it makes the native calls {sampling: 'bilinear'} makes, with the same arguments, except that the last one goes to
// 'remapTrilinear' + entry; it takes the plane classes and channel counts 'bilinear' takes and refuses what 'bilinear' refuses, forward
// loops included; 'cubic' keeps throwing; the calls of 'nearest' and 'bilinear' are what they were.  Prints one JSON line {failures, checks}.
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

// ---- the entry chosen and its arguments: those of 'bilinear', the name apart
for (const [name, make] of Object.entries(makers)) {
    for (const loop of ['inverse', 'warp']) {
        for (const [Cls, channels] of [[Float32Array, 1], [Uint8Array, 4], [Uint8ClampedArray, 3], [Float32Array, 2]]) {
            const what = `${name} ${loop} ${Cls.name} x ${channels}`;
            take();
            const a = make(), b = make();
            const rb = a.remap(new Cls(W * H * channels), { channels, sampling: 'bilinear', loop });
            const tb = take();
            const rt = b.remap(new Cls(W * H * channels), { channels, sampling: 'trilinear', loop });
            const tt = take();
            ok(tb.length === tt.length && tt.length >= 2, `${what}: call counts ${tb.map((t) => t[0])} / ${tt.map((t) => t[0])}`);
            tb.slice(0, -1).forEach((t, i) => ok(JSON.stringify(t) === JSON.stringify(tt[i]), `${what}: call ${i} differs: ${t[0]} / ${(tt[i] || [])[0]}`));
            const lb = tb[tb.length - 1], lt = tt[tt.length - 1];
            ok(lb[0] === 'remap' + entryOf[name] && lt[0] === 'remapTrilinear' + entryOf[name], `${what}: entries ${lb[0]} / ${lt[0]}`);
            ok(JSON.stringify(lb.slice(1)) === JSON.stringify(lt.slice(1)), `${what}: the arguments behind the entry differ`);
            ok(lt[2] === Cls.name && lt[3] === channels && lt[4] === W && lt[5] === H, `${what}: the plane's part of the call ${lt.slice(2)}`);
            ok(tt.filter((t) => t[0].startsWith('remap') || t[0].startsWith('field')).length === 1, `${what}: one native field-side entry`);
            ok(rt.data instanceof Cls && rt.channels === channels && rt.width === rb.width && rt.height === rb.height && rt.data.length === rt.width * rt.height * channels && rt.data.length > 0, `${what}: result shape`);
            ok(b._lastPath === null, `${what}: remap() must not record a path`);
            a.close(); b.close();
        }
    }
}

// ---- the refusals of 'bilinear', forward loops included; 'cubic' keeps throwing
{
    const h = makers.projective();
    const good = new Uint8Array(W * H);
    const bad = {
        'an Array': () => h.remap(Array.from(good), { sampling: 'trilinear' }),
        'a DataView': () => h.remap(new DataView(good.buffer), { sampling: 'trilinear' }),
        'a short plane': () => h.remap(good.subarray(1), { sampling: 'trilinear' }),
        'a plane of another channel count': () => h.remap(good, { channels: 2, sampling: 'trilinear' }),
        'channels 0': () => h.remap(good, { channels: 0, sampling: 'trilinear' }),
        'channels 1.5': () => h.remap(good, { channels: 1.5, sampling: 'trilinear' }),
        'Int16Array': () => h.remap(new Int16Array(W * H), { sampling: 'trilinear' }),
        'Uint32Array': () => h.remap(new Uint32Array(W * H), { sampling: 'trilinear' }),
        'Float64Array': () => h.remap(new Float64Array(W * H), { sampling: 'trilinear' }),
        '5 channels': () => h.remap(new Float32Array(W * H * 5), { channels: 5, sampling: 'trilinear' }),
        'a forward loop': () => h.remap(good, { sampling: 'trilinear', loop: 'forward' }),
        "loop 'scatter'": () => h.remap(good, { sampling: 'trilinear', loop: 'scatter' }),
        "sampling 'cubic'": () => h.remap(good, { sampling: 'cubic' }),
        "sampling 'Trilinear'": () => h.remap(good, { sampling: 'Trilinear' }),
        'sampling 2': () => h.remap(good, { sampling: 2 }),
    };
    take();
    for (const [what, fn] of Object.entries(bad)) {
        const e = thrown(fn);
        ok(typeof e === 'string' && e.startsWith('remap'), `${what} must throw a bare string (${e})`);
    }
    ok(!take().some((t) => t[0].startsWith('remap') || t[0].startsWith('field')), 'a refused remap reaches no field-side entry point');
    // a same-size affine frame dispatches forward: {loop: 'warp'} refuses 'trilinear' as it refuses 'bilinear'
    const s = new Homography('affine', W, H);
    s.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    s.setDestinyPoints([[5, 3], [W + 5, 3], [5, H + 3]], false);
    const eb = thrown(() => s.remap(good, { sampling: 'bilinear', loop: 'warp' })), et = thrown(() => s.remap(good, { sampling: 'trilinear', loop: 'warp' }));
    ok(typeof eb === 'string' && eb === et, `a forward dispatch refuses both alike (${eb} / ${et})`);
    ok(typeof thrown(() => new Homography('projective').remap(good, { sampling: 'trilinear' })) === 'string', 'no image: a bare string');
    const none = new Homography('affine', W, H);
    none.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    none.setDestinyPoints([[0, 5], [10, 5], [20, 5]], false);
    take();
    const r = none.remap(new Float32Array(W * H * 3), { channels: 3, sampling: 'trilinear' });
    ok(r.data instanceof Float32Array && r.data.length === 0 && r.width === 0 && r.height === 0 && r.channels === 3, `empty window: ${JSON.stringify(r)}`);
    ok(!take().some((t) => t[0].startsWith('remap')), 'an empty window reaches no remap entry point');
}

// ---- 'nearest' and 'bilinear' call what they called: 'remap' + entry behind sourceField()'s own calls, the format in its place
for (const [name, make] of Object.entries(makers)) {
    for (const [sampling, fmt, fmtName] of [['nearest', 0, 'index'], ['bilinear', 1, 'coords'], [undefined, 0, 'index']]) {
        const what = `${name} ${sampling}`;
        take();
        const a = make();
        a.sourceField(fmtName);
        const tf = take();
        const b = make();
        b.remap(new Uint8Array(W * H * 2), sampling === undefined ? { channels: 2 } : { channels: 2, sampling });
        const tr = take();
        ok(tf.length === tr.length, `${what}: call counts`);
        tf.forEach((t, i) => ok(t[0].replace(/^field/, 'remap') === String((tr[i] || [])[0]) && t[1] === (tr[i] || [])[1], `${what}: call ${i}: ${t[0]} / ${(tr[i] || [])[0]}`));
        const last = tr[tr.length - 1], args = JSON.parse(last[1]);
        ok(last[0] === 'remap' + entryOf[name] && !tr.some((t) => t[0].includes('Trilinear')), `${what}: the entry ${last[0]}`);
        ok(args.length === (name === 'piecewise' ? 1 : 7) && args[args.length - 1] === fmt, `${what}: the field arguments ${last[1].slice(0, 80)}`);
        ok(last[2] === 'Uint8Array' && last[3] === 2 && last[4] === W && last[5] === H && last.length === 6, `${what}: the plane's part ${last.slice(2)}`);
        a.close(); b.close();
    }
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length ? 1 : 0);
