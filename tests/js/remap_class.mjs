// CPU: remap(plane, options) of the drop-in class over tests/js/mock_remap_addon.cjs (run with HGWARP_ADDON pointing at it): for every
// transform and loop it makes the field-side addon calls sourceField() makes, with the same arguments -- 'remap' + entry in place of
// 'field' + entry, the plane behind them --, no forward entry call under {loop: 'inverse'}; every bad plane or option throws a bare string;
// an empty window returns empty data of the plane's class.  Prints one JSON line {failures, checks}.
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
function lcgImage(w, h, seed) {
    const data = new Uint8ClampedArray(w * h * 4);
    let s = seed >>> 0;
    for (let i = 0; i < data.length; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; data[i] = s >>> 24 || 1; }
    return { data, width: w, height: h };
}
const W = 96, H = 64, nx = 4, ny = 4;
const img = lcgImage(W, H, 7);
const img32 = new Uint32Array(img.data.buffer);
Homography.triangulate = () => gridTriangles(nx, ny);
const grid = [];
for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
const inner = (i, j) => i > 0 && i < nx && j > 0 && j < ny;
const bent = grid.map(([x, y], k) => inner(k % (nx + 1), Math.floor(k / (nx + 1))) ? [x + 5 * Math.sin(y / 9), y + 4 * Math.cos(x / 11)] : [x, y]);
const makers = {
    affine: (o) => { const h = new Homography('affine', W, H, o); h.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false); h.setDestinyPoints([[5, 3], [W + 5, 3], [5, H + 3]], false); return h; },
    projective: (o) => { const h = new Homography('projective', W, H, o); h.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false); h.setDestinyPoints([[4, 0], [W, 6], [0, H - 2], [W - 3, H]], false); return h; },
    piecewise: (o) => { const h = new Homography('piecewiseaffine', W, H, o); h.setSourcePoints(grid, img, W, H, false); h.setDestinyPoints(bent, false); return h; },
};
const sameBytes = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);

// ---- the same field-side calls as sourceField(), for every transform, loop and format
for (const [name, make] of Object.entries(makers)) {
    for (const loop of ['inverse', 'warp', 'forward']) {
        for (const sampling of ['nearest', 'bilinear']) {
            const fmt = sampling === 'nearest' ? 'index' : 'coords', what = `${name} ${loop} ${sampling}`;
            take();
            const a = make({});
            const eField = thrown(() => a.sourceField(fmt, { loop }));
            const tField = take();
            const b = make({});
            let r;
            const eRemap = thrown(() => { r = b.remap(new Float32Array(W * H * 2), { channels: 2, sampling, loop }); });
            const tRemap = take();
            ok((eField === undefined) === (eRemap === undefined), `${what}: sourceField threw ${eField}, remap threw ${eRemap}`);
            if (eRemap !== undefined) { ok(typeof eRemap === 'string' && eRemap.startsWith('remap'), `${what}: a refusal must be a bare string of remap's (${eRemap})`); continue; }
            ok(tField.length === tRemap.length && tField.length >= 2, `${what}: call counts ${tField.map((t) => t[0])} / ${tRemap.map((t) => t[0])}`);
            tField.forEach((t, i) => {
                const u = tRemap[i] || [];
                ok(t[0].replace(/^field/, 'remap') === String(u[0]).replace(/^field/, 'remap') && t[1] === u[1], `${what}: call ${i}: ${t[0]} / ${u[0]} or their arguments differ`);
            });
            const last = tRemap[tRemap.length - 1];
            ok(last[0].startsWith('remap') && last[2] === 'Float32Array' && last[3] === 2 && last[4] === W && last[5] === H, `${what}: the plane's part of the call ${last}`);
            ok(tRemap.filter((t) => t[0].startsWith('field') || t[0].startsWith('remap')).length === 1, `${what}: one native field-side entry`);
            if (loop === 'inverse') ok(!tRemap.some((t) => t[0].includes('Forward')), `${what}: no forward entry call`);
            if (loop === 'forward') ok(last[0].includes('Forward'), `${what}: the forward entry`);
            ok(r.data instanceof Float32Array && r.channels === 2 && r.data.length === r.width * r.height * 2, `${what}: result shape`);
            ok(b._lastPath === null, `${what}: remap() must not record a path`);
            a.close(); b.close();
        }
    }
}

// ---- nearest remap of the picture's own pixels IS the warp (the mock's field is the oracle's)
for (const [name, make] of Object.entries(makers)) {
    const h = make({ sampling: 'bilinear' });                 // (independent of the instance's sampling mode)
    const r = h.remap(img32);
    ok(r.data instanceof Uint32Array && r.channels === 1, `${name}: class of the result`);
    const g = make({});
    const w = g.warp(null, false, true);
    ok(r.width === w.width && r.height === w.height && sameBytes(new Uint8Array(r.data.buffer), new Uint8Array(w.data.buffer, w.data.byteOffset, w.data.length)), `${name}: remap(image as Uint32Array) is the inverse warp`);
    const viaWarp = make({}).remap(img32, { loop: 'warp' }), direct = make({}).warp();
    ok(sameBytes(new Uint8Array(viaWarp.data.buffer), new Uint8Array(direct.data.buffer, direct.data.byteOffset, direct.data.length)), `${name}: {loop: 'warp'} is warp()`);
    const four = make({}).remap(new Uint8Array(img.data.buffer), { channels: 4 });
    ok(four.data instanceof Uint8Array && sameBytes(four.data, new Uint8Array(r.data.buffer)), `${name}: 4 x Uint8 pixels equal 1 x Uint32`);
    const clamped = make({}).remap(img.data, { channels: 4, sampling: 'bilinear' });
    ok(clamped.data instanceof Uint8ClampedArray && clamped.data.length === r.data.length * 4, `${name}: a bilinear Uint8ClampedArray plane`);
}

// ---- every bad plane or option throws a bare string
{
    const h = makers.projective({});
    const good = new Uint8Array(W * H);
    const bad = {
        'an Array': () => h.remap(Array.from(good)),
        'null': () => h.remap(null),
        'a DataView': () => h.remap(new DataView(good.buffer)),
        'an ArrayBuffer': () => h.remap(good.buffer),
        'a short plane': () => h.remap(good.subarray(1)),
        'a long plane': () => h.remap(new Uint8Array(W * H + 1)),
        'a plane of another channel count': () => h.remap(good, { channels: 2 }),
        'channels 0': () => h.remap(good, { channels: 0 }),
        'channels 1.5': () => h.remap(good, { channels: 1.5 }),
        "channels '1'": () => h.remap(good, { channels: '1' }),
        '3-byte pixels': () => h.remap(new Uint8Array(W * H * 3), { channels: 3 }),
        '32-byte pixels': () => h.remap(new Float64Array(W * H * 4), { channels: 4 }),
        'bilinear Int16Array': () => h.remap(new Int16Array(W * H), { sampling: 'bilinear' }),
        'bilinear Float64Array': () => h.remap(new Float64Array(W * H), { sampling: 'bilinear' }),
        'bilinear 5 channels': () => h.remap(new Float32Array(W * H * 5), { channels: 5, sampling: 'bilinear' }),
        "sampling 'cubic'": () => h.remap(good, { sampling: 'cubic' }),
        'sampling 1': () => h.remap(good, { sampling: 1 }),
        "loop 'scatter'": () => h.remap(good, { loop: 'scatter' }),
        'bilinear with a forward loop': () => h.remap(good, { sampling: 'bilinear', loop: 'forward' }),
    };
    take();
    for (const [what, fn] of Object.entries(bad)) {
        const e = thrown(fn);
        ok(typeof e === 'string' && e.startsWith('remap'), `${what} must throw a bare string (${e})`);
    }
    ok(!take().some((t) => t[0].startsWith('remap') || t[0].startsWith('field')), 'a refused remap reaches no field-side entry point');
    ok(h.remap(good, null).data.length > 0 && h.remap(good).channels === 1, 'null options and the defaults');
    const a = makers.affine({});
    ok(typeof thrown(() => a.remap(new Uint8Array(W * H), { sampling: 'bilinear', loop: 'warp' })) === 'string', "bilinear with {loop: 'warp'} on a same-size affine frame (forward) throws");
    const none = new Homography('projective');
    ok(typeof thrown(() => none.remap(good)) === 'string', 'no image: a bare string');
    // stale piecewise matrices: sourceField's rule
    const p = makers.piecewise({});
    p.setSourcePoints(grid.map(([x, y]) => [x * 0.9, y * 0.9]), null, W, H, false);
    ok(typeof thrown(() => p.remap(good)) === 'string', 'stale piecewise matrices must throw a string');
}

// ---- the empty window
{
    const h = new Homography('affine', W, H);
    h.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    h.setDestinyPoints([[0, 5], [10, 5], [20, 5]], false);
    const [, , ow, oh] = h._window();
    ok(!(ow * oh >= 1), `the degenerate destination must give an empty window (${ow} x ${oh})`);
    take();
    for (const [plane, opt] of [[new Uint16Array(W * H), {}], [new Float32Array(W * H * 3), { channels: 3, sampling: 'bilinear' }]]) {
        const r = h.remap(plane, opt);
        ok(r.data instanceof plane.constructor && r.data.length === 0 && r.width === 0 && r.height === 0 && r.channels === (opt.channels || 1), `empty window: ${JSON.stringify(r)}`);
    }
    ok(!take().some((t) => t[0].startsWith('remap')), 'an empty window reaches no remap entry point');
    ok(typeof thrown(() => h.remap(new Uint16Array(3))) === 'string', 'empty window: a wrong length still throws');
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length ? 1 : 0);
