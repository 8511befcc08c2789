// CPU: transformPoints(points, {to}) of the drop-in class over tests/js/mock_points_addon.cjs (run with HGWARP_ADDON pointing at it): for
// every transform and direction it makes the field-side addon calls sourceField() makes for loop 'forward' ('output') resp. 'inverse'
// ('source'), with the same arguments -- 'points' + entry in place of 'field' + entry, the list behind them; the stale-state refusals and
// repairStaleMap are sourceField's; a bad `to` or list throws a bare string; an empty window gives all NaN and no addon call; the state the
// reference can see is the same after a call.  Prints one JSON line {ok, fails, checks}.
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
const pairs = [[1, 2], [3.5, 4.25], [-0.5, 7], [NaN, 1]];
const flat = Float32Array.from(pairs.flat());
const visible = (h) => JSON.stringify([h._map === null ? null : [h._map.kind, Array.from(h._map.pts), h._map.width, h._map.height, h._map.yOff],
                                       h._pm === null || h._pm === undefined ? null : [Array.from(h._pm.src), Array.from(h._pm.dst)], h._lastPath]);

// ---- entry and arguments for each `to` x transform: sourceField's, the list behind them
for (const [name, make] of Object.entries(makers)) {
    for (const to of ['output', 'source', undefined]) {
        const what = `${name} ${to}`;
        const loop = to === 'source' ? 'inverse' : 'forward', fmt = to === 'source' ? 'coords' : 'index';
        take();
        const a = make({});
        const eField = thrown(() => a.sourceField(fmt, { loop }));
        const tField = take();
        const b = make({});
        const before = visible(b);
        let r;
        const ePts = thrown(() => { r = b.transformPoints(to === 'source' ? flat : pairs, to === undefined ? undefined : { to }); });
        const tPts = take();
        ok((eField === undefined) === (ePts === undefined), `${what}: sourceField threw ${eField}, transformPoints threw ${ePts}`);
        if (ePts !== undefined) { ok(typeof ePts === 'string' && ePts.startsWith('transformPoints'), `${what}: a refusal must be a bare string of transformPoints' (${ePts})`); continue; }
        ok(tField.length === tPts.length && tField.length >= 2, `${what}: call counts ${tField.map((t) => t[0])} / ${tPts.map((t) => t[0])}`);
        tField.forEach((t, i) => {
            const u = tPts[i] || [];
            ok(t[0].replace(/^field/, 'points') === String(u[0]).replace(/^field/, 'points') && t[1] === u[1], `${what}: call ${i}: ${t[0]} / ${u[0]} or their arguments differ`);
        });
        const last = tPts[tPts.length - 1];
        const kindName = name === 'piecewise' ? 'Piecewise' : 'Geometric';
        ok(last[0] === 'points' + (to === 'source' ? 'Inverse' : 'Forward') + kindName, `${what}: the entry ${last[0]}`);
        ok(last[2] === 'Float32Array' && last[3] === flat.length, `${what}: the list's part of the call ${last}`);
        ok(tPts.filter((t) => t[0].startsWith('field') || t[0].startsWith('remap') || t[0].startsWith('points')).length === 1, `${what}: one native geometry entry`);
        ok(r instanceof Float32Array && r.length === flat.length && r[0] === 1001 && r[3] === 1004.25, `${what}: the result is the addon's, a Float32Array of the list's length`);
        ok(visible(b) === before && b._lastPath === null, `${what}: transformPoints() must leave the state the reference can see alone`);
        a.close(); b.close();
    }
}

// ---- stale state: sourceField's refusals, and repairStaleMap
{
    const p = makers.piecewise({});
    p.warp(null, false, true);                                // the map field now holds the INVERSE map
    ok(typeof thrown(() => p.sourceField('index', { loop: 'forward' })) === 'string', 'premise: a forward field over a stale map is refused');
    const e = thrown(() => p.transformPoints(flat));
    ok(typeof e === 'string' && e.startsWith('transformPoints'), `to 'output' over a stale map must throw a string (${e})`);
    ok(p.transformPoints(flat, { to: 'source' }).length === flat.length, "to 'source' does not read the map field");
    const q = makers.piecewise({ repairStaleMap: true });
    q.warp(null, false, true);
    take();
    ok(q.transformPoints(flat).length === flat.length && take().some((t) => t[0] === 'pointsForwardPiecewise'), 'repairStaleMap: the forward form runs');
    const s = makers.piecewise({});
    s.setSourcePoints(grid.map(([x, y]) => [x * 0.9, y * 0.9]), null, W, H, false);
    for (const to of ['output', 'source']) ok(typeof thrown(() => s.transformPoints(flat, { to })) === 'string', `stale piecewise matrices, to '${to}': a string`);
    const t = makers.piecewise({ repairStaleMap: true });
    t.setSourcePoints(grid.map(([x, y]) => [x * 0.9, y * 0.9]), null, W, H, false);
    for (const to of ['output', 'source']) ok(t.transformPoints(flat, { to }).length === flat.length, `repairStaleMap with stale matrices, to '${to}'`);
}

// ---- bad arguments throw bare strings and reach no entry point
{
    const h = makers.projective({});
    const bad = {
        "to 'input'": () => h.transformPoints(flat, { to: 'input' }),
        'to 1': () => h.transformPoints(flat, { to: 1 }),
        'to null': () => h.transformPoints(flat, { to: null }),
        'an odd list': () => h.transformPoints(new Float32Array(3)),
        'a Float64Array': () => h.transformPoints(new Float64Array(4)),
        'null': () => h.transformPoints(null),
    };
    take();
    for (const [what, fn] of Object.entries(bad)) {
        const e = thrown(fn);
        ok(typeof e === 'string' && e.startsWith('transformPoints'), `${what} must throw a bare string (${e})`);
    }
    ok(!take().some((t) => t[0].startsWith('points')), 'a refused call reaches no points entry point');
    ok(h.transformPoints(flat, null).length === flat.length, 'null options');
    ok(h.transformPoints([]).length === 0 && h.transformPoints(new Float32Array(0), { to: 'source' }).length === 0, 'an empty list');
    const none = new Homography('projective');
    const e = thrown(() => none.transformPoints(flat));
    ok(typeof e === 'string' && e.startsWith('transformPoints'), `no image: a bare string (${e})`);
}

// ---- the empty window: all NaN, no addon call
{
    const h = new Homography('affine', W, H);
    h.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    h.setDestinyPoints([[0, 5], [10, 5], [20, 5]], false);
    const [, , ow, oh] = h._window();
    ok(!(ow * oh >= 1), `the degenerate destination must give an empty window (${ow} x ${oh})`);
    take();
    for (const to of ['output', 'source']) {
        const r = h.transformPoints(flat, { to });
        ok(r instanceof Float32Array && r.length === flat.length && r.every((v) => Number.isNaN(v)), `empty window, to '${to}': all NaN`);
        ok(new Uint32Array(r.buffer).every((v) => v === 0x7fc00000), `empty window, to '${to}': the quiet NaN pattern`);
    }
    ok(!take().some((t) => t[0].startsWith('points')), 'an empty window reaches no points entry point');
}
console.log(JSON.stringify({ ok: fails.length === 0, fails, checks }));
process.exit(fails.length ? 1 : 0);
