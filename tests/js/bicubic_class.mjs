// CPU: remap(plane, {sampling: 'bicubic'}) of the drop-in class over tests/js/mock_bicubic_addon.cjs (run with HGWARP_ADDON pointing at it):
// it makes the native calls {sampling: 'bilinear'} makes, with the same arguments, except that the last one goes to 'remapBicubic' + entry
// with B and C appended (Catmull-Rom by default; the three preset names; an array); a bad `cubic` and everything 'bilinear' refuses throw
// bare strings, forward loops included, and reach no entry point; 'cubic' keeps throwing; the calls of 'nearest', 'bilinear', 'trilinear'
// and 'anisotropic' are what they were.  Prints one JSON line {failures, checks}.
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
const W = 32, H = 20, nx = 4, ny = 4;
const img = { data: new Uint8ClampedArray(W * H * 4).fill(9), width: W, height: H };
Homography.triangulate = () => gridTriangles(nx, ny);
const grid = [];
for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
const large = grid.map(([x, y]) => [x * 3 + 2, y * 3 + 1]);          // a 3x enlargement: every warp of it takes the inverse loop
const makers = {
    affine: () => { const h = new Homography('affine', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false); h.setDestinyPoints([[2, 1], [W * 3 + 2, 1], [2, H * 3 + 1]], false); return h; },
    projective: () => { const h = new Homography('projective', W, H); h.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false); h.setDestinyPoints([[1, 0], [W * 3, 2], [0, H * 3], [W * 3 - 1, H * 3 + 1]], false); return h; },
    piecewise: () => { const h = new Homography('piecewiseaffine', W, H); h.setSourcePoints(grid, img, W, H, false); h.setDestinyPoints(large, false); return h; },
};
const entryOf = { affine: 'InverseGeometric', projective: 'InverseGeometric', piecewise: 'InversePiecewise' };

// ---- the entry chosen and its arguments: those of 'bilinear', the name apart, then B and C
for (const [name, make] of Object.entries(makers)) {
    for (const loop of ['inverse', 'warp']) {
        for (const [Cls, channels, cubic, want] of [[Float32Array, 1, undefined, [0, 0.5]], [Uint8Array, 4, 'catmull-rom', [0, 0.5]], [Uint8ClampedArray, 3, 'mitchell', [1 / 3, 1 / 3]],
                                                    [Float32Array, 2, 'b-spline', [1, 0]], [Uint8Array, 1, [0.37, 0.81], [0.37, 0.81]], [Uint8Array, 2, [0, 0], [0, 0]], [Float32Array, 4, [1, 1], [1, 1]]]) {
            const what = `${name} ${loop} ${Cls.name} x ${channels} cubic ${JSON.stringify(cubic)}`;
            take();
            const a = make(), b = make();
            const rb = a.remap(new Cls(W * H * channels), { channels, sampling: 'bilinear', loop });
            const tb = take();
            const rc = b.remap(new Cls(W * H * channels), cubic === undefined ? { channels, sampling: 'bicubic', loop } : { channels, sampling: 'bicubic', loop, cubic });
            const tc = take();
            ok(tb.length === tc.length && tc.length >= 2, `${what}: call counts ${tb.map((t) => t[0])} / ${tc.map((t) => t[0])}`);
            tb.slice(0, -1).forEach((t, i) => ok(JSON.stringify(t) === JSON.stringify(tc[i]), `${what}: call ${i} differs: ${t[0]} / ${(tc[i] || [])[0]}`));
            const lb = tb[tb.length - 1], lc = tc[tc.length - 1];
            ok(lb[0] === 'remap' + entryOf[name] && lc[0] === 'remapBicubic' + entryOf[name], `${what}: entries ${lb[0]} / ${lc[0]}`);
            ok(JSON.stringify(lb.slice(1)) === JSON.stringify(lc.slice(1, 6)), `${what}: the arguments behind the entry differ`);
            ok(lc.length === 8 && lc[6] === want[0] && lc[7] === want[1], `${what}: B and C reach the addon as ${lc[6]}, ${lc[7]}`);
            ok(lc[2] === Cls.name && lc[3] === channels && lc[4] === W && lc[5] === H, `${what}: the plane's part of the call ${lc.slice(2)}`);
            ok(tc.filter((t) => t[0].startsWith('remap') || t[0].startsWith('field')).length === 1, `${what}: one native field-side entry`);
            ok(rc.data instanceof Cls && rc.channels === channels && rc.width === rb.width && rc.height === rb.height && rc.data.length === rc.width * rc.height * channels && rc.data.length > 0, `${what}: result shape`);
            ok(b._lastPath === null, `${what}: remap() must not record a path`);
            a.close(); b.close();
        }
    }
}

// ---- a bad cubic, the refusals of 'bilinear', forward loops included; 'cubic' keeps throwing
{
    const h = makers.projective();
    const good = new Uint8Array(W * H);
    const bad = [];                                           // [label, fn] pairs: labels may repeat (JSON.stringify gives NaN and Infinity alike), cases may not get lost
    const badCubics = ['lanczos', [0.5], [2, 0], [NaN, 0], null, 7, [0, -0.1], [0, 0.5, 1], ['0', '0.5'], 'Mitchell', [Infinity, 0], [0, NaN], [-Infinity, 0], NaN, {}, 'toString', [], [[0, 0.5]], true];
    badCubics.forEach((v, n) => bad.push([`cubic #${n} ${Array.isArray(v) ? '[' + v.map(String).join(', ') + ']' : String(v)} (${typeof v})`, () => h.remap(good, { sampling: 'bicubic', cubic: v })]));
    const refusedByBilinear = {
        'an Array': (sampling) => h.remap(Array.from(good), { sampling }),
        'a DataView': (sampling) => h.remap(new DataView(good.buffer), { sampling }),
        'a short plane': (sampling) => h.remap(good.subarray(1), { sampling }),
        'a plane of another channel count': (sampling) => h.remap(good, { channels: 2, sampling }),
        'channels 0': (sampling) => h.remap(good, { channels: 0, sampling }),
        'Int16Array': (sampling) => h.remap(new Int16Array(W * H), { sampling }),
        'Float64Array': (sampling) => h.remap(new Float64Array(W * H), { sampling }),
        '5 channels': (sampling) => h.remap(new Float32Array(W * H * 5), { channels: 5, sampling }),
        'a forward loop': (sampling) => h.remap(good, { sampling, loop: 'forward' }),
        "loop 'scatter'": (sampling) => h.remap(good, { sampling, loop: 'scatter' }),
    };
    for (const [what, fn] of Object.entries(refusedByBilinear)) {
        ok(typeof thrown(() => fn('bilinear')) === 'string', `the premise: 'bilinear' refuses ${what}`);
        bad.push([what, () => fn('bicubic')]);
    }
    bad.push(["sampling 'cubic'", () => h.remap(good, { sampling: 'cubic' })]);
    bad.push(["sampling 'Bicubic'", () => h.remap(good, { sampling: 'Bicubic' })]);
    ok(bad.length === badCubics.length + Object.keys(refusedByBilinear).length + 2 && badCubics.length === 19 && badCubics.some((v) => Array.isArray(v) && Number.isNaN(v[0])),
        `every listed refusal is a case of its own (${bad.length})`);
    take();
    let ran = 0, named = 0;
    for (const [what, fn] of bad) {
        const e = thrown(fn);
        ran++;
        ok(typeof e === 'string' && e.startsWith('remap'), `${what} must throw a bare string (${e})`);
        if (what.startsWith('cubic #')) { named++; ok(String(e).includes('cubic'), `${what}: the refusal names the option (${e})`); }
    }
    ok(ran === bad.length && named === badCubics.length, `as many refusals ran as were listed (${ran} of ${bad.length}, ${named} of ${badCubics.length} bad cubics)`);
    ok(!take().some((t) => t[0].startsWith('remap') || t[0].startsWith('field')), 'a refused remap reaches no field-side entry point');
    ok(String(thrown(() => h.remap(good, { sampling: 'cubic' }))).includes("'bicubic'"), 'the sampling refusal lists bicubic');
    // the other samplings do not look at cubic
    for (const sampling of ['nearest', 'bilinear', 'trilinear', 'anisotropic']) ok(thrown(() => h.remap(good, { sampling, cubic: 'lanczos' })) === undefined, `'${sampling}' ignores cubic`);
    take();
    // a same-size affine frame dispatches forward: {loop: 'warp'} refuses 'bicubic' as it refuses 'bilinear', with the same string
    const s = new Homography('affine', W, H);
    s.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    s.setDestinyPoints([[5, 3], [W + 5, 3], [5, H + 3]], false);
    const eb = thrown(() => s.remap(good, { sampling: 'bilinear', loop: 'warp' })), ec = thrown(() => s.remap(good, { sampling: 'bicubic', loop: 'warp' }));
    ok(typeof eb === 'string' && eb === ec, `a forward dispatch refuses both alike (${eb} / ${ec})`);
    const ef = thrown(() => h.remap(good, { sampling: 'bilinear', loop: 'forward' })), eg = thrown(() => h.remap(good, { sampling: 'bicubic', loop: 'forward' }));
    ok(typeof ef === 'string' && ef === eg, `a forward loop refuses both alike (${ef} / ${eg})`);
    ok(!take().some((t) => t[0].startsWith('remap') || t[0].startsWith('field')), 'a refused loop reaches no field-side entry point');
    ok(typeof thrown(() => new Homography('projective').remap(good, { sampling: 'bicubic' })) === 'string', 'no image: a bare string');
    const none = new Homography('affine', W, H);
    none.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    none.setDestinyPoints([[0, 5], [10, 5], [20, 5]], false);
    take();
    const r = none.remap(new Float32Array(W * H * 3), { channels: 3, sampling: 'bicubic' });
    ok(r.data instanceof Float32Array && r.data.length === 0 && r.width === 0 && r.height === 0 && r.channels === 3, `empty window: ${JSON.stringify(r)}`);
    ok(!take().some((t) => t[0].startsWith('remap')), 'an empty window reaches no remap entry point');
}

// ---- 'nearest', 'bilinear', 'trilinear' and 'anisotropic' call what they called: the entry behind sourceField()'s own calls
for (const [name, make] of Object.entries(makers)) {
    for (const [sampling, fmt, fmtName, prefix, extra] of [['nearest', 0, 'index', 'remap', 0], ['bilinear', 1, 'coords', 'remap', 0], [undefined, 0, 'index', 'remap', 0],
                                                           ['trilinear', 1, 'coords', 'remapTrilinear', 0], ['anisotropic', 1, 'coords', 'remapAniso', 1]]) {
        const what = `${name} ${sampling}`;
        take();
        const a = make();
        a.sourceField(fmtName);
        const tf = take();
        const b = make();
        b.remap(new Uint8Array(W * H * 2), sampling === undefined ? { channels: 2 } : { channels: 2, sampling, cubic: 'mitchell' });
        const tr = take();
        ok(tf.length === tr.length, `${what}: call counts`);
        tf.forEach((t, i) => ok(t[0].replace(/^field/, prefix) === String((tr[i] || [])[0]) && t[1] === (tr[i] || [])[1], `${what}: call ${i}: ${t[0]} / ${(tr[i] || [])[0]}`));
        const last = tr[tr.length - 1], args = JSON.parse(last[1]);
        ok(last[0] === prefix + entryOf[name] && !tr.some((t) => t[0].includes('Bicubic')), `${what}: the entry ${last[0]}`);
        ok(args.length === (name === 'piecewise' ? 1 : 7) && args[args.length - 1] === fmt, `${what}: the field arguments ${last[1].slice(0, 80)}`);
        ok(last[2] === 'Uint8Array' && last[3] === 2 && last[4] === W && last[5] === H && last.length === 6 + extra, `${what}: the plane's part ${last.slice(2)}`);
        if (extra) ok(last[6] === 8, `${what}: maxAniso stays 8`);
        a.close(); b.close();
    }
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length ? 1 : 0);
