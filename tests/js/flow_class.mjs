// CPU: denseFlow(fromImages, toImages, options) of the drop-in class over tests/js/mock_flow_addon.cjs (run with HGWARP_ADDON pointing at
// it): the pictures go down packed, the option defaults (levels from the size, 4 iterations, radius 3, minEig 1, maxUpdate 1), the flags of
// what comes down, the bare strings thrown, the shape of the result; the state the reference can see is the same after a call.  Prints one
// JSON line {ok, fails, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const last = () => addon.flowCalls[addon.flowCalls.length - 1];
const visible = (h) => JSON.stringify([h._map === null ? null : h._map.kind, h._lastPath, h._image === null, h._srcPoints === null ? null : Array.from(h._srcPoints),
                                       h._dstPoints === null ? null : Array.from(h._dstPoints), h._sampling, h._width, h._height]);
const plane = (n, base) => Uint8Array.from({ length: n }, (_, i) => (base + i * 5) & 255);

const h = new Homography('piecewiseaffine', 12, 10);
const before = visible(h);
const n0 = addon.trace.length;
const W = 40, H = 33;

// ---- defaults: RGBA, the field comes down, nothing else
let r = h.denseFlow([plane(W * H * 4, 1), plane(W * H * 4, 2), plane(W * H * 4, 3)], [plane(W * H * 4, 9)], { width: W, height: H });
ok(visible(h) === before, 'denseFlow changed the state of the instance');
ok(addon.flowCalls.length === 1 && addon.trace.slice(n0).filter((x) => x[0] === 'denseFlow').length === 1, 'exactly one flow call');
let k = last();
ok(k.W === W && k.H === H && k.channels === 4 && k.nFrames === 3 && k.nToSets === 1, `shape: ${k.W} ${k.H} ${k.channels} ${k.nFrames} ${k.nToSets}`);
ok(k.levels === 2 && k.iterations === 4 && k.radius === 3 && k.minEig === 1 && k.maxUpdate === 1, `defaults: ${k.levels} ${k.iterations} ${k.radius} ${k.minEig} ${k.maxUpdate}`);
ok(k.flags === 1, `flags ${k.flags}`);
ok(k.from.length === 3 * W * H * 4 && k.from[0] === 1 && k.from[W * H * 4] === 2 && k.from[2 * W * H * 4 + 1] === 8 && k.to[0] === 9, 'the pictures go down packed, in order');
ok(Object.keys(r).sort().join() === 'field,frames,height,width', `keys: ${Object.keys(r)}`);
ok(r.field instanceof Float32Array && r.field.length === 3 * W * H * 2 && r.width === W && r.height === H && r.frames === 3 && r.field[8] === 2, 'the field');

// ---- the default levels: the coarsest level keeps 16 pixels on its shorter side
for (const [w, hh, want] of [[1920, 1080, 7], [3840, 2160, 8], [160, 224, 4], [31, 400, 2], [15, 400, 1], [1, 1, 1]]) {
    if (w * hh > 40000) continue;                                     // (the mock allocates what it returns)
    h.denseFlow([plane(w * hh, 1)], [plane(w * hh, 1)], { width: w, height: hh, channels: 1 });
    ok(last().levels === want, `default levels of ${w} x ${hh}: ${last().levels}`);
}

// ---- every option, grey planes, two TO pictures
r = h.denseFlow([plane(W * H, 1), plane(W * H, 2)], [plane(W * H, 3), new Uint8ClampedArray(W * H)],
                { width: W, height: H, channels: 1, levels: 6, iterations: 32, radius: 7, minEig: 0, maxUpdate: 4, residual: true, good: true });
k = last();
ok(k.channels === 1 && k.nToSets === 2 && k.levels === 6 && k.iterations === 32 && k.radius === 7 && k.minEig === 0 && k.maxUpdate === 4 && k.flags === 7, `options: ${JSON.stringify(k, (n, v) => (ArrayBuffer.isView(v) ? undefined : v))}`);
ok(Object.keys(r).sort().join() === 'field,frames,good,height,residual,width', `keys: ${Object.keys(r)}`);
ok(r.residual instanceof Uint8Array && r.residual.length === 2 * W * H && r.good.length === 2 * W * H && r.good[1] === 1, 'residual and good');

// ---- warp: the pictures come down, the field only if asked for
r = h.denseFlow([plane(W * H, 1), plane(W * H, 2)], [plane(W * H, 3)], { width: W, height: H, channels: 1, warp: true });
ok(last().flags === 8 && r.field === null, `warp alone: flags ${last().flags}`);
ok(Array.isArray(r.images) && r.images.length === 2 && r.images[1] instanceof Uint8Array && r.images[1].length === W * H && r.images[1][0] === ((W * H * 3) & 255), 'one picture per frame');
r = h.denseFlow([plane(W * H, 1)], [plane(W * H, 3)], { width: W, height: H, channels: 1, warp: true, field: true, good: true });
ok(last().flags === 13 && r.field instanceof Float32Array && r.images.length === 1 && r.good.length === W * H && !('residual' in r), `warp with the field: flags ${last().flags}`);
r = h.denseFlow([plane(W * H, 1)], [plane(W * H, 3)], { width: W, height: H, channels: 1, field: false, residual: true });
ok(last().flags === 2 && r.field === null && r.residual.length === W * H, 'the residual alone');

// ---- an empty set
r = h.denseFlow([], [plane(W * H, 3)], { width: W, height: H, channels: 1 });
ok(r.frames === 0 && r.field.length === 0 && last().nFrames === 0 && last().nToSets === 1, 'an empty set');

// ---- bare strings
const f1 = [plane(W * H, 1)], t1 = [plane(W * H, 3)], o1 = { width: W, height: H, channels: 1 };
const calls = addon.flowCalls.length;
for (const [fn, word] of [
    [() => h.denseFlow(f1, t1), 'options.width'],
    [() => h.denseFlow(f1, t1, { width: 0, height: H }), 'options.width'],
    [() => h.denseFlow(f1, t1, { width: W, height: 32769 }), 'options.width'],
    [() => h.denseFlow(f1, t1, { ...o1, channels: 3 }), 'options.channels'],
    [() => h.denseFlow(f1, t1, { ...o1, levels: 0 }), 'options.levels'],
    [() => h.denseFlow(f1, t1, { ...o1, levels: 8 }), 'options.levels'],
    [() => h.denseFlow(f1, t1, { ...o1, iterations: 0 }), 'options.iterations'],
    [() => h.denseFlow(f1, t1, { ...o1, iterations: 33 }), 'options.iterations'],
    [() => h.denseFlow(f1, t1, { ...o1, radius: 8 }), 'options.radius'],
    [() => h.denseFlow(f1, t1, { ...o1, radius: 1.5 }), 'options.radius'],
    [() => h.denseFlow(f1, t1, { ...o1, minEig: -1 }), 'options.minEig'],
    [() => h.denseFlow(f1, t1, { ...o1, minEig: NaN }), 'options.minEig'],
    [() => h.denseFlow(f1, t1, { ...o1, maxUpdate: 0 }), 'options.maxUpdate'],
    [() => h.denseFlow(f1, t1, { ...o1, maxUpdate: 4.5 }), 'options.maxUpdate'],
    [() => h.denseFlow('pictures', t1, o1), 'fromImages must be an array'],
    [() => h.denseFlow(f1, 7, o1), 'toImages must be an array'],
    [() => h.denseFlow([[1, 2, 3]], t1, o1), 'fromImages[0] must be a Uint8Array'],
    [() => h.denseFlow([plane(W * H - 1, 1)], t1, o1), 'fromImages[0] must hold'],
    [() => h.denseFlow(f1, [plane(W * H * 4, 1)], o1), 'toImages[0] must hold'],
    [() => h.denseFlow(f1, [], o1), 'toImages must hold between'],
    [() => h.denseFlow(f1, [t1[0], t1[0]], o1), 'toImages must hold between'],
]) {
    const e = thrown(fn);
    ok(typeof e === 'string' && e.includes(word), `expected a bare string with "${word}", got ${String(e)}`);
}
ok(addon.flowCalls.length === calls, 'a refused call reaches the addon');
ok(visible(h) === before, 'the state of the instance after all calls');

console.log(JSON.stringify({ ok: fails.length === 0, fails, checks }));
process.exit(fails.length === 0 ? 0 : 1);
