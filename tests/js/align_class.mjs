// CPU: refineAlignment(fromImages, toImages, matrices, options) of the drop-in class over tests/js/mock_align_addon.cjs (run with
// HGWARP_ADDON pointing at it): the option defaults; the pictures packed plane after plane; the level walk -- begin, then per level from the
// coarsest down: the matrices converted to the level, the level's call with the level's rectangle, the result converted back --, its
// matrices and its end (also after a throw); the shape of the result; the bare strings thrown; no image is needed and the state the
// reference can see is the same after a call.  Prints one JSON line {ok, fails, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const visible = (h) => JSON.stringify([h._map === null ? null : h._map.kind, h._pm === null || h._pm === undefined ? null : 1, h._lastPath, h._image === null,
                                       h._srcPoints === null ? null : Array.from(h._srcPoints), h._dstPoints === null ? null : Array.from(h._dstPoints), h._sampling]);
const since = (n) => addon.alignCalls.slice(n);

const W = 24, H = 20, TW = 40, TH = 36;
const img = (w, h, ch, seed) => Uint8Array.from({ length: w * h * ch }, (_, i) => (i * 7 + seed) & 255);
const f0 = img(W, H, 4, 1), f1 = new Uint8ClampedArray(img(W, H, 4, 2)), t0 = img(TW, TH, 4, 3);
const mats = Float64Array.from([1, 0, 8, 0, 1, 4, 0, 0, 1, 0, -2, 0, 1, 6, 0, 0]);

// ---- defaults: one level, one call, no conversion
const h = new Homography('projective', 64, 48);
const before = visible(h);
let n = addon.alignCalls.length;
const n0 = addon.trace.length;
const r = h.refineAlignment([f0, f1], [t0], mats, { width: W, height: H, toWidth: TW, toHeight: TH });
ok(visible(h) === before, 'refineAlignment changed the state of the instance');
let calls = since(n);
ok(calls.map((c) => c.fn).join() === 'alignBegin,alignLevel,alignEnd', `levels 1: the calls ${calls.map((c) => c.fn)}`);
ok(addon.trace.slice(n0).filter((t) => t[0] !== 'create').length === 3, 'no other addon call (besides the context)');
let b = calls[0], l = calls[1];
ok(b.Wf === W && b.Hf === H && b.F === 2 && b.Wt === TW && b.Ht === TH && b.S === 1 && b.channels === 4 && b.levels === 1, `begin: ${JSON.stringify([b.Wf, b.Hf, b.F, b.Wt, b.Ht, b.S, b.channels, b.levels])}`);
ok(b.from.length === 2 * W * H * 4 && b.from.slice(0, W * H * 4).every((v, i) => v === f0[i]) && b.from.slice(W * H * 4).every((v, i) => v === f1[i]), 'the FROM pictures, plane after plane');
ok(b.to.length === TW * TH * 4 && b.to.every((v, i) => v === t0[i]), 'the TO picture');
ok(l.kind === 1 && l.level === 0 && l.step === 2 && l.photometric === 1 && l.nIter === 10 && l.eps === 0.01 && l.minValid === 10, `defaults: ${JSON.stringify([l.kind, l.level, l.step, l.photometric, l.nIter, l.eps, l.minValid])}`);
ok(l.rect.join() === [0, 0, W, H].join(), `default rect: ${l.rect}`);
ok(l.matrices.join() === mats.join() && l.job === b.job && calls[2].job === b.job, 'the matrices as they stand; one job from begin to end');
// ---- the result
ok(Object.keys(r).sort().join() === 'gains,matrices,rms,status,updates', `keys: ${Object.keys(r)}`);
ok(r.matrices instanceof Float64Array && r.matrices.length === 16 && r.matrices[2] === 8.5 && r.matrices[10] === -1.5, 'matrices: what level 0 returned');
ok(r.status instanceof Int32Array && r.status.join() === '0,0' && r.updates instanceof Int32Array && r.updates.join() === '1,2', 'status / updates');
ok(r.rms instanceof Float64Array && r.rms.join() === '0.5,1.5' && r.gains instanceof Float64Array && r.gains.join() === '1,0,2,-1', `rms (the last) / gains: ${r.rms} / ${r.gains}`);
// ---- explicit options
n = addon.alignCalls.length;
h.refineAlignment([img(W, H, 1, 5)], [img(W, H, 1, 6)], [[1, 0, 0, 1, 3, 2, 0, 0]], { width: W, height: H, channels: 1, transform: 'affine', rect: [2, 3, 10, 9], step: 1, iterations: 0, eps: 0,
                                                                                       photometric: false, minValid: 50 });
calls = since(n);
b = calls[0]; l = calls[1];
ok(b.Wt === W && b.Ht === H && b.channels === 1 && b.S === 1, 'toWidth / toHeight default to width / height');
ok(l.kind === 0 && l.step === 1 && l.photometric === 0 && l.nIter === 0 && l.eps === 0 && l.minValid === 50 && l.rect.join() === '2,3,10,9', 'explicit options reach the addon');
ok(l.matrices.join() === '1,0,0,1,3,2,0,0', 'nested matrices are flattened');
h.refineAlignment([img(W, H, 4, 5)], [img(W, H, 4, 6)], [1, 0, 0, 1, 3, 2, 0, 0], { width: W, height: H, transform: 'affine', photometric: false });
ok(since(n).filter((c) => c.fn === 'alignLevel')[1].minValid === 6, 'minValid defaults to the number of parameters: 6');
h.refineAlignment([img(W, H, 4, 5)], [img(W, H, 4, 6)], mats.slice(0, 8), { width: W, height: H, photometric: false });
ok(since(n).filter((c) => c.fn === 'alignLevel')[2].minValid === 8, '... 8 projective');
n = addon.alignCalls.length;
const e0 = h.refineAlignment([], [], [], { width: W, height: H });
ok(e0.matrices.length === 0 && e0.status.length === 0 && since(n).length === 0, 'no frames: no addon call');

// ---- the level walk: 3 levels, pure translations (8, 4) and (-2, 6): a level halves them, the mock adds 0.5 to x at every level
n = addon.alignCalls.length;
const r3 = h.refineAlignment([f0, f1], [t0], mats, { width: W, height: H, toWidth: TW, toHeight: TH, levels: 3, rect: [3, 2, 18, 15], step: 1 });
calls = since(n);
ok(calls.map((c) => c.fn + (c.level !== undefined ? c.level : c.levelIn !== undefined ? c.levelIn + '>' + c.levelOut : '')).join() ===
   'alignBegin,alignScaleMatrix0>2,alignLevel2,alignScaleMatrix2>0,alignScaleMatrix0>1,alignLevel1,alignScaleMatrix1>0,alignLevel0,alignEnd', `the walk: ${calls.map((c) => c.fn)}`);
ok(calls[0].levels === 3, 'begin is told the levels');
const lv = calls.filter((c) => c.fn === 'alignLevel');
// x_k = (x_0 + 0.5) / 2^k - 0.5: a translation t becomes t / 2^k
ok(lv[0].matrices[2] === 2 && lv[0].matrices[5] === 1 && lv[0].matrices[10] === -0.5 && lv[0].matrices[13] === 1.5, `level 2 gets the matrices at level 2: ${lv[0].matrices}`);
ok(lv[1].matrices[2] === 5 && lv[1].matrices[5] === 2 && lv[1].matrices[10] === 0, `level 1 gets level 2's result at level 1 ((2 + 0.5) * 2 = 5): ${lv[1].matrices}`);
ok(lv[2].matrices[2] === 11 && lv[2].matrices[5] === 4 && lv[2].matrices[10] === 1, `level 0 gets level 1's result at level 0 ((5 + 0.5) * 2 = 11): ${lv[2].matrices}`);
ok(r3.matrices[2] === 11.5 && r3.matrices[10] === 1.5 && r3.status.join() === '0,0', 'the result is level 0\'s');
ok([0, 1, 3, 4, 6, 7, 8, 9, 11, 12, 14, 15].every((k) => lv[0].matrices[k] === mats[k] && r3.matrices[k] === mats[k]), 'a translation stays a translation');
// the rectangles: the level's pixels whose centres lie inside [3, 20] x [2, 16]
ok(lv[2].rect.join() === '3,2,18,15', `level 0 rect ${lv[2].rect}`);
ok(lv[1].rect.join() === '2,1,8,7', `level 1 rect ${lv[1].rect} (centres 2 k + 0.5: x 2..9, y 1..7 at level 1)`);
ok(lv[0].rect.join() === '1,1,4,3', `level 2 rect ${lv[0].rect} (centres 4 k + 1.5: x 1..4, y 1..3 at level 2)`);
ok(lv.every((c) => c.step === 1 && c.nIter === 10 && c.job === calls[0].job), 'the same step and iterations at every level, one job');
// a NaN row (a failed frame of the fit) passes through the conversions untouched
n = addon.alignCalls.length;
const nanMats = Float64Array.from(mats); nanMats.fill(NaN, 8);
h.refineAlignment([f0, f1], [t0], nanMats, { width: W, height: H, toWidth: TW, toHeight: TH, levels: 2 });
ok(since(n).filter((c) => c.fn === 'alignLevel')[0].matrices.slice(8).every(Number.isNaN), 'a NaN matrix reaches the level as NaN');
// the job ends when a level throws
n = addon.alignCalls.length;
const realLevel = addon.alignLevel;
addon.alignLevel = () => { throw ('boom'); };
const hb = new Homography('projective', 64, 48);
hb._native.alignLevel = addon.alignLevel;
const eb = thrown(() => hb.refineAlignment([f0], [t0], mats.slice(0, 8), { width: W, height: H, toWidth: TW, toHeight: TH }));
addon.alignLevel = realLevel;
hb._native.alignLevel = realLevel;
ok(eb === 'boom' && since(n).map((c) => c.fn).join() === 'alignBegin,alignEnd', `a throwing level still ends the job: ${since(n).map((c) => c.fn)}`);

// ---- the thrown strings
const n1 = addon.alignCalls.length;
const good = { width: W, height: H, toWidth: TW, toHeight: TH };
const call = (o, fr = [f0], to = [t0], m = mats.slice(0, 8)) => () => h.refineAlignment(fr, to, m, Object.assign({}, good, o));
const refusals = [
    [call({ transform: 'piecewiseaffine' }), 'transform'], [call({ transform: 1 }), 'transform'],
    [call({ width: 0 }), 'width'], [call({ height: 1.5 }), 'height'], [call({ width: undefined }), 'width'], [call({ toWidth: -1 }), 'toWidth'], [call({ toHeight: 40000 }), 'toHeight'],
    [call({ channels: 3 }), 'channels'], [call({ step: 0 }), 'step'], [call({ step: 65 }), 'step'], [call({ iterations: -1 }), 'iterations'], [call({ iterations: 65 }), 'iterations'],
    [call({ eps: -1 }), 'eps'], [call({ eps: NaN }), 'eps'], [call({ eps: '0.01' }), 'eps'], [call({ minValid: 9 }), 'minValid'], [call({ minValid: 1.5 }), 'minValid'],
    [call({ levels: 0 }), 'levels'], [call({ levels: 7 }), 'levels'], [call({ levels: 1.5 }), 'levels'],
    [call({ rect: [0, 0, W + 1, H] }), 'rect'], [call({ rect: [0, 0, 0, H] }), 'rect'], [call({ rect: [-1, 0, 4, 4] }), 'rect'], [call({ rect: [0, 0, 4] }), 'rect'],
    [call({}, 'x'), 'fromImages'], [call({}, [f0], 'x'), 'toImages'], [call({}, [f0], []), 'toImages'], [call({}, [f0], [t0, t0]), 'toImages'],
    [call({}, [f0.slice(1)]), 'fromImages 0'], [call({}, [f0, [1, 2]], [t0], mats), 'fromImages 1'], [call({}, [f0], [f0]), 'toImages 0'],
    [call({}, [f0], [t0], mats), 'matrices'], [call({}, [f0], [t0], 'x'), 'matrices'],
];
for (const [fn, word] of refusals) {
    const e = thrown(fn);
    ok(typeof e === 'string' && e.startsWith('refineAlignment:') && e.includes(word), `a refusal must be a bare string of refineAlignment naming ${word} (got ${e})`);
}
ok(addon.alignCalls.length === n1, 'a refused call reaches no addon function');
ok(visible(h) === before, 'the state of the instance after all of it');

const res = { ok: fails.length === 0, fails, checks };
console.log(JSON.stringify(res));
process.exit(res.ok ? 0 : 1);
