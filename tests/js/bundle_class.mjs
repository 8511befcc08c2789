// CPU: bundleAdjust(matrices, pairs, matchSets, options), chainMatrices(pairMatrices, pairs, options) and invertMatrix(m, options) of the
// drop-in class over tests/js/mock_bundle_addon.cjs (run with HGWARP_ADDON pointing at it): the option defaults, how the lists, the masks,
// the pairs and the fixed frames are marshalled, the bare strings thrown, the shape of the results parsed from the info block; no image is
// needed and the state the reference can see is the same after a call.  Prints one JSON line {ok, fails, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const last = () => addon.bundleCalls[addon.bundleCalls.length - 1];
const visible = (h) => JSON.stringify([h._map === null ? null : h._map.kind, h._pm === null || h._pm === undefined ? null : 1, h._lastPath, h._image === null,
                                       h._srcPoints === null ? null : Array.from(h._srcPoints), h._dstPoints === null ? null : Array.from(h._dstPoints), h._sampling]);

const I = [1, 0, 0, 0, 1, 0, 0, 0];
const mats = Float64Array.from([...I, ...I, ...I]);
const a = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]];
const b = Float32Array.from([1.5, 2.5, 3.5, 4.5, NaN, 0, Infinity, 1e30]);
const size = { width: 96, height: 64 };

// ---- defaults, padding, counts, pairs and the fixed frame; no image was ever set
const h = new Homography('projective', 64, 48);
const before = visible(h);
const n0 = addon.trace.length;
const r = h.bundleAdjust(mats, [[0, 1], [2, 1]], [a, b], size);
ok(visible(h) === before, 'bundleAdjust changed the state of the instance');
ok(addon.bundleCalls.length === 1 && addon.trace.slice(n0).filter((t) => t[0] !== 'create').length === 1, 'exactly one addon call (besides the context)');
let k = last();
ok(k.kind === 1 && k.W === 96 && k.H === 64 && k.nIter === 10 && k.eps === 0.01 && k.lambda === 1e-3 && k.huber === 0 && k.mask === null, `defaults: ${JSON.stringify([k.kind, k.nIter, k.eps, k.lambda, k.huber])}`);
ok(k.fixed.join() === '1,0,0' && k.pairs.join() === '0,1,2,1', `fixed ${k.fixed}, pairs ${k.pairs}`);
ok(k.nPoints === 3 && k.counts.join() === '3,2' && k.matches.length === 2 * 3 * 4, `padding: nPoints ${k.nPoints}, counts ${k.counts}`);
ok(Array.from(k.matches.slice(0, 12)).join() === a.flat().join(), 'pair 0: its matches');
ok(k.matches[12] === 1.5 && Object.is(k.matches[16], NaN) && k.matches[18] === Infinity && k.matches.slice(20).every((v) => v === 0), 'pair 1: copied as it stands, then zero padding');
ok(Array.from(k.matrices).join() === Array.from(mats).join(), 'the matrices go down as they are');
// ---- the result
ok(r.matrices instanceof Float64Array && r.matrices.length === 24 && r.matrices[0] === 2 && r.matrices[1] === 1, 'matrices');
ok(r.status === 0 && r.rounds === 3 && r.accepted === 2 && r.rmsFirst === 2.5 && r.rmsLast === 0.5, `the call's record: ${JSON.stringify([r.status, r.rounds, r.accepted, r.rmsFirst, r.rmsLast])}`);
ok(r.frames instanceof Int32Array && Array.from(r.frames).join() === '0,1,2', `frames ${Array.from(r.frames)}`);
ok(Array.isArray(r.pairs) && r.pairs.length === 2 && r.pairs[1].nValidFirst === 11 && r.pairs[1].nValidLast === 6 && r.pairs[1].rmsFirst === 1.5 && r.pairs[1].rmsLast === 1.25 && r.pairs[0].nValidFirst === 10,
   `pairs ${JSON.stringify(r.pairs)}`);
ok(Object.keys(r).sort().join() === 'accepted,frames,matrices,pairs,rmsFirst,rmsLast,rounds,status', `keys: ${Object.keys(r)}`);
// ---- options
const masks = [Uint8Array.from([1, 0, 1]), [0, 1]];
h.bundleAdjust(Array.from(mats), Int32Array.from([0, 1, 1, 2]), [a, b], { ...size, transform: 'affine', fixed: [2, 0], iterations: 0, eps: 0, lambda: 2, huber: 1.5, masks });
k = last();
ok(k.kind === 0 && k.fixed.join() === '1,0,1' && k.nIter === 0 && k.eps === 0 && k.lambda === 2 && k.huber === 1.5 && k.pairs.join() === '0,1,1,2', 'explicit options reach the addon');
ok(k.mask instanceof Uint8Array && Array.from(k.mask).join() === '1,0,1,0,1,0', `masks are padded with zeros: ${k.mask}`);
ok(h.bundleAdjust(mats, [], [], size).pairs.length === 0 && last().counts.length === 0 && last().nPoints === 0, 'no pairs');
const none = h.bundleAdjust([], [], [], size);
ok(none.matrices.length === 0 && none.frames.length === 0 && none.rounds === 0, 'no frames');
ok(h.bundleAdjust(mats, [[0, 1]], [[]], size) && last().nPoints === 0 && last().counts.join() === '0', 'an empty list');
// ---- chainMatrices and invertMatrix
const pm = Float64Array.from([...I, ...I]);
const c = h.chainMatrices(pm, [[0, 1], [2, 1]], { frames: 3 });
k = last();
ok(k.name === 'chain' && k.kind === 1 && k.nFrames === 3 && k.anchor === 0 && k.pairs.join() === '0,1,2,1' && k.pairMatrices.length === 16, 'chainMatrices: defaults');
ok(c instanceof Float64Array && c.length === 24 && c[23] === 23, 'chainMatrices: the result');
h.chainMatrices(Array.from(pm), Int32Array.from([0, 1, 2, 1]), { frames: 4, anchor: 3, transform: 'affine' });
ok(last().kind === 0 && last().anchor === 3 && last().nFrames === 4, 'chainMatrices: options');
ok(h.chainMatrices([], [], { frames: 0 }).length === 0, 'chainMatrices: no frames');
const inv = h.invertMatrix([1, 2, 3, 4, 5, 6, 7, 8]);
ok(last().name === 'invert' && last().kind === 1 && inv instanceof Float64Array && inv[7] === -8, 'invertMatrix: defaults');
h.invertMatrix(Float64Array.from(I), { transform: 'affine' });
ok(last().kind === 0, 'invertMatrix: affine');
ok(visible(h) === before, 'the helpers changed the state of the instance');
// ---- the thrown strings
const n1 = addon.bundleCalls.length;
const good = () => [mats, [[0, 1], [2, 1]], [a, b]];
const refusals = [
    [() => h.bundleAdjust(...good(), { ...size, transform: 'piecewiseaffine' }), 'transform'], [() => h.bundleAdjust(...good(), {}), 'width'],
    [() => h.bundleAdjust(...good(), { width: 96, height: 0 }), 'height'], [() => h.bundleAdjust(...good(), { ...size, iterations: 65 }), 'iterations'],
    [() => h.bundleAdjust(...good(), { ...size, iterations: 1.5 }), 'iterations'], [() => h.bundleAdjust(...good(), { ...size, eps: -1 }), 'eps'],
    [() => h.bundleAdjust(...good(), { ...size, eps: NaN }), 'eps'], [() => h.bundleAdjust(...good(), { ...size, lambda: 0 }), 'lambda'],
    [() => h.bundleAdjust(...good(), { ...size, lambda: Infinity }), 'lambda'], [() => h.bundleAdjust(...good(), { ...size, huber: -1 }), 'huber'],
    [() => h.bundleAdjust(...good(), { ...size, huber: '1' }), 'huber'], [() => h.bundleAdjust('x', [], [], size), 'matrices'],
    [() => h.bundleAdjust([1, 2, 3], [], [], size), '8 numbers'], [() => h.bundleAdjust(mats, 'x', [a, b], size), 'pairs'],
    [() => h.bundleAdjust(mats, [[0, 3], [2, 1]], [a, b], size), 'pair 0'], [() => h.bundleAdjust(mats, [[0, 1], [1, 1]], [a, b], size), 'pair 1'],
    [() => h.bundleAdjust(mats, [[0, 1], [2]], [a, b], size), 'two frame indices'], [() => h.bundleAdjust(mats, [[0, 1], [2, 1]], [a], size), 'one match list per pair'],
    [() => h.bundleAdjust(mats, [[0, 1], [2, 1]], [a, 'x'], size), 'match list 1'], [() => h.bundleAdjust(mats, [[0, 1], [2, 1]], [a, [[1, 2, 3]]], size), 'quadruples'],
    [() => h.bundleAdjust(...good(), { ...size, fixed: [] }), 'at least one'], [() => h.bundleAdjust(...good(), { ...size, fixed: [3] }), 'fixed'],
    [() => h.bundleAdjust(...good(), { ...size, fixed: 0 }), 'fixed'], [() => h.bundleAdjust(...good(), { ...size, masks: [masks[0]] }), 'one mask per pair'],
    [() => h.bundleAdjust(...good(), { ...size, masks: [masks[0], [1]] }), 'mask 1'],
    [() => h.chainMatrices(pm, [[0, 1], [2, 1]], {}), 'frames'], [() => h.chainMatrices(pm, [[0, 1], [2, 1]], { frames: 257 }), 'frames'],
    [() => h.chainMatrices(pm, [[0, 1], [2, 1]], { frames: 3, anchor: 3 }), 'anchor'], [() => h.chainMatrices(pm, [[0, 1]], { frames: 3 }), '8 numbers per pair'],
    [() => h.chainMatrices(pm, [[0, 1], [2, 5]], { frames: 3 }), 'pair 1'], [() => h.chainMatrices(pm, [[0, 1], [2, 1]], { frames: 3, transform: 'x' }), 'transform'],
    [() => h.chainMatrices('x', [], { frames: 3 }), 'pairMatrices'],
    [() => h.invertMatrix([1, 2, 3]), '8 numbers'], [() => h.invertMatrix('x'), '8 numbers'], [() => h.invertMatrix(I, { transform: 2 }), 'transform'],
];
for (const [fn, word] of refusals) {
    const e = thrown(fn);
    ok(typeof e === 'string' && e.includes(word) && /^(bundleAdjust|chainMatrices|invertMatrix): /.test(e), `a bare string naming '${word}': ${String(e)}`);
}
ok(addon.bundleCalls.length === n1, 'a refused call reaches the addon');
h.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails, checks }));
process.exit(fails.length === 0 ? 0 : 1);
