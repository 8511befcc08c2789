// CPU: matchDescriptors(querySets, trainSets, options) of the drop-in class over tests/js/mock_match_addon.cjs (run with HGWARP_ADDON
// pointing at it): the sets are padded to the longest and their rows to a stride of 16 bytes, their lengths go down as counts; the option
// defaults; the bare strings thrown; the shape of the result, which fitMatches accepts; no image is needed and the state the reference can
// see is the same after a call.  Prints one JSON line {ok, fails, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const last = () => addon.matchCalls[addon.matchCalls.length - 1];
const visible = (h) => JSON.stringify([h._map === null ? null : h._map.kind, h._pm === null || h._pm === undefined ? null : 1, h._lastPath, h._image === null,
                                       h._srcPoints === null ? null : Array.from(h._srcPoints), h._dstPoints === null ? null : Array.from(h._dstPoints), h._sampling]);
const rows = (n, bytes, base) => Uint8Array.from({ length: n * bytes }, (_, i) => (base + i) & 255);

// ---- defaults, padding and counts; no image was ever set
const h = new Homography('projective', 64, 48);
const before = visible(h);
const n0 = addon.trace.length;
const q = [rows(3, 32, 1), rows(2, 32, 101), rows(0, 32, 0)], t = [rows(4, 32, 7)];
const r = h.matchDescriptors(q, t);
ok(visible(h) === before, 'matchDescriptors changed the state of the instance');
ok(addon.matchCalls.length === 1 && addon.trace.slice(n0).filter((x) => x[0] !== 'create').length === 1, 'exactly one addon call (besides the context)');
let k = last();
ok(k.kind === 0 && k.descBytes === 32 && k.stride === 32 && k.ratio === 0.8 && k.maxDistance === 0xffffffff && k.crossCheck === 0 && k.qp === null && k.tp === null,
   `defaults: ${JSON.stringify([k.kind, k.descBytes, k.stride, k.ratio, k.maxDistance, k.crossCheck])}`);
ok(k.nQuery === 3 && k.nTrain === 4 && JSON.stringify(k.countsQ) === '[3,2,0]' && JSON.stringify(k.countsT) === '[4]', `padding: ${k.nQuery} ${k.nTrain} ${k.countsQ} ${k.countsT}`);
ok(k.query.length === 3 * 3 * 32 && k.query.slice(0, 96).join() === q[0].join() && k.query.slice(96, 160).join() === q[1].join() && k.query.slice(160).every((v) => v === 0),
   'the query sets, each padded to three rows');
ok(k.train.join() === t[0].join(), 'the train set as it stands');
// ---- the result
ok(Array.isArray(r) && r.length === 3 && r.every((x) => x.pairs instanceof Int32Array && x.matches === undefined), 'one record per frame, no matches without points');
ok(r[0].count === 1 && r[1].count === 2 && r[2].count === 0 && r[1].pairs.join() === '0,100,1,101' && r[2].pairs.length === 0, 'count and the pairs in use, none of the padding');
ok(Object.keys(r[0]).sort().join() === 'count,pairs', `keys: ${Object.keys(r[0])}`);
// ---- options: a row length that is no multiple of 16, points in both forms, two train sets
const q5 = [rows(2, 5, 1), rows(1, 5, 50)], t5 = [rows(1, 5, 9), rows(3, 5, 20)];
const r2 = h.matchDescriptors(q5, t5, { kind: 'u8', descBytes: 5, ratio: 0, maxDistance: 7, crossCheck: true,
                                        queryPoints: [[[1, 2], [3, 4]], Float32Array.from([5, 6])], trainPoints: [Float32Array.from([7, NaN]), [[9, 10], [11, 12], [13, 14]]] });
k = last();
ok(k.kind === 1 && k.descBytes === 5 && k.stride === 16 && k.ratio === 0 && k.maxDistance === 7 && k.crossCheck === 1, 'explicit options reach the addon');
ok(k.query.length === 2 * 2 * 16 && k.query.slice(0, 5).join() === q5[0].slice(0, 5).join() && k.query.slice(5, 16).every((v) => v === 0) &&
   k.query.slice(16, 21).join() === q5[0].slice(5).join() && k.query.slice(32, 37).join() === q5[1].join() && k.query.slice(37).every((v) => v === 0), 'rows padded to the stride');
ok(JSON.stringify(k.countsT) === '[1,3]' && k.nTrain === 3 && k.train.slice(48, 53).join() === t5[1].slice(0, 5).join(), 'two train sets');
ok(k.qp.join() === '1,2,3,4,5,6,0,0' && k.tp[0] === 7 && Object.is(k.tp[1], NaN) && Array.from(k.tp.slice(2, 6)).every((v) => v === 0) && k.tp.slice(6).join() === '9,10,11,12,13,14',
   'points: copied as they stand, padded with zeros');
ok(r2.length === 2 && r2[0].matches instanceof Float32Array && r2[0].matches.join() === '0,1,2,3' && r2[1].matches.join() === '1000,1001,1002,1003' && r2[1].count === 1,
   'matches: four floats per pair in use');
const fit = h.fitMatches(r2.map((x) => x.matches), { hypotheses: 4 });
ok(fit.counts.length === 2, 'the matches go into fitMatches as they are');
h.matchDescriptors(q, t, null);
ok(last().kind === 0 && last().ratio === 0.8, 'options null: the defaults');
h.matchDescriptors([rows(1, 128, 0)], [rows(1, 128, 0)], { kind: 'u8' });
ok(last().descBytes === 128 && last().stride === 128, "'u8' defaults to 128 bytes");
ok(h.matchDescriptors([], t).length === 0 && last().countsQ.length === 0, 'no frames');
// ---- the thrown strings
const n1 = addon.matchCalls.length;
const refusals = [
    [() => h.matchDescriptors(q, t, { kind: 'float' }), 'kind'], [() => h.matchDescriptors(q, t, { kind: 0 }), 'kind'],
    [() => h.matchDescriptors(q, t, { descBytes: 0 }), 'descBytes'], [() => h.matchDescriptors(q, t, { descBytes: 513 }), 'descBytes'], [() => h.matchDescriptors(q, t, { descBytes: 1.5 }), 'descBytes'],
    [() => h.matchDescriptors(q, t, { descBytes: 5 }), 'rows of descBytes'], [() => h.matchDescriptors([[1, 2]], t), 'query set 0'], [() => h.matchDescriptors(q, [new Float32Array(8)]), 'train set 0'],
    [() => h.matchDescriptors(q[0], t), 'querySets'], [() => h.matchDescriptors(q, t[0]), 'querySets'],
    [() => h.matchDescriptors(q, []), 'trainSets'], [() => h.matchDescriptors([q[0]], [t[0], t[0]]), 'trainSets'],
    [() => h.matchDescriptors(q, t, { ratio: -0.1 }), 'ratio'], [() => h.matchDescriptors(q, t, { ratio: 1.1 }), 'ratio'], [() => h.matchDescriptors(q, t, { ratio: NaN }), 'ratio'],
    [() => h.matchDescriptors(q, t, { ratio: '0.8' }), 'ratio'],
    [() => h.matchDescriptors(q, t, { maxDistance: -1 }), 'maxDistance'], [() => h.matchDescriptors(q, t, { maxDistance: 1.5 }), 'maxDistance'], [() => h.matchDescriptors(q, t, { maxDistance: 2 ** 32 }), 'maxDistance'],
    [() => h.matchDescriptors(q, t, { queryPoints: [[], [], []] }), 'come together'],
    [() => h.matchDescriptors(q, t, { queryPoints: [[[1, 2]], [], []], trainPoints: [new Float32Array(8)] }), 'queryPoints list 0'],
    [() => h.matchDescriptors(q, t, { queryPoints: [new Float32Array(6), new Float32Array(4)], trainPoints: [new Float32Array(8)] }), 'queryPoints'],
    [() => h.matchDescriptors(q, t, { queryPoints: [new Float32Array(6), new Float32Array(4), 'x'], trainPoints: [new Float32Array(8)] }), 'queryPoints list 2'],
];
for (const [fn, word] of refusals) {
    const e = thrown(fn);
    ok(typeof e === 'string' && e.startsWith('matchDescriptors:') && e.includes(word), `a refusal must be a bare string of matchDescriptors naming ${word} (got ${e})`);
}
ok(addon.matchCalls.length === n1, 'a refused call reaches no addon function');
ok(visible(h) === before, 'the state of the instance after all of it');

const res = { ok: fails.length === 0, fails, checks };
console.log(JSON.stringify(res));
process.exit(res.ok ? 0 : 1);
