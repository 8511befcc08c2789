// CPU: fitMatches(matchSets, options) of the drop-in class over tests/js/mock_fit_addon.cjs (run with HGWARP_ADDON pointing at it): the
// lists are padded to the longest and their lengths go down as counts; the option defaults; the bare strings thrown for an unknown
// transform, a list that does not hold quadruples, a bad threshold and a bad hypotheses count; the shape of the result; no image is needed
// and the state the reference can see is the same after a call.  Prints one JSON line {ok, fails, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const last = () => addon.fitCalls[addon.fitCalls.length - 1];
const visible = (h) => JSON.stringify([h._map === null ? null : h._map.kind, h._pm === null || h._pm === undefined ? null : 1, h._lastPath, h._image === null,
                                       h._srcPoints === null ? null : Array.from(h._srcPoints), h._dstPoints === null ? null : Array.from(h._dstPoints), h._sampling]);

const a = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]];                      // three matches as arrays
const b = Float32Array.from([1.5, 2.5, 3.5, 4.5, NaN, 0, Infinity, 1e30, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]);      // five, as a Float32Array
const c = [];                                                                // none

// ---- defaults, padding and counts; no image was ever set
const h = new Homography('projective', 64, 48);
const before = visible(h);
const n0 = addon.trace.length;
const r = h.fitMatches([a, b, c]);
ok(visible(h) === before, 'fitMatches changed the state of the instance');
ok(addon.fitCalls.length === 1 && addon.trace.slice(n0).filter((t) => t[0] !== 'create').length === 1, 'exactly one addon call (besides the context)');
let k = last();
ok(k.kind === 1 && k.threshold === 3 && k.nHyp === 1024 && k.seed === 0 && k.samples === null && k.refit === 1, `defaults: ${JSON.stringify([k.kind, k.threshold, k.nHyp, k.seed, k.samples, k.refit])}`);
ok(k.nPoints === 5 && JSON.stringify(k.counts) === '[3,5,0]', `padding: nPoints ${k.nPoints}, counts ${k.counts}`);
ok(k.matches.length === 3 * 5 * 4, 'packed length');
ok(Array.from(k.matches.slice(0, 12)).join() === a.flat().join() && k.matches.slice(12, 20).every((v) => v === 0), 'frame 0: its matches, then zero padding');
ok(Object.is(k.matches[24], NaN) && k.matches[26] === Infinity && k.matches[20] === 1.5 && k.matches[39] === 2, 'frame 1: copied as it stands, NaN and Infinity included');
ok(k.matches.slice(40).every((v) => v === 0), 'frame 2: all padding');
// ---- the result
ok(r.kind === 'projective' && r.matrices instanceof Float64Array && r.matrices.length === 24 && r.minimal instanceof Float64Array && r.minimal.length === 24, 'matrices / minimal');
ok(r.counts instanceof Int32Array && r.counts.length === 3 && r.best instanceof Int32Array && r.best.length === 3 && r.best[2] === 2, 'counts / best');
ok(Array.isArray(r.inliers) && r.inliers.length === 3 && r.inliers.every((m) => m instanceof Uint8Array), 'inliers: one Uint8Array per frame');
ok(r.inliers[0].length === 3 && r.inliers[1].length === 5 && r.inliers[2].length === 0 && r.inliers[0].every((v) => v === 1) && r.inliers[1].every((v) => v === 1), 'inliers: n_f flags each, none of the padding');
ok(Object.keys(r).sort().join() === 'best,counts,inliers,kind,matrices,minimal', `keys: ${Object.keys(r)}`);
// ---- options
const samples = Int32Array.from({ length: 2 * 3 * 4 }, (_, i) => i % 3);
const r2 = h.fitMatches([a, a], { transform: 'affine', threshold: 0, hypotheses: 3, seed: 0xffffffff, refit: false, samples });
k = last();
ok(r2.kind === 'affine' && k.kind === 0 && k.threshold === 0 && k.nHyp === 3 && k.seed === 0xffffffff && k.refit === 0 && k.samples === samples, 'explicit options reach the addon');
h.fitMatches([a], { hypotheses: 0 });
ok(last().nHyp === 0 && last().refit === 1, 'hypotheses 0: least squares');
h.fitMatches([a], null);
ok(last().nHyp === 1024 && last().kind === 1, 'options null: the defaults');
ok(h.fitMatches([]).matrices.length === 0 && last().counts.length === 0, 'no frames');
ok(h.fitMatches([a], { samples: [[[0, 1, 2, 3], [2, 1, 0, 3]]], hypotheses: 2 }) && last().samples instanceof Int32Array && Array.from(last().samples).join() === '0,1,2,3,2,1,0,3', 'nested sample arrays are flattened');
// ---- the thrown strings
const n1 = addon.fitCalls.length;
const refusals = [
    [() => h.fitMatches([a], { transform: 'piecewiseaffine' }), 'transform'], [() => h.fitMatches([a], { transform: 1 }), 'transform'],
    [() => h.fitMatches([[1, 2, 3, 4, 5]]), 'quadruples'], [() => h.fitMatches([Float32Array.from([1, 2, 3])]), 'quadruples'], [() => h.fitMatches([a, 'x']), 'match list 1'],
    [() => h.fitMatches(a[0]), 'match list 0'], [() => h.fitMatches('x'), 'matchSets'],
    [() => h.fitMatches([a], { threshold: -1 }), 'threshold'], [() => h.fitMatches([a], { threshold: NaN }), 'threshold'], [() => h.fitMatches([a], { threshold: Infinity }), 'threshold'],
    [() => h.fitMatches([a], { threshold: '3' }), 'threshold'],
    [() => h.fitMatches([a], { hypotheses: -1 }), 'hypotheses'], [() => h.fitMatches([a], { hypotheses: 1.5 }), 'hypotheses'], [() => h.fitMatches([a], { hypotheses: 65537 }), 'hypotheses'],
    [() => h.fitMatches([a], { hypotheses: 0, refit: false }), 'hypotheses'],
    [() => h.fitMatches([a], { seed: -1 }), 'seed'], [() => h.fitMatches([a], { samples: new Int32Array(4), hypotheses: 2 }), 'samples'],
];
for (const [fn, word] of refusals) {
    const e = thrown(fn);
    ok(typeof e === 'string' && e.startsWith('fitMatches:') && e.includes(word), `a refusal must be a bare string of fitMatches naming ${word} (got ${e})`);
}
ok(addon.fitCalls.length === n1, 'a refused call reaches no addon function');
ok(visible(h) === before, 'the state of the instance after all of it');

const res = { ok: fails.length === 0, fails, checks };
console.log(JSON.stringify(res));
process.exit(res.ok ? 0 : 1);
