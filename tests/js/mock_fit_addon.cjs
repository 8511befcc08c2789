// mock_fit_addon.cjs -- tests/js/mock_points_addon.cjs plus the addon's fitMatches, with the same trace, for one purpose: checking without a
// GPU what fitMatches() of the drop-in class hands to the native layer (tests/js/fit_class.mjs; select it with HGWARP_ADDON=<this file>).
// TEST INFRASTRUCTURE ONLY.  fitMatches(ctx, kind, matches, nPoints, counts, threshold, nHyp, seed, samples, refit) records its arguments and
// returns arrays of the right shapes: matrices 8 f + k, minimal -(8 f + k), counts[f] = f + 1, best[f] = f, mask 1 in the first counts[f] slots
// of frame f and 7 in the padding -- the values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_points_addon.cjs'));

const mock = Object.assign({}, base);
mock.fitCalls = [];
mock.fitMatches = (c, kind, matches, nPoints, counts, threshold, nHyp, seed, samples, refit, ...rest) => {
    if (rest.length || !(matches instanceof Float32Array) || !(counts instanceof Int32Array) || matches.length !== counts.length * nPoints * 4 ||
        !(samples === null || samples instanceof Int32Array)) throw ('hgwarp mock: fitMatches arguments');
    base.trace.push(['fitMatches', kind, nPoints, Array.from(counts), threshold, nHyp, seed, samples === null ? null : samples.length, refit]);
    mock.fitCalls.push({ kind, matches: Float32Array.from(matches), nPoints, counts: Array.from(counts), threshold, nHyp, seed, samples, refit });
    const F = counts.length;
    const mask = new Uint8Array(F * nPoints).fill(7);
    for (let f = 0; f < F; f++) mask.fill(1, f * nPoints, f * nPoints + counts[f]);
    return { matrices: Float64Array.from({ length: 8 * F }, (_, k) => k), minimal: Float64Array.from({ length: 8 * F }, (_, k) => -k),
             counts: Int32Array.from({ length: F }, (_, f) => f + 1), best: Int32Array.from({ length: F }, (_, f) => f), mask };
};
module.exports = mock;
