// mock_match_addon.cjs -- tests/js/mock_fit_addon.cjs plus the addon's matchDescriptors, with the same trace, for one purpose: checking
// without a GPU what matchDescriptors() of the drop-in class hands to the native layer (tests/js/match_class.mjs; select it with
// HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.  matchDescriptors(ctx, kind, descBytes, stride, query, nQuery, countsQ, train, nTrain,
// countsT, ratio, maxDistance, crossCheck, queryPoints, trainPoints) records its arguments and returns arrays of the right shapes: frame f has
// min(f + 1, countsQ[f]) pairs (i, 100 f + i) at the front of its slots and -1 behind them, matches 1000 f + 4 k + c in slot k and NaN behind
// them -- the values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_fit_addon.cjs'));

const mock = Object.assign({}, base);
mock.matchCalls = [];
mock.matchDescriptors = (c, kind, descBytes, stride, query, nQuery, countsQ, train, nTrain, countsT, ratio, maxDistance, crossCheck, qp, tp, ...rest) => {
    const F = countsQ.length, S = countsT.length;
    if (rest.length || !(query instanceof Uint8Array) || !(train instanceof Uint8Array) || !(countsQ instanceof Int32Array) || !(countsT instanceof Int32Array) ||
        query.length !== F * nQuery * stride || train.length !== S * nTrain * stride || (qp === null) !== (tp === null) ||
        (qp !== null && (!(qp instanceof Float32Array) || !(tp instanceof Float32Array) || qp.length !== F * nQuery * 2 || tp.length !== S * nTrain * 2)))
        throw ('hgwarp mock: matchDescriptors arguments');
    base.trace.push(['matchDescriptors', kind, descBytes, stride, nQuery, Array.from(countsQ), nTrain, Array.from(countsT), ratio, maxDistance, crossCheck]);
    mock.matchCalls.push({ kind, descBytes, stride, query: Uint8Array.from(query), nQuery, countsQ: Array.from(countsQ), train: Uint8Array.from(train), nTrain,
                           countsT: Array.from(countsT), ratio, maxDistance, crossCheck, qp: qp === null ? null : Float32Array.from(qp), tp: tp === null ? null : Float32Array.from(tp) });
    const counts = Int32Array.from({ length: F }, (_, f) => Math.min(f + 1, countsQ[f]));
    const pairs = new Int32Array(F * nQuery * 2).fill(-1);
    const matches = qp === null ? null : new Float32Array(F * nQuery * 4).fill(NaN);
    for (let f = 0; f < F; f++) for (let k = 0; k < counts[f]; k++) {
        pairs[(f * nQuery + k) * 2] = k; pairs[(f * nQuery + k) * 2 + 1] = 100 * f + k;
        if (matches) for (let e = 0; e < 4; e++) matches[(f * nQuery + k) * 4 + e] = 1000 * f + 4 * k + e;
    }
    return { counts, pairs, matches };
};
module.exports = mock;
