// mock_bundle_addon.cjs -- tests/js/mock_fit_addon.cjs plus the addon's bundleAdjust, bundleChain and bundleInvert, with the same trace, for
// one purpose: checking without a GPU what bundleAdjust(), chainMatrices() and invertMatrix() of the drop-in class hand to the native layer
// (tests/js/bundle_class.mjs; select it with HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.  The calls record their arguments and
// return arrays of the right shapes: matrices + 1; an info block with status 0, rounds 3, accepted 2, rms 2.5 / 0.5, frame f's state f % 4
// and pair p's record { p + 10, p + 5, p + 0.5, p + 0.25 } -- the values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_fit_addon.cjs'));

const mock = Object.assign({}, base);
mock.bundleCalls = [];
mock.bundleAdjust = (c, kind, W, H, fixed, pairs, matches, nPoints, counts, mask, nIter, eps, lambda, huber, matrices, ...rest) => {
    if (rest.length || !(fixed instanceof Uint8Array) || !(pairs instanceof Int32Array) || !(matches instanceof Float32Array) || !(counts instanceof Int32Array) ||
        !(matrices instanceof Float64Array) || !(mask === null || mask instanceof Uint8Array) || pairs.length !== 2 * counts.length ||
        matches.length !== counts.length * nPoints * 4 || matrices.length !== 8 * fixed.length || (mask !== null && mask.length !== counts.length * nPoints))
        throw ('hgwarp mock: bundleAdjust arguments');
    base.trace.push(['bundleAdjust', kind, W, H, Array.from(fixed), Array.from(pairs), nPoints, Array.from(counts), mask === null ? null : mask.length, nIter, eps, lambda, huber]);
    mock.bundleCalls.push({ name: 'adjust', kind, W, H, fixed: Array.from(fixed), pairs: Array.from(pairs), matches: Float32Array.from(matches), nPoints, counts: Array.from(counts),
                            mask: mask === null ? null : Uint8Array.from(mask), nIter, eps, lambda, huber, matrices: Float64Array.from(matrices) });
    const F = fixed.length, P = counts.length;
    const info = new Uint8Array(F ? 48 + ((4 * F + 7) & ~7) + 24 * P : 0);
    if (F) {
        const v = new DataView(info.buffer);
        v.setInt32(0, 0, true); v.setInt32(4, 3, true); v.setInt32(8, 2, true); v.setInt32(12, 40, true); v.setInt32(16, 40, true);
        v.setFloat64(24, 2.5, true); v.setFloat64(32, 0.5, true); v.setFloat64(40, 1e-5, true);
        for (let f = 0; f < F; f++) v.setInt32(48 + 4 * f, f % 4, true);
        const o = 48 + ((4 * F + 7) & ~7);
        for (let p = 0; p < P; p++) { v.setInt32(o + 24 * p, p + 10, true); v.setInt32(o + 24 * p + 4, p + 5, true); v.setFloat64(o + 24 * p + 8, p + 0.5, true); v.setFloat64(o + 24 * p + 16, p + 0.25, true); }
    }
    return { matrices: Float64Array.from(matrices, (x) => x + 1), info };
};
mock.bundleChain = (kind, nFrames, pairs, pairMatrices, anchor, ...rest) => {
    if (rest.length || !(pairs instanceof Int32Array) || !(pairMatrices instanceof Float64Array) || pairMatrices.length !== 4 * pairs.length) throw ('hgwarp mock: bundleChain arguments');
    base.trace.push(['bundleChain', kind, nFrames, Array.from(pairs), anchor]);
    mock.bundleCalls.push({ name: 'chain', kind, nFrames, pairs: Array.from(pairs), pairMatrices: Float64Array.from(pairMatrices), anchor });
    return Float64Array.from({ length: 8 * nFrames }, (_, k) => k);
};
mock.bundleInvert = (kind, m, ...rest) => {
    if (rest.length || !(m instanceof Float64Array) || m.length !== 8) throw ('hgwarp mock: bundleInvert arguments');
    base.trace.push(['bundleInvert', kind]);
    mock.bundleCalls.push({ name: 'invert', kind, m: Float64Array.from(m) });
    return Float64Array.from(m, (x) => -x);
};
module.exports = mock;
