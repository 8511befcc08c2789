// mock_flow_addon.cjs -- tests/js/mock_fit_addon.cjs plus the addon's dense-flow function, with the same trace, for one purpose: checking
// without a GPU what denseFlow() of the drop-in class hands to the native layer (tests/js/flow_class.mjs; select it with
// HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.
//   denseFlow(ctx, from, to, W, H, channels, nFrames, nToSets, levels, iterations, radius, minEig, maxUpdate, flags) records its arguments and
//     returns { field, residual, good, images }: what the flags ask for (1 field, 2 residual, 4 good, 8 images), null otherwise; field word k
//     = k / 4, residual byte k = k & 255, good byte k = k & 1, images byte k = (k * 3) & 255.  The values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_fit_addon.cjs'));

const mock = Object.assign({}, base);
mock.flowCalls = [];
mock.denseFlow = (c, from, to, W, H, channels, nFrames, nToSets, levels, iterations, radius, minEig, maxUpdate, flags, ...rest) => {
    if (rest.length || !(from instanceof Uint8Array) || !(to instanceof Uint8Array) || from.length !== nFrames * W * H * channels ||
        to.length !== nToSets * W * H * channels || !Number.isInteger(flags) || flags < 0 || flags > 15)
        throw ('hgwarp mock: denseFlow arguments');
    base.trace.push(['denseFlow', W, H, channels, nFrames, nToSets, levels, iterations, radius, minEig, maxUpdate, flags]);
    mock.flowCalls.push({ from: Uint8Array.from(from), to: Uint8Array.from(to), W, H, channels, nFrames, nToSets, levels, iterations, radius, minEig, maxUpdate, flags });
    const n = nFrames * W * H;
    return {
        field: (flags & 1) ? Float32Array.from({ length: n * 2 }, (_, k) => k / 4) : null,
        residual: (flags & 2) ? Uint8Array.from({ length: n }, (_, k) => k & 255) : null,
        good: (flags & 4) ? Uint8Array.from({ length: n }, (_, k) => k & 1) : null,
        images: (flags & 8) ? Uint8Array.from({ length: n * channels }, (_, k) => (k * 3) & 255) : null,
    };
};
module.exports = mock;
