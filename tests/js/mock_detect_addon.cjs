// mock_detect_addon.cjs -- tests/js/mock_match_addon.cjs plus the addon's detectAndDescribe, with the same trace, for one purpose: checking
// without a GPU what detectAndDescribe() of the drop-in class hands to the native layer (tests/js/detect_class.mjs; select it with
// HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.  detectAndDescribe(ctx, planes, nPlanes, width, height, channels, cell, perCell,
// minResponse) records its arguments and returns arrays of the right shapes: nSlots = ceil(width / cell) ceil(height / cell) perCell; plane p
// has min(p + 1, nSlots) keypoints at (10 p + k, 100 p + k) with descriptor bytes (p + k + b) & 255 at the front of its slots, NaN points and
// zero rows behind them -- the values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_match_addon.cjs'));

const mock = Object.assign({}, base);
mock.detectCalls = [];
mock.detectAndDescribe = (c, planes, nPlanes, width, height, channels, cell, perCell, minResponse, ...rest) => {
    if (rest.length || !(planes instanceof Uint8Array) || planes.length !== nPlanes * width * height * channels || !Number.isInteger(minResponse))
        throw ('hgwarp mock: detectAndDescribe arguments');
    base.trace.push(['detectAndDescribe', nPlanes, width, height, channels, cell, perCell, minResponse]);
    mock.detectCalls.push({ planes: Uint8Array.from(planes), nPlanes, width, height, channels, cell, perCell, minResponse });
    const nSlots = Math.ceil(width / cell) * Math.ceil(height / cell) * perCell;
    const counts = Int32Array.from({ length: nPlanes }, (_, p) => Math.min(p + 1, nSlots));
    const points = new Float32Array(nPlanes * nSlots * 2).fill(NaN);
    const descriptors = new Uint8Array(nPlanes * nSlots * 32);
    for (let p = 0; p < nPlanes; p++) for (let k = 0; k < counts[p]; k++) {
        points[(p * nSlots + k) * 2] = 10 * p + k; points[(p * nSlots + k) * 2 + 1] = 100 * p + k;
        for (let b = 0; b < 32; b++) descriptors[(p * nSlots + k) * 32 + b] = (p + k + b) & 255;
    }
    return { nSlots, counts, points, descriptors };
};
module.exports = mock;
