// mock_tps_addon.cjs -- tests/js/mock_fit_addon.cjs plus the addon's thin-plate function, with the same trace, for one purpose: checking
// without a GPU what warpThinPlate() of the drop-in class hands to the native layer (tests/js/tps_class.mjs; select it with
// HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.
//   warpThinPlate(ctx, from, nFromSets, to, nToSets, nPoints, windows, smoothing, step, output, images | null, W, H, nImages) records its
//     arguments and returns { data, status }: the frames packed at the 256-byte grain, 4 bytes per pixel (8 for output 3), byte k of frame f
//     = (f * 16 + k) & 255; status[f] = f % 3.  The values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_fit_addon.cjs'));

const mock = Object.assign({}, base);
mock.tpsCalls = [];
mock.warpThinPlate = (c, from, nFromSets, to, nToSets, nPoints, windows, smoothing, step, output, images, W, H, nImages, ...rest) => {
    if (rest.length || !(from instanceof Float32Array) || !(to instanceof Float32Array) || !(windows instanceof Int32Array) || windows.length % 4 ||
        from.length !== nFromSets * nPoints * 2 || to.length !== nToSets * nPoints * 2 || (images !== null && !(images instanceof Uint8Array)) ||
        (output < 2 && (images === null || images.length !== nImages * W * H * 4)))
        throw ('hgwarp mock: warpThinPlate arguments');
    const F = windows.length / 4, px = output === 3 ? 8 : 4;
    base.trace.push(['warpThinPlate', nFromSets, nToSets, nPoints, F, smoothing, step, output, W, H, nImages]);
    mock.tpsCalls.push({ from: Float32Array.from(from), nFromSets, to: Float32Array.from(to), nToSets, nPoints, windows: Array.from(windows), smoothing, step, output,
                         images: images === null ? null : Uint8Array.from(images), W, H, nImages });
    let total = 0;
    for (let f = 0; f < F; f++) total += (Math.max(windows[4 * f + 2], 0) * Math.max(windows[4 * f + 3], 0) * px + 255) & ~255;
    const data = new Uint8Array(total);
    let off = 0;
    for (let f = 0; f < F; f++) {
        const n = Math.max(windows[4 * f + 2], 0) * Math.max(windows[4 * f + 3], 0) * px;
        for (let k = 0; k < n; k++) data[off + k] = (f * 16 + k) & 255;
        off += (n + 255) & ~255;
    }
    return { data, status: Int32Array.from({ length: F }, (_, f) => f % 3) };
};
module.exports = mock;
