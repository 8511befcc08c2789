// mock_mosaic_addon.cjs -- tests/js/mock_sampling_addon.cjs plus the MOSAIC entry points of the addon (mosaicInverseGeometric /
// mosaicInversePiecewise), recorded with their arguments in `trace`, for one purpose: checking without a GPU which native calls
// h.mosaic(dstPointSets, options) of the drop-in class makes (tests/js/mosaic_class.mjs; select it with HGWARP_ADDON=<this file>).
// TEST INFRASTRUCTURE ONLY.  The result only has the right classes and lengths here.
'use strict';
const base = require('./mock_sampling_addon.cjs');

const trace = [];
const plain = (a) => (ArrayBuffer.isView(a) ? Array.from(a) : a);
function mosaicOf(entry, nHead) {
    return (c, ...args) => {
        const head = args.slice(0, nHead), [mode, feather, canvas, wantWeight, W, H] = args.slice(nHead);
        const geoms = head[nHead - 1];
        trace.push({ entry, head: head.map(plain), mode, feather, canvas: plain(canvas), wantWeight, W, H, sampling: c.sampling || 0,
                     image: c.images ? c.images.map((im) => im[0]) : (c.image ? c.image[0] : null), mesh: c.mesh ? c.mesh.src.length : 0 });
        base.calls.push(entry);
        if (args.length !== nHead + 6 || !(canvas instanceof Int32Array) || canvas.length !== 4 || ![0, 1, 2].includes(mode) || typeof feather !== 'number' || !(feather > 0) ||
            typeof wantWeight !== 'boolean' || !(geoms instanceof Int32Array) || geoms.length < 4 || geoms.length % 4 || W !== c.W || H !== c.H || (!c.image && !c.images))
            throw ('hgwarp mock: mosaic arguments');
        const n = Math.max(canvas[2], 0) * Math.max(canvas[3], 0);
        return wantWeight ? { data: new Uint8ClampedArray(n * 4), weight: new Float32Array(n) } : { data: new Uint8ClampedArray(n * 4) };
    };
}
module.exports = Object.assign({}, base, { trace, mosaicInverseGeometric: mosaicOf('mosaicInverseGeometric', 4), mosaicInversePiecewise: mosaicOf('mosaicInversePiecewise', 2) });
