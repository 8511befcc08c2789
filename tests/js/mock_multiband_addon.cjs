// mock_multiband_addon.cjs -- tests/js/mock_mosaic_gain_addon.cjs plus the MULTI-BAND entry points of the addon
// (mosaicMultibandInverseGeometric / mosaicMultibandInversePiecewise), recorded with their arguments in `bandCalls`, for one purpose: checking
// without a GPU what h.mosaic(dstPointSets, { blend: 'multiband', ... }) of the drop-in class hands down (tests/js/multiband_class.mjs;
// select it with HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.  The result only has the right classes and lengths: labels name
// frame (pixel index % F) of the call, -1 at pixel 0; gains are the given ones, or 1 + k / 8 for frame k where they are to be fitted.
'use strict';
const base = require('./mock_mosaic_gain_addon.cjs');

const bandCalls = [];
const plain = (a) => (ArrayBuffer.isView(a) ? Array.from(a) : a);
function multibandOf(entry, nHead) {
    return (c, ...args) => {
        const head = args.slice(0, nHead), [bands, feather, canvas, wantWeight, W, H, wantLabels, ex] = args.slice(nHead);
        const geoms = head[nHead - 1], F = geoms instanceof Int32Array ? geoms.length / 4 : 0;
        bandCalls.push({ entry, head: head.map(plain), bands, feather, canvas: plain(canvas), wantWeight, W, H, wantLabels, n: args.length,
                         exposure: ex instanceof Float32Array ? { gains: Array.from(ex) } : (ex instanceof Float64Array ? { sigmas: Array.from(ex) } : null) });
        base.calls.push(entry);
        if (args.length < nHead + 7 || args.length > nHead + 8 || !(canvas instanceof Int32Array) || canvas.length !== 4 || !Number.isInteger(bands) || bands < 1 || bands > 8 ||
            typeof feather !== 'number' || !(feather > 0) || typeof wantWeight !== 'boolean' || typeof wantLabels !== 'boolean' || !(geoms instanceof Int32Array) || geoms.length < 4 ||
            geoms.length % 4 || W !== c.W || H !== c.H || (!c.image && !c.images) ||
            (args.length === nHead + 8 && !((ex instanceof Float32Array && ex.length === F) || (ex instanceof Float64Array && ex.length === 2))))
            throw ('hgwarp mock: multiband mosaic arguments');
        const n = Math.max(canvas[2], 0) * Math.max(canvas[3], 0);
        const res = { data: new Uint8ClampedArray(n * 4) };
        if (wantWeight) res.weight = new Float32Array(n);
        if (wantLabels) res.labels = Int32Array.from({ length: n }, (_, i) => (i === 0 ? -1 : i % F));
        if (args.length === nHead + 8) res.gains = ex instanceof Float32Array ? Float32Array.from(ex) : Float32Array.from({ length: F }, (_, k) => 1 + k / 8);
        return res;
    };
}
module.exports = Object.assign({}, base, { bandCalls, mosaicMultibandInverseGeometric: multibandOf('mosaicMultibandInverseGeometric', 4),
                                           mosaicMultibandInversePiecewise: multibandOf('mosaicMultibandInversePiecewise', 2) });
