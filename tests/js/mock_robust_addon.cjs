// mock_robust_addon.cjs -- tests/js/mock_mosaic_addon.cjs plus the ROBUST mosaic entry points of the addon (mosaicRobustInverseGeometric /
// mosaicRobustInversePiecewise), recorded with their arguments in the same `trace`, for one purpose: checking without a GPU which native
// calls h.mosaic(dstPointSets, { blend: 'median' | 'trimmed' | 'min' | 'max' }) of the drop-in class makes (tests/js/robust_class.mjs;
// select it with HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.  The result only has the right classes and lengths here.
'use strict';
const base = require('./mock_mosaic_addon.cjs');

const plain = (a) => (ArrayBuffer.isView(a) ? Array.from(a) : a);
function robustOf(entry, nHead) {
    return (c, ...args) => {
        const head = args.slice(0, nHead), [mode, trim, canvas, wantWeight, W, H, exposure] = args.slice(nHead);
        const geoms = head[nHead - 1];
        base.trace.push({ entry, head: head.map(plain), mode, trim, canvas: plain(canvas), wantWeight, W, H, nArgs: args.length - nHead,
                          exposure: exposure === undefined ? null : [exposure.constructor.name, Array.from(exposure)] });
        base.calls.push(entry);
        if ((args.length !== nHead + 6 && args.length !== nHead + 7) || !(canvas instanceof Int32Array) || canvas.length !== 4 || ![0, 1, 2, 3].includes(mode) ||
            typeof trim !== 'number' || !(trim >= 0 && trim < 0.5) || typeof wantWeight !== 'boolean' || !(geoms instanceof Int32Array) || geoms.length < 4 || geoms.length % 4 ||
            W !== c.W || H !== c.H || (!c.image && !c.images) || (exposure !== undefined && !(exposure instanceof Float32Array) && !(exposure instanceof Float64Array)))
            throw ('hgwarp mock: robust mosaic arguments');
        const n = Math.max(canvas[2], 0) * Math.max(canvas[3], 0), F = geoms.length / 4;
        const res = { data: new Uint8ClampedArray(n * 4) };
        if (wantWeight) res.weight = new Float32Array(n);
        if (exposure !== undefined) res.gains = exposure instanceof Float32Array ? Float32Array.from(exposure) : new Float32Array(F).fill(1);
        return res;
    };
}
module.exports = Object.assign({}, base, { mosaicRobustInverseGeometric: robustOf('mosaicRobustInverseGeometric', 4), mosaicRobustInversePiecewise: robustOf('mosaicRobustInversePiecewise', 2) });
