// mock_mosaic_gain_addon.cjs -- tests/js/mock_mosaic_addon.cjs plus the optional last argument of its two mosaic entry points, `exposure`
// (a Float32Array of one gain per frame, or a Float64Array [sigmaN, sigmaG]), recorded in `exposures`, for one purpose: checking without a GPU
// what h.mosaic(dstPointSets, { exposure }) of the drop-in class hands down (tests/js/mosaic_gain_class.mjs; select it with
// HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.  A call without the argument goes to the wrapped mock as it is, which refuses any
// argument count but its own; with it, the result also carries `gains`: the given ones, or 1 + k / 8 for frame k where they are to be fitted.
'use strict';
const base = require('./mock_mosaic_addon.cjs');

const exposures = [];
function withExposure(entry, nArgs) {
    return (c, ...args) => {
        if (args.length <= nArgs) { exposures.push({ entry, exposure: null, n: args.length }); return base[entry](c, ...args); }
        const ex = args[nArgs], geoms = args[nArgs - 7], F = geoms.length / 4;
        exposures.push({ entry, exposure: ex instanceof Float32Array ? { gains: Array.from(ex) } : (ex instanceof Float64Array ? { sigmas: Array.from(ex) } : { other: String(ex) }), n: args.length });
        if (args.length !== nArgs + 1 || !((ex instanceof Float32Array && ex.length === F) || (ex instanceof Float64Array && ex.length === 2)))
            throw ('hgwarp mock: exposure argument');
        const res = base[entry](c, ...args.slice(0, nArgs));
        res.gains = ex instanceof Float32Array ? Float32Array.from(ex) : Float32Array.from({ length: F }, (_, k) => 1 + k / 8);
        return res;
    };
}
module.exports = Object.assign({}, base, { exposures, mosaicInverseGeometric: withExposure('mosaicInverseGeometric', 10), mosaicInversePiecewise: withExposure('mosaicInversePiecewise', 8) });
