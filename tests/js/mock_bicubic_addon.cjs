// mock_bicubic_addon.cjs -- tests/js/mock_aniso_addon.cjs plus the BICUBIC remap entry points of the addon ('remapBicubic' + entry for the
// two inverse entries: the remap* arguments followed by B and C), traced like the others, for one purpose: checking without a GPU which
// native call remap(plane, {sampling: 'bicubic'}) of the drop-in class makes (tests/js/bicubic_class.mjs; select it with
// HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.  The result only has the right class and length here.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_aniso_addon.cjs'));
const fields = require(path.join(__dirname, 'mock_field_addon.cjs'));      // (untraced)

const plain = (a) => (ArrayBuffer.isView(a) ? Array.from(a) : a);
const mock = Object.assign({}, base);
const inRange = (v) => typeof v === 'number' && v >= 0 && v <= 1;
function bicubicOf(entry, nField, fmtAt) {
    return (c, ...args) => {
        const fieldArgs = args.slice(0, nField), [plane, channels, W, H, B, C] = args.slice(nField);
        base.trace.push(['remapBicubic' + entry, JSON.stringify(fieldArgs.map(plain)), plane.constructor.name, channels, W, H, B, C]);
        if (args.length !== nField + 6 || plane.length !== W * H * channels || fieldArgs[fmtAt] !== 1 || !inRange(B) || !inRange(C))
            throw ('hgwarp mock: remapBicubic arguments');
        const field = fields['field' + entry](c, ...fieldArgs);
        return new plane.constructor(field.length / 2 * channels);
    };
}
mock.remapBicubicInverseGeometric = bicubicOf('InverseGeometric', 7, 6);
mock.remapBicubicInversePiecewise = bicubicOf('InversePiecewise', 1, 0);
module.exports = mock;
