// mock_trilinear_addon.cjs -- tests/js/mock_remap_addon.cjs plus the TRILINEAR remap entry points of the addon ('remapTrilinear' + entry for
// the two inverse entries; there is no forward one), traced like the others, for one purpose: checking without a GPU which native call
// remap(plane, {sampling: 'trilinear'}) of the drop-in class makes (tests/js/trilinear_class.mjs; select it with HGWARP_ADDON=<this file>).
// TEST INFRASTRUCTURE ONLY.  The result only has the right class and length here -- its values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_remap_addon.cjs'));
const fields = require(path.join(__dirname, 'mock_field_addon.cjs'));      // (untraced)

const plain = (a) => (ArrayBuffer.isView(a) ? Array.from(a) : a);
const mock = Object.assign({}, base);
function trilinearOf(entry, nField, fmtAt) {
    return (c, ...args) => {
        const fieldArgs = args.slice(0, nField), [plane, channels, W, H] = args.slice(nField);
        base.trace.push(['remapTrilinear' + entry, JSON.stringify(fieldArgs.map(plain)), plane.constructor.name, channels, W, H]);
        if (args.length !== nField + 4 || plane.length !== W * H * channels || fieldArgs[fmtAt] !== 1) throw ('hgwarp mock: remapTrilinear arguments');
        const field = fields['field' + entry](c, ...fieldArgs);
        return new plane.constructor(field.length / 2 * channels);
    };
}
mock.remapTrilinearInverseGeometric = trilinearOf('InverseGeometric', 7, 6);
mock.remapTrilinearInversePiecewise = trilinearOf('InversePiecewise', 1, 0);
module.exports = mock;
