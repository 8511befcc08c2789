// mock_aniso_addon.cjs -- tests/js/mock_trilinear_addon.cjs plus the ANISOTROPIC remap entry points of the addon ('remapAniso' + entry for
// the two inverse entries: the trilinear arguments followed by maxAniso), traced like the others, for one purpose: checking without a GPU
// which native call remap(plane, {sampling: 'anisotropic'}) of the drop-in class makes (tests/js/aniso_class.mjs; select it with
// HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.  The result only has the right class and length here.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_trilinear_addon.cjs'));
const fields = require(path.join(__dirname, 'mock_field_addon.cjs'));      // (untraced)

const plain = (a) => (ArrayBuffer.isView(a) ? Array.from(a) : a);
const mock = Object.assign({}, base);
function anisoOf(entry, nField, fmtAt) {
    return (c, ...args) => {
        const fieldArgs = args.slice(0, nField), [plane, channels, W, H, maxAniso] = args.slice(nField);
        base.trace.push(['remapAniso' + entry, JSON.stringify(fieldArgs.map(plain)), plane.constructor.name, channels, W, H, maxAniso]);
        if (args.length !== nField + 5 || plane.length !== W * H * channels || fieldArgs[fmtAt] !== 1 || !Number.isInteger(maxAniso) || maxAniso < 1 || maxAniso > 16)
            throw ('hgwarp mock: remapAniso arguments');
        const field = fields['field' + entry](c, ...fieldArgs);
        return new plane.constructor(field.length / 2 * channels);
    };
}
mock.remapAnisoInverseGeometric = anisoOf('InverseGeometric', 7, 6);
mock.remapAnisoInversePiecewise = anisoOf('InversePiecewise', 1, 0);
module.exports = mock;
