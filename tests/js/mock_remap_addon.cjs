// mock_remap_addon.cjs -- tests/js/mock_field_addon.cjs plus the REMAP entry points of the addon, with a trace of every field-side call
// and its arguments, for one purpose: checking without a GPU that remap() of the drop-in class asks the native layer for exactly the
// field sourceField() would (tests/js/remap_class.mjs; select it with HGWARP_ADDON=<this file>).
// TEST INFRASTRUCTURE ONLY.  remap<Entry>(ctx, <field<Entry>'s arguments>, plane, channels, W, H) gathers the plane through the mock's own
// index field; a bilinear remap only has the right class and length here -- its values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_field_addon.cjs'));

const trace = [];                                            // [name, JSON of the arguments after the context]
const plain = (a) => (ArrayBuffer.isView(a) ? Array.from(a) : a);
const mock = Object.assign({}, base, { trace });
for (const name of ['setImage', 'piecewiseSetMesh', 'piecewisePrepare', 'fieldInverseGeometric', 'fieldInversePiecewise', 'fieldForwardGeometric', 'fieldForwardPiecewise']) {
    mock[name] = (c, ...args) => { trace.push([name, JSON.stringify(args.map(plain))]); return base[name](c, ...args); };
}
function remapOf(entry, nField, fmtAt) {
    return (c, ...args) => {
        const fieldArgs = args.slice(0, nField), [plane, channels, W, H] = args.slice(nField);
        trace.push(['remap' + entry, JSON.stringify(fieldArgs.map(plain)), plane.constructor.name, channels, W, H]);
        if (args.length !== nField + 4 || plane.length !== W * H * channels) throw ('hgwarp mock: remap arguments');
        const fmt = fmtAt < 0 ? 0 : fieldArgs[fmtAt];
        const field = base['field' + entry](c, ...fieldArgs), px = fmt === 0 ? field.length : field.length / 2;
        const out = new plane.constructor(px * channels);
        if (fmt === 0) for (let i = 0; i < px; i++) if (field[i] >= 0) for (let k = 0; k < channels; k++) out[i * channels + k] = plane[field[i] * channels + k];
        return out;
    };
}
mock.remapInverseGeometric = remapOf('InverseGeometric', 7, 6);
mock.remapInversePiecewise = remapOf('InversePiecewise', 1, 0);
mock.remapForwardGeometric = remapOf('ForwardGeometric', 6, -1);
mock.remapForwardPiecewise = remapOf('ForwardPiecewise', 7, -1);
module.exports = mock;
