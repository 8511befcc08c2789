// mock_field_addon.cjs -- tests/js/mock_addon.cjs plus the FIELD entry points of the addon, for one purpose: running
// tests/js/field_forward_gpu.mjs without a GPU (select it with HGWARP_ADDON=<this file>), so that the class's side of sourceField(format,
// {loop}) -- which loop it picks, what it hands to the native layer, what it refuses -- is checked in the build container.
// TEST INFRASTRUCTURE ONLY.  An index field is the JavaScript oracle's warp of an image whose pixel i holds the uint32 i + 1, minus 1 (the
// model of tests/hgtest/fwd_field.py); a coordinate field only says where that index is -1 (NaN) -- its values are the GPU tests' business.
'use strict';
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon.cjs'));

function ranked(c, warp) {
    const keep = c.image, n = c.W * c.H, rank = new Uint32Array(n);
    for (let i = 0; i < n; i++) rank[i] = i + 1;
    c.image = new Uint8ClampedArray(rank.buffer);
    try {
        const out = warp();
        return Int32Array.from(new Uint32Array(out.buffer, out.byteOffset, out.length / 4), (v) => v - 1);
    } finally { c.image = keep; }
}
const coords = (idx) => { const f = new Float32Array(2 * idx.length); idx.forEach((v, i) => { f[2 * i] = f[2 * i + 1] = v < 0 ? NaN : 0; }); return f; };

mock.setSampling = () => {};
mock.fieldForwardPiecewise = (c, dst, maxX, maxY, xo, yo, ow, oh) => ranked(c, () => mock.warpForwardPiecewise(c, dst, maxX, maxY, xo, yo, ow, oh));
mock.fieldForwardGeometric = (c, kind, m, xo, yo, ow, oh) => ranked(c, () => mock.warpForwardGeometric(c, kind, m, xo, yo, ow, oh));
mock.fieldInversePiecewise = (c, fmt) => { const idx = ranked(c, () => mock.warpInversePiecewise(c)); return fmt === 0 ? idx : coords(idx); };
mock.fieldInverseGeometric = (c, kind, inv, xo, yo, ow, oh, fmt) => { const idx = ranked(c, () => mock.warpInverseGeometric(c, kind, inv, xo, yo, ow, oh)); return fmt === 0 ? idx : coords(idx); };
module.exports = mock;
