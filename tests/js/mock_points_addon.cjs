// mock_points_addon.cjs -- tests/js/mock_remap_addon.cjs plus the POINTS entry points of the addon, with the same trace, for one purpose:
// checking without a GPU that transformPoints() of the drop-in class asks the native layer for exactly the geometry sourceField() would
// (tests/js/points_class.mjs; select it with HGWARP_ADDON=<this file>).
// TEST INFRASTRUCTURE ONLY.  points<Entry>(ctx, <field<Entry>'s arguments>, points) returns a Float32Array of the list's length holding
// each coordinate plus 1000: the values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_remap_addon.cjs'));

const plain = (a) => (ArrayBuffer.isView(a) ? Array.from(a) : a);
const mock = Object.assign({}, base);
function pointsOf(entry, nField) {
    return (c, ...args) => {
        const fieldArgs = args.slice(0, nField), pts = args[nField];
        base.trace.push(['points' + entry, JSON.stringify(fieldArgs.map(plain)), pts.constructor.name, pts.length]);
        if (args.length !== nField + 1 || !(pts instanceof Float32Array) || pts.length % 2) throw ('hgwarp mock: points arguments');
        return Float32Array.from(pts, (v) => v + 1000);
    };
}
mock.pointsInverseGeometric = pointsOf('InverseGeometric', 7);
mock.pointsInversePiecewise = pointsOf('InversePiecewise', 1);
mock.pointsForwardGeometric = pointsOf('ForwardGeometric', 6);
mock.pointsForwardPiecewise = pointsOf('ForwardPiecewise', 7);
module.exports = mock;
