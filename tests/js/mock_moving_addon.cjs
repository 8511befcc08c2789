// mock_moving_addon.cjs -- mock_sampling_addon.cjs plus the batch entry point for frames that bring their own source points
// (warpInversePiecewiseSrcBatch of lib/hgwarp.node), answered by the JavaScript oracle's loop once per frame with exactly the source points,
// source minima, destiny points, window and image the class hands over.  TEST INFRASTRUCTURE ONLY (tests/js/moving_class.mjs;
// HGWARP_ADDON=<this file>): it proves what the class asks the native layer for; that the native layer computes it is what the GPU tests prove.
'use strict';
const path = require('path');
const base = require('./mock_sampling_addon.cjs');
const core = require(path.join(__dirname, '..', '..', 'oracle', 'hg_oracle_core.cjs'));

const shim = Object.assign({}, base, {
    srcBatchFrames: 0,
    warpInversePiecewiseSrcBatch(c, src, mins, dst, g, own, images, w, h) {
        base.calls.push('warpInversePiecewiseSrcBatch');
        if (images) base.setImages(c, images, w, h);
        if (!c.image && !c.images) throw ('hgwarp mock: no source image');
        const n = c.mesh.src.length, F = g.length / 4, out = [];
        if (src.length !== F * n || dst.length !== F * n || mins.length !== 2 * F) throw ('hgwarp mock: warpInversePiecewiseSrcBatch: sizes do not match the mesh');
        for (let k = 0; k < F; k++) {
            const img = c.images ? c.images[k % c.images.length] : c.image;
            out.push(core.warpInversePiecewise(src.subarray(k * n, (k + 1) * n), dst.subarray(k * n, (k + 1) * n), c.mesh.tris, img, c.W, c.H,
                                               mins[2 * k], mins[2 * k + 1], g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]).out);
        }
        shim.srcBatchFrames += F;
        return out;
    },
});
module.exports = shim;
