// mock_camera_addon.cjs -- tests/js/mock_fit_addon.cjs plus the addon's camera functions, with the same trace, for one purpose: checking
// without a GPU what warpCamera() and cameraFromMatrices() of the drop-in class hand to the native layer (tests/js/camera_class.mjs; select
// it with HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.
//   cameraPackRecord(R, fx, fy, cx, cy, dist | null, W, H) -> Float64Array(32): the slots of the header's record, r2_max = Infinity without
//     a distortion and 1 with one, a_c = atan2(R6, R8); throws for an R whose first entry is not finite.
//   cameraLimits(record, W, H, surface, scale, u0, v0) -> Int32Array [round(u0) - 10 - surface, round(v0) - 5, W + 20, H + 10].
//   cameraFocals(H) -> Float64Array [|h2| + 100, |h5| + 200, h6 !== 0, h7 !== 0].
//   cameraRotation(H, kFrom, kTo) records its arguments and returns the identity.
//   warpCamera(ctx, records, windows, surface, scale, u0, v0, output, images | null, W, H, nImages) records its arguments and returns
//     { data }: the frames packed at the 256-byte grain, 4 bytes per pixel (8 for output 3), byte k of frame f = (f * 16 + k) & 255.
// The values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_fit_addon.cjs'));

const mock = Object.assign({}, base);
mock.cameraCalls = [];
mock.rotationCalls = [];
mock.cameraPackRecord = (R, fx, fy, cx, cy, dist, W, H, ...rest) => {
    if (rest.length || !(R instanceof Float64Array) || R.length !== 9 || (dist !== null && (!(dist instanceof Float64Array) || dist.length !== 5)))
        throw ('hgwarp mock: cameraPackRecord arguments');
    if (!Number.isFinite(R[0])) throw ('hg_camera_pack_record failed: every number must be finite');
    base.trace.push(['cameraPackRecord', fx, fy, cx, cy, dist === null ? null : Array.from(dist), W, H]);
    const rec = new Float64Array(32);
    rec.set(R, 0);
    rec.set([fx, fy, cx, cy], 9);
    if (dist !== null) rec.set(dist, 13);
    rec[18] = dist === null ? Infinity : 1;
    rec[19] = Math.atan2(R[6], R[8]);
    return rec;
};
mock.cameraLimits = (record, W, H, surface, scale, u0, v0, ...rest) => {
    if (rest.length || !(record instanceof Float64Array) || record.length !== 32) throw ('hgwarp mock: cameraLimits arguments');
    base.trace.push(['cameraLimits', W, H, surface, scale, u0, v0]);
    return Int32Array.from([Math.round(u0) - 10 - surface, Math.round(v0) - 5, W + 20, H + 10]);
};
mock.cameraFocals = (m, ...rest) => {
    if (rest.length || !(m instanceof Float64Array) || m.length !== 9) throw ('hgwarp mock: cameraFocals arguments');
    base.trace.push(['cameraFocals', Array.from(m)]);
    return Float64Array.from([Math.abs(m[2]) + 100, Math.abs(m[5]) + 200, m[6] !== 0 ? 1 : 0, m[7] !== 0 ? 1 : 0]);
};
mock.cameraRotation = (m, kFrom, kTo, ...rest) => {
    if (rest.length || !(m instanceof Float64Array) || m.length !== 9 || !(kFrom instanceof Float64Array) || kFrom.length !== 4 || !(kTo instanceof Float64Array) || kTo.length !== 4)
        throw ('hgwarp mock: cameraRotation arguments');
    mock.rotationCalls.push({ m: Array.from(m), kFrom: Array.from(kFrom), kTo: Array.from(kTo) });
    return Float64Array.from([1, 0, 0, 0, 1, 0, 0, 0, 1]);
};
mock.warpCamera = (c, records, windows, surface, scale, u0, v0, output, images, W, H, nImages, ...rest) => {
    if (rest.length || !(records instanceof Float64Array) || !(windows instanceof Int32Array) || windows.length % 4 || records.length !== (windows.length / 4) * 32 ||
        (images !== null && !(images instanceof Uint8Array)) || (output < 2 && (images === null || images.length !== nImages * W * H * 4)))
        throw ('hgwarp mock: warpCamera arguments');
    const F = windows.length / 4, px = output === 3 ? 8 : 4;
    base.trace.push(['warpCamera', F, surface, scale, u0, v0, output, W, H, nImages]);
    mock.cameraCalls.push({ records: Float64Array.from(records), windows: Array.from(windows), surface, scale, u0, v0, output,
                            images: images === null ? null : Uint8Array.from(images), W, H, nImages });
    let total = 0;
    for (let f = 0; f < F; f++) total += (Math.max(windows[4 * f + 2], 0) * Math.max(windows[4 * f + 3], 0) * px + 255) & ~255;
    const data = new Uint8Array(total);
    let off = 0;
    for (let f = 0; f < F; f++) {
        const n = Math.max(windows[4 * f + 2], 0) * Math.max(windows[4 * f + 3], 0) * px;
        for (let k = 0; k < n; k++) data[off + k] = (f * 16 + k) & 255;
        off += (n + 255) & ~255;
    }
    return { data };
};
module.exports = mock;
