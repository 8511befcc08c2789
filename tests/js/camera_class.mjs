// CPU: warpCamera(cameras, options) and cameraFromMatrices(matrix, options) of the drop-in class over tests/js/mock_camera_addon.cjs (run
// with HGWARP_ADDON pointing at it): the records it packs, the default window from the addon's cameraLimits, the option defaults and the
// codes of surfaces and outputs; the bare strings thrown; the shape of the result; the state the reference can see is the same after a
// call.  Prints one JSON line {ok, fails, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const last = () => addon.cameraCalls[addon.cameraCalls.length - 1];
const visible = (h) => JSON.stringify([h._map === null ? null : h._map.kind, h._lastPath, h._image === null, h._srcPoints === null ? null : Array.from(h._srcPoints),
                                       h._dstPoints === null ? null : Array.from(h._dstPoints), h._sampling, h._width, h._height]);
const image = (w, h, base) => ({ data: Uint8ClampedArray.from({ length: w * h * 4 }, (_, i) => (base + i) & 255), width: w, height: h });

const I = [1, 0, 0, 0, 1, 0, 0, 0, 1];
const yaw = (t) => [[Math.cos(t), 0, -Math.sin(t)], [0, 1, 0], [Math.sin(t), 0, Math.cos(t)]];
const cam0 = { rotation: I, focal: 80 }, cam1 = { rotation: yaw(0.5), focal: [90, 91], principal: [5.5, 4.25], distortion: [-0.1, 0.01, 0, 0.001, 0] };
const h = new Homography('projective', 12, 10);
h.setImage(image(12, 10, 3));
const before = visible(h);
const n0 = addon.trace.length;

// ---- defaults: a picture by the index field on the sphere, the instance's image, the windows of cameraLimits
let r = h.warpCamera([cam0, cam1], { scale: 50 });
ok(visible(h) === before, 'warpCamera changed the state of the instance');
ok(addon.cameraCalls.length === 1 && addon.trace.slice(n0).filter((x) => x[0] === 'warpCamera').length === 1, 'exactly one camera call');
let k = last();
ok(k.surface === 2 && k.scale === 50 && k.u0 === 0 && k.v0 === 0 && k.output === 0, `defaults: ${k.surface} ${k.scale} ${k.u0} ${k.v0} ${k.output}`);
ok(k.records.length === 64 && k.records.slice(0, 9).join() === I.join() && k.records[9] === 80 && k.records[10] === 80, 'record 0: R and one focal length for both axes');
ok(k.records[11] === 6 && k.records[12] === 5 && k.records[18] === Infinity, 'record 0: the principal point defaults to the centre; no distortion');
ok(k.records[32 + 9] === 90 && k.records[32 + 10] === 91 && k.records[32 + 11] === 5.5 && k.records[32 + 12] === 4.25, 'record 1: [fx, fy] and the principal point');
ok(k.records.slice(32 + 13, 32 + 18).join() === '-0.1,0.01,0,0.001,0' && k.records[32 + 18] === 1, 'record 1: the distortion');
ok(Math.abs(k.records[32 + 19] - 0.5) < 1e-15 && k.records[32 + 2] === -Math.sin(0.5), 'record 1: rows of three flatten row-major; a_c');
ok(k.windows.join() === '-12,-5,32,20,-12,-5,32,20', `the windows of cameraLimits: ${k.windows}`);
ok(addon.trace.slice(n0).filter((x) => x[0] === 'cameraLimits').every((x) => x.slice(1).join() === '12,10,2,50,0,0'), 'cameraLimits gets the source size and the canvas');
ok(k.W === 12 && k.H === 10 && k.nImages === 1 && k.images.length === 480 && k.images[5] === 8, 'the instance\'s image goes down');
ok(Array.isArray(r) && r.length === 2, 'one record per frame');
ok(Object.keys(r[0]).sort().join() === 'data,height,width,x,y', `keys: ${Object.keys(r[0])}`);
ok(r[0].data instanceof Uint8ClampedArray && r[0].data.length === 32 * 20 * 4 && r[0].width === 32 && r[0].height === 20 && r[0].x === -12 && r[0].y === -5, 'frame 0');
ok(r[1].data.length === 32 * 20 * 4 && r[1].data[0] === 16 && r[1].data[5] === 21, 'frame 1 starts at its 256-byte grain');

// ---- options
r = h.warpCamera([cam0], { surface: 'cylinder', scale: 33.5, center: [100.25, -7], sampling: 'bilinear', window: { x: -1, y: -2, width: 5, height: 3 } });
k = last();
ok(k.surface === 1 && k.scale === 33.5 && k.u0 === 100.25 && k.v0 === -7 && k.output === 1 && k.windows.join() === '-1,-2,5,3', 'explicit options reach the addon');
ok(r[0].data.length === 60 && r[0].x === -1 && r[0].y === -2, 'the explicit window');
r = h.warpCamera([cam0], { surface: 'plane', scale: 80, center: [6.4, 5.5] });
k = last();
ok(k.surface === 0 && k.windows.join() === '-4,1,32,20', `the default window follows the surface and the centre: ${k.windows}`);
r = h.warpCamera([cam0, cam1], { scale: 50, output: 'index', window: [{ x: 0, y: 0, width: 3, height: 2 }, { x: 1, y: 1, width: 0, height: 4 }] });
k = last();
ok(k.output === 2 && k.images === null && k.nImages === 0 && k.W === 12 && k.H === 10, 'a field needs the size only');
ok(r[0].data instanceof Int32Array && r[0].data.length === 6 && r[1].data.length === 0 && r[1].width === 0, 'index: one int32 per pixel; an empty window');
r = h.warpCamera([cam0], { scale: 50, output: 'coords', images: [image(7, 5, 1), image(7, 5, 9)] });
k = last();
ok(k.output === 3 && k.W === 7 && k.H === 5 && k.images === null && k.records[11] === 3.5 && k.records[12] === 2.5, 'coords with the size of the given images');
ok(r[0].data instanceof Float32Array && r[0].data.length === 27 * 15 * 2, 'coords: two float32 per pixel');
r = h.warpCamera([cam0, cam1, cam0], { scale: 50, images: [image(7, 5, 1), image(7, 5, 9)] });
k = last();
ok(k.output === 0 && k.nImages === 2 && k.images.length === 2 * 7 * 5 * 4 && k.images[140] === 9 && r.length === 3, 'two sources for three frames');
r = h.warpCamera([], { scale: 50 });
ok(Array.isArray(r) && r.length === 0 && last().windows.length === 0, 'no cameras: no frames');

// ---- refusals: bare strings, nothing reaches the addon's warpCamera
const calls = addon.cameraCalls.length;
const refused = [
    [() => h.warpCamera('cameras', { scale: 50 }), 'cameras must be an array'],
    [() => h.warpCamera([cam0]), 'options.scale'],
    [() => h.warpCamera([cam0], { scale: 0 }), 'options.scale'],
    [() => h.warpCamera([cam0], { scale: NaN }), 'options.scale'],
    [() => h.warpCamera([cam0], { scale: 50, surface: 'torus' }), 'options.surface'],
    [() => h.warpCamera([cam0], { scale: 50, center: [1] }), 'options.center'],
    [() => h.warpCamera([cam0], { scale: 50, center: [1, Infinity] }), 'options.center'],
    [() => h.warpCamera([cam0], { scale: 50, output: 'rgba' }), 'options.output'],
    [() => h.warpCamera([cam0], { scale: 50, sampling: 'bicubic' }), 'options.sampling'],
    [() => h.warpCamera([cam0], { scale: 50, window: { x: 0.5, y: 0, width: 4, height: 4 } }), 'options.window'],
    [() => h.warpCamera([cam0, cam1], { scale: 50, window: [{ x: 0, y: 0, width: 4, height: 4 }] }), 'one window per frame'],
    [() => h.warpCamera([cam0], { scale: 50, images: [] }), 'options.images'],
    [() => h.warpCamera([cam0], { scale: 50, images: [image(7, 5, 1), image(7, 6, 1)] }), 'one size'],
    [() => h.warpCamera([7], { scale: 50 }), 'camera 0 must be'],
    [() => h.warpCamera([cam0, { rotation: [1, 0, 0], focal: 80 }], { scale: 50 }), 'camera 1: rotation'],
    [() => h.warpCamera([{ rotation: I, focal: -1 }], { scale: 50 }), 'focal must be'],
    [() => h.warpCamera([{ rotation: I, focal: [80] }], { scale: 50 }), 'focal must be'],
    [() => h.warpCamera([{ rotation: I }], { scale: 50 }), 'focal must be'],
    [() => h.warpCamera([{ rotation: I, focal: 80, principal: [1, NaN] }], { scale: 50 }), 'principal must be'],
    [() => h.warpCamera([{ rotation: I, focal: 80, distortion: [0.1, 0.2] }], { scale: 50 }), 'distortion must be'],
    [() => h.warpCamera([{ rotation: [NaN, 0, 0, 0, 1, 0, 0, 0, 1], focal: 80 }], { scale: 50 }), 'hg_camera_pack_record'],
];
for (const [fn, word] of refused) {
    const e = thrown(fn);
    ok(typeof e === 'string' && e.includes(word), `refusal "${word}": ${e}`);
}
ok(addon.cameraCalls.length === calls, 'a refused call does not reach the addon');
const bare = new Homography('projective');
const e = thrown(() => bare.warpCamera([cam0], { scale: 50 }));
ok(typeof e === 'string' && e.includes('must receive an image'), `no image: ${e}`);
ok(typeof thrown(() => bare.warpCamera([cam0], { scale: 50, output: 'coords' })) === 'string', 'no size for a field');

// ---- cameraFromMatrices
const M = [2, 0.5, 30, 0.25, 3, -40, 0.001, 0.002, 1];
let c = h.cameraFromMatrices(M);
let f = addon.trace.filter((x) => x[0] === 'cameraFocals').pop()[1];
ok(f.join() === M.join(), 'principal points (0, 0): the matrix goes to the focal estimate as it is');
ok(c.okFrom && c.okTo && c.focalFrom === 130 && c.focalTo === 240 && c.rotation instanceof Float64Array && c.rotation.length === 9, 'both focal lengths and a rotation');
let q = addon.rotationCalls[addon.rotationCalls.length - 1];
ok(q.m.join() === M.join() && q.kFrom.join() === '130,130,0,0' && q.kTo.join() === '240,240,0,0', 'the rotation gets the pixel matrix and both intrinsics');
c = h.cameraFromMatrices(M.slice(0, 8), { principalFrom: [10, 20], principalTo: [3, 4] });
f = addon.trace.filter((x) => x[0] === 'cameraFocals').pop()[1];
const col2 = [2 * 10 + 0.5 * 20 + 30, 0.25 * 10 + 3 * 20 - 40, 0.001 * 10 + 0.002 * 20 + 1];
ok(Math.abs(f[2] - (col2[0] - 3 * col2[2])) < 1e-12 && Math.abs(f[5] - (col2[1] - 4 * col2[2])) < 1e-12 && Math.abs(f[8] - col2[2]) < 1e-15, `8 numbers get h8 = 1; the shifts by the principal points: ${f}`);
ok(Math.abs(f[0] - (2 - 3 * 0.001)) < 1e-15 && Math.abs(f[4] - (3 - 4 * 0.002)) < 1e-15 && f[6] === 0.001, 'T_to^-1 H T_from, the other entries');
q = addon.rotationCalls[addon.rotationCalls.length - 1];
ok(q.kFrom.slice(2).join() === '10,20' && q.kTo.slice(2).join() === '3,4', 'the principal points reach the rotation');
const n_rot = addon.rotationCalls.length;
c = h.cameraFromMatrices([1, 0, 0, 0, 1, 0, 0, 0, 1]);
ok(!c.okFrom && !c.okTo && c.rotation === null && c.focalFrom === null && addon.rotationCalls.length === n_rot, 'no focal length, no rotation');
c = h.cameraFromMatrices([1, 0, 0, 0, 1, 0, 0, 0, 1], { focalFrom: 500, focalTo: [600, 610] });
q = addon.rotationCalls[addon.rotationCalls.length - 1];
ok(c.okFrom && c.okTo && c.focalFrom === 500 && c.focalTo.join() === '600,610' && q.kFrom.join() === '500,500,0,0' && q.kTo.join() === '600,610,0,0', 'given focal lengths skip the estimate');
for (const [fn, word] of [[() => h.cameraFromMatrices([1, 2, 3]), '9 (or 8)'], [() => h.cameraFromMatrices([1, 0, 0, 0, 1, 0, 0, 0, NaN]), '9 (or 8)'],
                          [() => h.cameraFromMatrices(M, { principalFrom: [1] }), 'principalFrom'], [() => h.cameraFromMatrices(M, { focalTo: -3 }), 'focalTo']]) {
    const e2 = thrown(fn);
    ok(typeof e2 === 'string' && e2.includes(word), `refusal "${word}": ${e2}`);
}
h.close(); bare.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails, checks }));
process.exit(fails.length === 0 ? 0 : 1);
