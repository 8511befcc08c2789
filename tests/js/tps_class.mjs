// CPU: warpThinPlate(sourcePoints, destinyPointSets, options) of the drop-in class over tests/js/mock_tps_addon.cjs (run with HGWARP_ADDON
// pointing at it): the destiny sets go down as the FROM lists and the source points as the one TO list; the default window is the integer
// bounding box of each destiny set; the option defaults and the codes of the outputs; the bare strings thrown; the shape of the result;
// the state the reference can see is the same after a call.  Prints one JSON line {ok, fails, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const last = () => addon.tpsCalls[addon.tpsCalls.length - 1];
const visible = (h) => JSON.stringify([h._map === null ? null : h._map.kind, h._lastPath, h._image === null, h._srcPoints === null ? null : Array.from(h._srcPoints),
                                       h._dstPoints === null ? null : Array.from(h._dstPoints), h._sampling, h._width, h._height]);
const image = (w, h, base) => ({ data: Uint8ClampedArray.from({ length: w * h * 4 }, (_, i) => (base + i) & 255), width: w, height: h });

const src = [[0, 0], [10, 0], [0, 8], [10, 8]];
const d0 = [[2.5, 1], [12, 1.5], [2, 9], [13.25, 9.75]], d1 = Float32Array.from([-3.5, -2, 6, -1, -3, 5, 7, 6.5]);
const h = new Homography('piecewiseaffine', 12, 10);
h.setImage(image(12, 10, 3));
const before = visible(h);
const n0 = addon.trace.length;

// ---- defaults: a picture by the index field, the instance's image, the bounding boxes
let r = h.warpThinPlate(src, [d0, d1]);
ok(visible(h) === before, 'warpThinPlate changed the state of the instance');
ok(addon.tpsCalls.length === 1 && addon.trace.slice(n0).filter((x) => x[0] === 'warpThinPlate').length === 1, 'exactly one thin-plate call');
let k = last();
ok(k.nFromSets === 2 && k.nToSets === 1 && k.nPoints === 4, `sets: ${k.nFromSets} ${k.nToSets} ${k.nPoints}`);
ok(k.from.join() === [...d0.flat(), ...d1].join() && k.to.join() === src.flat().join(), 'destiny sets are the FROM lists, the source points the TO list');
ok(k.smoothing === 0 && k.step === 1 && k.output === 0, `defaults: ${k.smoothing} ${k.step} ${k.output}`);
ok(k.windows.join() === '2,1,13,10,-4,-2,12,10', `bounding boxes: ${k.windows}`);
ok(k.W === 12 && k.H === 10 && k.nImages === 1 && k.images.length === 480 && k.images[5] === 8, 'the instance\'s image goes down');
ok(Array.isArray(r) && r.length === 2, 'one record per frame');
ok(Object.keys(r[0]).sort().join() === 'data,height,status,width,x,y', `keys: ${Object.keys(r[0])}`);
ok(r[0].data instanceof Uint8ClampedArray && r[0].data.length === 13 * 10 * 4 && r[0].width === 13 && r[0].height === 10 && r[0].x === 2 && r[0].y === 1 && r[0].status === 0, 'frame 0');
ok(r[1].data.length === 12 * 10 * 4 && r[1].x === -4 && r[1].y === -2 && r[1].status === 1 && r[1].data[0] === 16 && r[1].data[5] === 21, 'frame 1 starts at its 256-byte grain');

// ---- options
r = h.warpThinPlate(Float32Array.from(src.flat()), [d0], { smoothing: 0.5, step: 8, sampling: 'bilinear', window: { x: -1, y: -2, width: 5, height: 3 } });
k = last();
ok(k.smoothing === 0.5 && k.step === 8 && k.output === 1 && k.windows.join() === '-1,-2,5,3', 'explicit options reach the addon');
ok(r[0].data.length === 60 && r[0].x === -1 && r[0].y === -2, 'the explicit window');
r = h.warpThinPlate(src, [d0, d1], { output: 'index', window: [{ x: 0, y: 0, width: 3, height: 2 }, { x: 1, y: 1, width: 0, height: 4 }] });
k = last();
ok(k.output === 2 && k.images === null && k.nImages === 0 && k.W === 12 && k.H === 10, 'a field needs the size only');
ok(r[0].data instanceof Int32Array && r[0].data.length === 6 && r[1].data.length === 0 && r[1].width === 0, 'index: one int32 per pixel; an empty window');
r = h.warpThinPlate(src, [d0], { output: 'coords', images: [image(7, 5, 1), image(7, 5, 9)] });
k = last();
ok(k.output === 3 && k.W === 7 && k.H === 5 && k.images === null, 'coords with the size of the given images');
ok(r[0].data instanceof Float32Array && r[0].data.length === 13 * 10 * 2, 'coords: two float32 per pixel');
r = h.warpThinPlate(src, [d0, d1, d0], { images: [image(7, 5, 1), image(7, 5, 9)] });
k = last();
ok(k.output === 0 && k.nImages === 2 && k.images.length === 2 * 7 * 5 * 4 && k.images[140] === 9 && r[2].status === 2, 'two sources for three frames');
const nanSet = [[NaN, 1], [12, 1.5], [2, 9], [13, 9]];
r = h.warpThinPlate(src, [nanSet], { output: 'coords' });
ok(last().windows.join() === '0,0,0,0' && r[0].data.length === 0, 'a destiny set with a NaN gets an empty default window');

// ---- refusals: bare strings, nothing reaches the addon
const calls = addon.tpsCalls.length;
const refused = [
    [() => h.warpThinPlate(src.slice(0, 2), [d0.slice(0, 2)]), '3 to 1024 landmarks'],
    [() => h.warpThinPlate('points', [d0]), 'sourcePoints must be'],
    [() => h.warpThinPlate(Float32Array.from([1, 2, 3, 4, 5, 6, 7]), [d0]), 'x, y pairs'],
    [() => h.warpThinPlate(src, d0), 'same amount of destiny points'],
    [() => h.warpThinPlate(src, [7]), 'destiny point set 0 must be'],
    [() => h.warpThinPlate(src, 'sets'), 'destinyPointSets must be an array'],
    [() => h.warpThinPlate(src, [d0.slice(0, 3)]), 'same amount of destiny points'],
    [() => h.warpThinPlate(src, [d0], { smoothing: -1 }), 'options.smoothing'],
    [() => h.warpThinPlate(src, [d0], { smoothing: NaN }), 'options.smoothing'],
    [() => h.warpThinPlate(src, [d0], { step: 3 }), 'options.step'],
    [() => h.warpThinPlate(src, [d0], { output: 'rgba' }), 'options.output'],
    [() => h.warpThinPlate(src, [d0], { sampling: 'bicubic' }), 'options.sampling'],
    [() => h.warpThinPlate(src, [d0], { window: { x: 0.5, y: 0, width: 4, height: 4 } }), 'options.window'],
    [() => h.warpThinPlate(src, [d0, d1], { window: [{ x: 0, y: 0, width: 4, height: 4 }] }), 'one window per frame'],
    [() => h.warpThinPlate(src, [d0], { images: [] }), 'options.images'],
    [() => h.warpThinPlate(src, [d0], { images: [image(7, 5, 1), image(7, 6, 1)] }), 'one size'],
];
for (const [fn, word] of refused) {
    const e = thrown(fn);
    ok(typeof e === 'string' && e.includes(word), `refusal "${word}": ${e}`);
}
ok(addon.tpsCalls.length === calls, 'a refused call does not reach the addon');
const bare = new Homography('piecewiseaffine');
const e = thrown(() => bare.warpThinPlate(src, [d0]));
ok(typeof e === 'string' && e.includes('must receive an image'), `no image: ${e}`);
ok(typeof thrown(() => bare.warpThinPlate(src, [d0], { output: 'coords' })) === 'string', 'no size for a field');
h.close(); bare.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails, checks }));
process.exit(fails.length === 0 ? 0 : 1);
