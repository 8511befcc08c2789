// CPU: detectAndDescribe(images, options) of the drop-in class over tests/js/mock_detect_addon.cjs (run with HGWARP_ADDON pointing at it):
// the pictures are packed back to back; the option defaults; the bare strings thrown; the shape of the result, which matchDescriptors
// accepts as sets and points; no image is needed and the state the reference can see is the same after a call.  Prints one JSON line
// {ok, fails, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const last = () => addon.detectCalls[addon.detectCalls.length - 1];
const visible = (h) => JSON.stringify([h._map === null ? null : h._map.kind, h._pm === null || h._pm === undefined ? null : 1, h._lastPath, h._image === null,
                                       h._srcPoints === null ? null : Array.from(h._srcPoints), h._dstPoints === null ? null : Array.from(h._dstPoints), h._sampling]);
const pic = (n, base) => Uint8Array.from({ length: n }, (_, i) => (base + 3 * i) & 255);

// ---- defaults and packing; no image was ever set
const h = new Homography('projective', 64, 48);
const before = visible(h);
const n0 = addon.trace.length;
const W = 40, H = 36;
const imgs = [pic(W * H * 4, 1), pic(W * H * 4, 77), pic(W * H * 4, 200)];
const r = h.detectAndDescribe(imgs, { width: W, height: H });
ok(visible(h) === before, 'detectAndDescribe changed the state of the instance');
ok(addon.detectCalls.length === 1 && addon.trace.slice(n0).filter((x) => x[0] !== 'create').length === 1, 'exactly one addon call (besides the context)');
let k = last();
ok(k.nPlanes === 3 && k.width === W && k.height === H && k.channels === 4 && k.cell === 32 && k.perCell === 2 && k.minResponse === 1e10,
   `defaults: ${JSON.stringify([k.nPlanes, k.width, k.height, k.channels, k.cell, k.perCell, k.minResponse])}`);
ok(k.planes.length === 3 * W * H * 4 && imgs.every((im, f) => k.planes.slice(f * W * H * 4, (f + 1) * W * H * 4).join() === im.join()), 'the pictures back to back');
// ---- the result: 2 x 2 cells x 2 = 8 slots per picture, 1, 2, 3 keypoints
ok(Array.isArray(r) && r.length === 3 && r.every((x) => x.points instanceof Float32Array && x.descriptors instanceof Uint8Array), 'one record per picture');
ok(r.every((x, f) => x.count === f + 1 && x.points.length === 2 * x.count && x.descriptors.length === 32 * x.count), 'count, and only the slots in use');
ok(r[2].points.join() === '20,200,21,201,22,202' && r[1].descriptors[32] === 2 && r[1].descriptors[63] === 33, 'the values of the slots in use, none of the padding');
ok(Object.keys(r[0]).sort().join() === 'count,descriptors,points', `keys: ${Object.keys(r[0])}`);
// ---- the result goes into matchDescriptors as it stands
const m = h.matchDescriptors(r.slice(1).map((x) => x.descriptors), [r[0].descriptors], { queryPoints: r.slice(1).map((x) => x.points), trainPoints: [r[0].points] });
ok(m.length === 2 && m[0].matches instanceof Float32Array, 'descriptors and points through matchDescriptors');
const mk = addon.matchCalls[addon.matchCalls.length - 1];
ok(mk.kind === 0 && mk.descBytes === 32 && mk.nQuery === 3 && mk.nTrain === 1 && JSON.stringify(mk.countsQ) === '[2,3]', 'as binary rows of 32 bytes with their counts');
// ---- explicit options
h.detectAndDescribe([pic(W * H, 5)], { width: W, height: H, channels: 1, cell: 8, perCell: 16, minResponse: 1 });
k = last();
ok(k.channels === 1 && k.cell === 8 && k.perCell === 16 && k.minResponse === 1 && k.planes.length === W * H, 'explicit options reach the addon');
h.detectAndDescribe([new Uint8ClampedArray(W * H * 4)], { width: W, height: H, minResponse: 2 ** 53 });
ok(last().minResponse === 2 ** 53 && last().planes instanceof Uint8Array, 'a clamped array (ImageData) is a picture; 2^53 is legal');
ok(h.detectAndDescribe([], { width: W, height: H }).length === 0 && last().nPlanes === 0, 'no pictures');
// ---- the thrown strings
const n1 = addon.detectCalls.length;
const o = (x) => Object.assign({ width: W, height: H }, x);
const refusals = [
    [() => h.detectAndDescribe(imgs), 'width'], [() => h.detectAndDescribe(imgs, null), 'width'], [() => h.detectAndDescribe(imgs, { width: W }), 'height'],
    [() => h.detectAndDescribe(imgs, o({ width: 0 })), 'width'], [() => h.detectAndDescribe(imgs, o({ height: 32769 })), 'height'], [() => h.detectAndDescribe(imgs, o({ width: 40.5 })), 'width'],
    [() => h.detectAndDescribe(imgs, o({ channels: 3 })), 'channels'], [() => h.detectAndDescribe(imgs, o({ channels: '4' })), 'channels'],
    [() => h.detectAndDescribe(imgs, o({ cell: 7 })), 'cell'], [() => h.detectAndDescribe(imgs, o({ cell: 257 })), 'cell'], [() => h.detectAndDescribe(imgs, o({ cell: 16.5 })), 'cell'],
    [() => h.detectAndDescribe(imgs, o({ perCell: 0 })), 'perCell'], [() => h.detectAndDescribe(imgs, o({ perCell: 17 })), 'perCell'],
    [() => h.detectAndDescribe(imgs, o({ minResponse: 0 })), 'minResponse'], [() => h.detectAndDescribe(imgs, o({ minResponse: 1.5 })), 'minResponse'],
    [() => h.detectAndDescribe(imgs, o({ minResponse: 2 ** 53 + 2 })), 'minResponse'], [() => h.detectAndDescribe(imgs, o({ minResponse: NaN })), 'minResponse'],
    [() => h.detectAndDescribe(imgs, o({ minResponse: '5' })), 'minResponse'],
    [() => h.detectAndDescribe([], { width: 2048, height: 2048, cell: 8, perCell: 2 }), '65536'],
    [() => h.detectAndDescribe(imgs[0], o({})), 'images'], [() => h.detectAndDescribe([imgs[0], Array.from(imgs[1])], o({})), 'picture 1'],
    [() => h.detectAndDescribe([imgs[0], imgs[1].slice(1)], o({})), 'picture 1'], [() => h.detectAndDescribe(imgs, o({ channels: 1 })), 'picture 0'],
];
for (const [fn, word] of refusals) {
    const e = thrown(fn);
    ok(typeof e === 'string' && e.startsWith('detectAndDescribe:') && e.includes(word), `a refusal must be a bare string of detectAndDescribe naming ${word} (got ${e})`);
}
ok(addon.detectCalls.length === n1, 'a refused call reaches no addon function');
ok(visible(h) === before, 'the state of the instance after all of it');

const res = { ok: fails.length === 0, fails, checks };
console.log(JSON.stringify(res));
process.exit(res.ok ? 0 : 1);
