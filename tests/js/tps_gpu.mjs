// GPU: warpThinPlate() of the drop-in class on the real addon.  The picture of output 'image' must equal gathering the source through the
// call's own index field (zeros where the index is -1), for the instance's image and for two sources over three frames, at step 1 and on
// the lattice; a frame with a NaN landmark fails alone; 'coords' rounds to the index where it is covered.  Exit code 1 on a failure.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const W = 96, H = 64;
const image = (base) => ({ data: Uint8ClampedArray.from({ length: W * H * 4 }, (_, i) => ((i * 7 + (i >> 3) * 13 + base) & 255)), width: W, height: H });
const src = [], d0 = [], d1 = [];
for (let j = 0; j < 4; j++) for (let i = 0; i < 5; i++) {
    const x = 4 + i * 22, y = 3 + j * 19;
    src.push([x, y]);
    d0.push([x * 1.1 + 6 * Math.sin(y / 17) - 20, y * 0.9 + 5 * Math.cos(x / 23) + 4]);
    d1.push([x * 0.8 + 3 * Math.cos(y / 11) + 10, y * 1.2 - 4 * Math.sin(x / 19) - 15]);
}
const gather = (index, img) => {
    const out = new Uint8ClampedArray(index.length * 4);
    for (let k = 0; k < index.length; k++) if (index[k] >= 0) out.set(img.data.subarray(index[k] * 4, index[k] * 4 + 4), k * 4);
    return out;
};
const same = (a, b) => a.length === b.length && a.every((v, k) => v === b[k]);

const h = new Homography('piecewiseaffine', W, H);
const im0 = image(1), im1 = image(77);
h.setImage(im0);
for (const step of [1, 4]) {
    const pics = h.warpThinPlate(src, [d0, d1], { step });
    const idx = h.warpThinPlate(src, [d0, d1], { step, output: 'index' });
    for (let f = 0; f < 2; f++) {
        check(pics[f].status === 0 && idx[f].status === 0, `step ${step}: frame ${f} solves`);
        check(pics[f].width === idx[f].width && pics[f].height === idx[f].height && pics[f].x === idx[f].x && pics[f].y === idx[f].y, `step ${step}: frame ${f}: one window`);
        const covered = idx[f].data.reduce((n, v) => n + (v >= 0 ? 1 : 0), 0);
        check(covered > idx[f].data.length / 4 && idx[f].data.every((v) => v >= -1 && v < W * H), `step ${step}: frame ${f}: ${covered} of ${idx[f].data.length} pixels covered`);
        check(same(pics[f].data, gather(idx[f].data, im0)), `step ${step}: frame ${f}: the picture is the gather through its own index field`);
    }
}
// two sources over three frames, one of them with a NaN landmark
const bad = d0.map((p) => p.slice()); bad[3][1] = NaN;
const win = { x: -10, y: -5, width: 70, height: 41 };
const pics = h.warpThinPlate(src, [d0, bad, d1], { images: [im0, im1], window: win });
const idx = h.warpThinPlate(src, [d0, bad, d1], { images: [im0, im1], window: win, output: 'index' });
const co = h.warpThinPlate(src, [d0, bad, d1], { images: [im0, im1], window: win, output: 'coords' });
check(pics.map((p) => p.status).join() === '0,2,0', `statuses ${pics.map((p) => p.status)}`);
check(same(pics[0].data, gather(idx[0].data, im0)) && same(pics[2].data, gather(idx[2].data, im0)), 'frames 0 and 2 read source 0');
check(pics[1].data.every((v) => v === 0) && idx[1].data.every((v) => v === -1) && co[1].data.every((v) => Number.isNaN(v)), 'the failed frame is empty');
let agree = true;
for (let k = 0; k < idx[2].data.length; k++) {
    const x = co[2].data[2 * k], y = co[2].data[2 * k + 1];
    if (Number.isNaN(x) !== (idx[2].data[k] < 0)) agree = false;
}
check(agree, 'coords and index agree on the coverage');
const bl = h.warpThinPlate(src, [d0], { sampling: 'bilinear', window: win });
check(bl[0].data.length === pics[0].data.length && bl[0].data.some((v) => v !== 0), 'a bilinear picture');
h.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails }));
process.exit(fails.length === 0 ? 0 : 1);
