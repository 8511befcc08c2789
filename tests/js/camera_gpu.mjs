// GPU: warpCamera() of the drop-in class on the real addon.  The picture of output 'image' must equal gathering the source through the
// call's own index field (zeros where the index is -1), on the three surfaces, with the default windows (hg_camera_limits) and with two
// sources over three frames; 'coords' and 'index' agree on the coverage; a camera looking away is empty; cameraFromMatrices gives back the
// focal lengths and the rotation of a synthetic homography.  Exit code 1 on a failure.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const W = 96, H = 64;
const image = (base) => ({ data: Uint8ClampedArray.from({ length: W * H * 4 }, (_, i) => ((i * 7 + (i >> 3) * 13 + base) & 255)), width: W, height: H });
const yaw = (t) => [[Math.cos(t), 0, -Math.sin(t)], [0, 1, 0], [Math.sin(t), 0, Math.cos(t)]];
const gather = (index, img) => {
    const out = new Uint8ClampedArray(index.length * 4);
    for (let k = 0; k < index.length; k++) if (index[k] >= 0) out.set(img.data.subarray(index[k] * 4, index[k] * 4 + 4), k * 4);
    return out;
};
const same = (a, b) => a.length === b.length && a.every((v, k) => v === b[k]);

const h = new Homography('projective', W, H);
const im0 = image(1), im1 = image(77);
h.setImage(im0);
const cams = [{ rotation: yaw(-0.4), focal: 80, principal: [47.6, 31.7] }, { rotation: yaw(0.45), focal: [82, 81], distortion: [-0.08, 0.01, 0.001, 0, 0] }];
for (const surface of ['plane', 'cylinder', 'sphere']) {
    const opt = { surface, scale: 80, center: [3.3, -2.7] };
    const pics = h.warpCamera(cams, opt);
    const idx = h.warpCamera(cams, { ...opt, output: 'index' });
    const co = h.warpCamera(cams, { ...opt, output: 'coords' });
    for (let f = 0; f < 2; f++) {
        check(pics[f].width === idx[f].width && pics[f].height === idx[f].height && pics[f].x === idx[f].x && pics[f].y === idx[f].y, `${surface}: frame ${f}: one window`);
        check(pics[f].width >= 0.8 * W && pics[f].width < 4 * W && pics[f].height >= 0.8 * H && pics[f].height < 3 * H, `${surface}: frame ${f}: a window of the picture's order: ${pics[f].width} x ${pics[f].height}`);
        const covered = idx[f].data.reduce((n, v) => n + (v >= 0 ? 1 : 0), 0);
        check(covered > W * H / 2 && idx[f].data.every((v) => v >= -1 && v < W * H), `${surface}: frame ${f}: ${covered} of ${idx[f].data.length} pixels covered`);
        check(same(pics[f].data, gather(idx[f].data, im0)), `${surface}: frame ${f}: the picture is the gather through its own index field`);
        let agree = true, border = true;
        for (let k = 0; k < idx[f].data.length; k++) {       // the index is the rounded coordinate where that lies in the array, else -1
            const x = co[f].data[2 * k], y = co[f].data[2 * k + 1];
            const at = Math.floor(y + 0.5) * W + Math.floor(x + 0.5);
            const want = Number.isNaN(x) || at < 0 || at >= W * H ? -1 : at;
            // (the coordinate is the float32 of the double the index was rounded from: a tie of the double may round the other way)
            const tie = Math.abs(x + 0.5 - Math.round(x + 0.5)) < 1e-4 || Math.abs(y + 0.5 - Math.round(y + 0.5)) < 1e-4;
            if (idx[f].data[k] !== want && !(tie && !Number.isNaN(x))) agree = false;
        }
        for (let x = 0; x < idx[f].width; x++) if (idx[f].data[x] >= 0 || idx[f].data[(idx[f].height - 1) * idx[f].width + x] >= 0) border = false;
        check(agree, `${surface}: frame ${f}: coords and index agree on the coverage`);
        check(border, `${surface}: frame ${f}: the margin rows of the default window are empty`);
    }
}
// two sources over three frames in one window; the third camera looks away
const win = { x: -60, y: -40, width: 130, height: 75 };
const three = [cams[0], cams[1], { rotation: yaw(Math.PI - 0.1), focal: 80 }];
const pics = h.warpCamera(three, { scale: 80, images: [im0, im1], window: win });
const idx = h.warpCamera(three, { scale: 80, images: [im0, im1], window: win, output: 'index' });
check(same(pics[0].data, gather(idx[0].data, im0)) && same(pics[1].data, gather(idx[1].data, im1)), 'frame 0 reads source 0, frame 1 source 1');
check(idx[0].data.some((v) => v >= 0) && idx[1].data.some((v) => v >= 0), 'both frames see their window');
check(pics[2].data.every((v) => v === 0) && idx[2].data.every((v) => v === -1), 'a camera looking away is empty');
const bl = h.warpCamera([cams[1]], { scale: 80, sampling: 'bilinear', window: win });
check(bl[0].data.length === pics[0].data.length && bl[0].data.some((v) => v !== 0), 'a bilinear picture');
// from a homography to a camera: H = K_to R K_from^-1 in pixel coordinates, principal points (48, 32) and (50, 30)
const R = yaw(0.3), kf = [700, 700, 48, 32], kt = [640, 640, 50, 30];
const mul = (a, b) => a.map((row) => [0, 1, 2].map((j) => row[0] * b[0][j] + row[1] * b[1][j] + row[2] * b[2][j]));
const Kt = [[kt[0], 0, kt[2]], [0, kt[1], kt[3]], [0, 0, 1]], Kfi = [[1 / kf[0], 0, -kf[2] / kf[0]], [0, 1 / kf[1], -kf[3] / kf[1]], [0, 0, 1]];
const Hm = mul(mul(Kt, R), Kfi).flat();
const c = h.cameraFromMatrices(Hm, { principalFrom: [48, 32], principalTo: [50, 30] });
check(c.okFrom && c.okTo && Math.abs(c.focalFrom / 700 - 1) < 1e-9 && Math.abs(c.focalTo / 640 - 1) < 1e-9, `the focal lengths: ${c.focalFrom} ${c.focalTo}`);
check(c.rotation !== null && R.flat().every((v, k) => Math.abs(v - c.rotation[k]) < 1e-9), 'the rotation');
h.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails }));
process.exit(fails.length === 0 ? 0 : 1);
