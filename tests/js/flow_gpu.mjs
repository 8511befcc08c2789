// GPU: denseFlow() of the drop-in class on the real addon.  With warp: true the pictures that come down must equal gathering the FROM
// pictures bilinearly through the call's own field (the rule of hg_remap_bilinear_u8_device, in f32 by Math.fround), byte for byte; a FROM
// picture that is the TO picture moved by two columns gives a flow of two columns over the interior; identical pictures give the identity
// field, a zero residual and themselves.  Exit code 1 on a failure.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const W = 72, H = 50, f = Math.fround;
const picture = (dx, dy, ch) => Uint8Array.from({ length: W * H * ch }, (_, i) => {
    const p = Math.floor(i / ch), c = i % ch, x = p % W - dx, y = Math.floor(p / W) - dy;
    return c === 3 ? 255 : Math.round(128 + 50 * Math.sin(x / 3.1 + c) * Math.cos(y / 4.3) + 40 * Math.sin((x + 2 * y) / 6.7));
});
const clamp = (v, n) => Math.min(Math.min(Math.max(v, 0), 2147483520), n - 1);
const gather = (field, frame, img, ch) => {
    const out = new Uint8Array(W * H * ch);
    for (let p = 0; p < W * H; p++) {
        const sx = field[(frame * W * H + p) * 2], sy = field[(frame * W * H + p) * 2 + 1];
        if (!Number.isFinite(sx) || !Number.isFinite(sy)) continue;
        const x0 = Math.floor(sx), y0 = Math.floor(sy), fx = f(sx - x0), fy = f(sy - y0), gx = f(1 - fx), gy = f(1 - fy);
        const c0 = clamp(x0, W), c1 = clamp(x0 + 1, W), r0 = clamp(y0, H) * W, r1 = clamp(y0 + 1, H) * W;
        for (let c = 0; c < ch; c++) {
            const p00 = img[(r0 + c0) * ch + c], p01 = img[(r0 + c1) * ch + c], p10 = img[(r1 + c0) * ch + c], p11 = img[(r1 + c1) * ch + c];
            const v = f(f(f(f(p00 * gx) + f(p01 * fx)) * gy) + f(f(f(p10 * gx) + f(p11 * fx)) * fy));
            out[p * ch + c] = Math.min(255, Math.floor(f(v + 0.5)));
        }
    }
    return out;
};
const same = (a, b) => a.length === b.length && a.every((v, k) => v === b[k]);
const median = (a) => Float64Array.from(a).sort()[a.length >> 1];

const h = new Homography('piecewiseaffine', W, H);
for (const ch of [4, 1]) {
    const to = picture(0, 0, ch), from = [picture(2, 0, ch), picture(-1, 1, ch), to];
    const r = h.denseFlow(from, [to], { width: W, height: H, channels: ch, warp: true, field: true, residual: true, good: true });
    check(r.frames === 3 && r.field.length === 3 * W * H * 2 && r.images.length === 3 && r.residual.length === 3 * W * H && r.good.length === 3 * W * H, `${ch} channels: shapes`);
    for (let k = 0; k < 3; k++) check(same(r.images[k], gather(r.field, k, from[k], ch)), `${ch} channels: frame ${k}: the picture is the bilinear gather through its own field`);
    const us = [], vs = [];
    for (let y = 12; y < H - 12; y++) for (let x = 12; x < W - 12; x++) { us.push(r.field[(y * W + x) * 2] - x); vs.push(r.field[(y * W + x) * 2 + 1] - y); }
    check(Math.abs(median(us) - 2) < 0.05 && Math.abs(median(vs)) < 0.05, `${ch} channels: frame 0 is two columns off: median flow ${median(us)}, ${median(vs)}`);
    let ident = true;
    for (let p = 0; p < W * H; p++) ident = ident && r.field[(2 * W * H + p) * 2] === p % W && r.field[(2 * W * H + p) * 2 + 1] === Math.floor(p / W) && r.residual[2 * W * H + p] === 0;
    check(ident && same(r.images[2], to), `${ch} channels: identical pictures give the identity field, a zero residual and themselves`);
    check(r.good.slice(0, W * H).reduce((n, v) => n + v, 0) > W * H / 2, `${ch} channels: most pixels are good`);
    const alone = h.denseFlow(from, [to], { width: W, height: H, channels: ch });
    check(same(new Uint32Array(alone.field.buffer, alone.field.byteOffset, alone.field.length), new Uint32Array(r.field.buffer, r.field.byteOffset, r.field.length)) && !('images' in alone), `${ch} channels: the field alone is the same field`);
}
h.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails }));
process.exit(fails.length === 0 ? 0 : 1);
