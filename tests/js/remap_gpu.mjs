// GPU: remap(plane, options) of the drop-in class on the real addon.  For an affine, a projective and a piecewise instance:
//   remap(new Uint32Array(image.data.buffer))  is warp(null, false, true).data viewed as 32-bit pixels;
//   {loop: 'warp'} on a same-size frame (affine, piecewise: the forward loop) is warp().data;
//   a Uint8Array label plane equals the host gather over sourceField('index').data;
//   Float32Array and Uint8Array bilinear planes equal a Math.fround model over sourceField('coords').data, bit for bit.
// Prints one JSON line; exit code 1 on a mismatch.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';

function lcgBytes(n, seed) {
    const data = new Uint8ClampedArray(n);
    let s = seed >>> 0;
    for (let i = 0; i < n; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; data[i] = s >>> 24 || 1; }
    return data;
}
const W = 160, H = 100, nx = 8, ny = 5;
const img = { data: lcgBytes(W * H * 4, 53), width: W, height: H };
const img32 = new Uint32Array(img.data.buffer);
const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const report = {};
const fr = Math.fround;
const same = (a, b) => a.length === b.length && a.every((v, i) => Object.is(v, b[i]) || v === b[i]);
const bytesOf = (t) => new Uint8Array(t.buffer, t.byteOffset, t.byteLength);

// the library's bilinear remap in f32, one rounding per operation (include/hgwarp.h, hg_remap_bilinear_f32_device / _u8_device)
function tap(v, n) { return Math.min(Math.min(Math.max(v, 0), 2147483520), n - 1); }
function bilinearModel(coords, plane, ch, u8) {
    const n = coords.length / 2, out = new plane.constructor(n * ch);
    for (let i = 0; i < n; i++) {
        const sx = coords[2 * i], sy = coords[2 * i + 1];
        if (!Number.isFinite(sx) || !Number.isFinite(sy)) continue;
        const x0 = Math.floor(sx), y0 = Math.floor(sy);
        const fx = fr(sx - x0), fy = fr(sy - y0), gx = fr(1 - fx), gy = fr(1 - fy);
        const c0 = tap(x0, W), c1 = tap(fr(x0 + 1), W), r0 = tap(y0, H), r1 = tap(fr(y0 + 1), H);
        for (let k = 0; k < ch; k++) {
            const p00 = plane[(r0 * W + c0) * ch + k], p01 = plane[(r0 * W + c1) * ch + k], p10 = plane[(r1 * W + c0) * ch + k], p11 = plane[(r1 * W + c1) * ch + k];
            const top = fr(fr(fr(p00 * gx) + fr(p01 * fx)) * gy), bot = fr(fr(fr(p10 * gx) + fr(p11 * fx)) * fy);
            const v = fr(top + bot);
            out[i * ch + k] = u8 ? Math.min(255, Math.floor(fr(v + 0.5))) : v;
        }
    }
    return out;
}

function planesThrough(h, name) {
    // the picture's own pixels: the inverse warp
    const r = h.remap(img32), w = h.warp(null, false, true);
    check(r.data instanceof Uint32Array && r.channels === 1 && r.width === w.width && r.height === w.height, `${name}: shape of remap(image)`);
    check(same(bytesOf(r.data), bytesOf(w.data)), `${name}: remap(image as Uint32Array) must be warp(null, false, true).data`);
    check(bytesOf(r.data).some((v) => v !== 0), `${name}: an all-zero warp proves nothing`);
    // a label plane: the host gather over the index field
    const labels = new Uint8Array(W * H);
    for (let i = 0; i < labels.length; i++) labels[i] = 1 + (i * 7) % 250;
    const idx = h.sourceField('index').data, lab = h.remap(labels);
    const wantLab = Uint8Array.from(idx, (v) => (v >= 0 ? labels[v] : 0));
    check(lab.data instanceof Uint8Array && same(lab.data, wantLab), `${name}: Uint8Array labels against the host gather`);
    // 16-byte pixels of doubles
    const dbl = new Float64Array(W * H * 2);
    for (let i = 0; i < dbl.length; i++) dbl[i] = Math.sin(i) * 1e3;
    const d2 = h.remap(dbl, { channels: 2 });
    let badD = 0;
    for (let i = 0; i < idx.length; i++) for (let k = 0; k < 2; k++) if (d2.data[2 * i + k] !== (idx[i] >= 0 ? dbl[2 * idx[i] + k] : 0)) badD++;
    check(d2.data instanceof Float64Array && badD === 0, `${name}: 16-byte pixels (${badD} differ)`);
    // bilinear planes against the Math.fround model over the coordinate field
    const co = h.sourceField('coords').data;
    let nan = 0;
    for (let i = 0; i < co.length; i += 2) if (Number.isNaN(co[i])) nan++;
    for (const ch of [1, 3, 4]) {
        const f32 = new Float32Array(W * H * ch);
        for (let i = 0; i < f32.length; i++) f32[i] = fr(Math.cos(i * 0.37) * 100);
        const gotF = h.remap(f32, { channels: ch, sampling: 'bilinear' });
        check(gotF.data instanceof Float32Array && same(bytesOf(gotF.data), bytesOf(bilinearModel(co, f32, ch, false))), `${name}: Float32Array bilinear, ${ch} channels`);
        const u8 = new Uint8Array(lcgBytes(W * H * ch, 90 + ch).buffer);
        const gotU = h.remap(u8, { channels: ch, sampling: 'bilinear' });
        check(gotU.data instanceof Uint8Array && same(gotU.data, bilinearModel(co, u8, ch, true)), `${name}: Uint8Array bilinear, ${ch} channels`);
    }
    const cl = h.remap(img.data, { channels: 4, sampling: 'bilinear' });
    check(cl.data instanceof Uint8ClampedArray && same(cl.data, bilinearModel(co, img.data, 4, true)), `${name}: Uint8ClampedArray RGBA bilinear`);
    report[name] = { width: r.width, height: r.height, uncovered: nan };
}

// ---- affine: same size (warp() takes the forward loop), a half-pixel mirror
{
    const make = () => { const g = new Homography('affine', W, H); g.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false); g.setDestinyPoints([[W + 0.5, 0], [0.5, 0], [W + 0.5, H]], false); return g; };
    const g = make();
    const viaWarp = g.remap(img32, { loop: 'warp' }), viaFwd = g.remap(img32, { loop: 'forward' });
    const w = g.warp();
    check(g._lastPath === '_geometricWarp', `affine: warp() must take the forward loop (${g._lastPath})`);
    check(same(bytesOf(viaWarp.data), bytesOf(w.data)) && same(viaWarp.data, viaFwd.data), "affine: {loop: 'warp'} must be warp().data");
    planesThrough(g, 'affine');
    g.close();
}
// ---- projective
{
    const p = new Homography('projective', W, H);
    p.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    p.setDestinyPoints([[W / 10, 0], [W, H / 4], [W / 10, H], [W, H * 0.8]], false);
    planesThrough(p, 'projective');
    check(same(p.remap(img32, { loop: 'warp' }).data, p.remap(img32).data), "projective: {loop: 'warp'} is the inverse loop");
    p.close();
}
// ---- piecewise: same size, the border vertices stay, the inner ones move (warp() takes the forward loop)
{
    Homography.triangulate = () => gridTriangles(nx, ny);
    const grid = [];
    for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
    const inner = (i, j) => i > 0 && i < nx && j > 0 && j < ny;
    const dst = grid.map(([x, y], k) => inner(k % (nx + 1), Math.floor(k / (nx + 1))) ? [x + 7 * Math.sin(y / 17), y + 6 * Math.cos(x / 23)] : [x, y]);
    const h = new Homography('piecewiseaffine', W, H);
    h.setSourcePoints(grid, img, W, H, false);
    h.setDestinyPoints(dst, false);
    const viaWarp = h.remap(img32, { loop: 'warp' });
    check(h._lastPath === null, 'piecewise: remap() must not record a path');
    const w = h.warp();
    check(h._lastPath === '_piecewiseAffineWarp' && w.width === W && w.height === H, `piecewise: warp() must take the forward loop on a same-size frame (${h._lastPath})`);
    check(same(bytesOf(viaWarp.data), bytesOf(w.data)), "piecewise: {loop: 'warp'} on a same-size frame must be warp().data");
    planesThrough(h, 'piecewise');
    h.close();
}

console.log(JSON.stringify({ ok: fails.length === 0, fails, report }));
process.exit(fails.length === 0 ? 0 : 1);
