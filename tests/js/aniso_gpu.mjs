// GPU: remap(plane, {sampling: 'anisotropic'}) of the drop-in class on the real addon, for an affine, a projective and a piecewise shrink of
// a 64 x 40 source that squeeze one axis much more than the other.  Prints one JSON line: per case the window, the coordinate field
// (sourceField('coords'), base64) and the SHA-256 of the Uint8Array x 4 result with the default maxAniso (8) and of the Float32Array x 1
// result with maxAniso 3 -- tests/test_gpu_aniso.py sends the same planes through the same fields by ctypes and compares the hashes.
// Checked here: classes and shapes, maxAniso 1 IS 'trilinear', the default is 8, and the instance's own sampling mode and path record stay
// as they were.  Exit code 1 on a failure.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';
import { createHash } from 'crypto';

const W = 64, H = 40, nx = 4, ny = 4;
const u8 = new Uint8Array(W * H * 4);
for (let i = 0; i < u8.length; i++) u8[i] = (i * 7 + (i >> 3) * 13) & 255;
const f32 = new Float32Array(W * H);
for (let i = 0; i < f32.length; i++) f32[i] = ((i * 37) % 1001) * 0.25 - 100;
const img = { data: new Uint8ClampedArray(u8.buffer.slice(0)), width: W, height: H };
const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const bytesOf = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength);
const sha = (t) => createHash('sha256').update(bytesOf(t)).digest('hex');
const cases = {};

function through(h, name) {
    const co = h.sourceField('coords');
    const a = h.remap(u8, { channels: 4, sampling: 'anisotropic' }), b = h.remap(f32, { sampling: 'anisotropic', maxAniso: 3 });
    const a8 = h.remap(u8, { channels: 4, sampling: 'anisotropic', maxAniso: 8 }), a1 = h.remap(u8, { channels: 4, sampling: 'anisotropic', maxAniso: 1 });
    const tri = h.remap(u8, { channels: 4, sampling: 'trilinear' });
    check(a.data instanceof Uint8Array && a.channels === 4 && a.width === co.width && a.height === co.height && a.data.length === co.width * co.height * 4, `${name}: shape of the Uint8Array result`);
    check(b.data instanceof Float32Array && b.channels === 1 && b.data.length === co.width * co.height, `${name}: shape of the Float32Array result`);
    check(sha(a.data) === sha(a8.data), `${name}: the default maxAniso is 8`);
    check(sha(a1.data) === sha(tri.data), `${name}: maxAniso 1 is 'trilinear'`);
    check(a.data.some((v) => v !== 0) && a.data.some((v, i) => v !== tri.data[i]), `${name}: an oblique shrink must not come out as 'trilinear' gives it`);
    check(h._lastPath === null && h.sampling === 'nearest', `${name}: remap() must leave the path record and the sampling mode alone`);
    const cl = h.remap(img.data, { channels: 4, sampling: 'anisotropic' });
    check(cl.data instanceof Uint8ClampedArray && sha(cl.data) === sha(a.data), `${name}: a Uint8ClampedArray plane gives the Uint8Array bytes`);
    cases[name] = { width: co.width, height: co.height, coords: bytesOf(co.data).toString('base64'), u8x4: sha(a.data), f32x1: sha(b.data) };
}

{
    const g = new Homography('affine', W, H);
    g.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    g.setDestinyPoints([[1.5, 2], [W * 0.6 + 1.5, 3], [0.5, H * 0.15 + 2]], false);
    through(g, 'affine');
    g.close();
}
{
    const p = new Homography('projective', W, H);
    p.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    p.setDestinyPoints([[8, 0], [W * 0.5, 0], [0, H * 0.3], [W * 0.7, H * 0.3]], false);
    through(p, 'projective');
    p.close();
}
{
    Homography.triangulate = () => gridTriangles(nx, ny);
    const grid = [];
    for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
    const dst = grid.map(([x, y]) => [x * 0.6 + 2 * Math.sin(y / 17), y * 0.15 + 1.0 * Math.cos(x / 23) + 2]);
    const h = new Homography('piecewiseaffine', W, H);
    h.setSourcePoints(grid, img, W, H, false);
    h.setDestinyPoints(dst, false);
    through(h, 'piecewise');
    h.close();
}
console.log(JSON.stringify({ ok: fails.length === 0, fails, W, H, cases }));
process.exit(fails.length === 0 ? 0 : 1);
