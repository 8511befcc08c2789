// GPU: remap(plane, {sampling: 'bicubic'}) of the drop-in class on the real addon, for an affine, a projective and a piecewise 3x
// enlargement of a 16 x 10 source.  Prints one JSON line: per case the window, the coordinate field (sourceField('coords'), base64) and
// the SHA-256 of the Uint8Array x 4 and the Float32Array x 1 result, each with the default cubic (Catmull-Rom) and with [1/3, 1/3] --
// tests/test_gpu_bicubic.py sends the same planes through the same fields by ctypes and compares the hashes.
// Checked here: classes and shapes, the default IS 'catmull-rom', the names are their pairs, the result is not 'bilinear''s, and the
// instance's own sampling mode and path record stay as they were.  Exit code 1 on a failure.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';
import { createHash } from 'crypto';

const W = 16, H = 10, nx = 2, ny = 2;
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
    const a = h.remap(u8, { channels: 4, sampling: 'bicubic' }), b = h.remap(f32, { sampling: 'bicubic', cubic: [1 / 3, 1 / 3] });
    const am = h.remap(u8, { channels: 4, sampling: 'bicubic', cubic: [1 / 3, 1 / 3] }), bd = h.remap(f32, { sampling: 'bicubic' });
    const bil = h.remap(u8, { channels: 4, sampling: 'bilinear' });
    check(a.data instanceof Uint8Array && a.channels === 4 && a.width === co.width && a.height === co.height && a.data.length === co.width * co.height * 4, `${name}: shape of the Uint8Array result`);
    check(b.data instanceof Float32Array && b.channels === 1 && b.data.length === co.width * co.height, `${name}: shape of the Float32Array result`);
    check(co.width <= 48 && co.height <= 32 && co.width > 2 * W && co.height > 2 * H, `${name}: the window ${co.width} x ${co.height} is an enlargement of at most 48 x 32`);
    check(sha(a.data) === sha(h.remap(u8, { channels: 4, sampling: 'bicubic', cubic: 'catmull-rom' }).data), `${name}: the default cubic is 'catmull-rom'`);
    check(sha(a.data) === sha(h.remap(u8, { channels: 4, sampling: 'bicubic', cubic: [0, 0.5] }).data), `${name}: 'catmull-rom' is [0, 0.5]`);
    check(sha(am.data) === sha(h.remap(u8, { channels: 4, sampling: 'bicubic', cubic: 'mitchell' }).data), `${name}: 'mitchell' is [1/3, 1/3]`);
    check(a.data.some((v) => v !== 0) && a.data.some((v, i) => v !== bil.data[i]) && a.data.some((v, i) => v !== am.data[i]), `${name}: the cubics must differ from 'bilinear' and from one another`);
    check(h._lastPath === null && h.sampling === 'nearest', `${name}: remap() must leave the path record and the sampling mode alone`);
    const cl = h.remap(img.data, { channels: 4, sampling: 'bicubic' });
    check(cl.data instanceof Uint8ClampedArray && sha(cl.data) === sha(a.data), `${name}: a Uint8ClampedArray plane gives the Uint8Array bytes`);
    cases[name] = { width: co.width, height: co.height, coords: bytesOf(co.data).toString('base64'), u8x4: sha(a.data), f32x1: sha(b.data), u8x4_mitchell: sha(am.data), f32x1_default: sha(bd.data) };
}

{
    const g = new Homography('affine', W, H);
    g.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    g.setDestinyPoints([[1.5, 2], [W * 2.7 + 1.5, 3], [0.5, H * 2.8 + 2]], false);
    through(g, 'affine');
    g.close();
}
{
    const p = new Homography('projective', W, H);
    p.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    p.setDestinyPoints([[3, 0], [W * 2.8, 1], [0, H * 2.9], [W * 2.9, H * 3]], false);
    through(p, 'projective');
    p.close();
}
{
    Homography.triangulate = () => gridTriangles(nx, ny);
    const grid = [];
    for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
    const dst = grid.map(([x, y]) => [x * 2.8 + 1.5 * Math.sin(y / 7), y * 2.9 + 1.0 * Math.cos(x / 9) + 1]);
    const h = new Homography('piecewiseaffine', W, H);
    h.setSourcePoints(grid, img, W, H, false);
    h.setDestinyPoints(dst, false);
    through(h, 'piecewise');
    h.close();
}
console.log(JSON.stringify({ ok: fails.length === 0, fails, W, H, cases }));
process.exit(fails.length === 0 ? 0 : 1);
