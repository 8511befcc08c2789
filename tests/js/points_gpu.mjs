// GPU: transformPoints() of the drop-in class on the real addon, both directions, for an affine, a projective and a piecewise instance.
// Here: to 'source' at every integer window pixel is sourceField('coords'), bit for bit; the results have the list's length; NaN comes in
// pairs.  The bits of two seeded fractional lists and the state they were computed for (window, matrices, mesh) go out in one JSON line:
// tests/test_gpu_points.py runs the ctypes entry points on the same state and compares.  Exit code 1 on a mismatch.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';

function lcgImage(w, h, seed) {                              // (workloads.lcg_image: no `|| 1`)
    const data = new Uint8ClampedArray(w * h * 4);
    let s = seed >>> 0;
    for (let i = 0; i < data.length; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; data[i] = s >>> 24; }
    return { data, width: w, height: h };
}
const W = 160, H = 96, nx = 6, ny = 4, seed = 43;
const img = lcgImage(W, H, seed);
const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const report = {};
const bits = (f) => Array.from(new Uint32Array(f.buffer, f.byteOffset, f.length));

let s = 12345;
const rnd = () => { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; return s / 4294967296; };
const list = (x0, y0, w, h, n) => { const p = new Float32Array(2 * n); for (let i = 0; i < n; i++) { p[2 * i] = x0 - 2 + rnd() * (w + 4); p[2 * i + 1] = y0 - 2 + rnd() * (h + 4); } return p; };
const special = [-0.5, 0, 3.5, 2, NaN, 1, 1, Infinity, 1e30, 1, 10.25, 20.75];
const pointsSource = Float32Array.from([...list(0, 0, W + 20, H + 20, 300), ...special]);
const pointsOutput = Float32Array.from([...list(0, 0, W, H, 300), ...special]);

function both(h, name, extra) {
    const [xo, yo, ow, oh] = h._window();
    const co = h.sourceField('coords');
    const px = new Float32Array(2 * ow * oh);
    for (let r = 0; r < oh; r++) for (let c = 0; c < ow; c++) { px[2 * (r * ow + c)] = c; px[2 * (r * ow + c) + 1] = r; }
    const at = h.transformPoints(px, { to: 'source' });
    const a = new Uint32Array(at.buffer, at.byteOffset, at.length), b = new Uint32Array(co.data.buffer, co.data.byteOffset, co.data.length);
    let bad = 0, mapped = 0;
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) bad++; if (a[i] !== 0x7fc00000) mapped++; }
    check(at.length === co.data.length && bad === 0, `${name}: to 'source' at the integer pixels differs from sourceField('coords') in ${bad} words`);
    check(mapped > 0 && mapped < a.length, `${name}: the window must hold mapped and unmapped pixels (${mapped})`);
    const toSource = h.transformPoints(pointsSource, { to: 'source' }), toOutput = h.transformPoints(Array.from({ length: pointsOutput.length / 2 }, (_, i) => [pointsOutput[2 * i], pointsOutput[2 * i + 1]]));
    for (const [r, what] of [[toSource, 'source'], [toOutput, 'output']]) {
        check(r instanceof Float32Array && r.length === pointsSource.length, `${name} to '${what}': a Float32Array of the list's length`);
        let half = 0, ok = 0;
        for (let i = 0; i < r.length; i += 2) { if (Number.isNaN(r[i]) !== Number.isNaN(r[i + 1])) half++; if (!Number.isNaN(r[i])) ok++; }
        check(half === 0 && ok > 100 && ok < r.length / 2, `${name} to '${what}': NaN in one word only (${half}) or nothing / everything mapped (${ok})`);
    }
    check(h._lastPath === null, `${name}: transformPoints() must not record a path`);
    report[name] = Object.assign({ geom: [xo, yo, ow, oh], to_source_bits: bits(toSource), to_output_bits: bits(toOutput) }, extra());
}

{
    const a = new Homography('affine', W, H);
    a.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    a.setDestinyPoints([[5, 3], [W * 1.2 + 5, 9], [-4, H * 1.1 + 3]], false);
    both(a, 'affine', () => ({ inverse: Array.from(a._solve(a._dstPoints, a._srcPoints)), forward: Array.from(a._transformMatrix) }));
    a.close();
    const g = new Homography('projective', W, H);
    g.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    g.setDestinyPoints([[W / 10, 0], [W * 1.2, H / 4], [W / 10, H * 1.1], [W * 1.2, H * 0.8]], false);
    both(g, 'projective', () => ({ inverse: Array.from(g._solve(g._dstPoints, g._srcPoints)), forward: Array.from(g._transformMatrix) }));
    g.close();
    Homography.triangulate = () => gridTriangles(nx, ny);
    const grid = [];
    for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
    const p = new Homography('piecewiseaffine', W, H, { repairStaleMap: true });
    p.setSourcePoints(grid, img, W, H, false);
    p.setDestinyPoints(grid.map(([x, y]) => [x * 1.1, 7 + y * 1.15 + Math.sin((8 * x) / Math.PI) * 7]), false);
    both(p, 'piecewise', () => ({ src: Array.from(p._srcPoints), dst: Array.from(p._dstPoints), tris: Array.from(p._triangles),
                                   min_src: [p._minSrcX, p._minSrcY], max_src: [p._maxSrcX, p._maxSrcY] }));
    let threw = null;
    try { p.transformPoints(pointsSource, { to: 'sideways' }); } catch (e) { threw = e; }
    check(typeof threw === 'string', "a bad `to` must throw a string");
    p.close();
}

console.log(JSON.stringify({ ok: fails.length === 0, fails, W, H, seed, points_source: Array.from(pointsSource), points_output: Array.from(pointsOutput), report }));
process.exit(fails.length === 0 ? 0 : 1);
