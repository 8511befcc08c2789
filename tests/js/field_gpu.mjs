// GPU: sourceField() of the drop-in class on the real addon.  For a projective and a piecewise instance the pixels gathered through
// sourceField('index') must be warp(null, false, true).data, byte for byte; sourceField('coords') is NaN only where the index is -1, and for
// the projective instance -- whose loop :997-1011 is written again below in plain JS doubles -- NaN exactly where the loop's coordinate fails
// its bounds test, the loop's coordinate rounded to f32 elsewhere, and the index the loop's own.  Prints one JSON line; exit code 1 on a mismatch.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';

function lcgImage(w, h, seed) {
    const data = new Uint8ClampedArray(w * h * 4);
    let s = seed >>> 0;
    for (let i = 0; i < data.length; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; data[i] = s >>> 24; }
    return { data, width: w, height: h };
}
const W = 320, H = 200, nx = 8, ny = 5;
const img = lcgImage(W, H, 43);
const img32 = new Uint32Array(img.data.buffer);
const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const report = {};

function gatherEqualsWarp(h, name) {
    const idx = h.sourceField('index'), co = h.sourceField('coords'), r = h.warp(null, false, true);
    check(idx.data instanceof Int32Array && co.data instanceof Float32Array, `${name}: array types`);
    check(idx.width === r.width && idx.height === r.height && co.width === r.width && co.height === r.height, `${name}: window`);
    check(idx.data.length === r.width * r.height && co.data.length === 2 * r.width * r.height, `${name}: lengths`);
    const out32 = new Uint32Array(r.data.buffer, r.data.byteOffset, r.width * r.height);
    let bad = 0, covered = 0, nan = 0, nanWithIndex = 0, halfNan = 0;
    for (let i = 0; i < idx.data.length; i++) {
        const v = idx.data[i];
        if (v >= 0) covered++;
        if ((v >= 0 && v < W * H ? img32[v] : 0) !== out32[i] || v < -1 || v >= W * H) bad++;
        const nx_ = Number.isNaN(co.data[2 * i]), ny_ = Number.isNaN(co.data[2 * i + 1]);
        if (nx_ !== ny_) halfNan++;
        if (nx_) { nan++; if (v !== -1) nanWithIndex++; }
    }
    check(bad === 0, `${name}: ${bad} gathered pixels differ from warp(null, false, true)`);
    check(covered > 0 && covered < idx.data.length, `${name}: the window must hold covered and uncovered pixels (${covered})`);
    check(halfNan === 0 && nanWithIndex === 0, `${name}: NaN coordinates with an index (${nanWithIndex}) or in one word only (${halfNan})`);
    report[name] = { width: r.width, height: r.height, covered, nan };
    return { idx, co };
}

// ---- projective
{
    const g = new Homography('projective', W, H);
    g.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    g.setDestinyPoints([[W / 10, 0], [W, H / 4], [W / 10, H], [W, H * 0.8]], false);
    const { idx, co } = gatherEqualsWarp(g, 'projective');
    const m = g._solve(g._dstPoints, g._srcPoints), [xo, yo, ow, oh] = g._window();
    let wrongNan = 0, wrongCo = 0, wrongIdx = 0;
    for (let r = 0; r < oh; r++) for (let c = 0; c < ow; c++) {
        const x = c + xo, y = r + yo, i = r * ow + c;
        const den = m[6] * x + m[7] * y + 1;                                                     // applyProjectiveTransformToPoint :1401
        const sx = (m[0] * x + m[1] * y + m[2]) / den, sy = (m[3] * x + m[4] * y + m[5]) / den;
        const inb = sx >= 0 && sx < W && sy >= 0 && sy < H;                                      // :1001
        if (Number.isNaN(co.data[2 * i]) !== !inb) wrongNan++;
        if (inb && (co.data[2 * i] !== Math.fround(sx) || co.data[2 * i + 1] !== Math.fround(sy))) wrongCo++;
        const flat = Math.round(sy) * W + Math.round(sx);
        if (idx.data[i] !== (inb && flat >= 0 && flat < W * H ? flat : -1)) wrongIdx++;
    }
    check(wrongNan === 0 && wrongCo === 0 && wrongIdx === 0, `projective: against the loop in JS: NaN ${wrongNan}, coordinates ${wrongCo}, indices ${wrongIdx}`);
    let threw = null;
    try { g.sourceField('nearest'); } catch (e) { threw = e; }
    check(typeof threw === 'string', 'an unknown format must throw a string');
    // the field is independent of the sampling mode
    const b = new Homography('projective', W, H, { sampling: 'bilinear' });
    b.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    b.setDestinyPoints([[W / 10, 0], [W, H / 4], [W / 10, H], [W, H * 0.8]], false);
    const bi = b.sourceField('index');
    check(bi.data.length === idx.data.length && bi.data.every((v, i) => v === idx.data[i]), 'projective: index field under bilinear sampling');
    b.close();
    g.close();
}

// ---- piecewise
{
    Homography.triangulate = () => gridTriangles(nx, ny);
    const grid = [];
    for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
    const h = new Homography('piecewiseaffine', W, H);
    h.setSourcePoints(grid, img, W, H, false);
    h.setDestinyPoints(grid.map(([x, y]) => [x * 1.3, 9 + y * 1.25 + Math.sin((8 * x) / Math.PI) * 9]), false);
    gatherEqualsWarp(h, 'piecewise');
    // a reference-state quirk (source points replaced after the last setDestinyPoints): refused with a string, not a wrong field
    h.setSourcePoints(grid.map(([x, y]) => [x * 0.9, y * 0.9]), null, W, H, false);
    let threw = null;
    try { h.sourceField('index'); } catch (e) { threw = e; }
    check(typeof threw === 'string', 'stale piecewise matrices must throw a string');
    h.close();
}

console.log(JSON.stringify({ ok: fails.length === 0, fails, report }));
process.exit(fails.length === 0 ? 0 : 1);
