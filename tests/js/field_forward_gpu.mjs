// GPU: sourceField(format, {loop}) of the drop-in class on the real addon.  For a same-size piecewise instance and a same-size affine one --
// warp() sends both through the forward (scatter) loops -- the pixels gathered through sourceField('index', {loop: 'warp'}) must be
// warp().data, byte for byte, holes included; with {loop: 'inverse'} (the default) they are warp(null, false, true).data, as before.  'forward'
// is 'warp' here; under bilinear sampling 'warp' is the inverse loop.  Refusals are strings: 'coords' with a forward loop, an unknown loop, a
// forward piecewise loop over a stale map (after an inverse warp) unless repairStaleMap is set.  Prints one JSON line; exit code 1 on a mismatch.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';

function lcgImage(w, h, seed) {
    const data = new Uint8ClampedArray(w * h * 4);
    let s = seed >>> 0;
    for (let i = 0; i < data.length; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; data[i] = s >>> 24 || 1; }     // (no zero byte: a hole is told from a copied pixel)
    return { data, width: w, height: h };
}
const W = 320, H = 200, nx = 8, ny = 5;
const img = lcgImage(W, H, 47);
const img32 = new Uint32Array(img.data.buffer);
const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const report = {};
const thrown = (fn) => { try { fn(); } catch (e) { return e; } return undefined; };
const sameData = (a, b) => a.data.length === b.data.length && a.data.every((v, i) => v === b.data[i]);

function gathered(field, r, name) {
    check(field.data instanceof Int32Array && field.width === r.width && field.height === r.height && field.data.length === r.width * r.height, `${name}: type / window`);
    const out32 = new Uint32Array(r.data.buffer, r.data.byteOffset, r.width * r.height);
    let bad = 0, holes = 0;
    for (let i = 0; i < field.data.length; i++) {
        const v = field.data[i];
        if (v < 0) holes++;
        if (v < -1 || v >= W * H || (v >= 0 ? img32[v] : 0) !== out32[i]) bad++;
    }
    check(bad === 0, `${name}: ${bad} gathered pixels differ from the warp`);
    return holes;
}

function bothLoops(h, name, forwardPath) {
    // the forward field first: the instance's map field still holds the forward map of its mesh
    const fw = h.sourceField('index', { loop: 'warp' }), ff = h.sourceField('index', { loop: 'forward' });
    check(h._lastPath === null, `${name}: sourceField() must not record a path`);
    const r = h.warp();
    check(h._lastPath === forwardPath, `${name}: warp() must take the forward loop (${h._lastPath})`);
    check(r.width === W && r.height === H, `${name}: a same-size window (${r.width} x ${r.height})`);
    const holes = gathered(fw, r, `${name} {loop: 'warp'}`);
    check(sameData(fw, ff), `${name}: 'forward' must equal 'warp' where warp() dispatches forward`);
    check(typeof thrown(() => h.sourceField('coords', { loop: 'warp' })) === 'string', `${name}: 'coords' with a forward loop must throw a string`);
    check(typeof thrown(() => h.sourceField('coords', { loop: 'forward' })) === 'string', `${name}: 'coords' with {loop: 'forward'} must throw a string`);
    check(typeof thrown(() => h.sourceField('index', { loop: 'scatter' })) === 'string', `${name}: an unknown loop must throw a string`);
    // the inverse field: the default, unchanged
    const inv = h.sourceField('index', { loop: 'inverse' }), dflt = h.sourceField('index'), co = h.sourceField('coords', { loop: 'inverse' });
    check(sameData(inv, dflt), `${name}: {loop: 'inverse'} must be the default`);
    check(co.data instanceof Float32Array && co.data.length === 2 * inv.data.length, `${name}: 'coords' of the inverse loop`);
    const ri = h.warp(null, false, true);
    const invHoles = gathered(inv, ri, `${name} {loop: 'inverse'}`);
    check(!sameData(inv, fw), `${name}: the forward and the inverse field must differ somewhere`);
    report[name] = { width: r.width, height: r.height, forward_holes: holes, inverse_uncovered: invHoles };
}

// ---- piecewise, same size: the border vertices stay, the inner ones move
{
    Homography.triangulate = () => gridTriangles(nx, ny);
    const grid = [];
    for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
    const inner = (i, j) => i > 0 && i < nx && j > 0 && j < ny;
    const dst = grid.map(([x, y], k) => inner(k % (nx + 1), Math.floor(k / (nx + 1))) ? [x + 11 * Math.sin(y / 17), y + 9 * Math.cos(x / 23)] : [x, y]);
    const make = (options) => { const h = new Homography('piecewiseaffine', W, H, options); h.setSourcePoints(grid, img, W, H, false); h.setDestinyPoints(dst, false); return h; };
    const h = make({});
    bothLoops(h, 'piecewise', '_piecewiseAffineWarp');
    check(report.piecewise && report.piecewise.forward_holes > 0, 'piecewise: the forward warp of a deformed mesh has holes');
    // the inverse warp above left its own map in the shared field: the forward loop would now read that stale map
    check(typeof thrown(() => h.sourceField('index', { loop: 'warp' })) === 'string', 'piecewise: a forward loop over a stale map must throw a string');
    check(typeof thrown(() => h.sourceField('index', { loop: 'forward' })) === 'string', "piecewise: {loop: 'forward'} over a stale map must throw a string");
    check(h.sourceField('index').data.length === W * H, 'piecewise: the inverse field does not mind the stale map');
    h.close();
    // ... unless repairStaleMap is set
    const rep = make({ repairStaleMap: true });
    rep.warp(null, false, true);
    const held = rep._map;
    const fw = rep.sourceField('index', { loop: 'warp' });
    check(rep._map === held, 'piecewise: sourceField() must not record a map');
    gathered(fw, rep.warp(), 'piecewise, repairStaleMap');
    // source points replaced after the last setDestinyPoints: matrices of an older point set
    const st = make({});
    st.setSourcePoints(grid.map(([x, y]) => [x * 0.97, y * 0.97]), null, W, H, false);
    check(typeof thrown(() => st.sourceField('index', { loop: 'forward' })) === 'string', 'piecewise: stale matrices must throw a string');
    st.close();
    rep.close();
    // bilinear sampling: warp() takes the inverse loop, and so does {loop: 'warp'}
    const b = make({ sampling: 'bilinear' });
    check(sameData(b.sourceField('index', { loop: 'warp' }), b.sourceField('index')), "piecewise: {loop: 'warp'} under bilinear sampling is the inverse field");
    check(b.sourceField('coords', { loop: 'warp' }).data instanceof Float32Array, "piecewise: 'coords' with {loop: 'warp'} under bilinear sampling");
    b.close();
}

// ---- affine, same size: a mirror with a half-pixel shift (every destination x is a Math.round tie)
{
    const g = new Homography('affine', W, H);
    g.setSourcePoints([[0, 0], [W, 0], [0, H]], img, W, H, false);
    g.setDestinyPoints([[W + 0.5, 0], [0.5, 0], [W + 0.5, H]], false);
    bothLoops(g, 'affine', '_geometricWarp');
    g.close();
}

// ---- projective: warp() never takes the forward loop; 'forward' still has a field of the window's size
{
    const p = new Homography('projective', W, H);
    p.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
    p.setDestinyPoints([[W / 10, 0], [W, H / 4], [W / 10, H], [W, H * 0.8]], false);
    check(sameData(p.sourceField('index', { loop: 'warp' }), p.sourceField('index')), "projective: {loop: 'warp'} is the inverse field");
    const f = p.sourceField('index', { loop: 'forward' }), [, , ow, oh] = p._window();
    check(f.data instanceof Int32Array && f.data.length === ow * oh && f.data.some((v) => v >= 0) && f.data.every((v) => v >= -1 && v < W * H), "projective: {loop: 'forward'}");
    p.close();
}

console.log(JSON.stringify({ ok: fails.length === 0, fails, report }));
process.exit(fails.length === 0 ? 0 : 1);
