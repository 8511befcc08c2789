// CPU: the {sampling} option of the drop-in class over tests/js/mock_sampling_addon.cjs (run with HGWARP_ADDON pointing at it).
// Prints one JSON line {failures, checks}.
import { Homography } from '../../homography.js_amd/js/Homography.mjs';
import { gridTriangles } from '../../homography.js_amd/js/delaunay.mjs';
import { createRequire } from 'module';

const require = createRequire(import.meta.url);
const addon = require(process.env.HGWARP_ADDON);
const calls = addon.calls;
const fails = [];
let checks = 0;
const ok = (c, m) => { checks++; if (!c) fails.push(m); };
const take = () => calls.splice(0, calls.length);
const fwd = (log) => log.filter((n) => n.startsWith('warpForward'));
const firstWarp = (log) => log.findIndex((n) => n.startsWith('warp'));
function lcgImage(w, h, seed) {
    const data = new Uint8ClampedArray(w * h * 4);
    let s = seed >>> 0;
    for (let i = 0; i < data.length; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; data[i] = s >>> 24; }
    return { data, width: w, height: h };
}
const W = 96, H = 64, nx = 4, ny = 4;
const img = lcgImage(W, H, 5);
Homography.triangulate = () => gridTriangles(nx, ny);
const grid = [];
for (let j = 0; j <= ny; j++) for (let i = 0; i <= nx; i++) grid.push([i * W / nx, j * H / ny]);
const shrink = grid.map(([x, y]) => [x / 1.1, y / 1.1]);                 // 1.1 x shrink: the reference's forward scatter (:421-422)
const tri3 = [[0, 0], [W, 0], [0, H]], moved3 = [[5, 3], [W + 5, 3], [5, H + 3]];   // same-size affine: forward loop (:426-427)

function run(mode, fn) {
    take();
    const opts = mode === undefined ? {} : { sampling: mode };
    fn(opts);
    return take();
}
// same-size affine
for (const mode of [undefined, 'nearest', 'bilinear']) {
    const log = run(mode, (o) => { const h = new Homography('affine', W, H, o); h.setSourcePoints(tri3, img, W, H, false); h.setDestinyPoints(moved3, false); h.warp(); });
    const bil = mode === 'bilinear';
    ok(fwd(log).length === (bil ? 0 : 1), `affine same size, ${mode}: forward calls ${fwd(log)}`);
    ok(log.includes('warpInverseGeometric') === bil, `affine same size, ${mode}: inverse call`);
    ok(log.filter((n) => n.startsWith('setSampling')).length === (bil ? 1 : 0), `affine, ${mode}: setSampling calls ${log}`);
    if (bil) ok(log.indexOf('setSampling:1') >= 0 && log.indexOf('setSampling:1') < firstWarp(log), `affine: mode after the first warp ${log}`);
}
// 1.1 x piecewise shrink, warp() and warpBatch()
for (const mode of [undefined, 'bilinear']) {
    const bil = mode === 'bilinear';
    let log = run(mode, (o) => { const h = new Homography('piecewiseaffine', W, H, o); h.setSourcePoints(grid, img, W, H, false); h.setDestinyPoints(shrink, false); h.warp(); });
    ok(fwd(log).length === (bil ? 0 : 1), `piecewise shrink, ${mode}: forward calls ${log}`);
    ok(log.includes('warpInversePiecewise') === bil, `piecewise shrink, ${mode}: inverse call ${log}`);
    if (bil) ok(log.indexOf('setSampling:1') >= 0 && log.indexOf('setSampling:1') < firstWarp(log), `piecewise: mode after the first warp ${log}`);
    log = run(mode, (o) => { const h = new Homography('piecewiseaffine', W, H, o); h.setSourcePoints(grid, img, W, H, false); h.warpBatch([shrink, grid]); });
    ok(fwd(log).length === (bil ? 0 : 1), `warpBatch shrink, ${mode}: forward calls ${log}`);
    ok(log.includes('warpInversePiecewiseBatch') === bil, `warpBatch, ${mode}: inverse batch ${log}`);
    ok(log.filter((n) => n.startsWith('setSampling')).length === (bil ? 1 : 0), `warpBatch, ${mode}: setSampling calls ${log}`);
    if (bil) ok(log.indexOf('setSampling:1') < firstWarp(log), `warpBatch: mode after the first warp ${log}`);
    log = run(mode, (o) => { const h = new Homography('affine', W, H, o); h.setSourcePoints(tri3, img, W, H, false); h.warpBatch([moved3, moved3]); });
    ok(fwd(log).length === (bil ? 0 : 1), `affine warpBatch, ${mode}: forward calls ${log}`);
    log = run(mode, (o) => { const h = new Homography('piecewiseaffine', W, H, o); h.setSourcePoints(grid, img, W, H, false); h.warpBatch([shrink, grid], { devices: [0] }); });
    ok(log.filter((n) => n.startsWith('multiSetSampling')).length === (bil ? 1 : 0), `warpBatch devices, ${mode}: ${log}`);
    if (bil) ok(log.indexOf('multiSetSampling:1') >= 0 && log.indexOf('multiSetSampling:1') < log.indexOf('warpInversePiecewiseBatch'), `devices: mode after the warp ${log}`);
}
// switching on a live instance reaches the context; back to nearest is one more call
{
    const log = run(undefined, () => {
        const h = new Homography('projective', W, H);
        h.setSourcePoints([[0, 0], [W, 0], [0, H], [W, H]], img, W, H, false);
        h.setDestinyPoints([[4, 0], [W, 6], [0, H - 2], [W - 3, H]], false);
        h.warp(); h.sampling = 'bilinear'; h.warp(); h.sampling = 'bilinear'; h.sampling = 'nearest'; h.warp();
        ok(h.sampling === 'nearest', 'sampling getter');
    });
    ok(JSON.stringify(log) === JSON.stringify(['warpInverseGeometric', 'setSampling:1', 'warpInverseGeometric', 'setSampling:0', 'warpInverseGeometric']), `switching: ${log}`);
}
// bad modes throw bare strings, in the class's style
for (const bad of ['cubic', 'Bilinear', 1, null]) {
    let e = null;
    try { new Homography('auto', null, null, { sampling: bad }); } catch (x) { e = x; }
    ok(typeof e === 'string' && e.includes('sampling'), `constructor with sampling ${bad}: ${e}`);
    e = null;
    const h = new Homography('auto');
    try { h.sampling = bad; } catch (x) { e = x; }
    ok(typeof e === 'string' && h.sampling === 'nearest', `setter with ${bad}: ${e}`);
}
console.log(JSON.stringify({ failures: fails, checks }));
process.exit(fails.length ? 1 : 0);
