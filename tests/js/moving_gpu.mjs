// GPU: warpBatch(dst, {sourcePoints, images}) of the drop-in class on the real addon, for the point sets tests/test_gpu_moving.py hands over
// in a JSON file (argv[2]: W, H, seed0, tris, src[f], dst[f] as float32 values).  Prints one JSON line: per frame the sha256 of the class's
// output, its size and the source minima the class used, in bilinear mode and in nearest mode (where warp() must pick the inverse loop for
// these sets); the Python side compares the hashes with the CPU oracle's.  Also checks the batch against the class's own frame loop.
import fs from 'fs';
import crypto from 'crypto';
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const sha = (t) => crypto.createHash('sha256').update(Buffer.from(t.buffer, t.byteOffset, t.byteLength)).digest('hex');
function lcgImage(w, h, seed) {
    const data = new Uint8ClampedArray(w * h * 4);
    let s = seed >>> 0;
    for (let i = 0; i < data.length; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; data[i] = s >>> 24; }
    return { data, width: w, height: h };
}
const inp = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const { W, H, seed0 } = inp, F = inp.src.length;
Homography.triangulate = () => Uint32Array.from(inp.tris);
const images = inp.src.map((_, f) => lcgImage(W, H, seed0 + f));
const sets = (a) => a.map((p) => Float32Array.from(p));
const out = { failures: [] };

for (const mode of ['bilinear', 'nearest']) {
    const h = new Homography('piecewiseaffine', W, H, { sampling: mode });
    const mins = [];
    const orig = h._native.warpInversePiecewiseSrcBatch;
    let seen = null;
    h._native.warpInversePiecewiseSrcBatch = (...a) => { seen = Array.from(a[2]); return orig(...a); };     // (the minima the class hands to the addon)
    const frames = h.warpBatch(sets(inp.dst), { sourcePoints: sets(inp.src), images });
    h._native.warpInversePiecewiseSrcBatch = orig;
    if (seen === null || seen.length !== 2 * F) out.failures.push(`${mode}: the frames did not go out as one batch of ${F}`);
    if (h._lastPath !== '_inversePiecewiseAffineWarp') out.failures.push(`${mode}: last path ${h._lastPath}`);
    out[mode === 'bilinear' ? 'bilinear' : 'nearest_inverse'] = frames.map((r, f) => ({ sha: sha(r.data), w: r.width, h: r.height, min: seen ? seen.slice(2 * f, 2 * f + 2) : null }));
    // the class's own loop, frame for frame
    const g = new Homography('piecewiseaffine', W, H, { sampling: mode });
    for (let f = 0; f < F; f++) {
        g.setSourcePoints(Float32Array.from(inp.src[f])); g.setDestinyPoints(Float32Array.from(inp.dst[f]));
        const r = g.warp(images[f]);
        if (sha(r.data) !== sha(frames[f].data) || r.width !== frames[f].width || r.height !== frames[f].height) out.failures.push(`${mode}: frame ${f} of the batch differs from the loop's`);
    }
    h.close(); g.close();
}
console.log(JSON.stringify(out));
