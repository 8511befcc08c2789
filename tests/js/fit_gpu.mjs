// GPU: fitMatches() of the drop-in class on the real addon.  The planted case comes from the JSON file named on the command line (written
// by tests/test_gpu_fit.py: per kind F lists of N matches, base64 float32); the results go out as base64 in one JSON line, which the test
// compares bit for bit with the ctypes call on the same matches.  The fitted affine matrices are then fed to the geometric batch path the
// class already has (warpForwardGeometricBatch): it must run and draw.  Exit code 1 on a failure.
import fs from 'fs';
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const cs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const b64 = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength).toString('base64');
const f32 = (s) => { const b = Buffer.from(s, 'base64'); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };
const W = 64, H = 48;
const data = new Uint8ClampedArray(W * H * 4);
for (let i = 0; i < data.length; i++) data[i] = (i * 7 + (i >> 3) * 13) & 255 || 1;

const h = new Homography('projective', W, H);
const cases = {};
for (const kind of ['affine', 'projective']) {
    const all = f32(cs[kind]);
    const lists = [];
    for (let f = 0; f < cs.F; f++) {
        const l = all.slice(f * cs.N * 4, (f + 1) * cs.N * 4);
        lists.push(f % 2 ? Array.from({ length: cs.N }, (_, i) => Array.from(l.slice(4 * i, 4 * i + 4))) : l);      // both accepted forms
    }
    lists[cs.F - 1] = lists[cs.F - 1].slice(0, cs.short * (lists[cs.F - 1] instanceof Float32Array ? 4 : 1));        // a shorter last list: padding and counts
    const r = h.fitMatches(lists, { transform: kind, threshold: cs.threshold, hypotheses: cs.hypotheses, seed: cs.seed });
    check(r.kind === kind && r.matrices.length === 8 * cs.F && r.inliers.length === cs.F && r.inliers[cs.F - 1].length === cs.short, `${kind}: shape of the result`);
    check(Array.from(r.best).every((b) => b >= 0) && Array.from(r.counts).every((c, f) => c === r.inliers[f].reduce((s, v) => s + v, 0)), `${kind}: counts equal the masks' sums`);
    cases[kind] = { matrices: b64(r.matrices), minimal: b64(r.minimal), counts: Array.from(r.counts), best: Array.from(r.best), inliers: r.inliers.map((m) => b64(m)) };
    if (kind === 'affine') {
        h._native.setImage(h._ctx, data, W, H);
        const geoms = new Int32Array(cs.F * 4);
        for (let f = 0; f < cs.F; f++) geoms.set([0, 0, W, H], 4 * f);
        const frames = h._native.warpForwardGeometricBatch(h._ctx, 0, r.matrices, geoms);
        check(frames.length === cs.F && frames.every((fr) => fr.length === W * H * 4 && fr.some((v) => v !== 0)), 'the fitted matrices through warpForwardGeometricBatch: frames with pixels');
    }
}
h.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails, cases }));
process.exit(fails.length === 0 ? 0 : 1);
