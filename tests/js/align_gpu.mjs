// GPU: refineAlignment() of the drop-in class on the real addon.  The planted cases come from the JSON file named on the command line
// (written by tests/test_gpu_align.py: per kind the RGBA FROM and TO planes and the start matrices, base64); the results go out as base64 in
// one JSON line, which the test compares bit for bit with the ctypes call on the same planes.  A walk over two levels must run, end every
// frame with a status of a frame that moved, and land near the one-level result.  Exit code 1 on a failure.
import fs from 'fs';
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const cs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const b64 = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength).toString('base64');
const bytes = (s) => { const b = Buffer.from(s, 'base64'); return new Uint8Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };

const h = new Homography('projective', 64, 48);
const cases = {};
for (const kind of ['affine', 'projective']) {
    const c = cs[kind];
    const from = c.from.map((s, f) => (f % 2 ? new Uint8ClampedArray(bytes(s)) : bytes(s)));      // both accepted forms
    const to = c.to.map(bytes);
    const mats = new Float64Array(bytes(c.matrices).buffer);
    const opts = { width: c.width, height: c.height, toWidth: c.toWidth, toHeight: c.toHeight, channels: 4, transform: kind, rect: c.rect, step: c.step,
                   iterations: c.iterations, eps: c.eps, photometric: true };
    const r = h.refineAlignment(from, to, mats, opts);
    const F = from.length;
    check(r.matrices.length === 8 * F && r.status.length === F && r.updates.length === F && r.rms.length === F && r.gains.length === 2 * F, `${kind}: shape of the result`);
    check(Array.from(r.status).every((s) => s === 0 || s === 1), `${kind}: every frame moved (${Array.from(r.status)})`);
    cases[kind] = { matrices: b64(r.matrices), status: Array.from(r.status), updates: Array.from(r.updates), rms: b64(r.rms), gains: b64(r.gains) };
    const r2 = h.refineAlignment(from, to, mats, Object.assign({}, opts, { levels: 2 }));
    check(Array.from(r2.status).every((s) => s === 0 || s === 1), `${kind}: two levels: every frame moved (${Array.from(r2.status)})`);
    let far = 0;
    for (let k = 0; k < 8 * F; k++) far = Math.max(far, Math.abs(r2.matrices[k] - r.matrices[k]));
    check(far < 0.05, `${kind}: two levels land near one level (largest entry difference ${far})`);
}
h.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails, cases }));
process.exit(fails.length === 0 ? 0 : 1);
