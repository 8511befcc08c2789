// GPU: bundleAdjust(), chainMatrices() and invertMatrix() of the drop-in class on the real addon.  The cases come from the JSON file named
// on the command line (written by tests/test_gpu_bundle.py: per kind the matrices, the pairs, one match list per pair, a mask per pair and
// the options, arrays as base64); the results go out as base64 in one JSON line, which the test compares bit for bit with the ctypes calls
// on the same inputs.  Exit code 1 on a failure.
import fs from 'fs';
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const cs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const b64 = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength).toString('base64');
const raw = (s) => { const b = Buffer.from(s, 'base64'); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length); };

const h = new Homography('projective', 64, 48);
const cases = {};
for (const [name, c] of Object.entries(cs)) {
    const mats = new Float64Array(raw(c.matrices));
    const lists = c.matches.map((m, p) => {
        const l = new Float32Array(raw(m));
        return p % 2 ? Array.from({ length: l.length / 4 }, (_, i) => Array.from(l.slice(4 * i, 4 * i + 4))) : l;      // both accepted forms
    });
    const masks = c.masks === null ? undefined : c.masks.map((m) => new Uint8Array(raw(m)));
    const r = h.bundleAdjust(mats, c.pairs, lists, { transform: c.transform, width: c.width, height: c.height, fixed: c.fixed, iterations: c.iterations, eps: c.eps,
                                                     lambda: c.lambda, huber: c.huber, masks });
    check(r.matrices.length === mats.length && r.frames.length === mats.length / 8 && r.pairs.length === c.pairs.length, `${name}: shape of the result`);
    check(r.rmsLast <= r.rmsFirst && r.accepted >= 1, `${name}: the rms falls`);
    const pm = new Float64Array(raw(c.pairMatrices));
    const chained = h.chainMatrices(pm, c.pairs, { frames: mats.length / 8, anchor: c.anchor, transform: c.transform });
    const inverse = new Float64Array(mats.length);
    for (let f = 0; f < mats.length / 8; f++) inverse.set(h.invertMatrix(r.matrices.slice(8 * f, 8 * f + 8), { transform: c.transform }), 8 * f);
    cases[name] = { matrices: b64(r.matrices), status: r.status, rounds: r.rounds, accepted: r.accepted, rms: b64(Float64Array.from([r.rmsFirst, r.rmsLast])),
                    frames: Array.from(r.frames), nValid: r.pairs.map((p) => [p.nValidFirst, p.nValidLast]),
                    pairRms: b64(Float64Array.from(r.pairs.flatMap((p) => [p.rmsFirst, p.rmsLast]))), chained: b64(chained), inverse: b64(inverse) };
}
h.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails, cases }));
process.exit(fails.length === 0 ? 0 : 1);
