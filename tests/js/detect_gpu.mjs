// GPU: detectAndDescribe() -> matchDescriptors() -> fitMatches() of the drop-in class on the real addon, on one pair of pictures.  The case
// comes from the JSON file named on the command line (written by tests/test_gpu_detect.py: a frame and a keyframe as RGBA, base64, and the
// settings).  The results go out as base64 in one JSON line, which the test compares word for word with the ctypes calls and the numpy
// models.  Exit code 1 on a failure.
import fs from 'fs';
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const cs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const b64 = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength).toString('base64');
const u8 = (s) => { const b = Buffer.from(s, 'base64'); return new Uint8Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };

const h = new Homography('projective', 64, 48);
const out = {};
const sides = {};
for (const name of ['frame', 'key']) {
    const c = cs[name];
    const r = h.detectAndDescribe([u8(c.data)], { width: c.width, height: c.height, cell: cs.cell, perCell: cs.perCell, minResponse: cs.minResponse });
    check(r.length === 1 && r[0].points.length === 2 * r[0].count && r[0].descriptors.length === 32 * r[0].count && r[0].count > 0, `${name}: shape of the result`);
    sides[name] = r[0];
    out[name] = { count: r[0].count, points: b64(r[0].points), descriptors: b64(r[0].descriptors) };
}
const m = h.matchDescriptors([sides.frame.descriptors], [sides.key.descriptors], { ratio: 0.8, queryPoints: [sides.frame.points], trainPoints: [sides.key.points] });
check(m.length === 1 && m[0].count > 0, 'some pairs');
out.match = { count: m[0].count, pairs: b64(m[0].pairs), matches: b64(m[0].matches) };
const fit = h.fitMatches([m[0].matches], { transform: 'projective', threshold: cs.threshold, hypotheses: cs.nHyp, seed: cs.seed, refit: false });
check(fit.counts.length === 1 && fit.inliers[0].length === m[0].count, 'the matches through fitMatches');
out.fit = { count: fit.counts[0], best: fit.best[0], minMatrix: b64(fit.minimal) };
h.close();
console.log(JSON.stringify(Object.assign({ ok: fails.length === 0, fails }, out)));
process.exit(fails.length === 0 ? 0 : 1);
