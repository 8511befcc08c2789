// GPU: matchDescriptors() of the drop-in class on the real addon.  The cases come from the JSON file named on the command line (written by
// tests/test_gpu_match.py: per kind F query sets of nq rows and ONE train set of nt rows at their stride, with points, base64); the last
// query set is cut to `short` rows (padding and counts).  The results go out as base64 in one JSON line, which the test compares word for
// word with the ctypes call.  The matches of the binary case are then fed to fitMatches: it must run.  Exit code 1 on a failure.
import fs from 'fs';
import { Homography } from '../../homography.js_amd/js/Homography.mjs';

const fails = [];
const check = (ok, what) => { if (!ok) fails.push(what); };
const cs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const b64 = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength).toString('base64');
const u8 = (s) => { const b = Buffer.from(s, 'base64'); return new Uint8Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };
const f32 = (s) => new Float32Array(u8(s).buffer);

const h = new Homography('projective', 64, 48);
const cases = {};
for (const kind of ['bits', 'u8']) {
    const c = cs[kind], nb = c.bytes;                              // (the test's stride equals the row length here)
    const query = u8(c.query), train = u8(c.train), qpts = f32(c.qpts), tpts = f32(c.tpts);
    const qs = [], qp = [];
    for (let f = 0; f < cs.F; f++) {
        const n = f === cs.F - 1 ? cs.short : cs.nq;
        qs.push(query.slice(f * cs.nq * nb, (f * cs.nq + n) * nb));
        const p = qpts.slice(f * cs.nq * 2, (f * cs.nq + n) * 2);
        qp.push(f % 2 ? Array.from({ length: n }, (_, i) => [p[2 * i], p[2 * i + 1]]) : p);      // both accepted forms
    }
    const r = h.matchDescriptors(qs, [train], { kind, descBytes: nb, ratio: cs.ratio, crossCheck: true, queryPoints: qp, trainPoints: [tpts] });
    check(r.length === cs.F && r.every((x) => x.pairs.length === 2 * x.count && x.matches.length === 4 * x.count), `${kind}: shape of the result`);
    check(r.some((x) => x.count > 0) && r[cs.F - 1].count <= cs.short, `${kind}: some pairs`);
    cases[kind] = { counts: r.map((x) => x.count), pairs: r.map((x) => b64(x.pairs)), matches: r.map((x) => b64(x.matches)) };
    if (kind === 'bits') {
        const fit = h.fitMatches(r.map((x) => x.matches), { transform: 'affine', hypotheses: 16 });
        check(fit.counts.length === cs.F && fit.inliers.every((m, f) => m.length === r[f].count), 'the matches through fitMatches');
    }
}
h.close();
console.log(JSON.stringify({ ok: fails.length === 0, fails, cases }));
process.exit(fails.length === 0 ? 0 : 1);
