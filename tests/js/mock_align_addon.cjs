// mock_align_addon.cjs -- tests/js/mock_fit_addon.cjs plus the addon's alignment functions, with the same trace, for one purpose: checking
// without a GPU what refineAlignment() of the drop-in class hands to the native layer and in which order (tests/js/align_class.mjs; select it
// with HGWARP_ADDON=<this file>).  TEST INFRASTRUCTURE ONLY.
//   alignBegin(ctx, from, Wf, Hf, F, to, Wt, Ht, S, channels, levels) records its arguments and returns a job { id, F, open: true };
//   alignScaleMatrix(kind, matrices, levelIn, levelOut) is the real conversion in doubles, S M S^-1 with S = [e 0 o; 0 e o; 0 0 1], e = 2^(in - out),
//     o = (e - 1) / 2 (rows with an entry that is not finite are copied);
//   alignLevel(ctx, job, kind, level, rect, step, photometric, nIter, eps, minValid, matrices) records its arguments and returns the matrices with
//     0.5 added to the x translation, status[f] = level, updates[f] = f + 1, nValid (10 f, 10 f + 1), rms (f, f + 0.5), gains (1 + f, -f);
//   alignEnd(ctx, job) closes the job.  The values are the GPU tests' business.
'use strict';
const path = require('path');
const base = require(path.join(__dirname, 'mock_fit_addon.cjs'));

const mock = Object.assign({}, base);
mock.alignCalls = [];
let jobs = 0;
mock.alignBegin = (c, from, Wf, Hf, F, to, Wt, Ht, S, channels, levels, ...rest) => {
    if (rest.length || !(from instanceof Uint8Array) || !(to instanceof Uint8Array) || from.length !== F * Wf * Hf * channels || to.length !== S * Wt * Ht * channels)
        throw ('hgwarp mock: alignBegin arguments');
    const job = { id: ++jobs, F, open: true };
    base.trace.push(['alignBegin', Wf, Hf, F, Wt, Ht, S, channels, levels]);
    mock.alignCalls.push({ fn: 'alignBegin', from: Uint8Array.from(from), to: Uint8Array.from(to), Wf, Hf, F, Wt, Ht, S, channels, levels, job: job.id });
    return job;
};
mock.alignScaleMatrix = (kind, matrices, levelIn, levelOut, ...rest) => {
    if (rest.length || !(matrices instanceof Float64Array) || matrices.length % 8) throw ('hgwarp mock: alignScaleMatrix arguments');
    const e = 2 ** (levelIn - levelOut), o = (e - 1) / 2, oi = (1 / e - 1) / 2;
    const out = new Float64Array(matrices.length);
    for (let f = 0; f < matrices.length / 8; f++) {
        const m = matrices.slice(8 * f, 8 * f + 8);
        if (!m.every(Number.isFinite)) { out.set(m, 8 * f); continue; }
        const a = kind === 1 ? [m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], 1] : [m[0], m[2], m[4], m[1], m[3], m[5], 0, 0, 1];
        const b = [];
        for (let r = 0; r < 3; r++) b.push(a[3 * r] / e, a[3 * r + 1] / e, a[3 * r] * oi + a[3 * r + 1] * oi + a[3 * r + 2]);
        const s = [];
        for (let k = 0; k < 3; k++) { s[k] = e * b[k] + o * b[6 + k]; s[3 + k] = e * b[3 + k] + o * b[6 + k]; s[6 + k] = b[6 + k]; }
        out.set(kind === 1 ? s.slice(0, 8).map((v) => v / s[8]) : [s[0], s[3], s[1], s[4], s[2], s[5], 0, 0], 8 * f);
    }
    base.trace.push(['alignScaleMatrix', kind, levelIn, levelOut]);
    mock.alignCalls.push({ fn: 'alignScaleMatrix', kind, levelIn, levelOut, matrices: Float64Array.from(matrices), out: Float64Array.from(out) });
    return out;
};
mock.alignLevel = (c, job, kind, level, rect, step, photometric, nIter, eps, minValid, matrices, ...rest) => {
    if (rest.length || !job || !job.open || !(rect instanceof Int32Array) || rect.length !== 4 || !(matrices instanceof Float64Array) || matrices.length !== 8 * job.F)
        throw ('hgwarp mock: alignLevel arguments');
    base.trace.push(['alignLevel', kind, level, Array.from(rect), step, photometric, nIter, eps, minValid]);
    mock.alignCalls.push({ fn: 'alignLevel', job: job.id, kind, level, rect: Array.from(rect), step, photometric, nIter, eps, minValid, matrices: Float64Array.from(matrices) });
    const F = job.F, out = Float64Array.from(matrices);
    for (let f = 0; f < F; f++) out[8 * f + (kind === 1 ? 2 : 4)] += 0.5;
    return { matrices: out, status: Int32Array.from({ length: F }, () => level), updates: Int32Array.from({ length: F }, (_, f) => f + 1),
             nValid: Int32Array.from({ length: 2 * F }, (_, k) => 10 * (k >> 1) + (k & 1)), rms: Float64Array.from({ length: 2 * F }, (_, k) => (k >> 1) + 0.5 * (k & 1)),
             gains: Float64Array.from({ length: 2 * F }, (_, k) => (k & 1 ? -(k >> 1) : 1 + (k >> 1))) };
};
mock.alignEnd = (c, job, ...rest) => {
    if (rest.length || !job || !job.open) throw ('hgwarp mock: alignEnd arguments');
    job.open = false;
    base.trace.push(['alignEnd', job.id]);
    mock.alignCalls.push({ fn: 'alignEnd', job: job.id });
};
module.exports = mock;
