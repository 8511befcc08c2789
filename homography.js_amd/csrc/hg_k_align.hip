// hg_k_align.hip -- refining frame transforms on the pixels by Gauss-Newton (include/hgwarp.h, "refining transforms on the pixels"; DESIGN.md
// §4.17).  Per pass two launches over all frames:
//   k_align_accumulate  one workgroup per (frame, chunk of kAlignChunk samples): every lane walks its samples in a stride of the workgroup and
//                       keeps the pass's sums -- the upper triangle of J^T J, J^T r, sum r r, the valid count -- in f64 registers; the
//                       workgroup adds them through a fixed tree in LDS, kAlignRed sums at a time, and writes ONE partial record.  A
//                       workgroup whose frame has stopped reads the frame's flag and returns
//   k_align_update      one workgroup per frame: lane k adds entry k of the chunk records in ascending chunk order; one lane then solves,
//                       moves the iterate, tests displacement, rms and min_valid, sets the flag, and writes matrix and info when the frame stops
//   k_align_luma        (4-channel planes, once per call) the detector's luma of every pixel into a one-byte plane, so that the passes do not
//                       redo 12 lumas per sample
// No floating-point atomics: two runs of one call give the same bits.  The rules live in hg_align_dev.h.  The kernels need that header only,
// so a host check compiles this file behind a thread-index shim (tests/cpp/align_check.cpp); the launchers are compiled under hipcc only.
#ifdef __HIPCC__
#include "hg_kernels.h"
#endif
#include "hg_align_dev.h"

namespace hg {

#ifndef __HIPCC__
// (under hipcc hg_kernels.h declares it)
struct AlignArgs {
    int kind, photometric; const uint8_t *from; int Wf, Hf; size_t from_stride; const uint8_t *to; int Wt, Ht, n_to_sets; size_t to_stride;
    int rx, ry, rw, rh, step, nx, n_samples, n_chunks, n_frames, n_iter; double eps; int min_valid;
    const double *mats_in; double *mats_out; AlignInfo *info; double *sums; AlignState *state; double *part;
};
#endif

constexpr int kAlignRed = 23;           // sums per round of the workgroup's tree (23 x 256 doubles of LDS; 67 values at P = 10: three rounds)

// ------------------------------------------------------------------------------------------------ k_align_luma
__global__ __launch_bounds__(kAlignBlock) void k_align_luma(const uint8_t *__restrict__ src, size_t src_stride, uint32_t n_px, uint8_t *__restrict__ dst)
{
    const uint8_t *__restrict__ s = src + (size_t)blockIdx.y * src_stride;
    uint8_t *__restrict__ d = dst + (size_t)blockIdx.y * (size_t)n_px;
    for (uint32_t i = blockIdx.x * kAlignBlock + threadIdx.x; i < n_px; i += gridDim.x * kAlignBlock) {
        const uint8_t *p = s + (size_t)i * 4;
        d[i] = (uint8_t)((77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8);
    }
}

// ------------------------------------------------------------------------------------------------ k_align_accumulate
template <int KIND, int PHOTO>
__global__ __launch_bounds__(kAlignBlock) void k_align_accumulate(AlignArgs a, int pass)
{
    constexpr int P = (KIND == 1 ? 8 : 6) + (PHOTO ? 2 : 0), NS = P * (P + 1) / 2 + P + 1, NV = NS + 1;
    constexpr int ROUNDS = (NV + kAlignRed - 1) / kAlignRed;
    __shared__ double sh[kAlignRed * kAlignBlock];
    const int f = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const AlignGeom g = align_geom(a.Wf, a.Hf, a.Wt, a.Ht, a.rx, a.ry, a.rw, a.rh);
    double h[8], gain = 1.0, bias = 0.0;
    if (pass == 0) {
        align_normalise(KIND, a.mats_in + (size_t)f * 8, g, h);
    } else {
        const AlignState *st = a.state + f;
        if (st->phase == 2) return;                            // (uniform over the workgroup: nobody reaches a barrier)
#pragma unroll
        for (int k = 0; k < 8; k++) h[k] = st->h[k];
        gain = st->gain; bias = st->bias;
    }
    const uint8_t *__restrict__ from = a.from + (size_t)f * a.from_stride;
    const uint8_t *__restrict__ to = a.to + (size_t)(f % a.n_to_sets) * a.to_stride;
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] = 0.0;
    double cnt = 0.0;
    for (int k = 0; k < kAlignChunk / kAlignBlock; k++) {
        const int s = chunk * kAlignChunk + k * kAlignBlock + tid;
        if (s >= a.n_samples) break;
        const int j = s / a.nx, i = s - j * a.nx;
        const int px = a.rx + i * a.step, py = a.ry + j * a.step;          // (inside the FROM plane: the API checked the rectangle)
        double xn, yn, D, un, vn, u, v;
        align_warp<KIND>(h, g, (double)px, (double)py, xn, yn, D, un, vn, u, v);
        if (!align_valid(u, v, D, a.Wt, a.Ht)) continue;
        double I, dx, dy, r, J[P];
        align_taps(to, a.Wt, u, v, I, dx, dy);
        align_row<KIND, PHOTO>(g, (double)from[(size_t)py * (size_t)a.Wf + (size_t)px], gain, bias, xn, yn, D, un, vn, I, dx, dy, r, J);
        int idx = 0;
#pragma unroll
        for (int p = 0; p < P; p++) {
#pragma unroll
            for (int q = p; q < P; q++) acc[idx++] += J[p] * J[q];
        }
#pragma unroll
        for (int p = 0; p < P; p++) acc[idx++] += J[p] * r;
        acc[idx] += r * r;
        cnt += 1.0;
    }
    double *__restrict__ out = a.part + ((size_t)f * a.n_chunks + chunk) * kAlignRec;
#pragma unroll
    for (int round = 0; round < ROUNDS; round++) {
        const int v0 = round * kAlignRed;
        const int nv = NV - v0 < kAlignRed ? NV - v0 : kAlignRed;
#pragma unroll
        for (int q = 0; q < kAlignRed; q++) {
            const int v = v0 + q;
            if (v < NS) sh[q * kAlignBlock + tid] = acc[v]; else if (v == NS) sh[q * kAlignBlock + tid] = cnt;
        }
        __syncthreads();
#pragma unroll
        for (int s = kAlignBlock / 2; s > 0; s >>= 1) {
            for (int idx = tid; idx < nv * s; idx += kAlignBlock) {
                const int q = idx / s, l = idx - q * s;
                sh[q * kAlignBlock + l] += sh[q * kAlignBlock + l + s];
            }
            __syncthreads();
        }
        if (tid < nv) out[(v0 + tid) == NS ? kAlignSums : (v0 + tid)] = sh[tid * kAlignBlock];      // (the count sits behind the 66 slots of the sums)
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ k_align_update
// The frame stops: status, matrix and info.  copy: the input's bits instead of the iterate.
__device__ inline void align_finish(const AlignArgs &a, int kind, int f, AlignState *st, const AlignGeom &g, int status, bool copy, int n_first, int n_last)
{
    double m[8];
    const double *in = a.mats_in + (size_t)f * 8;
    if (copy) { for (int k = 0; k < 8; k++) m[k] = in[k]; }
    else align_denormalise(kind, st->h, g, m);
    for (int k = 0; k < 8; k++) a.mats_out[(size_t)f * 8 + k] = m[k];
    AlignInfo o;
    o.status = status; o.updates = st->updates; o.n_valid_first = n_first; o.n_valid_last = n_last;
    o.rms_first = st->rms_first; o.rms_last = st->rms_last;
    o.gain = copy ? 1.0 : st->gain; o.bias = copy ? 0.0 : st->bias;
    a.info[f] = o;
    st->phase = 2;
}

template <int KIND, int PHOTO>
__global__ __launch_bounds__(kAlignBlock) void k_align_update(AlignArgs a, int pass)
{
    constexpr int P = (KIND == 1 ? 8 : 6) + (PHOTO ? 2 : 0), NS = P * (P + 1) / 2 + P + 1, TRI = P * (P + 1) / 2;
    __shared__ double S[kAlignRec];
    __shared__ double A[10 * 11];
    const int f = blockIdx.x, tid = threadIdx.x;
    AlignState *st = a.state + f;
    if (pass > 0 && st->phase == 2) return;                    // (uniform over the workgroup)
    if (tid <= NS) {
        const double *__restrict__ p = a.part + (size_t)f * a.n_chunks * kAlignRec + (tid == NS ? kAlignSums : tid);
        double s = 0.0;
#pragma unroll 8
        for (int c = 0; c < a.n_chunks; c++) s += p[(size_t)c * kAlignRec];
        S[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const AlignGeom g = align_geom(a.Wf, a.Hf, a.Wt, a.Ht, a.rx, a.ry, a.rw, a.rh);
    const double qnan = NAN;
    const int n = (int)S[NS];
    if (pass == 0) {
        const double *in = a.mats_in + (size_t)f * 8;
        bool fin = true;
        for (int k = 0; k < (KIND == 1 ? 8 : 6); k++) fin = fin && align_finite(in[k]);
        align_normalise(KIND, in, g, st->h);
        st->gain = 1.0; st->bias = 0.0; st->rms_first = qnan; st->rms_last = qnan;
        st->phase = 0; st->pending = 1; st->updates = 0; st->n_first = n;
        if (a.sums) {
            double *o = a.sums + (size_t)f * kAlignSums;
            for (int k = 0; k < kAlignSums; k++) o[k] = k < NS ? S[k] : 0.0;
        }
        if (!fin) { align_finish(a, KIND, f, st, g, 5, true, 0, 0); return; }
    }
    if (n < a.min_valid) { align_finish(a, KIND, f, st, g, 2, true, st->n_first, n); return; }
    const double rms = sqrt(S[NS - 1] / (double)n);
    if (pass == 0) st->rms_first = rms;
    st->rms_last = rms;
    if (st->phase == 1 || a.n_iter == 0) {                     // this pass evaluated the final iterate
        const bool worse = rms > st->rms_first;
        align_finish(a, KIND, f, st, g, worse ? 4 : st->pending, worse || st->updates == 0, st->n_first, n);
        return;
    }
    // J^T J delta = J^T r
    constexpr int ld = P + 1;
    int idx = 0;
    for (int p = 0; p < P; p++) for (int q = p; q < P; q++) { A[p * ld + q] = S[idx]; A[q * ld + p] = S[idx]; idx++; }
    for (int p = 0; p < P; p++) A[p * ld + P] = S[TRI + p];
    align_gauss(A, P, ld);
    double hn[8], gain = st->gain, bias = st->bias;
    for (int k = 0; k < 8; k++) hn[k] = st->h[k];
    bool fin = true;
    for (int k = 0; k < P; k++) fin = fin && align_finite(A[k * ld + P]);
    for (int k = 0; k < (KIND == 1 ? 8 : 6); k++) hn[align_slot(KIND, k)] += A[k * ld + P];
    if (PHOTO) { gain += A[(P - 2) * ld + P]; bias += A[(P - 1) * ld + P]; }
    for (int k = 0; k < 8; k++) fin = fin && align_finite(hn[k]);
    fin = fin && align_finite(gain) && align_finite(bias);
    if (!fin) { align_finish(a, KIND, f, st, g, 3, true, st->n_first, n); return; }
    const double disp = align_displacement(KIND, st->h, hn, g);
    for (int k = 0; k < 8; k++) st->h[k] = hn[k];
    st->gain = gain; st->bias = bias;
    st->updates += 1;
    if (disp < a.eps) { st->pending = 0; st->phase = 1; }
    else if (st->updates == a.n_iter) { st->pending = 1; st->phase = 1; }
}

// ------------------------------------------------------------------------------------------------ launches
#ifdef __HIPCC__
void launch_align_luma(const uint8_t *src, size_t src_stride, int W, int H, int n_planes, uint8_t *dst, hipStream_t stream)
{
    if (n_planes <= 0) return;
    const uint32_t n_px = (uint32_t)W * (uint32_t)H;
    const uint32_t blocks = std::min<uint32_t>((n_px + kAlignBlock * 8 - 1) / (kAlignBlock * 8), 4096u);
    hipLaunchKernelGGL(k_align_luma, dim3(std::max<uint32_t>(blocks, 1u), n_planes), dim3(kAlignBlock), 0, stream, src, src_stride, n_px, dst);
}

template <int KIND, int PHOTO>
static void align_passes(const AlignArgs &a, hipStream_t stream)
{
    for (int pass = 0; pass <= a.n_iter; pass++) {
        hipLaunchKernelGGL((k_align_accumulate<KIND, PHOTO>), dim3(a.n_chunks, a.n_frames), dim3(kAlignBlock), 0, stream, a, pass);
        hipLaunchKernelGGL((k_align_update<KIND, PHOTO>), dim3(a.n_frames), dim3(kAlignBlock), 0, stream, a, pass);
    }
}

void launch_align(const AlignArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0) return;
    if (a.kind == 1) { if (a.photometric) align_passes<1, 1>(a, stream); else align_passes<1, 0>(a, stream); }
    else { if (a.photometric) align_passes<0, 1>(a, stream); else align_passes<0, 0>(a, stream); }
}
#endif

} // namespace hg
