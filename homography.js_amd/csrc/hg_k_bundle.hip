// hg_k_bundle.hip -- adjusting the transforms of a frame set over all pairs by Levenberg-Marquardt (include/hgwarp.h, "adjusting a frame set
// over all pairs").  Every round of a call is queued at once; the kernels of rounds after the stop read the flag and return.
//   k_bundle_init        normalises the input matrices into iterate buffer 0 and resets the state
//   k_bundle_pass        one workgroup per (pair, chunk of kBundleChunk slots): 128 lanes write the two rows [J_a | J_b | r] of their slots into
//                        LDS, then lane e owns entry e of the record -- the upper triangle of the weighted Gram matrix of those rows -- and
//                        adds the tile's slots in ascending order: one f64 accumulator per lane instead of 153
//   k_bundle_reduce      one workgroup per pair: lane e adds entry e of the pair's chunk records in ascending chunk order
//   k_bundle_decide      one workgroup: the cost of what the pass evaluated, accept or reject, lambda, the stop tests, and on the stop every
//                        output.  One lane decides
//   k_bundle_assemble    one workgroup per free frame: its P rows of H and of the gradient from the records that touch it, ascending pair index
//   k_bundle_round_small N <= kBundleLdsCap: ONE workgroup per round beside the pass -- the pass's reduction, the decision, then assembly, damping,
//                        factorisation (Cholesky, the gradient as row N so that the forward substitution is part of it), back substitution
//                        and the candidate, H and g in LDS throughout
//   k_bundle_damp, _chol_diag, _chol_panel, _chol_trail, _back_large   the same arithmetic, blocked right-looking in the caller's scratch
// Every entry of the factor is a_ij minus l_ik l_jk for k = 0, 1, .. j - 1, one at a time, whichever path: the two paths give the same bits.
// No floating-point atomics.  The rules live in hg_bundle_dev.h; the launchers are compiled under hipcc only.
#ifdef __HIPCC__
#include "hg_kernels.h"
#endif
#include "hg_bundle_dev.h"

namespace hg {

// ------------------------------------------------------------------------------------------------ k_bundle_init
__global__ __launch_bounds__(kBundleBlock) void k_bundle_init(BundleArgs a)
{
    const int tid = threadIdx.x;
    const AlignGeom g = align_geom(a.W, a.H, a.W, a.H, 0, 0, a.W, a.H);
    const int np = bundle_p(a.kind);
    for (int f = tid; f < a.n_frames; f += kBundleBlock) {
        const double *in = a.mats_in + (size_t)f * 8;
        bool fin = true;
        for (int k = 0; k < np; k++) fin = fin && align_finite(in[k]);
        double h[8];
        align_normalise(a.kind, in, g, h);
        for (int k = 0; k < 8; k++) fin = fin && align_finite(h[k]);
        for (int k = 0; k < 8; k++) a.iter[(size_t)f * 8 + k] = fin ? h[k] : (double)NAN;
        a.good[f] = fin ? 1 : 0;
    }
    if (tid == 0) {
        BundleState *st = a.state;
        st->cost = 0.0; st->lambda = a.lambda0; st->rms_first = NAN;
        st->cur = 0; st->done = 0; st->sing = 0; st->fresh = 1; st->rounds = 0; st->accepted = 0; st->n_cur = 0; st->n_first = 0;
    }
}

// ------------------------------------------------------------------------------------------------ k_bundle_pass
template <int KIND>
__global__ __launch_bounds__(kBundleBlock) void k_bundle_pass(BundleArgs a, int pass)
{
    constexpr int P = KIND == 1 ? 8 : 6, NV = 2 * P + 1, NE = NV * (NV + 1) / 2, STR = 2 * NV + 3;
    __shared__ double V[kBundleTile * STR];
    const BundleState *st = a.state;
    if (pass > 0 && (st->done != 0 || st->sing != 0)) return;          // (uniform over the workgroup)
    const int tid = threadIdx.x;
    const int pair = a.work[2 * blockIdx.x], chunk = a.work[2 * blockIdx.x + 1];
    const int fa = a.pairs4[4 * pair], fb = a.pairs4[4 * pair + 1], count = a.pairs4[4 * pair + 2];
    const double *__restrict__ X = a.iter + (size_t)(pass == 0 ? 0 : (st->cur ^ 1)) * (size_t)a.n_frames * 8;
    const AlignGeom g = align_geom(a.W, a.H, a.W, a.H, 0, 0, a.W, a.H);
    double ha[8], hb[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { ha[k] = X[(size_t)fa * 8 + k]; hb[k] = X[(size_t)fb * 8 + k]; }
    int ei = 0, ej = 0;                                                // this lane's entry of the triangle
    if (tid < NE) { int rem = tid; while (rem >= NV - ei) { rem -= NV - ei; ei++; } ej = ei + rem; }
    const float4 *__restrict__ M = reinterpret_cast<const float4 *>(a.matches) + (size_t)pair * (size_t)a.n_points;
    const uint8_t *__restrict__ mask = a.mask ? a.mask + (size_t)pair * (size_t)a.n_points : nullptr;
    double acc = 0.0;
    for (int t = 0; t < kBundleChunk / kBundleTile; t++) {
        const int base = chunk * kBundleChunk + t * kBundleTile;
        if (base >= count) break;                                      // (uniform)
        const int n = count - base < kBundleTile ? count - base : kBundleTile;
        if (tid < n) {
            const int s = base + tid;
            const float4 m = M[s];
            double vx[NV], vy[NV], w = 0.0, rho = 0.0;
            const bool ok = bundle_slot<KIND>(ha, hb, g, m.x, m.y, m.z, m.w, mask ? mask[s] != 0 : true, a.huber, vx, vy, w, rho);
            double *row = V + tid * STR;
#pragma unroll
            for (int k = 0; k < NV; k++) { row[k] = ok ? vx[k] : 0.0; row[NV + k] = ok ? vy[k] : 0.0; }
            row[2 * NV] = ok ? w : 0.0; row[2 * NV + 1] = ok ? rho : 0.0; row[2 * NV + 2] = ok ? 1.0 : 0.0;
        }
        __syncthreads();
        if (tid < NE - 1) {
            for (int q = 0; q < n; q++) {
                const double *row = V + q * STR;
                acc += row[2 * NV] * ((row[ei] * row[ej]) + (row[NV + ei] * row[NV + ej]));
            }
        } else if (tid <= NE) {                                        // the cost in place of sum w r r, then the count
            for (int q = 0; q < n; q++) acc += V[q * STR + 2 * NV + 1 + (tid - (NE - 1))];
        }
        __syncthreads();
    }
    if (tid <= NE) a.part[(size_t)blockIdx.x * kBundleRec + tid] = acc;
}

// ------------------------------------------------------------------------------------------------ k_bundle_reduce
// Lane e < kBundleRec adds entry e of the pair's chunk records in ascending chunk order into record buffer `buf` (and into d_pair_sums in pass 0).
__device__ inline void bundle_reduce_pair(const BundleArgs &a, int pair, int pass, int buf, int tid)
{
    if (tid >= kBundleRec) return;
    const int np = bundle_p(a.kind), nv = 2 * np + 1, ne = nv * (nv + 1) / 2;
    const int count = a.pairs4[4 * pair + 2], first = a.pairs4[4 * pair + 3];
    const int nchunks = (count + kBundleChunk - 1) / kBundleChunk;
    double s = 0.0;
    if (tid <= ne) {
        const double *__restrict__ p = a.part + (size_t)first * kBundleRec + tid;
        for (int c = 0; c < nchunks; c++) s += p[(size_t)c * kBundleRec];
    }
    a.recs[((size_t)buf * a.n_pairs + pair) * kBundleRec + tid] = s;
    if (pass == 0 && a.sums) a.sums[(size_t)pair * kBundleRec + tid] = s;
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_reduce(BundleArgs a, int pass)
{
    const BundleState *st = a.state;
    if (pass > 0 && (st->done != 0 || st->sing != 0)) return;
    bundle_reduce_pair(a, blockIdx.x, pass, pass == 0 ? 0 : (st->cur ^ 1), threadIdx.x);
}

// ------------------------------------------------------------------------------------------------ k_bundle_decide
// All lanes of one workgroup call it after the pass of `round` and its reduction.  False (for all of them) when the call has stopped.
__device__ inline bool bundle_decide(const BundleArgs &a, int round)
{
    __shared__ double s_c[kBundleBlock], s_n[kBundleBlock], s_d[kBundleBlock];
    __shared__ int s_bad, s_stop, s_copy, s_cur;
    BundleState *st = a.state;
    if (round > 0 && st->done != 0) return false;                      // (uniform)
    const int tid = threadIdx.x, F = a.n_frames;
    const int np = bundle_p(a.kind), nv = 2 * np + 1, ne = nv * (nv + 1) / 2;
    const int cur = st->cur, sing = st->sing;
    const int ebuf = round == 0 ? 0 : (cur ^ 1);                       // what the pass before this launch evaluated
    const double *__restrict__ R = a.recs + (size_t)ebuf * a.n_pairs * kBundleRec;
    const AlignGeom g = align_geom(a.W, a.H, a.W, a.H, 0, 0, a.W, a.H);
    double c = 0.0, n = 0.0, d = 0.0;
    int bad = 0;
    if (!sing) {
        for (int p = tid; p < a.n_pairs; p += kBundleBlock) { c += R[(size_t)p * kBundleRec + ne - 1]; n += R[(size_t)p * kBundleRec + ne]; }
        if (round > 0) {
            const double *Xc = a.iter + (size_t)cur * F * 8, *Xn = a.iter + (size_t)(cur ^ 1) * F * 8;
            for (int f = tid; f < F; f += kBundleBlock) {
                if (a.cls[f] != 0 || a.good[f] == 0) continue;
                for (int k = 0; k < 8; k++) if (!align_finite(Xn[(size_t)f * 8 + k])) bad = 1;
                const double df = align_displacement(a.kind, Xc + (size_t)f * 8, Xn + (size_t)f * 8, g);
                if (!(df <= d)) d = df;
            }
        }
    }
    if (tid == 0) { s_bad = 0; s_stop = 0; s_copy = 0; }
    s_c[tid] = c; s_n[tid] = n; s_d[tid] = d;
    __syncthreads();
    if (bad) s_bad = 1;
    for (int s = kBundleBlock / 2; s > 0; s >>= 1) {
        if (tid < s) { s_c[tid] += s_c[tid + s]; s_n[tid] += s_n[tid + s]; if (!(s_d[tid + s] <= s_d[tid])) s_d[tid] = s_d[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {                                                    // one lane decides
        const double C = s_c[0];
        const int nval = (int)s_n[0];
        int status = -1;
        if (round == 0) {
            st->cost = C; st->n_cur = nval; st->n_first = nval; st->rms_first = sqrt(C / (double)nval);
            if (a.n_iter == 0) status = 1;
        } else {
            st->rounds = round;
            if (sing) status = 3;
            else {
                const bool accept = s_bad == 0 && nval >= st->n_cur && C < st->cost;
                if (accept) {
                    st->cur = cur ^ 1; st->cost = C; st->n_cur = nval; st->accepted += 1; st->fresh = 1;
                    const double l = st->lambda / 10.0;
                    st->lambda = l > 1e-12 ? l : 1e-12;
                    if (s_d[0] < a.eps) status = 0;
                } else {
                    st->fresh = 0;
                    st->lambda = st->lambda * 10.0;
                    if (st->lambda > 1e12) status = 2;
                }
                if (status < 0 && round == a.n_iter) status = 1;
            }
        }
        if (status >= 0) {
            BundleInfo o;
            o.status = status; o.rounds = st->rounds; o.accepted = st->accepted; o.n_valid_first = st->n_first; o.n_valid_last = st->n_cur; o.pad = 0;
            o.rms_first = st->rms_first; o.rms_last = sqrt(st->cost / (double)st->n_cur); o.lambda_last = st->lambda;
            *reinterpret_cast<BundleInfo *>(a.info) = o;
            st->done = 1;
            s_stop = 1; s_copy = st->accepted == 0 ? 1 : 0;
        }
        s_cur = st->cur;
    }
    __syncthreads();
    int32_t *finfo = reinterpret_cast<int32_t *>(a.info + sizeof(BundleInfo));
    BundlePairInfo *pinfo = reinterpret_cast<BundlePairInfo *>(a.info + sizeof(BundleInfo) + (((size_t)F * 4 + 7) & ~(size_t)7));
    if (round == 0) {
        for (int p = tid; p < a.n_pairs; p += kBundleBlock) {
            const double pc = R[(size_t)p * kBundleRec + ne - 1], pn = R[(size_t)p * kBundleRec + ne];
            BundlePairInfo o;
            o.n_valid_first = (int)pn; o.n_valid_last = (int)pn; o.rms_first = sqrt(pc / pn); o.rms_last = o.rms_first;
            pinfo[p] = o;
        }
    }
    if (!s_stop) return true;
    if (round > 0) {
        const double *__restrict__ Rc = a.recs + (size_t)s_cur * a.n_pairs * kBundleRec;
        for (int p = tid; p < a.n_pairs; p += kBundleBlock) {
            const double pc = Rc[(size_t)p * kBundleRec + ne - 1], pn = Rc[(size_t)p * kBundleRec + ne];
            pinfo[p].n_valid_last = (int)pn; pinfo[p].rms_last = sqrt(pc / pn);
        }
    }
    const double *Xc = a.iter + (size_t)s_cur * F * 8;
    for (int f = tid; f < F; f += kBundleBlock) {
        const int cls = a.cls[f], good = a.good[f];
        double m[8];
        const double *in = a.mats_in + (size_t)f * 8;
        if (s_copy || cls != 0 || !good) { for (int k = 0; k < 8; k++) m[k] = in[k]; }
        else align_denormalise(a.kind, Xc + (size_t)f * 8, g, m);
        for (int k = 0; k < 8; k++) a.mats_out[(size_t)f * 8 + k] = m[k];
        finfo[f] = cls != 0 ? cls : (good ? 0 : 3);
    }
    return false;
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_decide(BundleArgs a, int round) { (void)bundle_decide(a, round); }

// ------------------------------------------------------------------------------------------------ k_bundle_assemble
// The records that touch free frame fi, in ascending pair index, added into its P rows of H (row stride N, zeroed by the caller) and its part of g.
__device__ inline void bundle_assemble_frame(const BundleArgs &a, int fi, const double *__restrict__ R, double *Hm, double *gm, int tid)
{
    const int np = bundle_p(a.kind), nv = 2 * np + 1, N = a.N;
    double *Hr = Hm + (size_t)fi * np * N;
    double *gr = gm + (size_t)fi * np;
    const int r = tid / np, c = tid - r * np;
    for (int e = a.rowptr[fi]; e < a.rowptr[fi + 1]; e++) {
        const int pair = a.ent[e] >> 1, side = a.ent[e] & 1;
        const double *rec = R + (size_t)pair * kBundleRec;
        const int other = a.pairs4[4 * pair + (side ? 0 : 1)];
        if (tid < np * np) {
            const int lo = r < c ? r : c, hi = r < c ? c : r;
            Hr[(size_t)r * N + fi * np + c] += rec[bundle_tri(nv, side * np + lo, side * np + hi)];
            if (a.cls[other] == 0) {
                const int oj = a.fidx[other];
                Hr[(size_t)r * N + oj * np + c] += side == 0 ? rec[bundle_tri(nv, r, np + c)] : rec[bundle_tri(nv, c, np + r)];
            }
        }
        if (tid < np) gr[tid] -= rec[bundle_tri(nv, side * np + tid, 2 * np)];
    }
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_assemble(BundleArgs a)
{
    const BundleState *st = a.state;
    if (st->done != 0 || st->fresh == 0) return;                       // (a rejected round: H and the gradient stand)
    const int np = bundle_p(a.kind), N = a.N;
    const int fi = blockIdx.x, tid = threadIdx.x;
    double *Hr = a.Hm + (size_t)fi * np * N;
    for (int k = tid; k < np * N; k += kBundleBlock) Hr[k] = 0.0;
    if (tid < np) a.Hm[(size_t)N * N + (size_t)fi * np + tid] = 0.0;
    __syncthreads();
    bundle_assemble_frame(a, fi, a.recs + (size_t)st->cur * a.n_pairs * kBundleRec, a.Hm, a.Hm + (size_t)N * N, tid);
}

// ------------------------------------------------------------------------------------------------ the factorisation
// Cholesky of the leading cols x cols block of A (row stride ld) in place, the rows below it (up to `rows`) solved along: right-looking, column
// by column, every entry a_ic -= a_ij a_cj one j at a time.  All lanes of the workgroup call it; false (for all of them) at a pivot that is not
// positive and finite.
__device__ inline bool bundle_chol(double *A, int rows, int cols, int ld, int tid, int nt)
{
    for (int j = 0; j < cols; j++) {
        const double d = A[j * ld + j];
        if (!(d > 0.0) || !(d < INFINITY)) return false;
        const double l = sqrt(d);
        __syncthreads();
        for (int i = j + tid; i < rows; i += nt) A[i * ld + j] = i == j ? l : A[i * ld + j] / l;
        __syncthreads();
        for (int i = j + 1 + (tid >> 5); i < rows; i += nt >> 5)      // (a wave row of 32 columns per step: neighbouring lanes, neighbouring words)
            for (int c = j + 1 + (tid & 31); c < cols && c <= i; c += 32) A[i * ld + c] -= A[i * ld + j] * A[c * ld + j];
        __syncthreads();
    }
    return true;
}

// L^T x = y in place in y (LDS), L lower triangular with row stride ld: x_k = y_k / l_kk, then y_i -= l_ki x_k for i < k, k descending.  Row
// k - 1 is fetched while row k is used.  E = elements of a row per lane.
template <int E>
__device__ inline void bundle_back(const double *__restrict__ L, size_t ld, int n, double *y, int tid, int nt)
{
    double nd = 0.0, nx[E];
    if (n > 0) {
        nd = L[(size_t)(n - 1) * ld + (n - 1)];
#pragma unroll
        for (int e = 0; e < E; e++) { const int i = tid + e * nt; nx[e] = i < n - 1 ? L[(size_t)(n - 1) * ld + i] : 0.0; }
    }
    for (int k = n - 1; k >= 0; k--) {
        const double cd = nd;
        double cx[E];
#pragma unroll
        for (int e = 0; e < E; e++) cx[e] = nx[e];
        if (k > 0) {
            nd = L[(size_t)(k - 1) * ld + (k - 1)];
#pragma unroll
            for (int e = 0; e < E; e++) { const int i = tid + e * nt; nx[e] = i < k - 1 ? L[(size_t)(k - 1) * ld + i] : 0.0; }
        }
        const double xk = y[k] / cd;
        __syncthreads();
        if (tid == 0) y[k] = xk;
#pragma unroll
        for (int e = 0; e < E; e++) { const int i = tid + e * nt; if (i < k) y[i] -= cx[e] * xk; }
        __syncthreads();
    }
}

// The candidate: the current iterate plus delta on the parameters of the free frames.
__device__ inline void bundle_candidate(const BundleArgs &a, int cur, const double *delta, int tid, int nt)
{
    const int np = bundle_p(a.kind), F = a.n_frames;
    const double *Xc = a.iter + (size_t)cur * F * 8;
    double *Xn = a.iter + (size_t)(cur ^ 1) * F * 8;
    for (int idx = tid; idx < F * 8; idx += nt) {
        const int f = idx >> 3, k = bundle_param(a.kind, idx & 7);
        double v = Xc[idx];
        if (a.cls[f] == 0 && k >= 0) v += delta[a.fidx[f] * np + k];
        Xn[idx] = v;
    }
}

// The small path's round in ONE workgroup: the reduction of the pass before it, the decision, and -- unless the call stopped -- assembly,
// damping, factorisation, substitution and the candidate of the next round, H and g in LDS throughout.
__global__ __launch_bounds__(kBundleBlock) void k_bundle_round_small(BundleArgs a, int round)
{
#ifdef __HIPCC__
    extern __shared__ double s_A[];                                    // (N + 1) x N, sized by the launch
#else
    double *s_A = g_bundle_host_lds;                                   // (a host check supplies the block: tests/cpp/bundle_check.cpp)
#endif
    BundleState *st = a.state;
    if (round > 0 && st->done != 0) return;                            // (uniform)
    const int tid = threadIdx.x, N = a.N;
    if (round == 0 || st->sing == 0) {
        const int buf = round == 0 ? 0 : (st->cur ^ 1);
        for (int pair = 0; pair < a.n_pairs; pair++) bundle_reduce_pair(a, pair, round, buf, tid);
    }
    __syncthreads();
    if (!bundle_decide(a, round)) return;
    __syncthreads();
    const double lambda = st->lambda;
    const int cur = st->cur;
    for (int idx = tid; idx < (N + 1) * N; idx += kBundleBlock) s_A[idx] = 0.0;
    __syncthreads();
    const double *__restrict__ R = a.recs + (size_t)cur * a.n_pairs * kBundleRec;
    for (int fi = 0; fi < a.n_free; fi++) bundle_assemble_frame(a, fi, R, s_A, s_A + (size_t)N * N, tid);
    __syncthreads();
    for (int i = tid; i < N; i += kBundleBlock) s_A[i * N + i] = s_A[i * N + i] + lambda;
    __syncthreads();
    if (!bundle_chol(s_A, N + 1, N, N, tid, kBundleBlock)) { if (tid == 0) st->sing = 1; return; }
    bundle_back<1>(s_A, (size_t)N, N, s_A + (size_t)N * N, tid, kBundleBlock);
    bundle_candidate(a, cur, s_A + (size_t)N * N, tid, kBundleBlock);
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_damp(BundleArgs a)
{
    const BundleState *st = a.state;
    if (st->done != 0) return;
    const size_t N = (size_t)a.N, total = (N + 1) * N;
    const double lambda = st->lambda;
    for (size_t idx = (size_t)blockIdx.x * kBundleBlock + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kBundleBlock) {
        const size_t i = idx / N, j = idx - i * N;
        a.Wm[idx] = i == j ? a.Hm[idx] + lambda : a.Hm[idx];
    }
}

__global__ __launch_bounds__(kBundleBlock) void k_bundle_chol_diag(BundleArgs a, int k0, int nb)
{
    __shared__ double s_D[kBundlePanel * kBundlePanel];
    BundleState *st = a.state;
    if (st->done != 0 || st->sing != 0) return;
    const int tid = threadIdx.x;
    const size_t N = (size_t)a.N;
    for (int idx = tid; idx < nb * nb; idx += kBundleBlock) { const int i = idx / nb, j = idx - i * nb; s_D[i * kBundlePanel + j] = a.Wm[(size_t)(k0 + i) * N + k0 + j]; }
    __syncthreads();
    if (!bundle_chol(s_D, nb, nb, kBundlePanel, tid, kBundleBlock)) { if (tid == 0) st->sing = 1; return; }
    for (int idx = tid; idx < nb * nb; idx += kBundleBlock) { const int i = idx / nb, j = idx - i * nb; if (j <= i) a.Wm[(size_t)(k0 + i) * N + k0 + j] = s_D[i * kBundlePanel + j]; }
}

// The rows below the diagonal block (the gradient's row N among them), one lane per row: x_c = (a_ic - x_0 l_c0 - .. - x_(c-1) l_c(c-1)) / l_cc.
__global__ __launch_bounds__(64) void k_bundle_chol_panel(BundleArgs a, int k0, int nb)
{
    __shared__ double s_D[kBundlePanel * kBundlePanel];
    const BundleState *st = a.state;
    if (st->done != 0 || st->sing != 0) return;
    const int tid = threadIdx.x;
    const size_t N = (size_t)a.N;
    for (int idx = tid; idx < nb * nb; idx += 64) { const int i = idx / nb, j = idx - i * nb; s_D[i * kBundlePanel + j] = a.Wm[(size_t)(k0 + i) * N + k0 + j]; }
    __syncthreads();
    const int i = k0 + nb + blockIdx.x * 64 + tid;
    if (i > a.N) return;
    double *__restrict__ row = a.Wm + (size_t)i * N + k0;
    double x[kBundlePanel];
#pragma unroll
    for (int c = 0; c < kBundlePanel; c++) x[c] = c < nb ? row[c] : 0.0;
#pragma unroll
    for (int c = 0; c < kBundlePanel; c++) {
        if (c < nb) {
            double v = x[c];
#pragma unroll
            for (int k = 0; k < c; k++) v -= x[k] * s_D[c * kBundlePanel + k];
            x[c] = v / s_D[c * kBundlePanel + c];
        }
    }
#pragma unroll
    for (int c = 0; c < kBundlePanel; c++) if (c < nb) row[c] = x[c];
}

// The trailing matrix, a 32 x 32 tile per workgroup (lower tiles only): a_ij -= l_ik l_jk for the panel's k in ascending order.
__global__ __launch_bounds__(kBundleBlock) void k_bundle_chol_trail(BundleArgs a, int k0, int nb)
{
    constexpr int T = kBundlePanel, LD = kBundlePanel + 1;
    __shared__ double s_I[T * LD], s_J[T * LD];
    const BundleState *st = a.state;
    if (st->done != 0 || st->sing != 0) return;
    if (blockIdx.x > blockIdx.y) return;                               // (x: the tile's column, y: its row)
    const int tid = threadIdx.x, N = a.N;
    const int r0 = k0 + nb, i0 = r0 + blockIdx.y * T, j0 = r0 + blockIdx.x * T;
    for (int idx = tid; idx < T * nb; idx += kBundleBlock) {
        const int r = idx / nb, k = idx - r * nb;
        s_I[r * LD + k] = i0 + r <= N ? a.Wm[(size_t)(i0 + r) * N + k0 + k] : 0.0;
        s_J[r * LD + k] = j0 + r < N ? a.Wm[(size_t)(j0 + r) * N + k0 + k] : 0.0;
    }
    __syncthreads();
    const int tx = tid & (T - 1), ty = tid / T;
    const int j = j0 + tx;
    if (j >= N) return;
#pragma unroll
    for (int m = 0; m < T / 8; m++) {
        const int i = i0 + ty + 8 * m;
        if (i > N || j > i) continue;
        double v = a.Wm[(size_t)i * N + j];
        for (int k = 0; k < nb; k++) v -= s_I[(ty + 8 * m) * LD + k] * s_J[tx * LD + k];
        a.Wm[(size_t)i * N + j] = v;
    }
}

__global__ __launch_bounds__(kBundleBackBlock) void k_bundle_back_large(BundleArgs a)
{
    __shared__ double s_y[kBundleMaxUnknowns];
    const BundleState *st = a.state;
    if (st->done != 0 || st->sing != 0) return;
    const int tid = threadIdx.x, N = a.N;
    const int cur = st->cur;
    for (int i = tid; i < N; i += kBundleBackBlock) s_y[i] = a.Wm[(size_t)N * N + i];
    __syncthreads();
    bundle_back<kBundleMaxUnknowns / kBundleBackBlock>(a.Wm, (size_t)N, N, s_y, tid, kBundleBackBlock);
    bundle_candidate(a, cur, s_y, tid, kBundleBackBlock);
}

// ------------------------------------------------------------------------------------------------ launches
#ifdef __HIPCC__
template <int KIND>
static hipError_t bundle_rounds(const BundleArgs &a, hipStream_t stream)
{
    const int N = a.N;
    const bool small = N <= kBundleLdsCap;
    const size_t small_lds = (size_t)(N + 1) * (size_t)N * 8;
    if (small && small_lds > 32768) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_bundle_round_small), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (kBundleLdsCap + 1) * kBundleLdsCap * 8);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_bundle_init, dim3(1), dim3(kBundleBlock), 0, stream, a);
    for (int round = 0; round <= a.n_iter; round++) {
        if (round > 0 && !small) {
            hipLaunchKernelGGL(k_bundle_assemble, dim3(a.n_free), dim3(kBundleBlock), 0, stream, a);
            hipLaunchKernelGGL(k_bundle_damp, dim3(1024), dim3(kBundleBlock), 0, stream, a);
            for (int k0 = 0; k0 < N; k0 += kBundlePanel) {
                const int nb = N - k0 < kBundlePanel ? N - k0 : kBundlePanel;
                const int below = N + 1 - (k0 + nb);                   // rows under the diagonal block, the gradient's included (>= 1)
                hipLaunchKernelGGL(k_bundle_chol_diag, dim3(1), dim3(kBundleBlock), 0, stream, a, k0, nb);
                hipLaunchKernelGGL(k_bundle_chol_panel, dim3((below + 63) / 64), dim3(64), 0, stream, a, k0, nb);
                if (k0 + nb < N) {
                    const int nt = (below + kBundlePanel - 1) / kBundlePanel;
                    hipLaunchKernelGGL(k_bundle_chol_trail, dim3(nt, nt), dim3(kBundleBlock), 0, stream, a, k0, nb);
                }
            }
            hipLaunchKernelGGL(k_bundle_back_large, dim3(1), dim3(kBundleBackBlock), 0, stream, a);
        }
        if (a.n_work > 0) hipLaunchKernelGGL((k_bundle_pass<KIND>), dim3(a.n_work), dim3(kBundleBlock), 0, stream, a, round);
        if (small) {                                                   // one launch per round beside the pass
            hipLaunchKernelGGL(k_bundle_round_small, dim3(1), dim3(kBundleBlock), small_lds, stream, a, round);
        } else {
            if (a.n_pairs > 0) hipLaunchKernelGGL(k_bundle_reduce, dim3(a.n_pairs), dim3(kBundleBlock), 0, stream, a, round);
            hipLaunchKernelGGL(k_bundle_decide, dim3(1), dim3(kBundleBlock), 0, stream, a, round);
        }
    }
    return hipGetLastError();
}

hipError_t launch_bundle(const BundleArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0) return hipSuccess;
    return a.kind == 1 ? bundle_rounds<1>(a, stream) : bundle_rounds<0>(a, stream);
}
#endif

} // namespace hg
