// hg_k_fit.hip -- fitting frame transforms to point matches by RANSAC (include/hgwarp.h, "fitting transforms to matches"):
//   k_fit_hypotheses  one lane per (frame, hypothesis): the sample (drawn or read), the minimal solve in registers, 8 doubles + a flag
//   k_fit_score       one workgroup per (frame, 256 hypotheses): every lane reprojects the frame's matches with ITS matrix; the matches go
//                     through LDS in tiles of kFitTile and every lane reads the same slot in a step (a broadcast); the count stays in a
//                     register; the best of the frame is a 64-bit atomicMax of (count << 32) | (0xffffffff - h): a total order
//   k_fit_finish      one workgroup per frame: the mask of the best hypothesis, then the normalised least-squares refit over its inliers
//                     with sums in a fixed order (lane-strided partial sums, a fixed tree over the workgroup: no floating-point atomics)
// The rules themselves live in hg_fit_dev.h.  The kernels need that header only, so a host check compiles this file behind a thread-index
// shim (tests/cpp/fit_check.cpp); the launcher is compiled under hipcc only.
#ifdef __HIPCC__
#include "hg_kernels.h"
#endif
#include "hg_fit_dev.h"

namespace hg {

// ------------------------------------------------------------------------------------------------ k_fit_hypotheses
// The LU keeps 64 doubles in registers: a kernel of its own with a small block, as k_solve_frames (hg_k_geo.hip).
__global__ __launch_bounds__(64) void k_fit_hypotheses(int kind, const float4 *__restrict__ matches, int n_points, const int32_t *__restrict__ counts,
                                                       int n_hyp, uint32_t seed, const int32_t *__restrict__ samples,
                                                       double *__restrict__ mats, int32_t *__restrict__ valid)
{
    const int h = blockIdx.x * 64 + threadIdx.x, f = blockIdx.y;
    if (h >= n_hyp) return;
    const int K = fit_k(kind);
    const int32_t count = counts[f];
    const size_t slot = (size_t)f * n_hyp + h;
    int32_t idx[4];
    bool ok;
    if (samples) {
#pragma unroll
        for (int k = 0; k < 4; k++) idx[k] = samples[slot * 4 + k];
        ok = fit_sample_ok(K, idx, count);
    } else {
        ok = fit_draw(K, seed, (uint32_t)f, (uint32_t)h, count, idx);
    }
    double m[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (ok) {
        float s[8], d[8];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const float4 q = (p < K) ? matches[(size_t)f * n_points + idx[p]] : make_float4(0.f, 0.f, 0.f, 0.f);      // (idx[p] < count <= n_points)
            s[2 * p] = q.x; s[2 * p + 1] = q.y; d[2 * p] = q.z; d[2 * p + 1] = q.w;
        }
        ok = fit_minimal(kind, s, d, m);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) mats[slot * 8 + k] = m[k];
    valid[slot] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ k_fit_score
template <int KIND>
__global__ __launch_bounds__(kFitHypBlock) void k_fit_score(const float4 *__restrict__ matches, int n_points, const int32_t *__restrict__ counts, int n_hyp,
                                                            double thr2, const double *__restrict__ mats, const int32_t *__restrict__ valid,
                                                            unsigned long long *__restrict__ best)
{
    __shared__ float4 tile[kFitTile];
    const int h = blockIdx.x * kFitHypBlock + threadIdx.x, f = blockIdx.y;
    const int32_t count = counts[f];
    const bool live = h < n_hyp;
    const size_t slot = (size_t)f * n_hyp + (live ? h : 0);
    double m[8];
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = mats[slot * 8 + k];
    const bool ok = live && valid[slot] != 0;
    const float4 *__restrict__ mf = matches + (size_t)f * n_points;
    uint32_t cnt = 0;
    for (int base = 0; base < count; base += kFitTile) {
        const int n = min(kFitTile, count - base);
        if ((int)threadIdx.x < n) {
            float4 q = mf[base + threadIdx.x];
            if (!fit_match_finite(q.x, q.y, q.z, q.w)) q.x = NAN;
            tile[threadIdx.x] = q;
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < n; j++) {
            const float4 q = tile[j];
            cnt += fit_inlier<KIND>(m, q.x, q.y, q.z, q.w, thr2) ? 1u : 0u;
        }
        __syncthreads();
    }
    if (ok) atomicMax(&best[f], ((unsigned long long)cnt << 32) | (unsigned long long)(0xffffffffu - (uint32_t)h));
}

// ------------------------------------------------------------------------------------------------ k_fit_finish
constexpr int kFitFinishBlock = 256;

// The sum of v over the workgroup in a fixed order, returned to every lane.
__device__ __forceinline__ double fit_block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = kFitFinishBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// Gaussian elimination with partial pivoting (first row with the largest magnitude) on the n x (n + r) augmented system A (row stride ld),
// in one lane; the solutions replace the right-hand sides.  A zero pivot leaves values that are not finite: the caller's fallback.
__device__ void fit_gauss(double *A, int n, int r, int ld)
{
    for (int k = 0; k < n; k++) {
        int pk = k;
        double bestv = fabs(A[k * ld + k]);
        for (int j = k + 1; j < n; j++) { const double v = fabs(A[j * ld + k]); if (bestv < v) { bestv = v; pk = j; } }
        if (pk != k) for (int j = 0; j < n + r; j++) { const double t = A[k * ld + j]; A[k * ld + j] = A[pk * ld + j]; A[pk * ld + j] = t; }
        const double akk = A[k * ld + k];
        for (int i = k + 1; i < n; i++) {
            const double l = A[i * ld + k] / akk;
            for (int j = k + 1; j < n + r; j++) A[i * ld + j] -= l * A[k * ld + j];
        }
    }
    for (int c = 0; c < r; c++) {
        for (int i = n - 1; i >= 0; i--) {
            double x = A[i * ld + n + c];
            for (int j = i + 1; j < n; j++) x -= A[i * ld + j] * A[j * ld + n + c];
            A[i * ld + n + c] = x / A[i * ld + i];
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(kFitFinishBlock) void k_fit_finish(const float4 *__restrict__ matches, int n_points, const int32_t *__restrict__ counts, int n_hyp,
                                                                double thr2, int refit, const double *__restrict__ hyp_mats,
                                                                const unsigned long long *__restrict__ best, double *__restrict__ out_mats,
                                                                double *__restrict__ out_min, int32_t *__restrict__ out_counts, int32_t *__restrict__ out_best,
                                                                uint8_t *__restrict__ out_mask)
{
    __shared__ double sh[kFitFinishBlock];
    __shared__ double A[8 * 9];
    __shared__ double res[8];
    constexpr int K = KIND == 1 ? 4 : 3;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int32_t count = counts[f];
    const bool all = n_hyp == 0;                                 // least squares without sampling: every finite match is an inlier
    const unsigned long long key = all ? 0ull : best[f];
    const bool have = key != 0ull;                               // a valid hypothesis exists
    const int32_t bh = have ? (int32_t)(0xffffffffu - (uint32_t)key) : -1;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double m[8];
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = have ? hyp_mats[((size_t)f * n_hyp + bh) * 8 + k] : qnan;
    const float4 *__restrict__ mf = matches + (size_t)f * n_points;

    auto inlier = [&](int i, float4 &q) -> bool {
        if (i >= count) return false;
        q = mf[i];
        if (!fit_match_finite(q.x, q.y, q.z, q.w)) return false;
        return all ? true : (have && fit_inlier<KIND>(m, q.x, q.y, q.z, q.w, thr2));
    };

    // the mask, and the inliers counted (integers: any order)
    double nin = 0.0, sx = 0.0, sy = 0.0, su = 0.0, sv = 0.0;
    for (int i = tid; i < n_points; i += kFitFinishBlock) {
        float4 q;
        const bool in = inlier(i, q);
        if (out_mask) out_mask[(size_t)f * n_points + i] = in ? 1 : 0;
        if (in) { nin += 1.0; sx += (double)q.x; sy += (double)q.y; su += (double)q.z; sv += (double)q.w; }
    }
    const double n = fit_block_sum(nin, sh);
    const int32_t n_in = all ? (int32_t)n : (have ? (int32_t)(key >> 32) : 0);
    if (tid == 0) {
        out_counts[f] = n_in;
        if (out_best) out_best[f] = bh;
        if (out_min) {
#pragma unroll
            for (int k = 0; k < 8; k++) out_min[(size_t)f * 8 + k] = m[k];
        }
    }
    const bool do_refit = refit != 0 && (all ? n_in >= K : (have && n_in > K));      // uniform over the workgroup
    if (!do_refit) {
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) out_mats[(size_t)f * 8 + k] = m[k];          // (all: NaNs, fewer than K matches remain)
        }
        return;
    }
    // normalisation: centroids to the origin, mean distance sqrt(2)
    const double cx = fit_block_sum(sx, sh) / n, cy = fit_block_sum(sy, sh) / n, cu = fit_block_sum(su, sh) / n, cv = fit_block_sum(sv, sh) / n;
    double dfs = 0.0, dts = 0.0;
    for (int i = tid; i < n_points; i += kFitFinishBlock) {
        float4 q;
        if (!inlier(i, q)) continue;
        const double ax = (double)q.x - cx, ay = (double)q.y - cy, au = (double)q.z - cu, av = (double)q.w - cv;
        dfs += sqrt((ax * ax) + (ay * ay));
        dts += sqrt((au * au) + (av * av));
    }
    const double sf = sqrt(2.0) / (fit_block_sum(dfs, sh) / n), st = sqrt(2.0) / (fit_block_sum(dts, sh) / n);
    // the normal equations' distinct sums: S[.] over [x y 1]^T [x y 1], then the same weighted by u, by v and by w = u u + v v
    double s1[5] = { 0, 0, 0, 0, 0 }, s_u[6] = { 0, 0, 0, 0, 0, 0 }, s_v[6] = { 0, 0, 0, 0, 0, 0 }, s_w[5] = { 0, 0, 0, 0, 0 };
    for (int i = tid; i < n_points; i += kFitFinishBlock) {
        float4 q;
        if (!inlier(i, q)) continue;
        const double x = ((double)q.x - cx) * sf, y = ((double)q.y - cy) * sf, u = ((double)q.z - cu) * st, v = ((double)q.w - cv) * st;
        const double xx = x * x, xy = x * y, yy = y * y;
        s1[0] += xx; s1[1] += xy; s1[2] += yy; s1[3] += x; s1[4] += y;
        s_u[0] += u * xx; s_u[1] += u * xy; s_u[2] += u * yy; s_u[3] += u * x; s_u[4] += u * y; s_u[5] += u;
        s_v[0] += v * xx; s_v[1] += v * xy; s_v[2] += v * yy; s_v[3] += v * x; s_v[4] += v * y; s_v[5] += v;
        if (KIND == 1) {
            const double w = (u * u) + (v * v);
            s_w[0] += w * xx; s_w[1] += w * xy; s_w[2] += w * yy; s_w[3] += w * x; s_w[4] += w * y;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; k++) s1[k] = fit_block_sum(s1[k], sh);
#pragma unroll
    for (int k = 0; k < 6; k++) { s_u[k] = fit_block_sum(s_u[k], sh); s_v[k] = fit_block_sum(s_v[k], sh); }
    if (KIND == 1) {
#pragma unroll
        for (int k = 0; k < 5; k++) s_w[k] = fit_block_sum(s_w[k], sh);
    }
    if (tid == 0) {
        double g[9];                                             // the normalised transform, row-major 3 x 3
        const double S[3][3] = { { s1[0], s1[1], s1[3] }, { s1[1], s1[2], s1[4] }, { s1[3], s1[4], n } };
        if (KIND == 1) {
            constexpr int ld = 9;
            for (int k = 0; k < 8 * 9; k++) A[k] = 0.0;
            const double U[3][2] = { { s_u[0], s_u[1] }, { s_u[1], s_u[2] }, { s_u[3], s_u[4] } };      // sum u [x y 1]^T [x y]
            const double V[3][2] = { { s_v[0], s_v[1] }, { s_v[1], s_v[2] }, { s_v[3], s_v[4] } };
            const double Wm[2][2] = { { s_w[0], s_w[1] }, { s_w[1], s_w[2] } };
            for (int a = 0; a < 3; a++) {
                for (int b = 0; b < 3; b++) { A[a * ld + b] = S[a][b]; A[(3 + a) * ld + 3 + b] = S[a][b]; }
                for (int b = 0; b < 2; b++) {
                    A[a * ld + 6 + b] = -U[a][b]; A[(6 + b) * ld + a] = -U[a][b];
                    A[(3 + a) * ld + 6 + b] = -V[a][b]; A[(6 + b) * ld + 3 + a] = -V[a][b];
                }
            }
            for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) A[(6 + a) * ld + 6 + b] = Wm[a][b];
            A[0 * ld + 8] = s_u[3]; A[1 * ld + 8] = s_u[4]; A[2 * ld + 8] = s_u[5];
            A[3 * ld + 8] = s_v[3]; A[4 * ld + 8] = s_v[4]; A[5 * ld + 8] = s_v[5];
            A[6 * ld + 8] = -s_w[3]; A[7 * ld + 8] = -s_w[4];
            fit_gauss(A, 8, 1, ld);
            for (int k = 0; k < 8; k++) g[k] = A[k * ld + 8];
            g[8] = 1.0;
        } else {
            constexpr int ld = 5;
            for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) A[a * ld + b] = S[a][b];
            A[0 * ld + 3] = s_u[3]; A[1 * ld + 3] = s_u[4]; A[2 * ld + 3] = s_u[5];
            A[0 * ld + 4] = s_v[3]; A[1 * ld + 4] = s_v[4]; A[2 * ld + 4] = s_v[5];
            fit_gauss(A, 3, 2, ld);
            g[0] = A[0 * ld + 3]; g[1] = A[1 * ld + 3]; g[2] = A[2 * ld + 3];
            g[3] = A[0 * ld + 4]; g[4] = A[1 * ld + 4]; g[5] = A[2 * ld + 4];
            g[6] = 0.0; g[7] = 0.0; g[8] = 1.0;
        }
        // T_to^-1 G T_from, with T = [s 0 -s c; 0 s -s c'; 0 0 1] and T^-1 = [1/s 0 c; 0 1/s c'; 0 0 1]
        double gt[9], hm[9];
        for (int r = 0; r < 3; r++) {
            gt[3 * r + 0] = g[3 * r + 0] * sf;
            gt[3 * r + 1] = g[3 * r + 1] * sf;
            gt[3 * r + 2] = (g[3 * r + 2] - (g[3 * r + 0] * (sf * cx))) - (g[3 * r + 1] * (sf * cy));
        }
        for (int c = 0; c < 3; c++) {
            hm[0 + c] = (gt[0 + c] / st) + (cu * gt[6 + c]);
            hm[3 + c] = (gt[3 + c] / st) + (cv * gt[6 + c]);
            hm[6 + c] = gt[6 + c];
        }
        double o[8];
        if (KIND == 1) {
            for (int k = 0; k < 8; k++) o[k] = hm[k] / hm[8];
        } else {                                                 // apply_affine's layout: px = o0 x + o2 y + o4, py = o1 x + o3 y + o5
            o[0] = hm[0]; o[2] = hm[1]; o[4] = hm[2]; o[1] = hm[3]; o[3] = hm[4]; o[5] = hm[5]; o[6] = 0.0; o[7] = 0.0;
        }
        bool fin = true;
        for (int k = 0; k < 8; k++) fin = fin && fit_finite(o[k]);
        for (int k = 0; k < 8; k++) res[k] = fin ? o[k] : m[k];  // (all: m is NaNs)
        for (int k = 0; k < 8; k++) out_mats[(size_t)f * 8 + k] = res[k];
    }
}

// ------------------------------------------------------------------------------------------------ launches
#ifdef __HIPCC__
void launch_fit(const FitArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0) return;
    const float4 *mt = reinterpret_cast<const float4 *>(a.matches);
    const double thr2 = a.threshold * a.threshold;
    if (a.n_hyp > 0) {
        hipLaunchKernelGGL(k_fit_hypotheses, dim3((a.n_hyp + 63) / 64, a.n_frames), dim3(64), 0, stream, a.kind, mt, a.n_points, a.counts, a.n_hyp, a.seed,
                           a.samples, a.hyp_mats, a.hyp_valid);
        const dim3 grid((a.n_hyp + kFitHypBlock - 1) / kFitHypBlock, a.n_frames);
        if (a.kind == 1) hipLaunchKernelGGL(k_fit_score<1>, grid, dim3(kFitHypBlock), 0, stream, mt, a.n_points, a.counts, a.n_hyp, thr2, a.hyp_mats, a.hyp_valid, a.best);
        else hipLaunchKernelGGL(k_fit_score<0>, grid, dim3(kFitHypBlock), 0, stream, mt, a.n_points, a.counts, a.n_hyp, thr2, a.hyp_mats, a.hyp_valid, a.best);
    }
    if (a.kind == 1)
        hipLaunchKernelGGL(k_fit_finish<1>, dim3(a.n_frames), dim3(kFitFinishBlock), 0, stream, mt, a.n_points, a.counts, a.n_hyp, thr2, a.refit, a.hyp_mats, a.best,
                           a.out_mats, a.out_min, a.out_counts, a.out_best, a.out_mask);
    else
        hipLaunchKernelGGL(k_fit_finish<0>, dim3(a.n_frames), dim3(kFitFinishBlock), 0, stream, mt, a.n_points, a.counts, a.n_hyp, thr2, a.refit, a.hyp_mats, a.best,
                           a.out_mats, a.out_min, a.out_counts, a.out_best, a.out_mask);
}
#endif

} // namespace hg
