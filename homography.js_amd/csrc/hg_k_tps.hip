// hg_k_tps.hip -- thin-plate splines through the landmark pairs of a frame set (include/hgwarp.h, "thin-plate splines").
//   k_tps_solve   one workgroup per frame: normalisation, the (N + 3) x (N + 3) system, Gaussian elimination with partial pivoting, the
//                 record.  The matrix lives in LDS while it fits kTpsLdsCap doubles (256 lanes), else in the caller's scratch (1024 lanes).
//                 Every entry is updated by one fixed expression per step whichever lane does it, and the pivot is a total order
//                 (largest magnitude, lowest row): two runs give the same bits.
//   k_tps_field   the source field of the spline: one wave per row of the window (4 rows per workgroup) walking 256-pixel pieces, a lane
//                 owns pixels c0 + lane + 64 k, so it carries four independent log chains and every store of the wave covers 64
//                 consecutive pixels.  NODES: the same walk over the lattice of a stepped field, values as f64 pairs into scratch.
//   k_tps_blend   a stepped field's pixels from their four nodes.
//   k_tps_points  point lists, one position per lane.
// Pixels, nodes and points go through the one tps_eval of hg_tps_dev.h, f64 with contraction off: a pixel on a node and a point on a pixel
// repeat the field's bits.  The record is read at lane-independent addresses (scalar loads).  Field values are stored through field_px
// (hg_field_dev.h), non-temporal.  The kernels need those two headers only, so a host check compiles this file behind a thread-index shim
// (tests/cpp/tps_check.cpp); the launchers are compiled under hipcc only.
#ifdef __HIPCC__
#include "hg_kernels.h"
#endif
#include "hg_tps_dev.h"
#include "hg_field_dev.h"

namespace hg {

constexpr int kTpsLdsM = 72;            // the largest M whose matrix stays in LDS
static_assert(kTpsLdsM * kTpsLdsM == kTpsLdsCap, "kTpsLdsCap is a square");

// ------------------------------------------------------------------------------------------------ k_tps_solve
template <bool LDS>
__global__ __launch_bounds__(LDS ? kTpsSolveBlock : kTpsSolveBlockBig) void k_tps_solve(TpsSolveArgs a)
{
    constexpr int B = LDS ? kTpsSolveBlock : kTpsSolveBlockBig;
    constexpr int MB = LDS ? kTpsLdsM : kTpsMaxM;
    __shared__ double s_a[LDS ? kTpsLdsCap : 1];
    __shared__ double s_b[2 * MB];                           // the two right-hand sides, then the solutions
    __shared__ double s_mag[B];
    __shared__ int s_row[B];
    __shared__ double s_norm[5];
    __shared__ int s_state;

    const int f = blockIdx.x, t = threadIdx.x;
    const int N = a.n_points, M = N + 3;
    const float *__restrict__ from = a.from + (size_t)(f % a.n_from_sets) * N * 2;
    const float *__restrict__ to = a.to + (size_t)(f % a.n_to_sets) * N * 2;
    double *rec = a.records + (size_t)f * tps_record_doubles(N);          // (written and read back across lanes: no __restrict__)
    double *A = LDS ? s_a : a.scratch + (size_t)f * M * M;

    // 1. the inputs: any coordinate that is not finite fails the frame
    if (t == 0) s_state = kTpsOk;
    __syncthreads();
    bool bad = false;
    for (int i = t; i < 2 * N; i += B) bad = bad || !tps_finite((double)from[i]) || !tps_finite((double)to[i]);
    if (bad) s_state = kTpsBadInput;
    __syncthreads();

    // 2. the normalisation, summed by one lane in index order
    if (t == 0 && s_state == kTpsOk) {
        double cx = 0.0, cy = 0.0, tx = 0.0, ty = 0.0;
        for (int i = 0; i < N; i++) { cx += (double)from[2 * i]; cy += (double)from[2 * i + 1]; tx += (double)to[2 * i]; ty += (double)to[2 * i + 1]; }
        cx /= (double)N; cy /= (double)N; tx /= (double)N; ty /= (double)N;
        double md = 0.0;
        for (int i = 0; i < N; i++) { const double ax = (double)from[2 * i] - cx, ay = (double)from[2 * i + 1] - cy; md += sqrt(ax * ax + ay * ay); }
        md /= (double)N;
        if (!(md > 0.0) || !tps_finite(md)) s_state = kTpsSingular;
        s_norm[0] = cx; s_norm[1] = cy; s_norm[2] = sqrt(2.0) / md; s_norm[3] = tx; s_norm[4] = ty;
    }
    __syncthreads();
    bool failed = s_state != kTpsOk;

    if (!failed) {
        const double cx = s_norm[0], cy = s_norm[1], s = s_norm[2], tx = s_norm[3], ty = s_norm[4];
        // 3. d_i into the record (read back below: global writes of the workgroup are visible behind the barrier), b_i into LDS
        for (int i = t; i < N; i += B) {
            rec[kTpsHead + 4 * i] = ((double)from[2 * i] - cx) * s;
            rec[kTpsHead + 4 * i + 1] = ((double)from[2 * i + 1] - cy) * s;
            s_b[i] = (double)to[2 * i] - tx;
            s_b[M + i] = (double)to[2 * i + 1] - ty;
        }
        if (t < 3) { s_b[N + t] = 0.0; s_b[M + N + t] = 0.0; }
        __syncthreads();
        // 4. [[K + lambda I, P], [P^T, 0]]
        for (int e = t; e < M * M; e += B) {
            const int i = e / M, j = e - i * M;
            double v = 0.0;
            if (i < N && j < N) {
                if (i == j) v = a.lambda;
                else {
                    const double ex = rec[kTpsHead + 4 * i] - rec[kTpsHead + 4 * j], ey = rec[kTpsHead + 4 * i + 1] - rec[kTpsHead + 4 * j + 1];
                    v = tps_u(ex * ex + ey * ey);
                }
            } else if (i < N || j < N) {
                const int p = i < N ? i : j, c = (i < N ? j : i) - N;
                v = c == 0 ? 1.0 : rec[kTpsHead + 4 * p + (c - 1)];
            }
            A[e] = v;
        }
        __syncthreads();
        // 5. elimination
        const int tx4 = t & 63, ty4 = t >> 6;
        for (int k = 0; k < M && !failed; k++) {
            double bm = -1.0;
            int br = k;
            for (int i = k + t; i < M; i += B) { const double m = fabs(A[(size_t)i * M + k]); if (m > bm) { bm = m; br = i; } }
            s_mag[t] = bm; s_row[t] = br;
            __syncthreads();
            for (int h = B / 2; h > 0; h >>= 1) {
                if (t < h) {
                    const double m2 = s_mag[t + h];
                    const int r2 = s_row[t + h];
                    if (m2 > s_mag[t] || (m2 == s_mag[t] && r2 < s_row[t])) { s_mag[t] = m2; s_row[t] = r2; }
                }
                __syncthreads();
            }
            const int p = s_row[0];
            const double piv = A[(size_t)p * M + k];
            if (!(fabs(piv) > 0.0) || !tps_finite(piv)) { failed = true; break; }       // (the same value in every lane)
            if (p != k) {
                __syncthreads();                                 // (every lane has read the pivot)
                for (int j = k + t; j < M; j += B) { const double u = A[(size_t)k * M + j]; A[(size_t)k * M + j] = A[(size_t)p * M + j]; A[(size_t)p * M + j] = u; }
                if (t < 2) { const double u = s_b[t * M + k]; s_b[t * M + k] = s_b[t * M + p]; s_b[t * M + p] = u; }
                __syncthreads();
            }
            for (int i = k + 1 + ty4; i < M; i += B / 64) {
                const double fct = A[(size_t)i * M + k] / piv;
                for (int j = k + 1 + tx4; j < M; j += 64) A[(size_t)i * M + j] = A[(size_t)i * M + j] - fct * A[(size_t)k * M + j];
                if (tx4 < 2) s_b[tx4 * M + i] = s_b[tx4 * M + i] - fct * s_b[tx4 * M + k];
            }
            __syncthreads();
        }
        // 6. back substitution, column by column
        for (int k = M - 1; k >= 0 && !failed; k--) {
            if (t < 2) s_b[t * M + k] = s_b[t * M + k] / A[(size_t)k * M + k];
            __syncthreads();
            const double xk = s_b[k], yk = s_b[M + k];
            for (int i = t; i < k; i += B) {
                const double aik = A[(size_t)i * M + k];
                s_b[i] = s_b[i] - aik * xk;
                s_b[M + i] = s_b[M + i] - aik * yk;
            }
            __syncthreads();
        }
        if (failed) { if (t == 0) s_state = kTpsSingular; }
        else {
            bool nf = false;
            for (int i = t; i < 2 * M; i += B) nf = nf || !tps_finite(s_b[i]);
            if (nf) s_state = kTpsSingular;
        }
        __syncthreads();
        failed = s_state != kTpsOk;
    }

    // 7. the record
    if (failed) {
        uint64_t *__restrict__ w = reinterpret_cast<uint64_t *>(rec);
        for (int i = t; i < tps_record_doubles(N); i += B) w[i] = kTpsNaN;
    } else {
        if (t < kTpsHead) {
            double v = 0.0;
            if (t < 5) v = s_norm[t];
            else if (t >= 8 && t < 14) v = s_b[((t - 8) & 1) * M + N + ((t - 8) >> 1)];
            rec[t] = v;
        }
        for (int i = t; i < N; i += B) { rec[kTpsHead + 4 * i + 2] = s_b[i]; rec[kTpsHead + 4 * i + 3] = s_b[M + i]; }
    }
    if (t == 0) a.status[f] = s_state;
}

// ------------------------------------------------------------------------------------------------ k_tps_field
__device__ __forceinline__ double tps_nan()
{
    const uint64_t u = kTpsNaN;
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}

template <int FMT, bool NODES>
__global__ __launch_bounds__(256) void k_tps_field(TpsFieldArgs a, const double *__restrict__ records, const TpsFrame *__restrict__ frames,
                                                   uint8_t *__restrict__ out)
{
    const int f = blockIdx.y;
    const TpsFrame fd = frames[f];
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    if (fd.obj_w <= 0 || fd.obj_h <= 0) return;
    const int OW = NODES ? tps_nodes(fd.obj_w, a.step) : fd.obj_w, OH = NODES ? tps_nodes(fd.obj_h, a.step) : fd.obj_h;
    if (r >= OH) return;
    const int mul = NODES ? a.step : 1;
    const double *__restrict__ rec = records + (size_t)f * tps_record_doubles(a.n_points);
    const bool failed = !(rec[2] == rec[2]);                 // (a failed frame's record is all NaN)
    const int lane = threadIdx.x;
    const double bw = (double)a.W, bh = (double)a.H, n_src_px = bw * bh;
    double X[4], Y[4], sx[4], sy[4];
#pragma unroll
    for (int k = 0; k < 4; k++) Y[k] = (double)((int64_t)r * mul + fd.y_off);
    uint8_t *__restrict__ row = out + (NODES ? fd.node_off + (uint64_t)r * (uint64_t)OW * 16 : fd.out_off + (uint64_t)r * (uint64_t)OW * (FMT == 0 ? 4 : 8));
    for (int64_t c0 = 0; c0 < OW; c0 += 256) {
#pragma unroll
        for (int k = 0; k < 4; k++) X[k] = (double)((c0 + lane + 64 * k) * mul + fd.x_off);
        if (failed) {
#pragma unroll
            for (int k = 0; k < 4; k++) { sx[k] = tps_nan(); sy[k] = tps_nan(); }
        } else tps_eval<4>(rec, a.n_points, X, Y, sx, sy);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t c = c0 + lane + 64 * k;
            if (c >= OW) continue;                           // the tail: nothing is written past the row
            if (NODES) {
                double *__restrict__ p = reinterpret_cast<double *>(row) + 2 * c;
                p[0] = sx[k]; p[1] = sy[k];
            } else {
                const bool cov = sx[k] >= 0 && sx[k] < bw && sy[k] >= 0 && sy[k] < bh;      // (NaN fails)
                int vx, vy;
                field_px<FMT>(cov, sx[k], sy[k], bw, n_src_px, vx, vy);
                if (FMT == 0) __builtin_nontemporal_store(vx, reinterpret_cast<int *>(row) + c);
                else { v2f v = { __int_as_float(vx), __int_as_float(vy) }; __builtin_nontemporal_store(v, reinterpret_cast<v2f *>(row) + c); }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ k_tps_blend
template <int FMT>
__global__ __launch_bounds__(256) void k_tps_blend(TpsFieldArgs a)
{
    const int f = blockIdx.y;
    const TpsFrame fd = a.frames[f];
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int OW = fd.obj_w;
    if (OW <= 0 || r >= fd.obj_h) return;
    const int step = a.step, nnx = tps_nodes(fd.obj_w, step), nny = tps_nodes(fd.obj_h, step);
    const int lane = threadIdx.x;
    const double bw = (double)a.W, bh = (double)a.H, n_src_px = bw * bh, inv = 1.0 / (double)step;       // (a power of two: exact)
    const int ky = min(r / step, nny - 2);
    const double fy = (double)(r - ky * step) * inv;
    const bool row_on = (r % step) == 0;
    const double *__restrict__ nd = reinterpret_cast<const double *>(a.nodes + fd.node_off);
    const double *__restrict__ n0 = nd + (size_t)ky * nnx * 2, *__restrict__ n1 = n0 + (size_t)nnx * 2;
    uint8_t *__restrict__ row = a.field + fd.out_off + (uint64_t)r * (uint64_t)OW * (FMT == 0 ? 4 : 8);
    for (int64_t c = lane; c < OW; c += 64) {
        const int ci = (int)c;
        double sx, sy;
        if (row_on && (ci % step) == 0) {                    // a pixel on a node: the node's value as it stands
            const double *__restrict__ p = nd + ((size_t)(r / step) * nnx + (size_t)(ci / step)) * 2;
            sx = p[0]; sy = p[1];
        } else {
            const int kx = min(ci / step, nnx - 2);
            const double fx = (double)(ci - kx * step) * inv;
            sx = tps_blend(n0[2 * kx], n0[2 * kx + 2], n1[2 * kx], n1[2 * kx + 2], fx, fy);
            sy = tps_blend(n0[2 * kx + 1], n0[2 * kx + 3], n1[2 * kx + 1], n1[2 * kx + 3], fx, fy);
        }
        const bool cov = sx >= 0 && sx < bw && sy >= 0 && sy < bh;
        int vx, vy;
        field_px<FMT>(cov, sx, sy, bw, n_src_px, vx, vy);
        if (FMT == 0) __builtin_nontemporal_store(vx, reinterpret_cast<int *>(row) + c);
        else { v2f v = { __int_as_float(vx), __int_as_float(vy) }; __builtin_nontemporal_store(v, reinterpret_cast<v2f *>(row) + c); }
    }
}

// ------------------------------------------------------------------------------------------------ k_tps_points
// Frame f reads list f % n_sets and writes n_pts pairs at f * n_pts.  A position that is not finite, a failed frame and a result with a NaN
// part hold 0x7fc00000 in both words.
__global__ __launch_bounds__(256) void k_tps_points(const double *__restrict__ records, int n_points, const float *__restrict__ points, int n_pts, int n_sets,
                                                    float *__restrict__ out)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pts) return;                                  // the tail: nothing is written past n_pts
    const double *__restrict__ rec = records + (size_t)f * tps_record_doubles(n_points);
    const v2f p = *reinterpret_cast<const v2f *>(points + 2 * ((size_t)(f % n_sets) * n_pts + i));
    const double X = (double)p.x, Y = (double)p.y;
    double sx = 0.0, sy = 0.0;
    bool ok = tps_finite(X) && tps_finite(Y) && rec[2] == rec[2];
    if (ok) tps_eval<1>(rec, n_points, &X, &Y, &sx, &sy);
    ok = ok && sx == sx && sy == sy;
    v2f v = { __int_as_float((int)kFieldNaN), __int_as_float((int)kFieldNaN) };
    if (ok) { v.x = (float)sx; v.y = (float)sy; }            // the one rounding to f32
    *reinterpret_cast<v2f *>(out + 2 * ((size_t)f * n_pts + i)) = v;
}

// ------------------------------------------------------------------------------------------------ launches
#ifdef __HIPCC__
void launch_tps_solve(const TpsSolveArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0) return;
    if (tps_in_lds(a.n_points)) hipLaunchKernelGGL(k_tps_solve<true>, dim3(a.n_frames), dim3(kTpsSolveBlock), 0, stream, a);
    else hipLaunchKernelGGL(k_tps_solve<false>, dim3(a.n_frames), dim3(kTpsSolveBlockBig), 0, stream, a);
}

void launch_tps_field(const TpsFieldArgs &a, int fmt, hipStream_t stream)
{
    if (a.n_frames <= 0 || a.max_h <= 0 || a.max_w <= 0) return;
    const dim3 block(64, 4), grid((a.max_h + 3) / 4, a.n_frames);
    if (a.step == 1) {
        if (fmt == 0) hipLaunchKernelGGL((k_tps_field<0, false>), grid, block, 0, stream, a, a.records, a.frames, a.field);
        else hipLaunchKernelGGL((k_tps_field<1, false>), grid, block, 0, stream, a, a.records, a.frames, a.field);
        return;
    }
    hipLaunchKernelGGL((k_tps_field<1, true>), dim3((tps_nodes(a.max_h, a.step) + 3) / 4, a.n_frames), block, 0, stream, a, a.records, a.frames, a.nodes);
    if (fmt == 0) hipLaunchKernelGGL(k_tps_blend<0>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_tps_blend<1>, grid, block, 0, stream, a);
}

void launch_tps_points(const double *records, int n_points, int n_frames, const float *points, int n_pts, int n_sets, float *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_pts <= 0) return;
    hipLaunchKernelGGL(k_tps_points, dim3((n_pts + 255) / 256, n_frames), dim3(256), 0, stream, records, n_points, points, n_pts, n_sets, out);
}
#endif

} // namespace hg
