// hg_spans.h -- the span machinery shared by the inverse piecewise kernels (hg_k_piecewise / _patch / _tile / _field.hip): the per-triangle
// solve and its taps, the row-list entry, the general path's span list and resolve, the self-span candidate scan, the "unsafe" bit.
// Included by hg_dev.h (and only there).  Plain inline functions: the LDS arrays and capacities are the calling kernel's, passed in.
// Citations are file:line into the reference's Homography.js (v1.8.0).  Design notes: DESIGN.md §4.
#pragma once

namespace hg {

// ------------------------------------------------------------------------------------------------ one triangle of one frame
// Vertex gather, forward / inverse matrix (:785-804, :1036-1038) and the three edge equations (:1141-1151) of triangle t of frame f.  A lane
// with `store` also writes what every consumer reads of them -- the taps and the inputs of the map path, record f * n_tris + t of fr.fwd,
// fr.inv, fr.segs -- each as soon as it is formed: the matrices are dead by the time the edges are (one store block after the edges:
// k_tri_setup 80 instead of 56-62 VGPRs, 6 waves per SIMD instead of 8).
__device__ __forceinline__ void tri_solve(const PwMesh &mesh, const PwFrames &fr, int f, int t, bool store, float d[6], float inv[6], Seg seg[3])
{
    const float *dp = fr.dst_pts + (size_t)f * mesh.n_pts * 2, *sp = frame_src(mesh, fr, f);
    float s[6], fwd[6];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t v = mesh.tris[3 * (size_t)t + k];
        if (v < (uint32_t)mesh.n_pts) {
            s[2 * k] = sp[2 * (size_t)v]; s[2 * k + 1] = sp[2 * (size_t)v + 1];
            d[2 * k] = dp[2 * (size_t)v];           d[2 * k + 1] = dp[2 * (size_t)v + 1];
        } else {                                   // typed-array read past the end: undefined -> NaN in the Float32Array(6)
            s[2 * k] = s[2 * k + 1] = d[2 * k] = d[2 * k + 1] = NAN;
        }
    }
    const size_t ft = (size_t)f * mesh.n_tris + t;
    solve_affine(s, d, fwd);
    invert_affine(fwd, inv);
    if (store) {
#pragma unroll
        for (int k = 0; k < 6; k++) fr.fwd[ft * 6 + k] = fwd[k];
        *reinterpret_cast<float4 *>(fr.inv + ft * kInvStride) = make_float4(inv[0], inv[1], inv[2], inv[3]);
        *reinterpret_cast<float4 *>(fr.inv + ft * kInvStride + 4) = make_float4(inv[4], inv[5], 0.f, 0.f);
    }
    define_seg(d[0], d[1], d[2], d[3], seg[0]);     // p0->p1
    define_seg(d[0], d[1], d[4], d[5], seg[1]);     // p0->p2
    define_seg(d[2], d[3], d[4], d[5], seg[2]);     // p1->p2
    if (store) { fr.segs[ft * 3] = seg[0]; fr.segs[ft * 3 + 1] = seg[1]; fr.segs[ft * 3 + 2] = seg[2]; }
}

// ------------------------------------------------------------------------------------------------ row lists (k_tri_spans*, RowLists)
// The cells [k, fin) of source row y's span (span_cells; k < fin), cut at output-row boundaries and appended to the lists of the OUTPUT rows
// they fall into.  r: y - yOff.  rowcnt / ent0: the frame's counters and first entry.
template <bool COMPACT>
__device__ __forceinline__ void file_row_span(int64_t k, int64_t fin, int64_t r, int obj_h, int W, int32_t *__restrict__ rowcnt, size_t ent0,
                                              const RowLists &rl, int t, const float inv[6])
{
    // usual case: the span sits in output row (y - yOff) (+objH when it wrapped); otherwise divide
    if (r < 0) r += obj_h;
    if (r < 0 || r >= obj_h || k < r * W || k >= (r + 1) * W) r = k / W;
    for (; r * W < fin; r++) {
        const int64_t lo = (k > r * W ? k : r * W) - r * W, hi = (fin < (r + 1) * W ? fin : (r + 1) * W) - r * W;
        const int slot = atomicAdd(&rowcnt[r], 1);
        if (slot < rl.cap) {
            const size_t idx = ent0 + (size_t)r * rl.cap + slot;
            const uint32_t lh = (uint32_t)lo | ((uint32_t)hi << 16);
            if (COMPACT) static_cast<uint2 *>(rl.ent)[idx] = make_uint2(lh, (uint32_t)t);
            else {
                uint4 *dst = static_cast<uint4 *>(rl.ent) + 2 * idx;
                dst[0] = make_uint4(lh, (uint32_t)t, __float_as_uint(inv[0]), __float_as_uint(inv[1]));
                dst[1] = make_uint4(__float_as_uint(inv[2]), __float_as_uint(inv[3]), __float_as_uint(inv[4]), __float_as_uint(inv[5]));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ general path (k_pw_fused, k_pw_field)
// Phase 1 of a one-row workgroup of 256 threads: every thread scans triangles; for each (triangle, source-row y) whose fillTriangle span can
// touch output row r it evaluates predictXLimits + the flat fill() indices exactly (span_cells) and appends the clipped span [lo, hi) x id
// to the LDS list.  Returns the number of spans met: beyond kRowSpanCap the list is incomplete and the caller flags the frame.
__device__ __forceinline__ int fused_row_spans(const PwFrames &fr, int f, int T, const FrameDesc &fd, int r, int *s_lo, int *s_hi, int *s_id, int *s_cnt)
{
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    const int W = fd.obj_w;
    const int64_t len = (int64_t)W * fd.obj_h;
    const int64_t row0 = (int64_t)r * W, row1 = row0 + W;
    const TriRange *__restrict__ trir = fr.trir + (size_t)f * T;
    const Seg *__restrict__ segs = fr.segs + (size_t)f * T * 3;
    for (int t = threadIdx.x; t < T; t += 256) {
        const TriRange tr = trir[t];
        if (tr.y_end <= tr.y_min) continue;
#pragma unroll 1
        for (int image = 0; image < 2; image++) {    // 0: indices >= 0;  1: negative indices wrapped by +len (= +objH rows)
            const int64_t shift = image ? fd.obj_h : 0;
            int64_t ylo = (int64_t)r - tr.a - shift + fd.y_off, yhi = (int64_t)r - tr.b - shift + fd.y_off;
            if (ylo < tr.y_min) ylo = tr.y_min;
            if (yhi > (int64_t)tr.y_end - 1) yhi = (int64_t)tr.y_end - 1;
#pragma unroll 1
            for (int64_t y = ylo; y <= yhi; y++) {
                int64_t k, fin;
                span_cells(segs + 3 * (size_t)t, (double)y, (double)fd.y_off, (double)W, len, k, fin);
                if (k < row0) k = row0;
                if (fin > row1) fin = row1;
                if (k < fin) {
                    const int slot = atomicAdd(s_cnt, 1);
                    if (slot < kRowSpanCap) { s_lo[slot] = (int)(k - row0); s_hi[slot] = (int)(fin - row0); s_id[slot] = t; }
                }
            }
        }
    }
    __syncthreads();
    return *s_cnt;
}

// Phase 2, per wave and 256-pixel window c0: the spans overlapping the window are found with one ballot per 64 spans, and each lane keeps
// max(id) over the spans covering its 4 pixels c0 + 4 lane + k ("last writer wins" of the sequential fill loop :852-858 == largest id).
__device__ __forceinline__ void fused_resolve_quad(const int *s_lo, const int *s_hi, const int *s_id, int cnt, int c0, int lane, int tid[4])
{
    const int cq = c0 + (lane << 2);
#pragma unroll
    for (int k = 0; k < 4; k++) tid[k] = -1;
    for (int j = 0; j < cnt; j += 64) {
        const int idx = j + lane;
        int lo = 0x7fffffff, hi = 0;
        if (idx < cnt) { lo = s_lo[idx]; hi = s_hi[idx]; }
        unsigned long long mask = __ballot(lo < c0 + 256 && hi > c0);
        while (mask) {
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int sl = s_lo[j + b], id = s_id[j + b];
            const unsigned span = (unsigned)(s_hi[j + b] - sl);
            const int d = cq - sl;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((unsigned)(d + k) < span) tid[k] = max(tid[k], id);
        }
    }
}

// ------------------------------------------------------------------------------------------------ self-span candidates (k_pw_rows<SELF>, k_pw_patch<SELF>, k_pw_tile)
// Input: what k_tri_setup wrote per (frame, triangle) -- the clamped row range [y_min, y_end) of fillTriangle's loop :1113-1120 and the bounds
// a, b on the output rows a row-y span can reach ((y - yOff) + b .. + a, objH further down when fill() wrapped a negative index: "image" 1; the
// enumeration k_pw_fused has always used).  Thread i tests triangle i (16 bytes each, one round trip for T <= nthreads): can one of its rows
// write into rows r0 .. r0 + nrows - 1?  Meshes beyond 1024 triangles: not the whole mesh but the entries k_tri_setup filed under the group's
// band of rows (row groups never straddle a band; an overfull band flagged the frame there).  `extra(i, bent)`: a further test on entry i
// (k_pw_tile: columns), bent the band's entries or nullptr.  Hits are compacted into the LDS candidate list {triangle | rows << 16, first source
// row} with one LDS atomic per wave.
// (int32 throughout: |yOff|, objH and the clamped row ranges are below 2^26 -- coordinates are limited to 2^24, hg_math.h -- and a, b are cell
//  offsets / W of a map with fewer than 2^31 cells)
// Candidate entries carry up to `chunk` source rows (one lane per row in the caller's span loop); a triangle that reaches more rows -- window
// borders, spans spilling over the row end (x-offset quirk) -- files a second entry for the rest, whose lanes loop if that is still more than
// `chunk` (a - b > 1: triangles wider than the map; rare).  *s_ncand counts every entry, also those beyond `cap` that are not stored.
struct AnyColumn {};        // `extra` of the kernels that take every candidate: no test is compiled (an always-true one costs the scan its 16-byte loads too)
template <class Extra>
__device__ __forceinline__ void self_candidates(const PwFrames &fr, int f, int T, const FrameDesc &fd, int r0, int nrows, int chunk, int nthreads,
                                                int *s_ncand, int *s_cand_tn, int *s_cand_y, int cap, Extra extra)
{
    const int lane = threadIdx.x & 63;
    const int g_lo = r0 + fd.y_off, g_hi = r0 + nrows - 1 + fd.y_off;
    const TriRange *__restrict__ trir = fr.trir + (size_t)f * T;
    int n_src = T;
    const int4 *__restrict__ bent = nullptr;
    if (fr.band_ent) {
        const int bandi = r0 >> fr.band_rows_log2;
        n_src = min(fr.band_cnt[(size_t)f * fr.band_stride + bandi], fr.band_cap);
        bent = fr.band_ent + ((size_t)f * fr.n_bands + bandi) * fr.band_cap * 2;      // (two int4 per entry; the second holds the column reach k_pw_tile uses)
    }
    for (int i0 = 0; i0 < n_src; i0 += nthreads) {
        const int i = i0 + (int)threadIdx.x;
        int t = i;
        TriRange tr = TriRange{0, 0, 0, 0};
        if (i < n_src) {
            if (bent) { const int4 e = bent[2 * i]; t = e.x; tr.y_min = e.y; tr.y_end = e.z; tr.a = (int16_t)(e.w & 0xffff); tr.b = e.w >> 16; }
            else tr = trir[i];
        }
        int ylo0 = max(g_lo - tr.a, tr.y_min), n0 = min(g_hi - tr.b, tr.y_end - 1) - ylo0 + 1;
        int ylo1 = max(g_lo - tr.a - fd.obj_h, tr.y_min), n1 = min(g_hi - tr.b - fd.obj_h, tr.y_end - 1) - ylo1 + 1;
        if constexpr (!std::is_same<Extra, AnyColumn>::value)      // (on the counts, not on tr: a test inside the block above splits its 16-byte loads into dwords)
            if (!(i < n_src && extra(i, bent))) { n0 = 0; n1 = 0; }
        const unsigned long long m0 = __ballot(n0 > 0), m1 = __ballot(n1 > 0);
        if ((m0 | m1) == 0ull) continue;                // (wave-uniform)
        const unsigned long long m0b = __ballot(n0 > chunk), m1b = __ballot(n1 > chunk);
        const int c0 = __popcll(m0), c0b = __popcll(m0b), c1 = __popcll(m1), c1b = __popcll(m1b);
        int base = 0;
        if (lane == 0) base = atomicAdd(s_ncand, c0 + c0b + c1 + c1b);
        base = __builtin_amdgcn_readfirstlane(base);
        auto below = [&](unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); };
        auto file = [&](int at, int y0, int n) { if (at < cap) { s_cand_tn[at] = t | (min(n, 0xffff) << 16); s_cand_y[at] = y0; } };
        if (n0 > 0) file(base + below(m0), ylo0, min(n0, chunk));
        if (n0 > chunk) file(base + c0 + below(m0b), ylo0 + chunk, n0 - chunk);
        if (m1) {
            if (n1 > 0) file(base + c0 + c0b + below(m1), ylo1, min(n1, chunk));
            if (n1 > chunk) file(base + c0 + c0b + c1 + below(m1b), ylo1 + chunk, n1 - chunk);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the "unsafe" bit of a span
// 1 unless both end pixels lo, hi - 1 of a span with record {m0, m2*y, m4, m1, m3*y, m5} are inside the source window, computed as the pixel
// bodies compute them (same fma, same rounding, same compares: the fp64 limits b*, or their high dwords hb where HIB) -- then every pixel
// between them is inside (sx, sy are monotone in x: one exact product, two monotone roundings), and a window or block whose pixels all
// resolve to such spans runs the pixel body without the bounds test :1047.  flag_spans (wave-uniform; host option): 0 = every span is unsafe.
template <bool HIB>
__device__ __forceinline__ int span_unsafe(bool flag_spans, const HiBounds &hb, double bx_lo, double bx_hi, double by_lo, double by_hi, int x_off,
                                           double m0, double m2y, double m4, double m1, double m3y, double m5, int lo, int hi)
{
    if (!flag_spans) return 1;
    const double xa = (double)(lo + x_off), xb = (double)(hi - 1 + x_off);
    double h[4] = { fma(m0, xa, m2y) + m4, fma(m1, xa, m3y) + m5, fma(m0, xb, m2y) + m4, fma(m1, xb, m3y) + m5 }, rd[4];
    round_x4(h, rd);
    const bool a = HIB ? hi_inb(hb, h[0], h[1]) : (bool)((int)(h[0] >= bx_lo) & (int)(h[0] < bx_hi) & (int)(h[1] >= by_lo) & (int)(h[1] < by_hi));
    const bool b = HIB ? hi_inb(hb, h[2], h[3]) : (bool)((int)(h[2] >= bx_lo) & (int)(h[2] < bx_hi) & (int)(h[3] >= by_lo) & (int)(h[3] < by_hi));
    return (a && b) ? 0 : 1;
}

} // namespace hg
