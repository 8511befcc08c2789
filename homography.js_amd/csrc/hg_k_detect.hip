// hg_k_detect.hip -- detecting and describing keypoints of plane sets (include/hgwarp.h, "detecting and describing keypoints"):
//   k_detect_cells     one workgroup per (plane, cell).  It walks the cell's share of the candidate zone in sub-tiles of kDetectTile: L with a
//                      halo of 5 goes into LDS, then the Sobel pair per pixel (halo 4), the three products summed over 7 columns (rows: halo 4,
//                      columns: halo 1), over 7 rows into R (halo 1), and the 3 x 3 test under the total order.  Two pixels of one 2 x 2 block are
//                      neighbours, so at most one of them is a candidate: every lane owns one block and one slot of the pool, no list is
//                      compacted.  The cell's running best per_cell joins the pool; an entry's rank is the number of entries that beat it --
//                      a total order, so the ranks are distinct -- and the entries ranked below per_cell are the new best; a byte flag per entry lets the
//                      count visit only the entries in use.  No atomics.
//   k_detect_compact   one workgroup per plane: an exclusive scan of the cell counts in cell order gives every cell its offset in the plane's
//                      list and the plane its count; positions, responses and indices go to their slots, the padding behind them.
//   k_detect_describe  one wavefront per slot: the 31 x 31 patch of L in LDS, m10 and m01 summed over the lanes, the bin, the 5 x 5 box sums
//                      at the 25 x 25 offsets the turned tests can reach (separably), eight tests per lane of the first 32, 32 bytes stored as
//                      two 16-byte words.
// The rules live in hg_detect_dev.h.  The kernels need that header only and cooperate through LDS and barriers alone, so a host check
// compiles this file behind a thread-index shim (tests/cpp/detect_check.cpp); the launcher is compiled under hipcc only.  Integer
// arithmetic throughout: the float32 positions are put together from their bits.
#ifdef __HIPCC__
#include "hg_kernels.h"
#endif
#include "hg_detect_dev.h"

namespace hg {

struct DetectRec { int64_t r; int32_t bin; int32_t idx; };       // a scratch record and a slot of d_info: 16 bytes; r == 0: none

// L at (x, y) of a plane of W columns; words: a 4-channel plane whose base is 4-byte aligned (uniform).
__device__ __forceinline__ int32_t detect_load(const uint8_t *__restrict__ plane, int W, int channels, bool words, int x, int y)
{
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    if (channels == 1) return plane[i];
    if (words) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(plane + 4 * i);
        return detect_luma(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u);
    }
    return detect_luma(plane[4 * i], plane[4 * i + 1], plane[4 * i + 2]);
}

// The float32 word of an integer 0 <= v < 2^24.
__device__ __forceinline__ uint32_t detect_float_bits(uint32_t v)
{
    if (v == 0) return 0u;
    const int e = 31 - __builtin_clz(v);
    return ((uint32_t)(127 + e) << 23) | ((v << (23 - e)) & 0x7fffffu);
}

// ------------------------------------------------------------------------------------------------ k_detect_cells
// rec: n_planes x cells x per_cell records (r == 0 beyond the cell's count); cnt: n_planes x cells.
__global__ __launch_bounds__(kDetectBlock) void k_detect_cells(const uint8_t *__restrict__ planes, int W, int H, size_t plane_stride, int channels, int cell,
                                                               int per_cell, int cells_x, int64_t min_response, DetectRec *__restrict__ rec,
                                                               int32_t *__restrict__ cnt)
{
    constexpr int T = kDetectTile, LS = T + 10, GS = T + 8, HS = T + 2;
    static_assert(kDetectBlock == (T / 2) * (T / 2) && (T + 10) * (T + 10) < (1 << 11), "one lane per 2 x 2 block of a sub-tile; the flat walks' reciprocal");
    __shared__ uint8_t sL[LS * LS];
    __shared__ int32_t sG[GS * GS];                              // Ix in the low half, Iy in the high half (each within +-1020)
    __shared__ int32_t sH[3][GS * HS];                           // the 7-column sums of Ix Ix, Iy Iy, Ix Iy: GS rows of HS
    __shared__ int64_t sR[HS * HS];
    __shared__ DetectRec pool[kDetectBlock + kDetectMaxPerCell]; // a slot per lane, then the running best
    __shared__ DetectRec next[kDetectMaxPerCell];
    __shared__ uint64_t flag_words[(kDetectBlock + kDetectMaxPerCell) / 8];      // one byte per pool entry: 1 = it holds a candidate
    uint8_t *flags = reinterpret_cast<uint8_t *>(flag_words);
    const int tid = threadIdx.x;
    const int c = blockIdx.x, p = blockIdx.y, n_cells = gridDim.x;
    const int cx0 = (c % cells_x) * cell, cy0 = (c / cells_x) * cell;
    // the cell's share of the candidate zone [16, W - 16) x [16, H - 16): empty for W < 33 or H < 33
    const int zx0 = max(cx0, kDetectMargin), zx1 = min(min(cx0 + cell, W), W - kDetectMargin);
    const int zy0 = max(cy0, kDetectMargin), zy1 = min(min(cy0 + cell, H), H - kDetectMargin);
    const uint8_t *__restrict__ plane = planes + (size_t)p * plane_stride;
    const bool words = channels == 4 && (reinterpret_cast<uintptr_t>(plane) & 3) == 0;
    DetectRec *best = pool + kDetectBlock;
    if (tid < kDetectMaxPerCell) best[tid] = DetectRec{0, 0, 0};
    for (int oy = zy0; oy < zy1; oy += T) {
        for (int ox = zx0; ox < zx1; ox += T) {                  // (uniform: the barriers below)
            const int tw = min(T, zx1 - ox), th = min(T, zy1 - oy);
            if (tid < kDetectMaxPerCell) next[tid] = DetectRec{0, 0, 0};
            // Each pass walks its rectangle flat, 256 entries a step: row = i / w by a Q20 reciprocal, exact for i < 2^11 and w <= 42
            // (i (w ceil(2^20 / w) - 2^20) < 2^11 * 42 < 2^20).
            // L of the pixels (ox - 5 + lx, oy - 5 + ly): inside the plane, since the zone keeps 16 from every border
            {
                const int w = tw + 10, n = w * (th + 10), inv = ((1 << 20) + w - 1) / w;
                for (int i = tid; i < n; i += kDetectBlock) {
                    const int ly = (i * inv) >> 20, lx = i - ly * w;
                    sL[ly * LS + lx] = (uint8_t)detect_load(plane, W, channels, words, ox - 5 + lx, oy - 5 + ly);
                }
            }
            __syncthreads();
            // Sobel at the pixels (ox - 4 + gx, oy - 4 + gy) = sL (gx + 1, gy + 1)
            {
                const int w = tw + 8, n = w * (th + 8), inv = ((1 << 20) + w - 1) / w;
                for (int i = tid; i < n; i += kDetectBlock) {
                    const int gy = (i * inv) >> 20, gx = i - gy * w;
                    const uint8_t *r0 = sL + gy * LS + gx, *r1 = r0 + LS, *r2 = r1 + LS;
                    const int32_t ix = ((int32_t)r0[2] + 2 * (int32_t)r1[2] + (int32_t)r2[2]) - ((int32_t)r0[0] + 2 * (int32_t)r1[0] + (int32_t)r2[0]);
                    const int32_t iy = ((int32_t)r2[0] + 2 * (int32_t)r2[1] + (int32_t)r2[2]) - ((int32_t)r0[0] + 2 * (int32_t)r0[1] + (int32_t)r0[2]);
                    sG[gy * GS + gx] = (int32_t)(((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16));
                }
            }
            __syncthreads();
            // the products summed over the columns hx .. hx + 6 of row hy
            {
                const int w = tw + 2, n = w * (th + 8), inv = ((1 << 20) + w - 1) / w;
                for (int i = tid; i < n; i += kDetectBlock) {
                    const int hy = (i * inv) >> 20, hx = i - hy * w;
                    int32_t a = 0, cc = 0, b = 0;
#pragma unroll
                    for (int k = 0; k < 7; k++) {
                        const int32_t v = sG[hy * GS + hx + k];
                        const int32_t ix = (int32_t)(int16_t)(uint16_t)((uint32_t)v & 0xffffu), iy = v >> 16;
                        a += ix * ix; cc += iy * iy; b += ix * iy;
                    }
                    sH[0][hy * HS + hx] = a; sH[1][hy * HS + hx] = cc; sH[2][hy * HS + hx] = b;
                }
            }
            __syncthreads();
            // R at the pixels (ox - 1 + rx, oy - 1 + ry)
            {
                const int w = tw + 2, n = w * (th + 2), inv = ((1 << 20) + w - 1) / w;
                for (int i = tid; i < n; i += kDetectBlock) {
                    const int ry = (i * inv) >> 20, rx = i - ry * w;
                    int32_t a = 0, cc = 0, b = 0;
#pragma unroll
                    for (int k = 0; k < 7; k++) { a += sH[0][(ry + k) * HS + rx]; cc += sH[1][(ry + k) * HS + rx]; b += sH[2][(ry + k) * HS + rx]; }
                    sR[ry * HS + rx] = detect_response(a, cc, b);
                }
            }
            __syncthreads();
            // the lane's 2 x 2 block: tile pixels (2 bx + i, 2 by + j) = sR (2 bx + i + 1, 2 by + j + 1); the 4 x 4 values around it stay inside
            // sR, and those beyond (tw + 2, th + 2) are only ever neighbours of pixels outside the tile
            {
                const int bx = tid & 15, by = tid >> 4;
                DetectRec mine{0, 0, 0};
                if (2 * bx < tw && 2 * by < th) {
                    int64_t r[4][4];
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int i = 0; i < 4; i++) r[j][i] = sR[(2 * by + j) * HS + 2 * bx + i];
#pragma unroll
                    for (int j = 0; j < 2; j++)
#pragma unroll
                        for (int i = 0; i < 2; i++) {
                            const int u = 2 * bx + i, v = 2 * by + j;
                            const int32_t idx = (oy + v) * W + ox + u;       // (W H <= 2^30)
                            const int64_t rc = r[j + 1][i + 1];
                            bool ok = u < tw && v < th && rc >= min_response;
#pragma unroll
                            for (int dj = -1; dj <= 1; dj++)
#pragma unroll
                                for (int di = -1; di <= 1; di++)
                                    if (dj != 0 || di != 0) ok = ok && detect_beats(rc, idx, r[j + 1 + dj][i + 1 + di], idx + dj * W + di);
                            if (ok) mine = DetectRec{rc, 0, idx};
                        }
                }
                pool[tid] = mine;
                flags[tid] = mine.r > 0 ? 1 : 0;
                if (tid < kDetectMaxPerCell) flags[kDetectBlock + tid] = best[tid].r > 0 ? 1 : 0;      // (best[tid] is this lane's own write)
            }
            __syncthreads();
            // ranks over the pool and the running best (min_response >= 1: an empty slot has r == 0): only the entries in use are visited, eight
            // flags per word; a flag byte holds one bit, so clearing the lowest bit of the word steps to the next entry
            for (int s = tid; s < kDetectBlock + kDetectMaxPerCell; s += kDetectBlock) {
                const DetectRec e = pool[s];
                if (e.r > 0) {
                    int rank = 0;
                    for (int w = 0; w < (kDetectBlock + kDetectMaxPerCell) / 8; w++)
                        for (uint64_t m = flag_words[w]; m != 0; m &= m - 1) {
                            const DetectRec o = pool[8 * w + (__builtin_ctzll(m) >> 3)];
                            rank += detect_beats(o.r, o.idx, e.r, e.idx) ? 1 : 0;
                        }
                    if (rank < per_cell) next[rank] = e;
                }
            }
            __syncthreads();
            if (tid < kDetectMaxPerCell) best[tid] = next[tid];
        }
    }
    __syncthreads();
    const size_t cell_id = (size_t)p * (size_t)n_cells + (size_t)c;
    if (tid < per_cell) rec[cell_id * (size_t)per_cell + tid] = best[tid];
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < per_cell; k++) n += best[k].r > 0 ? 1 : 0;
        cnt[cell_id] = n;
    }
}

// ------------------------------------------------------------------------------------------------ k_detect_compact
// list: n_planes x n_slots flat indices in list order, -1 beyond the count (what k_detect_describe reads, whichever outputs were asked for).
__global__ __launch_bounds__(kDetectBlock) void k_detect_compact(int W, int n_cells, int per_cell, size_t desc_stride, const DetectRec *__restrict__ rec,
                                                                 const int32_t *__restrict__ cnt, int32_t *__restrict__ list,
                                                                 int32_t *__restrict__ out_counts, uint2 *__restrict__ out_points,
                                                                 uint8_t *__restrict__ out_desc, DetectRec *__restrict__ out_info)
{
    __shared__ int32_t scan[kDetectBlock];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t n_slots = (size_t)n_cells * (size_t)per_cell, s0 = (size_t)p * n_slots;
    int total = 0;
    for (int base = 0; base < n_cells; base += kDetectBlock) {   // (every lane walks every step: the scan's barriers)
        const int c = base + tid;
        const int n = c < n_cells ? cnt[(size_t)p * n_cells + c] : 0;
        scan[tid] = n;                                           // inclusive prefix sum of the counts, in cell order
        __syncthreads();
        for (int s = 1; s < kDetectBlock; s <<= 1) {
            const int32_t v = tid >= s ? scan[tid - s] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int off = total + scan[tid] - n;
        total += scan[kDetectBlock - 1];
        __syncthreads();
        for (int r = 0; r < n; r++) {
            const DetectRec e = rec[((size_t)p * n_cells + c) * (size_t)per_cell + r];
            const size_t k = s0 + (size_t)(off + r);
            list[k] = e.idx;
            if (out_points) out_points[k] = make_uint2(detect_float_bits((uint32_t)(e.idx % W)), detect_float_bits((uint32_t)(e.idx / W)));
            if (out_info) out_info[k] = DetectRec{e.r, 0, e.idx};                 // (the bin: k_detect_describe)
        }
    }
    for (size_t k = s0 + (size_t)total + tid; k < s0 + n_slots; k += kDetectBlock) {      // the slots no keypoint fills
        list[k] = -1;
        if (out_points) out_points[k] = make_uint2(0x7fc00000u, 0x7fc00000u);
        if (out_info) out_info[k] = DetectRec{0, -1, -1};
        if (out_desc) {
            uint4 *row = reinterpret_cast<uint4 *>(out_desc + k * desc_stride);
            row[0] = make_uint4(0u, 0u, 0u, 0u); row[1] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (tid == 0) out_counts[p] = total;
}

// ------------------------------------------------------------------------------------------------ k_detect_describe
// table: kDetectBins x kDetectTests x {ax, ay, bx, by} int8, 4-byte aligned.
constexpr int kDescribeBlock = 64;
__global__ __launch_bounds__(kDescribeBlock) void k_detect_describe(const uint8_t *__restrict__ planes, int W, size_t plane_stride, int channels, size_t n_slots,
                                                                    size_t desc_stride, const int32_t *__restrict__ list, const int8_t *__restrict__ table,
                                                                    uint8_t *__restrict__ out_desc, DetectRec *__restrict__ out_info)
{
    constexpr int PS = 2 * kDetectDiscR + 1;                     // 31: the patch, offsets -15 .. 15
    constexpr int BS = 25, HR = 29;                              // box-sum offsets -12 .. 12; the rows -14 .. 14 their 5-column sums are needed at
    __shared__ uint8_t sP[PS * PS];
    __shared__ int32_t red[2][kDescribeBlock];
    __shared__ uint16_t sRow[HR * BS];                           // (<= 1275)
    __shared__ uint16_t sS[BS * BS];                             // (<= 6375)
    __shared__ uint32_t sBytes[8];
    const int tid = threadIdx.x, p = blockIdx.y;
    const size_t k = (size_t)p * n_slots + blockIdx.x;
    const int32_t idx = list[k];
    if (idx < 0) return;                                         // (uniform) padding: k_detect_compact wrote it
    const int x = idx % W, y = idx / W;
    const uint8_t *__restrict__ plane = planes + (size_t)p * plane_stride;
    const bool words = channels == 4 && (reinterpret_cast<uintptr_t>(plane) & 3) == 0;
    int32_t m10 = 0, m01 = 0;
    for (int i = tid; i < PS * PS; i += kDescribeBlock) {
        const int dy = i / PS - kDetectDiscR, dx = i % PS - kDetectDiscR;
        const int32_t l = detect_load(plane, W, channels, words, x + dx, y + dy);     // (a keypoint keeps 16 from every border)
        sP[i] = (uint8_t)l;
        if (dx * dx + dy * dy <= kDetectDiscR * kDetectDiscR) { m10 += dx * l; m01 += dy * l; }
    }
    red[0][tid] = m10; red[1][tid] = m01;
    __syncthreads();
    m10 = 0; m01 = 0;
    for (int j = 0; j < kDescribeBlock; j++) { m10 += red[0][j]; m01 += red[1][j]; }      // (integers: any order gives the same sum)
    const int bin = detect_bin(m10, m01);
    for (int i = tid; i < HR * BS; i += kDescribeBlock) {        // row offset i / BS - 14, column offset i % BS - 12: sP (.. + 15)
        const uint8_t *q = sP + (i / BS + 1) * PS + (i % BS + 1);
        sRow[i] = (uint16_t)((int)q[0] + q[1] + q[2] + q[3] + q[4]);
    }
    __syncthreads();
    for (int i = tid; i < BS * BS; i += kDescribeBlock) {
        const uint16_t *q = sRow + i;                            // the rows i / BS .. i / BS + 4 of sRow are the offsets - 2 .. + 2
        sS[i] = (uint16_t)((int)q[0] + q[BS] + q[2 * BS] + q[3 * BS] + q[4 * BS]);
    }
    __syncthreads();
    if (tid < 8) sBytes[tid] = 0u;
    __syncthreads();
    if (tid < 32) {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(table) + ((size_t)bin * kDetectTests + (size_t)tid * 8);
        uint32_t byte = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint32_t w = t[b];
            const int ax = (int8_t)(w & 255u), ay = (int8_t)((w >> 8) & 255u), bx = (int8_t)((w >> 16) & 255u), by = (int8_t)(w >> 24);
            byte |= (sS[(ay + 12) * BS + ax + 12] < sS[(by + 12) * BS + bx + 12] ? 1u : 0u) << b;
        }
        reinterpret_cast<uint8_t *>(sBytes)[tid] = (uint8_t)byte;
    }
    __syncthreads();
    if (out_desc && tid < 2) *reinterpret_cast<uint4 *>(out_desc + k * desc_stride + 16 * tid) = make_uint4(sBytes[4 * tid], sBytes[4 * tid + 1], sBytes[4 * tid + 2], sBytes[4 * tid + 3]);
    if (out_info && tid == 0) out_info[k].bin = bin;
}

// ------------------------------------------------------------------------------------------------ launches
#ifdef __HIPCC__
static_assert(sizeof(DetectRec) == 16, "a record is one 16-byte word");

void launch_detect(const DetectArgs &a, hipStream_t stream)
{
    if (a.n_planes <= 0) return;
    const int n_cells = a.cells_x * a.cells_y;
    DetectRec *rec = static_cast<DetectRec *>(a.ws_rec);
    hipLaunchKernelGGL(k_detect_cells, dim3(n_cells, a.n_planes), dim3(kDetectBlock), 0, stream, a.planes, a.W, a.H, a.plane_stride, a.channels, a.cell, a.per_cell,
                       a.cells_x, a.min_response, rec, a.ws_cnt);
    hipLaunchKernelGGL(k_detect_compact, dim3(a.n_planes), dim3(kDetectBlock), 0, stream, a.W, n_cells, a.per_cell, a.desc_stride, rec, a.ws_cnt, a.ws_list,
                       a.out_counts, static_cast<uint2 *>(a.out_points), static_cast<uint8_t *>(a.out_desc), static_cast<DetectRec *>(a.out_info));
    if (a.out_desc || a.out_info)
        hipLaunchKernelGGL(k_detect_describe, dim3(n_cells * a.per_cell, a.n_planes), dim3(kDescribeBlock), 0, stream, a.planes, a.W, a.plane_stride, a.channels,
                           (size_t)n_cells * a.per_cell, a.desc_stride, a.ws_list, a.ws_table, static_cast<uint8_t *>(a.out_desc), static_cast<DetectRec *>(a.out_info));
}
#endif

} // namespace hg
