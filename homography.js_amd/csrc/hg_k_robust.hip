// hg_k_robust.hip -- the frames of a set blended into one canvas by an order statistic (include/hgwarp.h, hg_mosaic_robust_device):
// k_mosaic_robust takes, per canvas pixel and channel, the median, a trimmed mean, the minimum or the maximum of the bytes of every frame
// whose window holds the pixel and whose HG_FIELD_COORDS field covers it, so that what moves through a minority of the frames drops out.
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  u8 only and integers only on the ranked values: no atomics, no floating point but
// the one multiply of a gain (a byte again before it is ranked), the same bytes on every run.  The numpy model of tests/hgtest/robust.py
// sorts; this kernel never does.  Design notes: DESIGN.md §4.20, figures: EXPERIMENTS.md "Robust mosaic".
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_robust_dev.h"

namespace hg {

// The mosaic's tiling: one canvas pixel per lane, 64 columns x 4 rows per block, one wave per row (its loads from one frame row are
// contiguous); block b owns tile (b % tiles_x, b / tiles_x).  Lanes beyond the canvas stay for the barrier and contribute nothing.
//  1. LIST.  Wave 0 lists the frames whose window meets the tile in LDS, in ascending order (mos_hits from the record alone, a ballot and a
//     prefix count per 64 records).  Every later walk runs over that list of n_hit frames, not over the table.
//  2. STAGE.  One walk of the list through global memory: a lane's contributor becomes one word (rob_pack: its C bytes, gained where there
//     are gains) and n counts them.  With n_hit <= cap (the slots this launch allocated: rob_cap, at most ROB_LMAX) the word goes to slot
//     n of the lane's LDS column, laid out [slot][lane]: lane l of a wave reads and writes bank l whatever its slot, and no lane touches
//     another lane's column, so the columns need no barrier.  The first two words also stay in registers: a lane with n <= 2 is done from
//     them (MEDIAN and TRIMMED of two values are their rounded mean) and takes no part in what follows.
//  3. SELECT, lanes with n > 2.  A selection, not a sort: for rank k of a channel, from bit 7 down, count the values that agree with the
//     bits decided so far and have this bit clear; k below the count keeps the bit clear, otherwise the bit is set and k drops by the
//     count.  Eight rounds resolve the two ranks rob_ranks names (lo == hi for MIN, MAX and an odd MEDIAN) on all C channels at once: one
//     LDS read per contributor and round.  Nothing is indexed at run time but LDS: counts, ranks and prefixes are 6 C registers.
//  4. TRIMMED adds one summing pass: with a = s_lo < b = s_hi the kept values are the copies of a from rank lo on (#{v <= a} - lo of them),
//     everything strictly between, and the copies of b up to rank hi (hi + 1 - #{v < b}); with a == b all hi - lo + 1 are a.
// A tile that more than cap frames hit (uniform over the block) stages nothing and runs the same rounds over the list in global
// memory instead -- count, 8 rounds and TRIMMED's pass: 9-10 walks, which L2 serves after the first.  Correct for every n <= 256 either way.
template <int C>
__global__ __launch_bounds__(256) void k_mosaic_robust(const MosaicFrame4 *__restrict__ frames, int n_frames, const uint8_t *__restrict__ coords,
                                                       const uint8_t *__restrict__ pixels, int mode, float trim, uint32_t cap, int cx, int cy, int cw,
                                                       int ch, uint32_t tiles_x, uint8_t *__restrict__ canvas, float *__restrict__ weight,
                                                       const float *__restrict__ gains)
{
    __shared__ uint16_t s_list[256];                              // (n_frames <= 256)
    __shared__ uint32_t s_n;
#ifdef __HIPCC__
    extern __shared__ uint32_t s_col[];                           // cap x 256 words, sized by the launch
#else
    __shared__ uint32_t s_col[ROB_LMAX * 256];
#endif
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t i0 = (int64_t)tx * 64, j0 = (int64_t)ty * 4;
    const int64_t X0 = cx + i0, Y0 = cy + j0, X1 = min(X0 + 64, (int64_t)cx + cw), Y1 = min(Y0 + 4, (int64_t)cy + ch);
    const uint32_t lane = threadIdx.x, wave = threadIdx.y, t = wave * 64 + lane;
    const int64_t i = i0 + lane, j = j0 + wave;
    const bool inb = i < cw && j < ch;
    const int64_t X = cx + i, Y = cy + j;
    if (wave == 0) {
        uint32_t k = 0;
        for (int base = 0; base < n_frames; base += 64) {
            const int f = base + (int)lane;
            const bool hit = f < n_frames && mos_hits(frames[f >> 2].f[f & 3], X0, X1, Y0, Y1);
            const uint64_t m = __ballot(hit);
            if (hit) s_list[k + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint16_t)f;
            k += (uint32_t)__builtin_popcountll(m);
        }
        if (lane == 0) s_n = k;
    }
    __syncthreads();
    const uint32_t n_hit = s_n;                                   // (<= n_frames <= 256)
    const bool staged = n_hit <= cap;                             // (uniform over the block)
    uint32_t *col = s_col + t;                                    // slot s of this lane: col[s * 256]

    // Step 2 of the header: listed frame f at this pixel -- false unless it contributes, else its bytes as one word.
    auto value = [&](uint32_t f, uint32_t *w) {
        float2 s;
        uint32_t p[C];
        if (!mos_fetch<uint8_t, C>(frames[f >> 2].f[f & 3], X, Y, coords, pixels, &s, p)) return false;
        if (gains) {
            const float g = gains[f];
#pragma unroll
            for (int c = 0; c < mos_stat_channels(C); c++) p[c] = rob_gained(g, p[c]);
        }
        *w = rob_pack<C>(p);
        return true;
    };

    uint32_t n = 0, w0 = 0, w1 = 0;
    for (uint32_t k = 0; k < n_hit; k++) {
        const uint32_t f = rob_uniform(s_list[k]);
        uint32_t w;
        if (!inb || !value(f, &w)) continue;
        if (staged) col[n * 256] = w;                             // (n < n_hit <= cap)
        if (n == 0) w0 = w; else if (n == 1) w1 = w;
        n++;
    }

    const uint32_t m = n > 2 ? n : 0;                             // what this lane walks in the rounds
    // Every contributor's word of a lane with m > 0, once, in ascending frame order: from its column, or from global memory again.
    auto walk = [&](auto &&body) {
        if (staged) {
#pragma unroll HG_ROBUST_UNROLL
            for (uint32_t s = 0; s < m; s++) body(col[s * 256]);
        } else {
            for (uint32_t k = 0; k < n_hit; k++) {
                const uint32_t f = rob_uniform(s_list[k]);
                uint32_t w;
                if (m && value(f, &w)) body(w);
            }
        }
    };

    uint32_t r[C];
#pragma unroll
    for (int c = 0; c < C; c++) r[c] = 0;
    if (__ballot(m != 0)) {                                      // (uniform over the wave)
        const bool two = mode == ROB_MEDIAN || mode == ROB_TRIMMED;
        uint32_t lo = 0, hi = 0;
        if (m) rob_ranks(mode, trim, n, &lo, &hi);
        uint32_t klo[C], khi[C], a[C], b[C];                      // the ranks left among the values that agree with the prefixes a, b
#pragma unroll
        for (int c = 0; c < C; c++) { klo[c] = lo; khi[c] = hi; a[c] = 0; b[c] = 0; }
        for (int bit = 7; bit >= 0; bit--) {
            uint32_t clo[C], chi[C];
#pragma unroll
            for (int c = 0; c < C; c++) { clo[c] = 0; chi[c] = 0; }
            walk([&](uint32_t w) {
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const uint32_t v = rob_byte(w, c) >> bit;
                    clo[c] += v == (a[c] >> bit) ? 1u : 0u;
                    if (two) chi[c] += v == (b[c] >> bit) ? 1u : 0u;
                }
            });
#pragma unroll
            for (int c = 0; c < C; c++) {
                if (klo[c] >= clo[c]) { klo[c] -= clo[c]; a[c] |= 1u << bit; }
                if (two && khi[c] >= chi[c]) { khi[c] -= chi[c]; b[c] |= 1u << bit; }
            }
        }
        if (!two) {
#pragma unroll
            for (int c = 0; c < C; c++) b[c] = a[c];
        }
        if (mode == ROB_TRIMMED) {
            uint32_t cle[C], clt[C], mid[C];
#pragma unroll
            for (int c = 0; c < C; c++) { cle[c] = 0; clt[c] = 0; mid[c] = 0; }
            walk([&](uint32_t w) {
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const uint32_t v = rob_byte(w, c);
                    cle[c] += v <= a[c] ? 1u : 0u;
                    clt[c] += v < b[c] ? 1u : 0u;
                    mid[c] += v > a[c] && v < b[c] ? v : 0u;
                }
            });
            const uint32_t kept = hi - lo + 1;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const uint32_t S = a[c] == b[c] ? a[c] * kept : a[c] * (cle[c] - lo) + mid[c] + b[c] * (hi + 1 - clt[c]);
                r[c] = rob_trimmed(S, kept);
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) r[c] = rob_middle(a[c], b[c]);
        }
    }
    if (n <= 2) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            const uint32_t x0 = rob_byte(w0, c), x1 = rob_byte(w1, c);
            r[c] = n < 2 ? x0 : mode == ROB_MIN ? min(x0, x1) : mode == ROB_MAX ? max(x0, x1) : rob_middle(x0, x1);      // (n == 0: w0 is 0)
        }
    }
    if (!inb) return;
    const uint64_t k = (uint64_t)j * (uint64_t)cw + (uint64_t)i;
    if (weight) __builtin_nontemporal_store((float)n, weight + k);
    uint8_t *__restrict__ o = canvas + k * C;
    if constexpr (C == 4) {
        if (!(reinterpret_cast<uintptr_t>(canvas) & 3)) { __builtin_nontemporal_store(r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24), reinterpret_cast<uint32_t *>(o)); return; }
    } else if constexpr (C == 2) {
        if (!(reinterpret_cast<uintptr_t>(canvas) & 1)) { __builtin_nontemporal_store((uint16_t)(r[0] | (r[1] << 8)), reinterpret_cast<uint16_t *>(o)); return; }
    }
#pragma unroll
    for (int c = 0; c < C; c++) __builtin_nontemporal_store((uint8_t)r[c], o + c);
}

// ------------------------------------------------------------------------------------------------ launcher
#ifdef __HIPCC__
void launch_mosaic_robust(const MosaicFrame4 *frames, int n_frames, const uint8_t *coords, const uint8_t *pixels, int channels, int mode, float trim,
                          int cx, int cy, int cw, int ch, uint8_t *canvas, float *weight, const float *gains, hipStream_t stream)
{
    if (cw <= 0 || ch <= 0) return;
    const uint32_t tiles_x = (uint32_t)(((int64_t)cw + 63) / 64);
    const uint64_t n_blocks = (uint64_t)tiles_x * (uint64_t)(((int64_t)ch + 3) / 4);      // (< 2^31 for a canvas of at most 2^31 pixels)
    const uint32_t cap = rob_cap(n_frames);
    for_elem_channels(1, channels, [&](auto, auto c) {
        auto *kernel = k_mosaic_robust<decltype(c)::value>;
        // (with the list the block passes the 64 KiB a kernel may take unasked; a refusal here shows as the launch's error)
        if (cap * 1024u > 32768u) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(ROB_LMAX * 1024u));
        hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(64, 4), cap * 1024u, stream, frames, n_frames, coords, pixels, mode, trim, cap, cx, cy, cw, ch,
                           tiles_x, canvas, weight, gains);
    });
}
#endif

} // namespace hg
