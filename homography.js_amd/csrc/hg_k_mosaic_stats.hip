// hg_k_mosaic_stats.hip -- the overlaps of a frame set measured on the device (include/hgwarp.h, hg_mosaic_overlap_stats_device):
// k_mosaic_stats counts, for every ordered pair of frames (a, b), the canvas pixels both contribute to (N_ab) and sums a's intensity over
// them (S_ab) -- what the gain solve of hg_mosaic_solve_gains needs, so that no frame has to come down.  Hand-written HIP for gfx950
// (MI355X / CDNA4), wave64.  Integers only: the result does not depend on the order of the additions.  The numpy model of
// tests/hgtest/mosaic_gain.py computes the same sums.  Design notes: DESIGN.md §4.12, figures: EXPERIMENTS.md F.10.
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_mosaic_dev.h"

namespace hg {

// Frames per side of the block's pair table: 64 x 64 entries in LDS (16 KiB).  A tile that more frames hit walks the pairs in
// chunks of this many; also the width of a wave, so that lane k of a wave keeps column k of the table's row in its registers.
// An entry is one 32-bit word, so that a pair costs one LDS atomic: the sum of a tile in the low 18 bits (256 lanes x 765 = 195 840
// < 2^18, so it never carries into the count), the count (at most 256) above them.
constexpr uint32_t MOS_STAT_K = 64;
constexpr uint32_t MOS_STAT_SUM_BITS = 18;

// A value every lane of the wave holds alike (an entry of the block's list, read from LDS), said so: the frame's record is then read on
// the scalar side, as the mosaic reads it.
__device__ __forceinline__ uint32_t mos_uniform(uint32_t v)
{
#ifdef __HIPCC__
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}

// The sum of v over the 64 lanes of the wave, in every lane.
__device__ __forceinline__ uint32_t mos_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The mosaic's tiling: one canvas pixel per lane, 64 columns x 4 rows per block, one wave per row; block b owns tile (b % tiles_x,
// b / tiles_x).  Lanes beyond the canvas stay (they vote `no` in every ballot).
//  1. Wave 0 lists the frames whose window meets the tile, in ascending order (a ballot and a prefix count per 64 records).
//  2. Per chunk B of MOS_STAT_K listed frames every wave takes one ballot per frame -- which of its lanes does b contribute to? -- and lane
//     k keeps the ballot of the chunk's frame k.
//  3. Per listed frame a: the lanes it contributes to (ballot ma) and their intensities' sum sa (one wave reduction).  Lane k then holds
//     m = ma & its ballot: N_ab of this wave is popcount(m) and S_ab is sa wherever m == ma -- within a tile nearly all lanes share one
//     contributor set -- ; only the pairs with a partial overlap inside the wave cost a reduction of their own.  Each lane adds its column
//     to the block's table in LDS, count and sum in one word.
//  4. The table's non-zero entries go to global memory with 64-bit atomic adds (vector instructions), once per block and chunk pair.
// Reads what k_mosaic_frames<uint8_t, C> reads of the same tile, through the same mos_covers / mos_fetch.
template <int C>
__global__ __launch_bounds__(256) void k_mosaic_stats(const MosaicFrame4 *__restrict__ frames, int n_frames, const uint8_t *__restrict__ coords,
                                                      const uint8_t *__restrict__ pixels, int cx, int cy, int cw, int ch, uint32_t tiles_x,
                                                      unsigned long long *__restrict__ stats)
{
    constexpr uint32_t K = MOS_STAT_K;
    __shared__ uint16_t s_list[256];                              // (n_frames <= 256)
    __shared__ uint32_t s_n;
    __shared__ uint32_t s_tab[K * K];
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t i0 = (int64_t)tx * 64, j0 = (int64_t)ty * 4;
    const int64_t X0 = cx + i0, Y0 = cy + j0, X1 = min(X0 + 64, (int64_t)cx + cw), Y1 = min(Y0 + 4, (int64_t)cy + ch);
    const uint32_t lane = threadIdx.x, wave = threadIdx.y, t = wave * 64 + lane;
    const int64_t i = i0 + lane, j = j0 + wave;
    const bool inb = i < cw && j < ch;
    const int64_t X = cx + i, Y = cy + j;
    if (wave == 0) {
        uint32_t n = 0;
        for (int base = 0; base < n_frames; base += 64) {
            const int f = base + (int)lane;
            const bool hit = f < n_frames && mos_hits(frames[f >> 2].f[f & 3], X0, X1, Y0, Y1);
            const uint64_t m = __ballot(hit);
            if (hit) s_list[n + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint16_t)f;
            n += (uint32_t)__builtin_popcountll(m);
        }
        if (lane == 0) s_n = n;
    }
    __syncthreads();
    const uint32_t n_hit = s_n;                                   // (<= n_frames <= 256)
    for (uint32_t b0 = 0; b0 < n_hit; b0 += K) {
        const uint32_t nb = min(K, n_hit - b0);
        uint64_t mine = 0;                                        // lane k: the lanes of this wave that frame b0 + k of the list contributes to
        for (uint32_t kb = 0; kb < nb; kb++) {
            const uint32_t f = mos_uniform(s_list[b0 + kb]);
            float2 s;
            uint64_t k;
            const uint64_t m = __ballot(inb && mos_covers(frames[f >> 2].f[f & 3], X, Y, coords, &s, &k));      // (the contributor bit alone: no pixel is read)
            if (lane == kb) mine = m;
        }
        for (uint32_t a0 = 0; a0 < n_hit; a0 += K) {
            const uint32_t na = min(K, n_hit - a0);
            for (uint32_t e = t; e < na * K; e += 256) s_tab[e] = 0;
            __syncthreads();
            for (uint32_t ka = 0; ka < na; ka++) {
                const uint32_t f = mos_uniform(s_list[a0 + ka]);
                float2 s;
                uint32_t p[C];
                const bool con = inb && mos_fetch<uint8_t, C>(frames[f >> 2].f[f & 3], X, Y, coords, pixels, &s, p);
                const uint64_t ma = __ballot(con);
                if (!ma) continue;                                // (uniform over the wave)
                uint32_t v = 0;
                if (con) {
#pragma unroll
                    for (int c = 0; c < mos_stat_channels(C); c++) v += p[c];
                }
                const uint32_t sa = mos_wave_sum(v);
                const uint64_t m = lane < nb ? ma & mine : 0;
                uint32_t sum = sa;
                uint64_t part = __ballot(m != 0 && m != ma);      // the columns whose overlap with a splits this wave
                while (part) {
                    const int kb = __builtin_ctzll(part);
                    part &= part - 1;
                    const uint64_t mk = __shfl(m, kb);
                    const uint32_t sk = mos_wave_sum((mk >> lane) & 1 ? v : 0u);
                    if (lane == (uint32_t)kb) sum = sk;
                }
                if (m) atomicAdd(&s_tab[ka * K + lane], ((uint32_t)__builtin_popcountll(m) << MOS_STAT_SUM_BITS) | sum);
            }
            __syncthreads();
            for (uint32_t e = t; e < na * K; e += 256) {
                const uint32_t w = s_tab[e], kb = e % K;
                if (!w) continue;                                 // (columns >= nb were zeroed and never added to)
                const uint64_t at = ((uint64_t)s_list[a0 + e / K] * (uint32_t)n_frames + s_list[b0 + kb]) * 2;
                atomicAdd(stats + at, (unsigned long long)(w >> MOS_STAT_SUM_BITS));
                if (w & ((1u << MOS_STAT_SUM_BITS) - 1u)) atomicAdd(stats + at + 1, (unsigned long long)(w & ((1u << MOS_STAT_SUM_BITS) - 1u)));
            }
            __syncthreads();                                      // (the table is zeroed again for the next chunk pair)
        }
    }
}

// ------------------------------------------------------------------------------------------------ launcher
#ifdef __HIPCC__
void launch_mosaic_stats(const MosaicFrame4 *frames, int n_frames, const uint8_t *coords, const uint8_t *pixels, int channels, int cx, int cy, int cw,
                         int ch, uint64_t *stats, hipStream_t stream)
{
    if (cw <= 0 || ch <= 0 || n_frames <= 0) return;
    const uint32_t tiles_x = (uint32_t)(((int64_t)cw + 63) / 64);
    const uint64_t n_blocks = (uint64_t)tiles_x * (uint64_t)(((int64_t)ch + 3) / 4);      // (< 2^31 for a canvas of at most 2^31 pixels)
    for_elem_channels(1, channels, [&](auto, auto c) {
        hipLaunchKernelGGL((k_mosaic_stats<decltype(c)::value>), dim3((uint32_t)n_blocks), dim3(64, 4), 0, stream, frames, n_frames, coords, pixels, cx, cy, cw, ch,
                           tiles_x, reinterpret_cast<unsigned long long *>(stats));
    });
}
#endif

} // namespace hg
