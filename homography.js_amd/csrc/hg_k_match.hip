// hg_k_match.hip -- matching feature descriptors of frame sets (include/hgwarp.h, "matching descriptors"):
//   k_match_bits<W>   binary descriptors.  One workgroup (one wavefront) per (frame, kMatchTQ rows of side A): every lane keeps ITS row in W
//                     registers as 32-bit words; the rows of side B go through LDS in tiles of kMatchTT and every lane reads the same row in a
//                     step (a broadcast); distance = popcount of the XOR per word; the running two nearest stay in two registers as packed words.
//   k_match_u8<KS>    byte descriptors on the matrix cores.  One workgroup of four wavefronts per (frame, kMatchTQ rows of A), 16 rows per
//                     wavefront as the A fragments of v_mfma_i32_16x16x64_i8 (KS k-steps of 64 bytes, in registers); the rows of B go through
//                     LDS in tiles of kMatchTT = 4 column blocks of 16.  |a - b|^2 = |a|^2 + |b|^2 - 2 a.b on bytes shifted by -128 (b ^ 0x80 as
//                     i8; the difference is unchanged), every partial sum an exact int32.  The epilogue folds the 16 lanes that share a row.
//   k_match_finish    one workgroup per frame: the distance cap, the ratio test and the cross-check, d_nn, a block prefix scan over the accept
//                     flags in query order, the compacted pairs and match slots, the padding, the count.
// Side A is the side whose rows get an answer, side B the one searched: A = query, B = train for the two nearest of every query.  Frame f
// reads list f % sets of either side.  The record a launch leaves per row of A is {j1, d1, d2, 0} (hg_match_dev.h: MatchTop2).
// The cross-check needs the best query of every train row.  Two forms, each kind on the one that measured faster (EXPERIMENTS.md,
// "Matching"): a second launch of the same kernel with the sides swapped (bits; and bytes under option "match_cross" 0), or, inside the one
// launch, a 64-bit atomicMin per train row on the word (d << 32) | i -- a total order, so the winner does not depend on scheduling --
// after the minimum over the workgroup's 64 rows was taken in registers and LDS (bytes: k_match_u8 with `keys`).
// The rules live in hg_match_dev.h.  k_match_bits and k_match_finish need that header only, so a host check compiles this file behind a
// thread-index shim (tests/cpp/match_check.cpp); the matrix-core kernel and the launcher are compiled under hipcc only.
#ifdef __HIPCC__
#include "hg_kernels.h"
#endif
#include "hg_match_dev.h"

namespace hg {

// The 16-byte chunk c of a descriptor row as four words: bytes at and beyond desc_bytes (padding, which may hold anything) become 0, data
// bytes are XORed with `flip` (0 for bits; 0x80808080 for bytes: b - 128 as i8).  A chunk that holds no data byte is not read.
__device__ __forceinline__ uint4 match_load_chunk(const uint8_t *__restrict__ row, int c, int desc_bytes, uint32_t flip)
{
    const int off = c * 16;
    if (off >= desc_bytes) return make_uint4(0u, 0u, 0u, 0u);
    const uint4 v = *reinterpret_cast<const uint4 *>(row + off);             // (stride is a multiple of 16 and >= desc_bytes: inside the row)
    return make_uint4((v.x ^ flip) & match_word_mask(desc_bytes, off), (v.y ^ flip) & match_word_mask(desc_bytes, off + 4),
                      (v.z ^ flip) & match_word_mask(desc_bytes, off + 8), (v.w ^ flip) & match_word_mask(desc_bytes, off + 12));
}

// ------------------------------------------------------------------------------------------------ k_match_bits
template <int W>
__global__ __launch_bounds__(kMatchTQ) void k_match_bits(const uint8_t *__restrict__ A, int n_a, int a_sets, const int32_t *__restrict__ cnt_a,
                                                         const uint8_t *__restrict__ B, int n_b, int b_sets, const int32_t *__restrict__ cnt_b,
                                                         int desc_bytes, size_t stride, uint4 *__restrict__ out)
{
    constexpr int C = W / 4;                                     // 16-byte chunks per row
    __shared__ uint4 tile[kMatchTT * C];
    const int f = blockIdx.y, base = blockIdx.x * kMatchTQ, tid = threadIdx.x;
    const int la = f % a_sets, lb = f % b_sets;
    const int ca = cnt_a[la], cb = cnt_b[lb];
    if (base >= ca) return;                                      // (uniform over the workgroup)
    const int i = base + tid;
    const bool live = i < ca;
    const uint8_t *__restrict__ arow = A + ((size_t)la * n_a + (live ? i : base)) * stride;
    uint32_t q[W];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint4 v = match_load_chunk(arow, c, desc_bytes, 0u);
        q[4 * c] = v.x; q[4 * c + 1] = v.y; q[4 * c + 2] = v.z; q[4 * c + 3] = v.w;
    }
    const uint8_t *__restrict__ bl = B + (size_t)lb * n_b * stride;
    MatchKeys2 top = match_keys2_empty();                        // words (d << 16) | j: d <= 4096, j < 65536
    for (int jb = 0; jb < cb; jb += kMatchTT) {
        const int n = min(kMatchTT, cb - jb);
        for (int k = tid; k < kMatchTT * C; k += kMatchTQ) {
            const int r = k / C, c = k % C;
            tile[k] = r < n ? match_load_chunk(bl + (size_t)(jb + r) * stride, c, desc_bytes, 0u) : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        for (int r = 0; r < n; r++) {
            uint32_t d = 0;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const uint4 t = tile[r * C + c];
                d += __popc(q[4 * c] ^ t.x) + __popc(q[4 * c + 1] ^ t.y) + __popc(q[4 * c + 2] ^ t.z) + __popc(q[4 * c + 3] ^ t.w);
            }
            match_push(top, (d << 16) | (uint32_t)(jb + r));
        }
        __syncthreads();
    }
    const MatchTop2 t2 = match_unpack(top, 16, 0);
    if (live) out[(size_t)f * n_a + i] = make_uint4((uint32_t)t2.j1, t2.d1, t2.d2, 0u);
}

// ------------------------------------------------------------------------------------------------ k_match_u8
#ifdef __HIPCC__
typedef int match_i32x4 __attribute__((ext_vector_type(4)));
constexpr int kMatchU8Block = 256;                               // four wavefronts of 16 rows of A each

// Sum of squares of the sixteen i8 of a chunk: v_dot4_i32_i8 of every word with itself, exact in int32.
__device__ __forceinline__ int32_t match_sumsq(const uint4 v)
{
    int32_t s = __builtin_amdgcn_sdot4((int)v.x, (int)v.x, 0, false);
    s = __builtin_amdgcn_sdot4((int)v.y, (int)v.y, s, false);
    s = __builtin_amdgcn_sdot4((int)v.z, (int)v.z, s, false);
    return __builtin_amdgcn_sdot4((int)v.w, (int)v.w, s, false);
}

template <int KS>
__global__ __launch_bounds__(kMatchU8Block) void k_match_u8(const uint8_t *__restrict__ A, int n_a, int a_sets, const int32_t *__restrict__ cnt_a,
                                                            const uint8_t *__restrict__ B, int n_b, int b_sets, const int32_t *__restrict__ cnt_b,
                                                            int desc_bytes, size_t stride, uint4 *__restrict__ out, unsigned long long *__restrict__ keys)
{
    static_assert(kMatchTQ == 64 && kMatchTT == 64, "four wavefronts of 16 rows; four column blocks of 16");
    constexpr int C = KS * 4;                                    // 16-byte chunks of data per row (K padded to KS * 64 with zeros on BOTH sides)
    constexpr int RS = C + 1;                                    // the LDS row stride in chunks: one chunk of padding spreads the rows over the banks
    __shared__ uint4 tile[kMatchTT * RS];
    __shared__ int32_t tnorm[kMatchTT];
    __shared__ uint32_t best_a[kMatchTT];                        // with keys: per row of B in the tile, the smallest (d << 6) | row of this workgroup
    const int f = blockIdx.y, base = blockIdx.x * kMatchTQ, tid = threadIdx.x;
    const int la = f % a_sets, lb = f % b_sets;
    const int ca = cnt_a[la], cb = cnt_b[lb];
    if (base >= ca) return;                                      // (uniform over the workgroup)
    const int lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;                   // the row (A) resp. column (B) this lane feeds, and its 16 bytes of every k-step
    // The A fragments.  Both operands are loaded by ONE lane -> k rule (bytes 16 kg .. 16 kg + 15 of k-step ks), so whichever k the hardware
    // gives a lane's bytes, a and b meet at the same k; only the row / column maps have to be right.
    const int ai = base + wave * 16 + r16;
    const uint8_t *__restrict__ arow = A + ((size_t)la * n_a + (ai < ca ? ai : base)) * stride;
    match_i32x4 afrag[KS];
    int32_t qs = 0;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
        const uint4 v = match_load_chunk(arow, ks * 4 + kg, desc_bytes, 0x80808080u);
        afrag[ks] = match_i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        qs += match_sumsq(v);
    }
    qs += __shfl_xor(qs, 16);
    qs += __shfl_xor(qs, 32);                                    // |a|^2 of row r16, in all four lanes that hold a part of it
    int32_t qn[4];                                               // ... of the rows this lane's accumulators belong to: row = 4 kg + reg
#pragma unroll
    for (int reg = 0; reg < 4; reg++) qn[reg] = __shfl(qs, kg * 4 + reg);
    const uint8_t *__restrict__ bl = B + (size_t)lb * n_b * stride;
    MatchTop2 top[4];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) top[reg] = match_top2_empty();
    for (int jb = 0; jb < cb; jb += kMatchTT) {
        const int n = min(kMatchTT, cb - jb);
        for (int k = tid; k < kMatchTT * C; k += kMatchU8Block) {
            const int r = k / C, c = k % C;
            tile[r * RS + c] = r < n ? match_load_chunk(bl + (size_t)(jb + r) * stride, c, desc_bytes, 0x80808080u) : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        {                                                        // |b|^2 of the tile's rows: four lanes per row
            const int r = tid >> 2, part = tid & 3;
            int32_t s = 0;
            for (int c = part; c < C; c += 4) s += match_sumsq(tile[r * RS + c]);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            if (part == 0) { tnorm[r] = s; best_a[r] = kMatchNone; }
        }
        __syncthreads();
        MatchKeys2 tk[4];                                        // the tile's two nearest per row of A: words (d << 6) | column, d < 2^25
#pragma unroll
        for (int reg = 0; reg < 4; reg++) tk[reg] = match_keys2_empty();
#pragma unroll
        for (int blk = 0; blk < kMatchTT / 16; blk++) {
            if (blk * 16 < n) {                                  // (uniform)
                const int col = blk * 16 + r16;
                match_i32x4 acc = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ks++) {
                    const uint4 v = tile[col * RS + ks * 4 + kg];
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afrag[ks], match_i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w}, acc, 0, 0, 0);
                }
                // C/D: column = lane & 15, row = 4 (lane >> 4) + reg
                if (col < n) {
                    const int32_t tn = tnorm[col];
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) match_push(tk[reg], ((uint32_t)((qn[reg] + tn) - 2 * acc[reg]) << 6) | (uint32_t)col);
                }
                if (keys) {                                      // (uniform) the nearest row of A for this column: the lane's 4 rows, the 4 lanes of the column, the 4 wavefronts
                    uint32_t m = kMatchNone;
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const int row = wave * 16 + kg * 4 + reg;
                        const uint32_t k = base + row < ca ? ((uint32_t)((qn[reg] + tnorm[col]) - 2 * acc[reg]) << 6) | (uint32_t)row : kMatchNone;
                        m = k < m ? k : m;
                    }
                    uint32_t o = (uint32_t)__shfl_xor((int)m, 16); m = o < m ? o : m;
                    o = (uint32_t)__shfl_xor((int)m, 32); m = o < m ? o : m;
                    if (kg == 0 && col < n) atomicMin(&best_a[col], m);
                }
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) match_merge(top[reg], match_unpack(tk[reg], 6, jb));
        __syncthreads();
        if (keys && tid < n && best_a[tid] != kMatchNone)
            atomicMin(&keys[(size_t)f * n_b + jb + tid], match_key(best_a[tid] >> 6, (uint32_t)base + (best_a[tid] & 63u)));
    }
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) {                       // the 16 lanes that share a row of A: any fold order gives the same record
            MatchTop2 o;
            o.d1 = (uint32_t)__shfl_xor((int)top[reg].d1, s);
            o.j1 = __shfl_xor(top[reg].j1, s);
            o.d2 = (uint32_t)__shfl_xor((int)top[reg].d2, s);
            match_merge(top[reg], o);
        }
        const int i = base + wave * 16 + kg * 4 + reg;
        if (r16 == 0 && i < ca) out[(size_t)f * n_a + i] = make_uint4((uint32_t)top[reg].j1, top[reg].d1, top[reg].d2, 0u);
    }
}
#endif

// ------------------------------------------------------------------------------------------------ k_match_finish
// fwd = n_frames x n_query records of the queries; the best query of the train rows comes as rev = n_frames x n_train records (the swapped
// launch) or as keys = n_frames x n_train words (d << 32) | i (the atomic form), both nullptr: no cross-check; none is read for a frame
// without train rows.  The points are copied as bits.
__global__ __launch_bounds__(kMatchFinishBlock) void k_match_finish(int n_query, int n_train, int n_train_sets, const int32_t *__restrict__ counts_q,
                                                                    const int32_t *__restrict__ counts_t, const uint4 *__restrict__ fwd,
                                                                    const uint4 *__restrict__ rev, const unsigned long long *__restrict__ keys, uint32_t max_distance, int ratio_on, double rr,
                                                                    const uint2 *__restrict__ qpts, const uint2 *__restrict__ tpts,
                                                                    int32_t *__restrict__ out_counts, uint4 *__restrict__ out_matches,
                                                                    int32_t *__restrict__ out_pairs, int32_t *__restrict__ out_nn)
{
    __shared__ int32_t scan[kMatchFinishBlock];
    const int f = blockIdx.x, tid = threadIdx.x, ts = f % n_train_sets;
    const int cq = counts_q[f], ct = counts_t[ts];
    const size_t q0 = (size_t)f * n_query;
    int total = 0;
    for (int base = 0; base < n_query; base += kMatchFinishBlock) {              // (every lane walks every step: the scan's barriers)
        const int i = base + tid;
        int32_t j1 = -1, d1 = -1, d2 = -1;
        bool ok = false;
        if (i < cq && ct >= 1) {
            const uint4 r = fwd[q0 + i];
            const MatchTop2 t{r.y, (int32_t)r.x, r.z};
            j1 = t.j1; d1 = (int32_t)t.d1; d2 = ct >= 2 ? (int32_t)t.d2 : -1;
            ok = match_passes(t, ct, max_distance, ratio_on, rr);
            if (ok && rev) ok = (int32_t)rev[(size_t)f * n_train + j1].x == i;
            if (ok && keys) ok = (int32_t)(uint32_t)keys[(size_t)f * n_train + j1] == i;
        }
        if (out_nn && i < n_query) {
            int32_t *o = out_nn + (q0 + i) * 4;
            o[0] = j1; o[1] = d1; o[2] = d2; o[3] = ok ? 1 : 0;
        }
        scan[tid] = ok ? 1 : 0;                                                  // inclusive prefix sum of the flags, in query order
        __syncthreads();
        for (int s = 1; s < kMatchFinishBlock; s <<= 1) {
            const int32_t v = tid >= s ? scan[tid - s] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int k = total + scan[tid] - 1;
        total += scan[kMatchFinishBlock - 1];
        __syncthreads();
        if (ok) {
            if (out_pairs) { out_pairs[(q0 + k) * 2] = i; out_pairs[(q0 + k) * 2 + 1] = j1; }
            if (out_matches) {
                const uint2 p = qpts[q0 + i], t = tpts[(size_t)ts * n_train + j1];
                out_matches[q0 + k] = make_uint4(p.x, p.y, t.x, t.y);
            }
        }
    }
    for (int k = total + tid; k < n_query; k += kMatchFinishBlock) {             // the slots no pair fills
        if (out_pairs) { out_pairs[(q0 + k) * 2] = -1; out_pairs[(q0 + k) * 2 + 1] = -1; }
        if (out_matches) out_matches[q0 + k] = make_uint4(0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0x7fc00000u);
    }
    if (tid == 0) out_counts[f] = total;
}

// ------------------------------------------------------------------------------------------------ launches
#ifdef __HIPCC__
// The records of every row of side A against side B, on the kernel of the kind and of the descriptor length.
static void launch_match_side(const MatchArgs &a, const uint8_t *A, int n_a, int a_sets, const int32_t *cnt_a, const uint8_t *B, int n_b, int b_sets,
                              const int32_t *cnt_b, uint4 *out, unsigned long long *keys, hipStream_t stream)
{
    const dim3 grid((n_a + kMatchTQ - 1) / kMatchTQ, a.n_frames);
#define HG_MATCH_LAUNCH(K, BLOCK, ...) hipLaunchKernelGGL(K, grid, dim3(BLOCK), 0, stream, A, n_a, a_sets, cnt_a, B, n_b, b_sets, cnt_b, a.desc_bytes, a.stride, out, ##__VA_ARGS__)
    if (a.kind == 0) {                                           // (keys: the matrix-core kernel only -- for bits the swapped launch measured faster)
        const int words = (a.desc_bytes + 3) / 4;
        if (words <= 8) HG_MATCH_LAUNCH(k_match_bits<8>, kMatchTQ);
        else if (words <= 16) HG_MATCH_LAUNCH(k_match_bits<16>, kMatchTQ);
        else if (words <= 32) HG_MATCH_LAUNCH(k_match_bits<32>, kMatchTQ);
        else HG_MATCH_LAUNCH(k_match_bits<128>, kMatchTQ);
    } else {
        const int steps = (a.desc_bytes + 63) / 64;
        if (steps <= 1) HG_MATCH_LAUNCH(k_match_u8<1>, kMatchU8Block, keys);
        else if (steps <= 2) HG_MATCH_LAUNCH(k_match_u8<2>, kMatchU8Block, keys);
        else if (steps <= 4) HG_MATCH_LAUNCH(k_match_u8<4>, kMatchU8Block, keys);
        else HG_MATCH_LAUNCH(k_match_u8<8>, kMatchU8Block, keys);
    }
#undef HG_MATCH_LAUNCH
}

void launch_match(const MatchArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0) return;
    const uint8_t *q = static_cast<const uint8_t *>(a.query), *t = static_cast<const uint8_t *>(a.train);
    const bool work = a.n_query > 0 && a.n_train > 0;
    if (work) {
        launch_match_side(a, q, a.n_query, a.n_frames, a.counts_q, t, a.n_train, a.n_train_sets, a.counts_t, a.ws_fwd, a.cross_check == 2 ? a.ws_keys : nullptr, stream);
        if (a.cross_check == 1) launch_match_side(a, t, a.n_train, a.n_train_sets, a.counts_t, q, a.n_query, a.n_frames, a.counts_q, a.ws_rev, nullptr, stream);
    }
    hipLaunchKernelGGL(k_match_finish, dim3(a.n_frames), dim3(kMatchFinishBlock), 0, stream, a.n_query, a.n_train, a.n_train_sets, a.counts_q, a.counts_t,
                       a.ws_fwd, (work && a.cross_check == 1) ? a.ws_rev : nullptr, (work && a.cross_check == 2) ? a.ws_keys : nullptr, a.max_distance, a.ratio_on, a.rr,
                       static_cast<const uint2 *>(a.query_pts), static_cast<const uint2 *>(a.train_pts), a.out_counts,
                       static_cast<uint4 *>(a.out_matches), a.out_pairs, a.out_nn);
}
#endif

} // namespace hg
