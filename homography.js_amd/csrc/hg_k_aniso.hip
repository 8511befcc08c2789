// hg_k_aniso.hip -- the anisotropic remap on the field seam (include/hgwarp.h, hg_remap_aniso_frames_device): k_remap_aniso_frames gathers a
// plane and its pyramid through a HG_FIELD_COORDS field as k_remap_trilinear_frames does, but takes N probes along the longer of the
// field's two steps, from the finer level(s) the shorter step allows, and averages them.
// Hand-written HIP for gfx950 (MI355X / CDNA4), wave64.  All arithmetic is f32 in the written order (contraction off); the numpy model of
// tests/hgtest/aniso.py follows it operation by operation.  Design notes: DESIGN.md §4.9, figures: EXPERIMENTS.md F.6.
#ifdef __HIPCC__
#include "hg_dev.h"
#endif
#include "hg_remap_dev.h"

namespace hg {

// k_remap_trilinear_frames' tri_sample_level with ONE tri_sample body for every level: the level's start, size and coordinate are selected
// first.  lvl_off[0] is 0 and level 0's start is the plane; pyr is only offset, never read, for k == 0.
template <typename E, int C>
__device__ __forceinline__ void aniso_sample_level(const E *__restrict__ plane, bool plane_wide, const uint8_t *__restrict__ pyr, bool pyr_wide,
                                                   const uint64_t *__restrict__ lvl_off, int W, int H, int k, float2 s, float r[C])
{
    const bool base = k == 0;
    const float inv = __uint_as_float((uint32_t)(127 - k) << 23);
    const float u = base ? s.x : ((s.x + 0.5f) * inv) - 0.5f, v = base ? s.y : ((s.y + 0.5f) * inv) - 0.5f;
    const E *__restrict__ lv = base ? plane : reinterpret_cast<const E *>(pyr + lvl_off[k]);
    tri_sample<E, C>(lv, base ? plane_wide : pyr_wide, pyr_size(W, k), pyr_size(H, k), u, v, r);
}

// One pixel per lane over the frame's flat list, read as obj_w x obj_h: the grid, the block search, the records and the level offsets are
// k_remap_trilinear_frames'.  The two steps of pixel (i, j) are LOADED as there.  The longer one is the major axis (the
// horizontal one on a tie), N = the smallest n <= max_aniso with n^2 * max(q_minor, 1) >= q_major probes are spread along it at the
// offsets ((p + 0.5) / N) - 0.5, and the level(s) come from q' = q_major / N^2 by the trilinear rule.  Every probe is the trilinear
// sample at its position; their sum in ascending p, divided by N, is the pixel.  N == 1 (max_aniso == 1, or nothing to gain): the
// trilinear pixel, bit for bit.  The probe loop's trip count is per lane; it keeps its state in registers (no array is indexed by p or
// by the level), and both levels of a probe run through one inlined body of the sampler.
template <typename E, int C>
__global__ __launch_bounds__(256) void k_remap_aniso_frames(const TriRemapFrame *__restrict__ frames, int n_frames, uint64_t blk_px,
                                                            const uint64_t *__restrict__ lvl_off, int levels, int max_aniso,
                                                            const uint8_t *__restrict__ coords, const uint8_t *__restrict__ planes,
                                                            const uint8_t *__restrict__ pyrs, int W, int H, uint8_t *__restrict__ out)
{
    const TriRemapFrame fr = remap_frame_of(frames, n_frames, blockIdx.x);
    const float2 *__restrict__ cf = reinterpret_cast<const float2 *>(coords + fr.fld_off);
    const E *__restrict__ src = reinterpret_cast<const E *>(planes + fr.plane_off);
    const uint8_t *__restrict__ pyr = pyrs + fr.pyr_off;           // (never read with levels == 1)
    E *__restrict__ o = reinterpret_cast<E *>(out + fr.out_off);
    const uint64_t p0 = (uint64_t)(blockIdx.x - fr.blk0) * blk_px;
    const uint64_t end = min(fr.n_px, p0 + blk_px);
    constexpr bool kBytes = sizeof(E) == 1 && (C == 2 || C == 4);
    const bool src_wide = kBytes && !(reinterpret_cast<uintptr_t>(src) & (C - 1));
    const bool pyr_wide = kBytes && !(reinterpret_cast<uintptr_t>(pyr) & (C - 1));      // (level offsets are multiples of 256)
    const bool out_wide = kBytes && !(reinterpret_cast<uintptr_t>(o) & (C - 1));
    const uint64_t ow = fr.obj_w, oh = fr.obj_h;
    const uint64_t row0 = p0 / ow, col0 = p0 - row0 * ow;        // (uniform over the block)
    for (uint64_t i = p0 + threadIdx.x; i < end; i += 256) {
        uint64_t px, py;
        remap_px_xy(col0 + (i - p0), ow, row0, &px, &py);
        const float2 s = cf[i];
        float v[C];
#pragma unroll
        for (int ch = 0; ch < C; ch++) v[ch] = 0.0f;
        if (remap_finite(s)) {
            float hx, hy, vx, vy;
            const float qh = remap_step(cf, s, px + 1 < ow, i + 1, px >= 1, i - 1, &hx, &hy);
            const float qv = remap_step(cf, s, py + 1 < oh, i + ow, py >= 1, i - ow, &vx, &vy);
            const bool hmaj = qh >= qv;
            const float mx = hmaj ? hx : vx, my = hmaj ? hy : vy, qM = hmaj ? qh : qv, qm = hmaj ? qv : qh;
            int N = 1;
            if (qM > 1.0f && qM < INFINITY) {
                const float qmc = fmaxf(qm, 1.0f);
                while (N < max_aniso && !((float)(N * N) * qmc >= qM)) N++;
            }
            const float fN = (float)N;
            const float q = N > 1 ? qM / (float)(N * N) : qM;      // (x / 1.0f is x)
            const RemapLevels lv = remap_levels(q, levels);
            const int k = lv.k, nl = lv.n;
            const float w = lv.w;                                  // weight of level k + 1
            for (int p = 0; p < N; p++) {
                float2 pr = s;
                if (N > 1) {
                    const float off = (((float)p + 0.5f) / fN) - 0.5f;
                    pr.x = s.x + mx * off; pr.y = s.y + my * off;
                }
                float r[C];
#pragma unroll 1
                for (int l = 0; l < nl; l++) {
                    float smp[C];
                    aniso_sample_level<E, C>(src, src_wide, pyr, pyr_wide, lvl_off, W, H, k + l, pr, smp);
#pragma unroll
                    for (int ch = 0; ch < C; ch++) r[ch] = l == 0 ? smp[ch] : r[ch] + (smp[ch] - r[ch]) * w;
                }
#pragma unroll
                for (int ch = 0; ch < C; ch++) v[ch] = p == 0 ? r[ch] : v[ch] + r[ch];
            }
            if (N > 1) {
#pragma unroll
                for (int ch = 0; ch < C; ch++) v[ch] = v[ch] / fN;
            }
        }
        remap_px_store<E, C>(o, i, out_wide, v);
    }
}

// ------------------------------------------------------------------------------------------------ launcher
#ifdef __HIPCC__
void launch_remap_aniso_frames(const TriRemapFrame *frames, int n_frames, uint32_t n_blocks, uint64_t blk_px, const uint64_t *lvl_off, int levels,
                               int max_aniso, const uint8_t *coords, const uint8_t *planes, const uint8_t *pyrs, int W, int H, int elem, int channels,
                               uint8_t *out, hipStream_t stream)
{
    if (n_frames <= 0 || n_blocks == 0) return;
    for_elem_channels(elem, channels, [&](auto e, auto c) {
        hipLaunchKernelGGL((k_remap_aniso_frames<decltype(e), decltype(c)::value>), dim3(n_blocks), dim3(256), 0, stream, frames, n_frames, blk_px, lvl_off, levels,
                           max_aniso, coords, planes, pyrs, W, H, out);
    });
}
#endif

} // namespace hg
