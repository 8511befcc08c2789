// remap_frames_check.cpp -- host check of the frame-set remap kernels (k_remap_index_frames, k_remap_bilinear_frames; hg_k_remap.hip).
// The kernel file itself is compiled for the CPU behind the thread-index shim (hip_host_shim.h) and run block by block, thread by thread,
// under AddressSanitizer + UndefinedBehaviorSanitizer: exact-size heap buffers, so any byte read or written outside a field, a plane, the
// frame table or the output is reported, and so is a misaligned wide load or store.  Results are compared with a plain scalar loop on the
// ragged frame set of tests/test_gpu_remap_frames.py (pixel counts 1, 3, 4, 5, 0, 255, 257, 1021, 60000), packed and deliberately misaligned
// layouts, 1 and 3 planes, both kernel forms, all pixel sizes / element types / channel counts, and 65535 one-pixel frames.
// A stand-alone program: host code only, no GPU.
#include "hip_host_shim.h"
#include "hg_k_remap.hip"
using namespace hg;

static uint32_t rng_s = 12345;
static uint32_t rnd() { rng_s = rng_s * 1664525u + 1013904223u; return rng_s >> 8; }

template <typename F> static void run_grid(uint32_t n_blocks, F f)
{
    for (uint32_t b = 0; b < n_blocks; b++) for (unsigned t = 0; t < 256; t++) { blockIdx = {b, 0, 0}; threadIdx = {t, 0, 0}; f(); }
}

static void blocks(std::vector<RemapFrame> &r, uint64_t px, uint32_t *nb) { uint64_t b = 0; for (auto &x : r) { x.blk0 = (uint32_t)b; b += (x.n_px + px - 1) / px; } *nb = (uint32_t)b; }

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf(__VA_ARGS__); printf("\n"); } } while (0)

static const uint64_t NPX[9] = {1, 3, 4, 5, 0, 255, 257, 1021, 60000};
static const int W = 97, H = 61;
static const size_t NSRC = (size_t)W * H;

template <typename T, bool PACK> static void index_case(int misalign, int n_planes, uint64_t blk_px)
{
    const size_t pb = sizeof(T);
    std::vector<RemapFrame> fr(9);
    size_t fo = 0, oo = 0;
    for (int f = 0; f < 9; f++) {
        fr[f] = {fo + (misalign ? 4 * (f % 3 + 1) : 0), oo + (misalign ? pb * (2 * f + 1) : 0), NPX[f], 0, (uint32_t)(f % n_planes)};
        fo += ((NPX[f] * 4 + 255) & ~255ull) + (misalign ? 512 : 0); oo += ((NPX[f] * pb + 255) & ~255ull) + (misalign ? 512 : 0);
    }
    uint32_t nb; blocks(fr, blk_px, &nb);
    const size_t stride = NSRC * pb + (misalign ? pb : 0);
    // exact-size heap buffers: ASan sees any byte read or written beyond them
    uint8_t *fld = (uint8_t *)aligned_alloc(16, (fo + 15) & ~15ull), *pl = (uint8_t *)aligned_alloc(16, (stride * n_planes + 15) & ~15ull);
    uint8_t *out = (uint8_t *)aligned_alloc(16, (oo + 15) & ~15ull), *ref = (uint8_t *)malloc(oo);
    memset(fld, 0x11, fo); memset(out, 0xA5, oo); memset(ref, 0xA5, oo);
    for (size_t i = 0; i < stride * n_planes; i++) pl[i] = 1 + rnd() % 150;
    for (int f = 0; f < 9; f++) {
        int32_t *p = (int32_t *)(fld + fr[f].fld_off);
        for (uint64_t i = 0; i < NPX[f]; i++) p[i] = (int32_t)(rnd() % (NSRC + 4)) - 2;
        if (NPX[f] >= 255) { p[0] = -1; p[1] = (int32_t)NSRC; p[2] = INT32_MIN; p[3] = INT32_MAX; p[4] = 0; p[5] = (int32_t)NSRC - 1; }
        for (uint64_t i = 0; i < NPX[f]; i++) {
            uint8_t *o = ref + fr[f].out_off + i * pb;
            if (p[i] >= 0 && (size_t)p[i] < NSRC) memcpy(o, pl + fr[f].plane * stride + (size_t)p[i] * pb, pb); else memset(o, 0, pb);
        }
    }
    std::vector<RemapFrame> tab = fr;                          // exact-size table
    run_grid(nb, [&] { k_remap_index_frames<T, PACK>(tab.data(), 9, blk_px, fld, pl, NSRC, stride, out); });
    CHECK(!memcmp(out, ref, oo), "index pb=%zu pack=%d misalign=%d planes=%d blk=%llu: output differs", pb, (int)PACK, misalign, n_planes, (unsigned long long)blk_px);
    free(fld); free(pl); free(out); free(ref);
}

static float ref_blend(const float *p00, const float *p01, const float *p10, const float *p11, float gx, float fx, float gy, float fy)
{
    volatile float a = *p00 * gx, b = *p01 * fx; volatile float t = a + b; volatile float top = t * gy;
    volatile float c = *p10 * gx, d = *p11 * fx; volatile float u = c + d; volatile float bot = u * fy;
    volatile float v = top + bot; return v;
}
static int ref_tap(float v, int n) { float c = v < 0 ? 0 : v; if (c > 2147483520.0f) c = 2147483520.0f; int64_t i = (int64_t)c; return (int)std::min<int64_t>(i, n - 1); }

template <typename E, int C> static void bilinear_case(int misalign, int n_planes, bool single)
{
    const size_t es = sizeof(E), px = es * C;
    const int F = single ? 1 : 9;
    std::vector<RemapFrame> fr(F);
    size_t fo = 0, oo = 0;
    for (int f = 0; f < F; f++) {
        const uint64_t n = single ? 1021 : NPX[f];
        fr[f] = {fo + (misalign ? 8 * (2 * f + 1) : 0), oo + (misalign ? es * (2 * f + 1) : 0), n, 0, (uint32_t)(f % n_planes)};
        fo += ((n * 8 + 255) & ~255ull) + (misalign ? 512 : 0); oo += ((n * px + 255) & ~255ull) + (misalign ? 512 : 0);
    }
    uint32_t nb; blocks(fr, 1024, &nb);
    const size_t stride = NSRC * px + (misalign ? 3 * es : 0), front = misalign ? es : 0;
    uint8_t *fld = (uint8_t *)aligned_alloc(16, (fo + 15) & ~15ull), *plbuf = (uint8_t *)aligned_alloc(16, (front + stride * n_planes + 15) & ~15ull), *pl = plbuf + front;
    uint8_t *out = (uint8_t *)aligned_alloc(16, (oo + 15) & ~15ull), *ref = (uint8_t *)malloc(oo);
    memset(fld, 0x11, fo); memset(out, 0xA5, oo); memset(ref, 0xA5, oo);
    for (int k = 0; k < n_planes; k++) for (size_t i = 0; i < NSRC * C; i++) {
        if (es == 1) pl[k * stride + i] = (uint8_t)(rnd() % 256); else { float v = (float)((int)(rnd() % 20001) - 10000) / 37.0f; memcpy(pl + k * stride + i * 4, &v, 4); }
    }
    for (int f = 0; f < F; f++) {
        float *p = (float *)(fld + fr[f].fld_off);
        for (uint64_t i = 0; i < fr[f].n_px; i++) { p[2 * i] = (float)(rnd() % 10300) / 100.0f - 2.5f; p[2 * i + 1] = (float)(rnd() % 6700) / 100.0f - 2.5f; if (i % 13 == 0) { p[2 * i] = floorf(p[2 * i]); p[2 * i + 1] = floorf(p[2 * i + 1]); } }
        if (fr[f].n_px >= 255) { const float sp[16] = {NAN, 3, 3, NAN, INFINITY, 2, 2, -INFINITY, 1e30f, 5, 5, -1e30f, -1e-30f, 7.5f, W - 0.5f, H - 0.5f}; memcpy(p, sp, sizeof sp); }
        const E *src = (const E *)(pl + fr[f].plane * stride);
        for (uint64_t i = 0; i < fr[f].n_px; i++) {
            const float sx = p[2 * i], sy = p[2 * i + 1];
            for (int ch = 0; ch < C; ch++) {
                float v = 0;
                if (std::isfinite(sx) && std::isfinite(sy)) {
                    const float x0 = floorf(sx), y0 = floorf(sy), fx = sx - x0, fy = sy - y0, gx = 1.0f - fx, gy = 1.0f - fy;
                    const int c0 = ref_tap(x0, W), c1 = ref_tap(x0 + 1.0f, W), r0 = ref_tap(y0, H), r1 = ref_tap(y0 + 1.0f, H);
                    float t[4] = {(float)src[((size_t)r0 * W + c0) * C + ch], (float)src[((size_t)r0 * W + c1) * C + ch], (float)src[((size_t)r1 * W + c0) * C + ch], (float)src[((size_t)r1 * W + c1) * C + ch]};
                    v = ref_blend(t, t + 1, t + 2, t + 3, gx, fx, gy, fy);
                }
                uint8_t *o = ref + fr[f].out_off + (i * C + ch) * es;
                if (es == 4) memcpy(o, &v, 4); else *o = (uint8_t)std::min(255.0f, floorf(v + 0.5f));
            }
        }
    }
    std::vector<RemapFrame> tab = fr;
    if (single) run_grid(nb, [&] { k_remap_bilinear_frames<E, C>(nullptr, tab[0], 1, 1024, fld, pl, 0, W, H, out); });
    else run_grid(nb, [&] { k_remap_bilinear_frames<E, C>(tab.data(), RemapFrame{}, F, 1024, fld, pl, stride, W, H, out); });
    CHECK(!memcmp(out, ref, oo), "bilinear es=%zu C=%d misalign=%d planes=%d single=%d: output differs", es, C, misalign, n_planes, (int)single);
    free(fld); free(plbuf); free(out); free(ref);
}

template <typename T> static void index_all()
{
    for (int mis = 0; mis < 2; mis++) for (int np : {1, 3}) { index_case<T, true>(mis, np, 4096); index_case<T, true>(mis, np, 8192); index_case<T, false>(mis, np, 1024); index_case<T, false>(mis, np, 2048); }
}
template <typename E, int C> static void bil_all() { for (int mis = 0; mis < 2; mis++) { for (int np : {1, 3}) bilinear_case<E, C>(mis, np, false); bilinear_case<E, C>(mis, 1, true); } }

int main()
{
    index_all<uint8_t>(); index_all<uint16_t>(); index_all<uint32_t>(); index_all<uint2>(); index_all<uint4>();
    bil_all<float, 1>(); bil_all<float, 2>(); bil_all<float, 3>(); bil_all<float, 4>();
    bil_all<uint8_t, 1>(); bil_all<uint8_t, 2>(); bil_all<uint8_t, 3>(); bil_all<uint8_t, 4>();
    // 65535 one-pixel frames: the frame of every block
    { std::vector<RemapFrame> fr(65535); for (int f = 0; f < 65535; f++) fr[f] = {4ull * f, 4ull * f, 1, (uint32_t)f, 0};
      std::vector<int32_t> fld(65535); std::vector<uint32_t> pl(NSRC), out(65535, 0xA5A5A5A5u); for (auto &v : pl) v = rnd() | 1; for (auto &v : fld) v = rnd() % NSRC;
      run_grid(65535, [&] { k_remap_index_frames<uint32_t, true>(fr.data(), 65535, 4096, (const uint8_t *)fld.data(), (const uint8_t *)pl.data(), NSRC, 0, (uint8_t *)out.data()); });
      bool ok = true; for (int f = 0; f < 65535; f++) ok &= out[f] == pl[fld[f]]; CHECK(ok, "65535 frames differ"); }
    printf(fails ? "FAILED %d\n" : "host check passed\n", fails);
    return fails != 0;
}
