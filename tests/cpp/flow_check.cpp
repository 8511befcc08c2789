// flow_check.cpp -- host check of the dense-flow kernels (homography.js_amd/csrc/hg_k_flow.hip): the kernel file itself is compiled for the CPU
// behind the thread-index shim (hip_host_shim.h; <hip/hip_runtime.h> resolves to tests/cpp/hip_stub) and runs under AddressSanitizer +
// UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside the planes, the pyramid levels, the flow buffers or
// the outputs is reported.  k_flow_iter cooperates across lanes through LDS, so its workgroup runs as 256 real threads: __syncthreads is a
// barrier over the block, LDS is static storage.  k_pyr_down (hg_k_pyramid.hip, the file itself), k_flow_up, k_flow_finish and
// k_field_compose_frames have no barrier: their lanes run one after the other.  The case comes from a file the test writes and the outputs go
// back into a file, which the test compares with the numpy model (tests/hgtest/flow.py) byte for byte.  A stand-alone program, no GPU.
//   in:  int32 W, H, F, S, levels, n_iter, radius, n_outer; double min_eig, max_update; F FROM planes, S TO planes (W x H bytes each);
//        n_outer (x, y) float32 coordinates
//   out: per frame the field, the flow pairs (W x H x 8 bytes each), the residual and the good bytes (W x H each); then n_outer pairs: the
//        coordinates chained with frame 0's field
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }

#include "hg_k_pyramid.hip"
#include "hg_k_flow.hip"
using namespace hg;

template <typename T> static T get(FILE *f) { T v; if (fread(&v, sizeof v, 1, f) != 1) { printf("short input\n"); exit(2); } return v; }
template <typename T> static T *block(size_t n, int fill, std::vector<void *> &owned)      // exactly n elements; nullptr for none
{
    if (!n) return nullptr;
    void *p = malloc(n * sizeof(T));
    owned.push_back(p);
    memset(p, fill, n * sizeof(T));
    return static_cast<T *>(p);
}

template <typename K> static void grid_64x4(unsigned gx, unsigned gy, unsigned gz, K kernel)
{
    for (unsigned bz = 0; bz < gz; bz++) for (unsigned by = 0; by < gy; by++) for (unsigned bx = 0; bx < gx; bx++)
        for (unsigned ty = 0; ty < 4; ty++) for (unsigned tx = 0; tx < 64; tx++) {
            gridDim = {gx, gy, gz}; blockIdx = {bx, by, bz}; threadIdx = {tx, ty, 0};
            kernel();
        }
}

struct Lane { const FlowIterArgs *a; unsigned t, gx, gy, gz; };

static void *iter_lane(void *arg)
{
    const Lane *l = (const Lane *)arg;
    threadIdx = {l->t, 0, 0};
    for (unsigned bz = 0; bz < l->gz; bz++) for (unsigned by = 0; by < l->gy; by++) for (unsigned bx = 0; bx < l->gx; bx++) {
        gridDim = {l->gx, l->gy, l->gz}; blockIdx = {bx, by, bz};
        if (l->a->radius <= 3) k_flow_iter<3>(*l->a); else k_flow_iter<kFlowMaxRadius>(*l->a);
        pthread_barrier_wait(&g_block);                       // (the next block reuses the static LDS)
    }
    return nullptr;
}

static void run_iter(const FlowIterArgs &a, int F)
{
    std::vector<Lane> lanes(kFlowBlock);
    std::vector<pthread_t> th(kFlowBlock);
    for (unsigned t = 0; t < (unsigned)kFlowBlock; t++) {
        lanes[t] = Lane{&a, t, (unsigned)(a.W + kFlowTileW - 1) / kFlowTileW, (unsigned)(a.H + kFlowTileH - 1) / kFlowTileH, (unsigned)F};
        if (pthread_create(&th[t], nullptr, iter_lane, &lanes[t])) { printf("cannot start a thread\n"); exit(2); }
    }
    for (unsigned t = 0; t < (unsigned)kFlowBlock; t++) pthread_join(th[t], nullptr);
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: flow_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t v[8];
    for (int k = 0; k < 8; k++) v[k] = get<int32_t>(f);
    const double min_eig = get<double>(f), max_update = get<double>(f);
    const int W = v[0], H = v[1], F = v[2], S = v[3], levels = v[4], n_iter = v[5], radius = v[6], n_outer = v[7];
    if (W < 1 || W > 256 || H < 1 || H > 256 || F < 1 || F > 8 || S < 1 || S > F || levels < 1 || levels > kFlowMaxLevels || n_iter < 1 || n_iter > kFlowMaxIter ||
        radius < 1 || radius > kFlowMaxRadius || n_outer < 0 || n_outer > 4096 || !(min_eig >= 0.0) || !(max_update > 0.0)) { printf("bad case\n"); return 2; }
    std::vector<void *> owned;
    const size_t n_px = (size_t)W * H;
    std::vector<uint8_t *> lf(levels), lt(levels);
    std::vector<int> w(levels), h(levels);
    lf[0] = block<uint8_t>(F * n_px, 0, owned); lt[0] = block<uint8_t>(S * n_px, 0, owned);
    float *outer = block<float>((size_t)n_outer * 2, 0, owned);
    if (fread(lf[0], n_px, F, f) != (size_t)F || fread(lt[0], n_px, S, f) != (size_t)S || fread(outer, 8, n_outer, f) != (size_t)n_outer) { printf("short input\n"); return 2; }
    fclose(f);
    pthread_barrier_init(&g_block, nullptr, kFlowBlock);

    w[0] = W; h[0] = H;
    for (int k = 1; k < levels; k++) {
        w[k] = (w[k - 1] + 1) >> 1; h[k] = (h[k - 1] + 1) >> 1;
        if (w[k - 1] == 1 && h[k - 1] == 1) { printf("bad case: too many levels\n"); return 2; }
        const size_t ns = (size_t)w[k - 1] * h[k - 1], nd = (size_t)w[k] * h[k];
        lf[k] = block<uint8_t>(F * nd, 0xEE, owned); lt[k] = block<uint8_t>(S * nd, 0xEE, owned);
        for (int side = 0; side < 2; side++) {
            const uint8_t *src = side ? lt[k - 1] : lf[k - 1];
            uint8_t *dst = side ? lt[k] : lf[k];
            const int np = side ? S : F;
            grid_64x4((unsigned)(w[k] + 63) / 64, (unsigned)(h[k] + 3) / 4, (unsigned)np,
                      [&] { k_pyr_down<uint8_t, 1>(src, ns, w[k - 1], h[k - 1], dst, nd, w[k], h[k], np); });
        }
    }

    uint8_t *good = block<uint8_t>(F * n_px, 0xA5, owned);
    float2 *cur = nullptr;
    for (int k = levels - 1; k >= 0; k--) {
        const size_t n = (size_t)F * w[k] * h[k];
        float2 *a = block<float2>(n, 0xEE, owned), *b = block<float2>(n, 0xEE, owned);
        if (k == levels - 1) memset(a, 0, n * sizeof(float2));
        else {
            FlowUpArgs ua{cur, w[k + 1], h[k + 1], a, w[k], h[k]};
            grid_64x4((unsigned)(w[k] + 63) / 64, (unsigned)(h[k] + 3) / 4, (unsigned)F, [&] { k_flow_up(ua); });
        }
        for (int it = 0; it < n_iter; it++) {
            const bool last = k == 0 && it == n_iter - 1;
            FlowIterArgs ia{lt[k], (size_t)w[k] * h[k], S, lf[k], (size_t)w[k] * h[k], w[k], h[k], radius, min_eig, max_update, a, b, last ? good : nullptr};
            run_iter(ia, F);
            std::swap(a, b);
        }
        cur = a;
    }
    std::vector<FlowOff> offs(F);
    for (int k = 0; k < F; k++) offs[k] = FlowOff{(uint64_t)k * n_px * 8, 0};
    uint8_t *field = block<uint8_t>(F * n_px * 8, 0xA5, owned), *flow = block<uint8_t>(F * n_px * 8, 0xA5, owned), *res = block<uint8_t>(F * n_px, 0xA5, owned);
    FlowFinishArgs fa{lt[0], n_px, S, lf[0], n_px, W, H, cur, offs.data(), field, flow, res};
    grid_64x4((unsigned)(W + 63) / 64, (unsigned)(H + 3) / 4, (unsigned)F, [&] { k_flow_finish(fa); });

    // the chained field: the n_outer coordinates as one frame through frame 0's field
    uint8_t *chained = block<uint8_t>((size_t)n_outer * 8, 0xA5, owned);
    if (n_outer) {
        RemapFrame fr{0, 0, (uint64_t)n_outer, 0, 0};
        const unsigned nb = (unsigned)(n_outer + 1023) / 1024;
        for (unsigned bx = 0; bx < nb; bx++) for (unsigned t = 0; t < 256; t++) {
            gridDim = {nb, 1, 1}; blockIdx = {bx, 0, 0}; threadIdx = {t, 0, 0};
            k_field_compose_frames(&fr, 1, 1024, reinterpret_cast<const uint8_t *>(outer), field, n_px * 8, W, H, chained);
        }
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    for (int k = 0; k < F; k++) {
        fwrite(field + k * n_px * 8, 8, n_px, o); fwrite(flow + k * n_px * 8, 8, n_px, o);
        fwrite(res + k * n_px, 1, n_px, o); fwrite(good + k * n_px, 1, n_px, o);
    }
    if (n_outer) fwrite(chained, 8, n_outer, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: %d x %d, %d frames on %d TO planes, %d levels, %d iterations, radius %d, %d chained positions\n", W, H, F, S, levels, n_iter, radius, n_outer);
    return 0;
}
