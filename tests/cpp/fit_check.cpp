// fit_check.cpp -- host check of the fitting kernels (homography.js_amd/csrc/hg_k_fit.hip): the kernel file itself is compiled for the CPU
// behind the thread-index shim (hip_host_shim.h; <hip/hip_runtime.h> resolves to tests/cpp/hip_stub) and runs under AddressSanitizer +
// UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside the matches, the samples, the scratch or an output
// is reported.  k_fit_score and k_fit_finish cooperate across lanes, so a block runs as 256 real threads: __syncthreads is a barrier over the
// block, LDS is static storage, atomicMax is the host's.  k_fit_hypotheses has no such traffic and runs lane by lane.  The case comes from a
// file the test writes and the outputs go back into a file, which the test compares with the numpy model.  A stand-alone program, no GPU.
//   in:  int32 kind, n_frames, n_points, n_hyp, refit, has_samples; uint32 seed; int32 pad; double threshold; n_frames int32 counts;
//        n_frames x n_points x 4 float32; with has_samples n_frames x n_hyp x 4 int32
//   out: n_frames x 8 doubles d_mats, the same d_min_mats, n_frames int32 d_counts, n_frames int32 d_best, n_frames x n_points bytes d_mask
//        (each filled with 0xA5 before)
#include <pthread.h>
#include "hip_host_shim.h"

struct float4 { float x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
#define __shared__ static
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
static inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
static inline unsigned long long atomicMax(unsigned long long *p, unsigned long long v)
{
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}

#include "hg_k_fit.hip"
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

struct Case {
    int kind, F, N, H, refit;
    uint32_t seed;
    double thr2;
    const float4 *matches; const int32_t *counts, *samples;
    double *hyp_mats; int32_t *valid; unsigned long long *best;
    double *mats, *min_mats; int32_t *out_counts, *out_best; uint8_t *mask;
};
struct Lane { const Case *c; unsigned t; };

static void *lane_main(void *arg)
{
    const Lane *l = (const Lane *)arg;
    const Case &c = *l->c;
    threadIdx = {l->t, 0, 0};
    if (c.H > 0) {
        const unsigned bx = (unsigned)((c.H + kFitHypBlock - 1) / kFitHypBlock);
        for (unsigned f = 0; f < (unsigned)c.F; f++) for (unsigned b = 0; b < bx; b++) {
            gridDim = {bx, (unsigned)c.F, 1}; blockIdx = {b, f, 0};
            if (c.kind == 1) k_fit_score<1>(c.matches, c.N, c.counts, c.H, c.thr2, c.hyp_mats, c.valid, c.best);
            else k_fit_score<0>(c.matches, c.N, c.counts, c.H, c.thr2, c.hyp_mats, c.valid, c.best);
            pthread_barrier_wait(&g_block);                   // (the next block reuses the static LDS)
        }
    }
    for (unsigned f = 0; f < (unsigned)c.F; f++) {
        gridDim = {(unsigned)c.F, 1, 1}; blockIdx = {f, 0, 0};
        if (c.kind == 1) k_fit_finish<1>(c.matches, c.N, c.counts, c.H, c.thr2, c.refit, c.hyp_mats, c.best, c.mats, c.min_mats, c.out_counts, c.out_best, c.mask);
        else k_fit_finish<0>(c.matches, c.N, c.counts, c.H, c.thr2, c.refit, c.hyp_mats, c.best, c.mats, c.min_mats, c.out_counts, c.out_best, c.mask);
        pthread_barrier_wait(&g_block);
    }
    return nullptr;
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: fit_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Case c;
    c.kind = get<int32_t>(f); c.F = get<int32_t>(f); c.N = get<int32_t>(f); c.H = get<int32_t>(f); c.refit = get<int32_t>(f);
    const int has_samples = get<int32_t>(f);
    c.seed = get<uint32_t>(f); (void)get<int32_t>(f);
    const double thr = get<double>(f);
    c.thr2 = thr * thr;
    if (c.kind < 0 || c.kind > 1 || c.F < 1 || c.F > 64 || c.N < 0 || c.N > 4096 || c.H < 0 || c.H > 4096) { printf("bad case\n"); return 2; }
    const size_t F = (size_t)c.F, N = (size_t)c.N, H = (size_t)c.H;
    std::vector<void *> owned;
    int32_t *counts = block<int32_t>(F, 0, owned);
    float4 *matches = block<float4>(F * N, 0, owned);
    int32_t *samples = has_samples ? block<int32_t>(F * H * 4, 0, owned) : nullptr;
    if (fread(counts, 4, F, f) != F || (F * N && fread(matches, 16, F * N, f) != F * N) || (samples && fread(samples, 16, F * H, f) != F * H)) { printf("short input\n"); return 2; }
    fclose(f);
    c.counts = counts; c.matches = matches; c.samples = samples;
    c.hyp_mats = block<double>(F * H * 8, 0xEE, owned); c.valid = block<int32_t>(F * H, 0xEE, owned);
    c.best = block<unsigned long long>(F, 0, owned);          // (zeroed, as the API does)
    c.mats = block<double>(F * 8, 0xA5, owned); c.min_mats = block<double>(F * 8, 0xA5, owned);
    c.out_counts = block<int32_t>(F, 0xA5, owned); c.out_best = block<int32_t>(F, 0xA5, owned); c.mask = block<uint8_t>(F * N, 0xA5, owned);
    if (c.H > 0) {
        const unsigned bx = (unsigned)((c.H + 63) / 64);
        for (unsigned fr = 0; fr < (unsigned)c.F; fr++) for (unsigned b = 0; b < bx; b++) for (unsigned t = 0; t < 64; t++) {
            gridDim = {bx, (unsigned)c.F, 1}; blockIdx = {b, fr, 0}; threadIdx = {t, 0, 0};
            k_fit_hypotheses(c.kind, c.matches, c.N, c.counts, c.H, c.seed, c.samples, c.hyp_mats, c.valid);
        }
    }
    pthread_barrier_init(&g_block, nullptr, 256);
    std::vector<Lane> lanes(256);
    std::vector<pthread_t> th(256);
    for (unsigned t = 0; t < 256; t++) {
        lanes[t] = Lane{&c, t};
        if (pthread_create(&th[t], nullptr, lane_main, &lanes[t])) { printf("cannot start a thread\n"); return 2; }
    }
    for (unsigned t = 0; t < 256; t++) pthread_join(th[t], nullptr);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(c.mats, 8, F * 8, o); fwrite(c.min_mats, 8, F * 8, o); fwrite(c.out_counts, 4, F, o); fwrite(c.out_best, 4, F, o);
    if (F * N) fwrite(c.mask, 1, F * N, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: kind %d, %d frames, %d matches, %d hypotheses\n", c.kind, c.F, c.N, c.H);
    return 0;
}
