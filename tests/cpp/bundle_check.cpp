// bundle_check.cpp -- host check of the bundle adjustment's kernels (homography.js_amd/csrc/hg_k_bundle.hip): the kernel file itself is
// compiled for the CPU behind the thread-index shim (hip_host_shim.h; <hip/hip_runtime.h> resolves to tests/cpp/hip_stub) and runs under
// AddressSanitizer + UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside the matches, the mask, the
// matrices, a part of the scratch or an output is reported.  The kernels cooperate across lanes, so a block runs as real threads (256, 64
// or 1024 of them, as the library launches it): __syncthreads is a barrier over the block, LDS is static storage, the one-workgroup solve's
// dynamic LDS a heap block of exactly (N + 1) N doubles.  The kernels are launched in the library's order; `large` forces the blocked
// factorisation at any N, which the library takes above kBundleLdsCap.  The host-built lists come from bundle_build_lists, the library's
// own.  The case comes from a file the test writes (tests/hgtest/bundle.py, pack) and the outputs go back into a file, which the test
// compares with the numpy model.  A stand-alone program, no GPU.
//   in:  int32 kind, W, H, n_frames, n_pairs, n_points, n_iter, large, want_sums, has_mask, 0, 0; double eps, lambda0, huber; int32 fixed[F],
//        pairs[2 NP], counts[NP]; float matches[NP n 4]; uint8 mask[NP n] (has_mask); double mats[F 8]
//   out: F x 8 doubles d_mats_out, the bytes of d_info, with want_sums NP x 154 doubles d_pair_sums (each filled with 0xA5 before)
#include <pthread.h>
#include <functional>
#include "hip_host_shim.h"

#define __shared__ static
struct float4 { float x, y, z, w; };
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
static double *g_bundle_host_lds;

#include "hg_k_bundle.hip"
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
template <typename T> static void fill_from(FILE *f, T *p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { printf("short input\n"); exit(2); } }

// One launch: `lanes` threads, thread t with threadIdx = {t, 0, 0}; the blocks run one after another (they share the static LDS).
struct Launch { unsigned lanes, gx, gy; std::function<void()> body; };
struct Lane { const Launch *l; unsigned t; };
static void *lane_main(void *arg)
{
    const Lane *ln = (const Lane *)arg;
    threadIdx = {ln->t, 0, 0};
    for (unsigned y = 0; y < ln->l->gy; y++) for (unsigned x = 0; x < ln->l->gx; x++) {
        gridDim = {ln->l->gx, ln->l->gy, 1}; blockIdx = {x, y, 0};
        ln->l->body();
        pthread_barrier_wait(&g_block);
    }
    return nullptr;
}
static void launch(unsigned lanes, unsigned gx, unsigned gy, std::function<void()> body)
{
    if (!gx || !gy) return;
    Launch l{lanes, gx, gy, body};
    pthread_barrier_init(&g_block, nullptr, lanes);
    std::vector<Lane> ln(lanes);
    std::vector<pthread_t> th(lanes);
    pthread_attr_t at;
    pthread_attr_init(&at);
    pthread_attr_setstacksize(&at, 1 << 19);
    for (unsigned t = 0; t < lanes; t++) {
        ln[t] = Lane{&l, t};
        if (pthread_create(&th[t], &at, lane_main, &ln[t])) { printf("cannot start a thread\n"); exit(2); }
    }
    for (unsigned t = 0; t < lanes; t++) pthread_join(th[t], nullptr);
    pthread_attr_destroy(&at);
    pthread_barrier_destroy(&g_block);
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: bundle_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t v[12];
    for (int k = 0; k < 12; k++) v[k] = get<int32_t>(f);
    const double eps = get<double>(f), lambda0 = get<double>(f), huber = get<double>(f);
    const int kind = v[0], W = v[1], H = v[2], F = v[3], NP = v[4], n = v[5], n_iter = v[6], large = v[7], want_sums = v[8], has_mask = v[9];
    if (kind < 0 || kind > 1 || W < 1 || H < 1 || F < 1 || F > 64 || NP < 0 || NP > 256 || n < 0 || n > 4096 || n_iter < 0 || n_iter > 64) { printf("bad case\n"); return 2; }
    std::vector<void *> owned;
    std::vector<int32_t> fixed32((size_t)F), pairs((size_t)NP * 2), counts((size_t)NP);
    fill_from(f, fixed32.data(), (size_t)F); fill_from(f, pairs.data(), (size_t)NP * 2); fill_from(f, counts.data(), (size_t)NP);
    std::vector<uint8_t> fixed((size_t)F);
    for (int k = 0; k < F; k++) fixed[(size_t)k] = fixed32[(size_t)k] ? 1 : 0;
    for (int p = 0; p < NP; p++)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= F || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= F || pairs[2 * p] == pairs[2 * p + 1] || counts[p] < 0 || counts[p] > n) { printf("bad case\n"); return 2; }
    float *matches = block<float>((size_t)NP * n * 4, 0, owned);
    fill_from(f, matches, (size_t)NP * n * 4);
    uint8_t *mask = has_mask ? block<uint8_t>((size_t)NP * n, 0, owned) : nullptr;
    if (has_mask) fill_from(f, mask, (size_t)NP * n);
    double *mats_in = block<double>((size_t)F * 8, 0, owned);
    fill_from(f, mats_in, (size_t)F * 8);
    fclose(f);

    BundleLists L;
    bundle_build_lists(F, fixed.data(), pairs.data(), NP, counts.data(), n, L);
    int32_t *ints = block<int32_t>(L.ints.size(), 0, owned);
    if (ints) memcpy(ints, L.ints.data(), L.ints.size() * 4);
    const int P = bundle_p(kind), N = P * L.n_free;
    const size_t info_bytes = sizeof(BundleInfo) + (((size_t)F * 4 + 7) & ~(size_t)7) + sizeof(BundlePairInfo) * (size_t)NP;
    BundleArgs a{};
    a.kind = kind; a.W = W; a.H = H; a.n_frames = F; a.n_pairs = NP; a.n_points = n; a.n_work = L.n_work; a.n_free = L.n_free; a.N = N;
    a.n_iter = N == 0 ? 0 : n_iter; a.eps = eps; a.lambda0 = lambda0; a.huber = huber;
    a.matches = matches; a.mask = mask;
    a.pairs4 = ints; a.work = ints + L.o_work; a.cls = ints + L.o_cls; a.fidx = ints + L.o_fidx; a.rowptr = ints + L.o_rowptr; a.ent = ints + L.o_ent;
    a.good = block<int32_t>((size_t)F, 0xEE, owned);
    a.mats_in = mats_in;
    a.mats_out = block<double>((size_t)F * 8, 0xA5, owned);
    a.info = block<uint8_t>(info_bytes, 0xA5, owned);
    a.sums = want_sums ? block<double>((size_t)NP * kBundleRec, 0xA5, owned) : nullptr;
    a.state = block<BundleState>(1, 0xEE, owned);
    a.iter = block<double>((size_t)2 * F * 8, 0xEE, owned);
    a.part = block<double>((size_t)L.n_work * kBundleRec, 0xEE, owned);
    a.recs = block<double>((size_t)2 * NP * kBundleRec, 0xEE, owned);
    a.Hm = large ? block<double>((size_t)(N + 1) * N, 0xEE, owned) : nullptr;       // (the one-workgroup round keeps H in its LDS block)
    a.Wm = large ? block<double>((size_t)(N + 1) * N, 0xEE, owned) : nullptr;
    g_bundle_host_lds = large ? nullptr : block<double>((size_t)(N + 1) * N, 0xEE, owned);

    launch(kBundleBlock, 1, 1, [&] { k_bundle_init(a); });
    for (int round = 0; round <= a.n_iter; round++) {
        if (round > 0 && large) {
            launch(kBundleBlock, (unsigned)a.n_free, 1, [&] { k_bundle_assemble(a); });
            launch(kBundleBlock, 2, 1, [&] { k_bundle_damp(a); });
            for (int k0 = 0; k0 < N; k0 += kBundlePanel) {
                const int nb = N - k0 < kBundlePanel ? N - k0 : kBundlePanel, below = N + 1 - (k0 + nb);
                launch(kBundleBlock, 1, 1, [&] { k_bundle_chol_diag(a, k0, nb); });
                launch(64, (unsigned)(below + 63) / 64, 1, [&] { k_bundle_chol_panel(a, k0, nb); });
                if (k0 + nb < N) { const unsigned nt = (unsigned)(below + kBundlePanel - 1) / kBundlePanel; launch(kBundleBlock, nt, nt, [&] { k_bundle_chol_trail(a, k0, nb); }); }
            }
            launch(kBundleBackBlock, 1, 1, [&] { k_bundle_back_large(a); });
        }
        if (kind == 1) launch(kBundleBlock, (unsigned)a.n_work, 1, [&] { k_bundle_pass<1>(a, round); });
        else launch(kBundleBlock, (unsigned)a.n_work, 1, [&] { k_bundle_pass<0>(a, round); });
        if (!large) launch(kBundleBlock, 1, 1, [&] { k_bundle_round_small(a, round); });
        else {
            launch(kBundleBlock, (unsigned)NP, 1, [&] { k_bundle_reduce(a, round); });
            launch(kBundleBlock, 1, 1, [&] { k_bundle_decide(a, round); });
        }
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(a.mats_out, 8, (size_t)F * 8, o); fwrite(a.info, 1, info_bytes, o);
    if (a.sums) fwrite(a.sums, 8, (size_t)NP * kBundleRec, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: kind %d, %d frames, %d pairs, %d unknowns, %s solve, %d rounds at most\n", kind, F, NP, N, large ? "blocked" : "one-workgroup", a.n_iter);
    return 0;
}
