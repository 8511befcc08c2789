// match_check.cpp -- host check of the matching kernels (homography.js_amd/csrc/hg_k_match.hip): the kernel file itself is compiled for the
// CPU behind the thread-index shim (hip_host_shim.h; <hip/hip_runtime.h> resolves to tests/cpp/hip_stub) and runs under AddressSanitizer +
// UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside the descriptors, the points, the scratch or an
// output is reported.  k_match_bits and k_match_finish cooperate across lanes, so a workgroup runs as real threads (64 resp. 256):
// __syncthreads is a barrier over the block, LDS is static storage.  What runs here: k_match_bits in all its widths, both of its launches
// (the two nearest of the queries; with the sides swapped, the best query of the train rows), k_match_finish, and through them the shared
// helpers of hg_match_dev.h (the byte mask, the packed two nearest, the acceptance tests) and the compaction; match_merge, which joins
// partial records, and the packed form are also checked on their own against a sort before every case.  What CANNOT run here:
// k_match_u8 -- its dot products are matrix-core instructions -- so HG_DESC_U8, and with it the atomic form of the cross-check, is pinned
// by tests/test_gpu_match.py alone; its fold uses the merge that does run here.  The case comes from a file the test writes and the
// outputs go back into a file, which the test compares with the numpy model.  A stand-alone program, no GPU.
//   in:  int32 desc_bytes, stride, n_frames, n_query, n_train, n_train_sets, cross_check, ratio_on, has_points, want (bit 0 matches, 1 pairs,
//        2 nn); uint32 max_distance; int32 pad; double rr; n_frames int32 counts_q; n_train_sets int32 counts_t; the query rows; the train
//        rows; with has_points the query points and the train points (float32 pairs)
//   out: n_frames int32 d_counts, n_frames x n_query x 16 bytes d_matches, x 8 bytes d_pairs, x 16 bytes d_nn (each filled with 0xA5 before;
//        an output that is not wanted stays so)
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
static inline int __popc(uint32_t v) { return __builtin_popcount(v); }

#include "hg_k_match.hip"
using namespace hg;

template <typename T> static T get(FILE *f) { T v; if (fread(&v, sizeof v, 1, f) != 1) { printf("short input\n"); exit(2); } return v; }
template <typename T> static T *block(size_t n, int fill, std::vector<void *> &owned)      // exactly n elements, 16-byte aligned; nullptr for none
{
    if (!n) return nullptr;
    const size_t bytes = n * sizeof(T);
    void *p = bytes % 16 ? malloc(bytes) : aligned_alloc(16, bytes);          // (what is read in 16-byte pieces has such a size; the size stays exact)
    owned.push_back(p);
    memset(p, fill, n * sizeof(T));
    return static_cast<T *>(p);
}

struct Case {
    int desc_bytes, F, NQ, NT, S, cross, ratio_on;
    size_t stride;
    uint32_t max_distance;
    double rr;
    const int32_t *cq, *ct; const uint8_t *query, *train; const uint2 *qpts, *tpts;
    uint4 *fwd, *rev;
    int32_t *out_counts; uint4 *out_matches; int32_t *out_pairs, *out_nn;
};
struct Lane { const Case *c; unsigned t; int phase; };

static void side(const Case &c, const uint8_t *A, int n_a, int a_sets, const int32_t *cnt_a, const uint8_t *B, int n_b, int b_sets, const int32_t *cnt_b, uint4 *out)
{
    const unsigned bx = (unsigned)((n_a + kMatchTQ - 1) / kMatchTQ);
    const int words = (c.desc_bytes + 3) / 4;
    for (unsigned f = 0; f < (unsigned)c.F; f++) for (unsigned b = 0; b < bx; b++) {
        gridDim = {bx, (unsigned)c.F, 1}; blockIdx = {b, f, 0};
        if (words <= 8) k_match_bits<8>(A, n_a, a_sets, cnt_a, B, n_b, b_sets, cnt_b, c.desc_bytes, c.stride, out);
        else if (words <= 16) k_match_bits<16>(A, n_a, a_sets, cnt_a, B, n_b, b_sets, cnt_b, c.desc_bytes, c.stride, out);
        else if (words <= 32) k_match_bits<32>(A, n_a, a_sets, cnt_a, B, n_b, b_sets, cnt_b, c.desc_bytes, c.stride, out);
        else k_match_bits<128>(A, n_a, a_sets, cnt_a, B, n_b, b_sets, cnt_b, c.desc_bytes, c.stride, out);
        pthread_barrier_wait(&g_block);                       // (the next block reuses the static LDS)
    }
}

static void *lane_main(void *arg)
{
    const Lane *l = (const Lane *)arg;
    const Case &c = *l->c;
    threadIdx = {l->t, 0, 0};
    if (l->phase == 0) {
        side(c, c.query, c.NQ, c.F, c.cq, c.train, c.NT, c.S, c.ct, c.fwd);
        if (c.cross) side(c, c.train, c.NT, c.S, c.ct, c.query, c.NQ, c.F, c.cq, c.rev);
        return nullptr;
    }
    const bool work = c.NQ > 0 && c.NT > 0;
    for (unsigned f = 0; f < (unsigned)c.F; f++) {
        gridDim = {(unsigned)c.F, 1, 1}; blockIdx = {f, 0, 0};
        k_match_finish(c.NQ, c.NT, c.S, c.cq, c.ct, c.fwd, (work && c.cross) ? c.rev : nullptr, nullptr, c.max_distance, c.ratio_on, c.rr, c.qpts, c.tpts,
                       c.out_counts, c.out_matches, c.out_pairs, c.out_nn);
        pthread_barrier_wait(&g_block);
    }
    return nullptr;
}

static int run_phase(const Case &c, int phase, unsigned n)
{
    pthread_barrier_init(&g_block, nullptr, n);
    std::vector<Lane> lanes(n);
    std::vector<pthread_t> th(n);
    for (unsigned t = 0; t < n; t++) {
        lanes[t] = Lane{&c, t, phase};
        if (pthread_create(&th[t], nullptr, lane_main, &lanes[t])) { printf("cannot start a thread\n"); return 2; }
    }
    for (unsigned t = 0; t < n; t++) pthread_join(th[t], nullptr);
    pthread_barrier_destroy(&g_block);
    return 0;
}

// The merge and the packed form against a sort, on their own: random (d, j) lists with many ties, split at random points into parts that
// are folded by match_push / match_unpack and joined by match_merge in both orders.
static int helpers_ok()
{
    uint32_t seed = 12345u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int round = 0; round < 2000; round++) {
        const int n = (int)(rnd() % 40), shift = round % 2 ? 16 : 6, span = round % 3 ? 5 : 4097;
        std::vector<uint32_t> d((size_t)n);
        for (auto &v : d) v = rnd() % (uint32_t)span;
        MatchTop2 want = match_top2_empty();                      // by the definition: the lowest j of the smallest d; the second of the sorted distances
        for (int j = 0; j < n; j++) if (d[j] < want.d1) { want.d1 = d[j]; want.j1 = j; }
        if (n >= 2) { std::vector<uint32_t> s = d; std::sort(s.begin(), s.end()); want.d2 = s[1]; }
        const int cut = n ? (int)(rnd() % (uint32_t)(n + 1)) : 0, j0 = (int)(rnd() % 1000);
        MatchKeys2 ka = match_keys2_empty(), kb = match_keys2_empty();
        for (int j = 0; j < cut; j++) match_push(ka, (d[j] << shift) | (uint32_t)j);
        for (int j = cut; j < n && j - cut < (1 << shift); j++) match_push(kb, (d[j] << shift) | (uint32_t)(j - cut));
        if (n - cut > (1 << shift)) continue;
        MatchTop2 a = match_unpack(ka, shift, j0), b = match_unpack(kb, shift, j0 + cut), ab = a, ba = b;
        match_merge(ab, b);
        match_merge(ba, a);
        const int32_t wj = want.j1 < 0 ? -1 : want.j1 + j0;
        if (ab.d1 != want.d1 || ab.j1 != wj || ab.d2 != want.d2 || ba.d1 != ab.d1 || ba.j1 != ab.j1 || ba.d2 != ab.d2) {
            printf("merge helpers differ from the sort: round %d, n %d, cut %d\n", round, n, cut);
            return 0;
        }
    }
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: match_check IN OUT\n"); return 2; }
    if (!helpers_ok()) return 3;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Case c;
    c.desc_bytes = get<int32_t>(f); c.stride = (size_t)get<int32_t>(f); c.F = get<int32_t>(f); c.NQ = get<int32_t>(f); c.NT = get<int32_t>(f);
    c.S = get<int32_t>(f); c.cross = get<int32_t>(f); c.ratio_on = get<int32_t>(f);
    const int has_points = get<int32_t>(f), want = get<int32_t>(f);
    c.max_distance = get<uint32_t>(f); (void)get<int32_t>(f);
    c.rr = get<double>(f);
    if (c.desc_bytes < 1 || c.desc_bytes > 512 || c.stride % 16 || c.stride < (size_t)c.desc_bytes || c.stride > 1024 || c.F < 1 || c.F > 16 || c.NQ < 0 ||
        c.NQ > 4096 || c.NT < 0 || c.NT > 4096 || c.S < 1 || c.S > c.F) { printf("bad case\n"); return 2; }
    const size_t F = (size_t)c.F, S = (size_t)c.S, NQ = (size_t)c.NQ, NT = (size_t)c.NT;
    std::vector<void *> owned;
    int32_t *cq = block<int32_t>(F, 0, owned), *ct = block<int32_t>(S, 0, owned);
    uint8_t *query = block<uint8_t>(F * NQ * c.stride, 0, owned), *train = block<uint8_t>(S * NT * c.stride, 0, owned);
    uint2 *qpts = has_points ? block<uint2>(F * NQ, 0, owned) : nullptr, *tpts = has_points ? block<uint2>(S * NT, 0, owned) : nullptr;
    bool ok = fread(cq, 4, F, f) == F && fread(ct, 4, S, f) == S;
    ok = ok && (!query || fread(query, c.stride, F * NQ, f) == F * NQ) && (!train || fread(train, c.stride, S * NT, f) == S * NT);
    ok = ok && (!qpts || fread(qpts, 8, F * NQ, f) == F * NQ) && (!tpts || fread(tpts, 8, S * NT, f) == S * NT);
    if (!ok) { printf("short input\n"); return 2; }
    fclose(f);
    for (size_t k = 0; k < F; k++) if (cq[k] < 0 || cq[k] > c.NQ) { printf("bad case\n"); return 2; }
    for (size_t k = 0; k < S; k++) if (ct[k] < 0 || ct[k] > c.NT) { printf("bad case\n"); return 2; }
    c.cq = cq; c.ct = ct; c.query = query; c.train = train; c.qpts = qpts; c.tpts = tpts;
    c.fwd = block<uint4>(F * NQ, 0xEE, owned); c.rev = c.cross ? block<uint4>(F * NT, 0xEE, owned) : nullptr;
    c.out_counts = block<int32_t>(F, 0xA5, owned);
    uint4 *m = block<uint4>(F * NQ, 0xA5, owned);
    int32_t *p = block<int32_t>(F * NQ * 2, 0xA5, owned), *nn = block<int32_t>(F * NQ * 4, 0xA5, owned);
    c.out_matches = (want & 1) && has_points ? m : nullptr; c.out_pairs = (want & 2) ? p : nullptr; c.out_nn = (want & 4) ? nn : nullptr;
    if (c.NQ > 0 && c.NT > 0 && run_phase(c, 0, kMatchTQ)) return 2;
    if (run_phase(c, 1, kMatchFinishBlock)) return 2;
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(c.out_counts, 4, F, o);
    if (F * NQ) { fwrite(m, 16, F * NQ, o); fwrite(p, 8, F * NQ, o); fwrite(nn, 16, F * NQ, o); }
    fclose(o);
    for (void *q : owned) free(q);
    printf("host check ran: %d bytes, %d frames, %d queries, %d train rows\n", c.desc_bytes, c.F, c.NQ, c.NT);
    return 0;
}
