// align_check.cpp -- host check of the alignment kernels (homography.js_amd/csrc/hg_k_align.hip): the kernel file itself is compiled for the
// CPU behind the thread-index shim (hip_host_shim.h; <hip/hip_runtime.h> resolves to tests/cpp/hip_stub) and runs under AddressSanitizer +
// UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside the planes, the matrices, the scratch or an output
// is reported.  Both kernels cooperate across lanes, so a block runs as 256 real threads: __syncthreads is a barrier over the block, LDS is
// static storage.  The passes are launched as the library launches them: the luma copies of 4-channel planes, then n_iter + 1 times
// accumulate and update over all frames.  The case comes from a file the test writes (tests/hgtest/align.py, pack) and the outputs go back
// into a file, which the test compares with the numpy model.  A stand-alone program, no GPU.
//   in:  int32 kind, photometric, Wf, Hf, n_frames, Wt, Ht, n_to_sets, channels, rx, ry, rw, rh, step, n_iter, min_valid, want_sums, pad;
//        int64 from_stride, to_stride; double eps; the FROM planes (stride apart, nothing behind the last), the TO planes, n_frames x 8 doubles
//   out: n_frames x 8 doubles d_mats_out, n_frames x 48 bytes d_info, with want_sums n_frames x 66 doubles d_sums (each filled with 0xA5 before)
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }

#include "hg_k_align.hip"
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

struct Job { AlignArgs a; int channels; const uint8_t *raw_from, *raw_to; size_t raw_fs, raw_ts; uint8_t *luma_from, *luma_to; };
struct Lane { const Job *j; unsigned t; };

template <int KIND, int PHOTO>
static void passes(const AlignArgs &a)
{
    for (int pass = 0; pass <= a.n_iter; pass++) {
        for (unsigned f = 0; f < (unsigned)a.n_frames; f++) for (unsigned c = 0; c < (unsigned)a.n_chunks; c++) {
            gridDim = {(unsigned)a.n_chunks, (unsigned)a.n_frames, 1}; blockIdx = {c, f, 0};
            k_align_accumulate<KIND, PHOTO>(a, pass);
            pthread_barrier_wait(&g_block);                   // (the next block reuses the static LDS)
        }
        for (unsigned f = 0; f < (unsigned)a.n_frames; f++) {
            gridDim = {(unsigned)a.n_frames, 1, 1}; blockIdx = {f, 0, 0};
            k_align_update<KIND, PHOTO>(a, pass);
            pthread_barrier_wait(&g_block);
        }
    }
}

static void *lane_main(void *arg)
{
    const Lane *l = (const Lane *)arg;
    const Job &j = *l->j;
    threadIdx = {l->t, 0, 0};
    if (j.channels == 4) {                                    // one block per plane, as a grid of 1 x planes
        for (unsigned f = 0; f < (unsigned)j.a.n_frames; f++) {
            gridDim = {1, (unsigned)j.a.n_frames, 1}; blockIdx = {0, f, 0};
            k_align_luma(j.raw_from, j.raw_fs, (uint32_t)j.a.Wf * (uint32_t)j.a.Hf, j.luma_from);
        }
        for (unsigned s = 0; s < (unsigned)j.a.n_to_sets; s++) {
            gridDim = {1, (unsigned)j.a.n_to_sets, 1}; blockIdx = {0, s, 0};
            k_align_luma(j.raw_to, j.raw_ts, (uint32_t)j.a.Wt * (uint32_t)j.a.Ht, j.luma_to);
        }
        pthread_barrier_wait(&g_block);
    }
    if (j.a.kind == 1) { if (j.a.photometric) passes<1, 1>(j.a); else passes<1, 0>(j.a); }
    else { if (j.a.photometric) passes<0, 1>(j.a); else passes<0, 0>(j.a); }
    return nullptr;
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: align_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t v[18];
    for (int k = 0; k < 18; k++) v[k] = get<int32_t>(f);
    const int64_t fs = get<int64_t>(f), ts = get<int64_t>(f);
    const double eps = get<double>(f);
    const int kind = v[0], photo = v[1], Wf = v[2], Hf = v[3], F = v[4], Wt = v[5], Ht = v[6], NT = v[7], ch = v[8], rx = v[9], ry = v[10], rw = v[11], rh = v[12],
              step = v[13], n_iter = v[14], min_valid = v[15], want_sums = v[16];
    const size_t fb = (size_t)Wf * Hf * ch, tb = (size_t)Wt * Ht * ch;
    if (kind < 0 || kind > 1 || photo < 0 || photo > 1 || F < 1 || F > 16 || NT < 1 || NT > F || (ch != 1 && ch != 4) || Wf < 1 || Hf < 1 || Wt < 1 || Ht < 1 ||
        Wf > 32768 || Hf > 32768 || Wt > 32768 || Ht > 32768 || rx < 0 || ry < 0 || rw < 1 || rh < 1 || rx + rw > Wf || ry + rh > Hf || step < 1 || step > 64 ||
        n_iter < 0 || n_iter > 64 || (size_t)fs < fb || (size_t)ts < tb) { printf("bad case\n"); return 2; }
    std::vector<void *> owned;
    const size_t from_bytes = (size_t)fs * (F - 1) + fb, to_bytes = (size_t)ts * (NT - 1) + tb;
    uint8_t *from = block<uint8_t>(from_bytes, 0, owned), *to = block<uint8_t>(to_bytes, 0, owned);
    double *mats_in = block<double>((size_t)F * 8, 0, owned);
    if (fread(from, 1, from_bytes, f) != from_bytes || fread(to, 1, to_bytes, f) != to_bytes || fread(mats_in, 8, (size_t)F * 8, f) != (size_t)F * 8) { printf("short input\n"); return 2; }
    fclose(f);
    Job j;
    j.channels = ch; j.raw_from = from; j.raw_to = to; j.raw_fs = (size_t)fs; j.raw_ts = (size_t)ts;
    j.luma_from = ch == 4 ? block<uint8_t>((size_t)F * Wf * Hf, 0xEE, owned) : nullptr;
    j.luma_to = ch == 4 ? block<uint8_t>((size_t)NT * Wt * Ht, 0xEE, owned) : nullptr;
    AlignArgs &a = j.a;
    a.kind = kind; a.photometric = photo;
    a.from = ch == 4 ? j.luma_from : from; a.Wf = Wf; a.Hf = Hf; a.from_stride = ch == 4 ? (size_t)Wf * Hf : (size_t)fs;
    a.to = ch == 4 ? j.luma_to : to; a.Wt = Wt; a.Ht = Ht; a.n_to_sets = NT; a.to_stride = ch == 4 ? (size_t)Wt * Ht : (size_t)ts;
    a.rx = rx; a.ry = ry; a.rw = rw; a.rh = rh; a.step = step;
    a.nx = (rw + step - 1) / step;
    a.n_samples = a.nx * ((rh + step - 1) / step);
    a.n_chunks = (a.n_samples + kAlignChunk - 1) / kAlignChunk;
    a.n_frames = F; a.n_iter = n_iter; a.eps = eps; a.min_valid = min_valid;
    a.mats_in = mats_in;
    a.mats_out = block<double>((size_t)F * 8, 0xA5, owned);
    a.info = block<AlignInfo>((size_t)F, 0xA5, owned);
    a.sums = want_sums ? block<double>((size_t)F * kAlignSums, 0xA5, owned) : nullptr;
    a.state = block<AlignState>((size_t)F, 0xEE, owned);
    a.part = block<double>((size_t)F * a.n_chunks * kAlignRec, 0xEE, owned);
    pthread_barrier_init(&g_block, nullptr, kAlignBlock);
    std::vector<Lane> lanes(kAlignBlock);
    std::vector<pthread_t> th(kAlignBlock);
    for (unsigned t = 0; t < (unsigned)kAlignBlock; t++) {
        lanes[t] = Lane{&j, t};
        if (pthread_create(&th[t], nullptr, lane_main, &lanes[t])) { printf("cannot start a thread\n"); return 2; }
    }
    for (unsigned t = 0; t < (unsigned)kAlignBlock; t++) pthread_join(th[t], nullptr);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(a.mats_out, 8, (size_t)F * 8, o); fwrite(a.info, sizeof(AlignInfo), (size_t)F, o);
    if (a.sums) fwrite(a.sums, 8, (size_t)F * kAlignSums, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: kind %d, photometric %d, %d frames, %d samples in %d chunks, %d updates at most\n", kind, photo, F, a.n_samples, a.n_chunks, n_iter);
    return 0;
}
