// tps_check.cpp -- host check of the thin-plate kernels (homography.js_amd/csrc/hg_k_tps.hip): the kernel file itself is compiled for the CPU
// behind the thread-index shim (hip_host_shim.h; <hip/hip_runtime.h> resolves to tests/cpp/hip_stub) and runs under AddressSanitizer +
// UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside the point lists, the records, the scratch, the
// nodes, the field or the point results is reported.  k_tps_solve cooperates across lanes, so its workgroup runs as real threads (256 with
// the matrix in LDS, 1024 with the matrix in scratch): __syncthreads is a barrier over the block, LDS is static storage.  The field, blend
// and point kernels have no barrier: their lanes run one after the other.  The case comes from a file the test writes and the outputs go
// back into a file, which the test compares with the numpy model (tests/hgtest/tps.py).  A stand-alone program, no GPU.
//   in:  int32 n_points, n_frames, n_from_sets, n_to_sets, W, H, fmt, step, n_pts, n_sets; double lambda; the from lists, the to lists
//        (float32), n_frames x 4 int32 windows, n_sets x n_pts x 2 float32 positions
//   out: the records, n_frames int32 status, the field (frames packed at the 256-byte grain, filled with 0xA5 before), n_frames x n_pts x 2
//        float32 point results
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
#define __builtin_amdgcn_readfirstlane(x) (x)
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }

#include "hg_k_tps.hip"
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

struct Lane { const TpsSolveArgs *a; unsigned t; bool lds; };

static void *solve_lane(void *arg)
{
    const Lane *l = (const Lane *)arg;
    threadIdx = {l->t, 0, 0};
    for (unsigned f = 0; f < (unsigned)l->a->n_frames; f++) {
        gridDim = {(unsigned)l->a->n_frames, 1, 1}; blockIdx = {f, 0, 0};
        if (l->lds) k_tps_solve<true>(*l->a); else k_tps_solve<false>(*l->a);
        pthread_barrier_wait(&g_block);                       // (the next block reuses the static LDS)
    }
    return nullptr;
}

template <typename K> static void grid_64x4(unsigned gx, unsigned gy, K kernel)
{
    for (unsigned by = 0; by < gy; by++) for (unsigned bx = 0; bx < gx; bx++) for (unsigned ty = 0; ty < 4; ty++) for (unsigned tx = 0; tx < 64; tx++) {
        gridDim = {gx, gy, 1}; blockIdx = {bx, by, 0}; threadIdx = {tx, ty, 0};
        kernel();
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: tps_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t v[10];
    for (int k = 0; k < 10; k++) v[k] = get<int32_t>(f);
    const double lambda = get<double>(f);
    const int N = v[0], F = v[1], NF = v[2], NT = v[3], W = v[4], H = v[5], fmt = v[6], step = v[7], n_pts = v[8], n_sets = v[9];
    if (N < 3 || N > kTpsMaxPoints || F < 1 || F > 16 || NF < 1 || NT < 1 || W < 1 || H < 1 || fmt < 0 || fmt > 1 || step < 1 || step > 32 || (step & (step - 1)) ||
        n_pts < 0 || n_pts > 4096 || n_sets < 1 || !(lambda >= 0.0)) { printf("bad case\n"); return 2; }
    std::vector<void *> owned;
    float *from = block<float>((size_t)NF * N * 2, 0, owned), *to = block<float>((size_t)NT * N * 2, 0, owned);
    int32_t *win = block<int32_t>((size_t)F * 4, 0, owned);
    float *pts = block<float>((size_t)n_sets * n_pts * 2, 0, owned);
    if (fread(from, 8, (size_t)NF * N, f) != (size_t)NF * N || fread(to, 8, (size_t)NT * N, f) != (size_t)NT * N || fread(win, 16, (size_t)F, f) != (size_t)F ||
        fread(pts, 8, (size_t)n_sets * n_pts, f) != (size_t)n_sets * n_pts) { printf("short input\n"); return 2; }
    fclose(f);

    // the solve
    const int M = N + 3, recd = tps_record_doubles(N);
    const bool lds = tps_in_lds(N);
    TpsSolveArgs sa{from, NF, to, NT, N, F, lambda, block<double>((size_t)F * recd, 0xA5, owned), block<int32_t>((size_t)F, 0xA5, owned),
                    lds ? nullptr : block<double>((size_t)F * M * M, 0xEE, owned)};
    const unsigned B = lds ? kTpsSolveBlock : kTpsSolveBlockBig;
    pthread_barrier_init(&g_block, nullptr, B);
    std::vector<Lane> lanes(B);
    std::vector<pthread_t> th(B);
    for (unsigned t = 0; t < B; t++) {
        lanes[t] = Lane{&sa, t, lds};
        if (pthread_create(&th[t], nullptr, solve_lane, &lanes[t])) { printf("cannot start a thread\n"); return 2; }
    }
    for (unsigned t = 0; t < B; t++) pthread_join(th[t], nullptr);

    // the field
    const size_t px = fmt == 0 ? 4 : 8;
    std::vector<TpsFrame> frames((size_t)F);
    size_t foff = 0, noff = 0;
    int mw = 0, mh = 0;
    for (int k = 0; k < F; k++) {
        const int w = win[4 * k + 2], h = win[4 * k + 3];
        frames[k] = TpsFrame{win[4 * k], win[4 * k + 1], w, h, foff, noff};
        if (w > 0 && h > 0) {
            foff += ((size_t)w * h * px + 255) & ~(size_t)255;
            if (step > 1) noff += ((size_t)tps_nodes(w, step) * tps_nodes(h, step) * 16 + 255) & ~(size_t)255;
            mw = std::max(mw, w); mh = std::max(mh, h);
        }
    }
    uint8_t *field = block<uint8_t>(foff, 0xA5, owned), *nodes = block<uint8_t>(noff, 0xEE, owned);
    TpsFieldArgs fa{sa.records, N, frames.data(), F, mw, mh, W, H, step, field, nodes};
    if (mw > 0) {
        const unsigned gx = (unsigned)(mh + 3) / 4;
        if (step == 1) {
            if (fmt == 0) grid_64x4(gx, F, [&] { k_tps_field<0, false>(fa, fa.records, fa.frames, fa.field); });
            else grid_64x4(gx, F, [&] { k_tps_field<1, false>(fa, fa.records, fa.frames, fa.field); });
        } else {
            grid_64x4((unsigned)(tps_nodes(mh, step) + 3) / 4, F, [&] { k_tps_field<1, true>(fa, fa.records, fa.frames, fa.nodes); });
            if (fmt == 0) grid_64x4(gx, F, [&] { k_tps_blend<0>(fa); }); else grid_64x4(gx, F, [&] { k_tps_blend<1>(fa); });
        }
    }

    // the point lists
    float *pout = block<float>((size_t)F * n_pts * 2, 0xA5, owned);
    for (unsigned fr = 0; fr < (unsigned)F && n_pts > 0; fr++) for (unsigned bx = 0; bx < (unsigned)(n_pts + 255) / 256; bx++) for (unsigned t = 0; t < 256; t++) {
        gridDim = {(unsigned)(n_pts + 255) / 256, (unsigned)F, 1}; blockIdx = {bx, fr, 0}; threadIdx = {t, 0, 0};
        k_tps_points(sa.records, N, pts, n_pts, n_sets, pout);
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(sa.records, 8, (size_t)F * recd, o); fwrite(sa.status, 4, (size_t)F, o);
    if (foff) fwrite(field, 1, foff, o);
    if (n_pts) fwrite(pout, 8, (size_t)F * n_pts, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: %d points, %d frames, matrix in %s, format %d, step %d, %d positions\n", N, F, lds ? "LDS" : "scratch", fmt, step, n_pts);
    return 0;
}
