// mosaic_gain_check.cpp -- host check of the mosaic's exposure kernels: k_mosaic_stats (hg_k_mosaic_stats.hip) and the gained instantiation
// of k_mosaic_frames (hg_k_mosaic.hip).  The kernel files themselves are compiled for the CPU behind the thread-index shim (hip_host_shim.h)
// and run under AddressSanitizer + UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside a field, a frame,
// the table, the gains, the statistics, the canvas or the weight plane is reported.  k_mosaic_stats talks across lanes, so a block runs as
// 256 real threads here: __syncthreads is a barrier over the block, a ballot, a shuffle and the wave reduction built on it exchange their
// values through one slot per lane between two barriers over the wave, LDS is static storage, the atomics are the host's.  The gained
// mosaic has no such traffic and runs thread by thread, as tests/cpp/mosaic_check.cpp runs the plain one.  The case comes from a file the
// test writes and the result goes back into a file, which the test compares with the numpy models.  A stand-alone program, no GPU.
//   in:  int32 kind (0: statistics, 1: gained mosaic), elem, C, W, H, mode, n_frames, cx, cy, cw, ch, pix_front, canvas_front, has_weight,
//        feather (the float's bits);  uint64 fld_bytes, pix_bytes;  n_frames x { int32 x_off, y_off, obj_w, obj_h; uint64 fld_off, pix_off };
//        kind 1: n_frames float gains;  the field buffer;  the pixel buffer
//   out: kind 0: n_frames x n_frames x 2 uint64;  kind 1: the canvas, then the weight plane if has_weight (both filled with 0xA5 before)
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
static pthread_barrier_t g_block, g_wave[4];
static uint64_t g_slot[4][64];
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
// every lane of the wave leaves its value, waits, reads what it needs, and waits again before the slots are reused
template <typename T, typename F> static inline T wave_exchange(T v, F pick)
{
    const unsigned w = threadIdx.y;
    uint64_t bits = 0;
    memcpy(&bits, &v, sizeof v);
    g_slot[w][threadIdx.x] = bits;
    pthread_barrier_wait(&g_wave[w]);
    const T r = pick(g_slot[w]);
    pthread_barrier_wait(&g_wave[w]);
    return r;
}
static inline uint64_t __ballot(int p)
{
    return wave_exchange<uint64_t>(p ? 1 : 0, [](const uint64_t *s) { uint64_t m = 0; for (int l = 0; l < 64; l++) m |= (s[l] & 1) << l; return m; });
}
template <typename T> static inline T __shfl(T v, int src) { return wave_exchange<T>(v, [=](const uint64_t *s) { T r; memcpy(&r, &s[src & 63], sizeof r); return r; }); }
template <typename T> static inline T __shfl_xor(T v, int mask)
{
    const unsigned l = threadIdx.x;
    return wave_exchange<T>(v, [=](const uint64_t *s) { T r; memcpy(&r, &s[(l ^ (unsigned)mask) & 63], sizeof r); return r; });
}
template <typename T> static inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

#include "hg_k_mosaic.hip"
#include "hg_k_mosaic_stats.hip"
using namespace hg;

template <typename T> static T get(FILE *f) { T v; if (fread(&v, sizeof v, 1, f) != 1) { printf("short input\n"); exit(2); } return v; }
// An exact-size heap block whose start is aligned to 16 bytes plus `front`.
static uint8_t *block(size_t front, size_t bytes, int fill, std::vector<void *> &owned)
{
    uint8_t *p = (uint8_t *)malloc(front + bytes);
    owned.push_back(p);
    memset(p, fill, front + bytes);
    return p + front;
}

struct Case {
    std::vector<MosaicFrame4> table;                          // exact size: quads of records, the last one filled with empty frames
    int n_frames, C, W, H, mode, cx, cy, cw, ch;
    float feather;
    const uint8_t *fld, *pix;
    uint8_t *canvas;
    float *weight;
    const float *gains;                                       // one per record of the table, exact size
    unsigned long long *stats;
    uint32_t tiles_x, n_blocks;
};
struct Lane { const Case *c; unsigned tx, ty; };

template <int C> static void stats_thread(const Case &c)
{
    for (uint32_t b = 0; b < c.n_blocks; b++) {
        gridDim = {c.n_blocks, 1, 1}; blockIdx = {b, 0, 0};
        k_mosaic_stats<C>(c.table.data(), c.n_frames, c.fld, c.pix, c.cx, c.cy, c.cw, c.ch, c.tiles_x, c.stats);
        pthread_barrier_wait(&g_block);                       // (the next block reuses the static LDS)
    }
}
static void *lane_main(void *arg)
{
    const Lane *l = (const Lane *)arg;
    threadIdx = {l->tx, l->ty, 0};
    switch (l->c->C) { case 1: stats_thread<1>(*l->c); break; case 2: stats_thread<2>(*l->c); break; case 3: stats_thread<3>(*l->c); break; default: stats_thread<4>(*l->c); }
    return nullptr;
}

template <typename E, int C> static void run_gain(const Case &c)
{
    for (uint32_t b = 0; b < c.n_blocks; b++) for (unsigned ty = 0; ty < 4; ty++) for (unsigned tx = 0; tx < 64; tx++) {
        gridDim = {c.n_blocks, 1, 1}; blockIdx = {b, 0, 0}; threadIdx = {tx, ty, 0};
        k_mosaic_frames<E, C, true>(c.table.empty() ? nullptr : c.table.data(), (int)c.table.size(), c.fld, c.pix, c.W, c.H, c.mode, c.feather, c.cx, c.cy, c.cw, c.ch,
                                    c.tiles_x, c.canvas, c.weight, c.gains);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: mosaic_gain_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Case c;
    const int kind = get<int32_t>(f), elem = get<int32_t>(f);
    c.C = get<int32_t>(f); c.W = get<int32_t>(f); c.H = get<int32_t>(f); c.mode = get<int32_t>(f); c.n_frames = get<int32_t>(f);
    c.cx = get<int32_t>(f); c.cy = get<int32_t>(f); c.cw = get<int32_t>(f); c.ch = get<int32_t>(f);
    const int pix_front = get<int32_t>(f), canvas_front = get<int32_t>(f), has_weight = get<int32_t>(f);
    c.feather = get<float>(f);
    const uint64_t fld_bytes = get<uint64_t>(f), pix_bytes = get<uint64_t>(f);
    if (c.cw < 1 || c.ch < 1 || c.n_frames < 0 || c.n_frames > 256 || c.C < 1 || c.C > 4 || (kind == 0 && elem != 1)) { printf("bad case\n"); return 2; }
    const size_t px = (size_t)c.C * (elem == 0 ? 4 : 1), F = (size_t)c.n_frames;
    c.table.assign((F + 3) / 4, MosaicFrame4{});
    for (size_t k = 0; k < F; k++) {
        MosaicFrame &r = c.table[k / 4].f[k % 4];
        r.x_off = get<int32_t>(f); r.y_off = get<int32_t>(f); r.obj_w = get<int32_t>(f); r.obj_h = get<int32_t>(f);
        r.fld_off = get<uint64_t>(f); r.pix_off = get<uint64_t>(f);
    }
    std::vector<void *> owned;
    float *gains = reinterpret_cast<float *>(block(0, c.table.size() * 16, 0, owned));
    for (size_t k = 0; k < c.table.size() * 4; k++) gains[k] = kind == 1 && k < F ? get<float>(f) : 1.0f;
    c.gains = gains;
    const size_t canvas_bytes = (size_t)c.cw * c.ch * px, weight_bytes = has_weight ? (size_t)c.cw * c.ch * 4 : 0, stats_bytes = F * F * 16;
    uint8_t *fld = block(0, fld_bytes, 0, owned), *pix = block((size_t)pix_front, pix_bytes, 0xEE, owned);
    c.canvas = block((size_t)canvas_front, canvas_bytes, 0xA5, owned);
    uint8_t *weight = block(0, weight_bytes, 0xA5, owned);
    c.stats = reinterpret_cast<unsigned long long *>(block(0, stats_bytes, 0, owned));
    if ((fld_bytes && fread(fld, 1, fld_bytes, f) != fld_bytes) || (pix_bytes && fread(pix, 1, pix_bytes, f) != pix_bytes)) { printf("short input\n"); return 2; }
    fclose(f);
    c.fld = fld; c.pix = pix;
    c.weight = has_weight ? reinterpret_cast<float *>(weight) : nullptr;
    c.tiles_x = (uint32_t)((c.cw + 63) / 64);
    c.n_blocks = c.tiles_x * (uint32_t)((c.ch + 3) / 4);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    if (kind == 0) {
        if (F) {
            pthread_barrier_init(&g_block, nullptr, 256);
            for (int w = 0; w < 4; w++) pthread_barrier_init(&g_wave[w], nullptr, 64);
            std::vector<Lane> lanes(256);
            std::vector<pthread_t> th(256);
            for (unsigned t = 0; t < 256; t++) {
                lanes[t] = Lane{&c, t % 64, t / 64};
                if (pthread_create(&th[t], nullptr, lane_main, &lanes[t])) { printf("cannot start a thread\n"); return 2; }
            }
            for (unsigned t = 0; t < 256; t++) pthread_join(th[t], nullptr);
        }
        fwrite(c.stats, 1, stats_bytes, o);
    } else {
#define RUN(E, CC) run_gain<E, CC>(c)
#define RUNE(E) switch (c.C) { case 1: RUN(E, 1); break; case 2: RUN(E, 2); break; case 3: RUN(E, 3); break; default: RUN(E, 4); break; }
        if (elem == 0) RUNE(float) else RUNE(uint8_t)
        fwrite(c.canvas, 1, canvas_bytes, o); fwrite(weight, 1, weight_bytes, o);
    }
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: kind %d, %d frames, %u blocks, mode %d\n", kind, c.n_frames, c.n_blocks, c.mode);
    return 0;
}
