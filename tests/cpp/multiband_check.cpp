// multiband_check.cpp -- host check of the multi-band mosaic's kernels: hg_k_multiband.hip itself, compiled for the CPU behind the
// thread-index shim (hip_host_shim.h) and run under AddressSanitizer + UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read
// or written outside a field, a frame, the tables, the work area, the canvas, the weight plane or the labels is reported.  k_mb_reduce
// stages its tile in LDS between two barriers, so a block of it runs as 256 real threads: __syncthreads is a barrier over the block and LDS
// is static storage.  The other kernels have no traffic between lanes and run thread by thread.  The case comes from a file the test
// writes -- the layout of the work area included, as the numpy model lays it out -- and the result goes back into a file, which the test
// compares with the model.  A stand-alone program, no GPU.
//   in:  int32 elem, C, W, H, L, n_frames, cx, cy, cw, ch, pix_front, canvas_front, has_weight, own_labels, n_part, pw, ph;  float feather;
//        uint64 fld_bytes, pix_bytes, labels_off, work_bytes, r_off[8];
//        n_frames x { int32 x_off, y_off, obj_w, obj_h; uint64 fld_off, pix_off; float gain };
//        n_part x { int32 index, gx, gy, gw, gh; uint64 flag_off, img_off[8], msk_off[8] };  the field buffer;  the pixel buffer
//   out: the canvas, the weight plane if has_weight, the labels (canvas, weight and labels filled with 0xA5 before)
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }

#include "hg_k_multiband.hip"
using namespace hg;

template <typename T> static T get(FILE *f) { T v; if (fread(&v, sizeof v, 1, f) != 1) { printf("short input\n"); exit(2); } return v; }
// An exact-size heap block whose start is aligned to 256 bytes plus `front`.
static uint8_t *block(size_t front, size_t bytes, int fill, std::vector<void *> &owned)
{
    void *raw = nullptr;
    if (posix_memalign(&raw, 256, front + bytes + (front + bytes == 0))) { printf("no memory\n"); exit(2); }
    owned.push_back(raw);
    memset(raw, fill, front + bytes);
    return (uint8_t *)raw + front;
}

struct Case {
    std::vector<MosaicFrame4> quads;
    std::vector<MbFrame> frames;
    MbCanvas cv;
    int elem, C, W, H;
    float feather;
    uint32_t blocks[kMbMaxBands];
    const uint8_t *fld, *pix;
    uint8_t *work, *canvas;
    float *weight;
    int32_t *labels;
};
struct Lane { const Case *c; unsigned tx, ty; int lv; };

template <typename E, int C> static void reduce_lane(const Lane &l)
{
    const Case &c = *l.c;
    for (uint32_t b = 0; b < c.blocks[l.lv]; b++) {
        gridDim = {c.blocks[l.lv], 1, 1}; blockIdx = {b, 0, 0};
        if (l.lv == 1) k_mb_reduce<E, C, true>(c.frames.data(), (int)c.frames.size(), l.lv, c.cv, c.pix, c.work);
        else k_mb_reduce<float, C, false>(c.frames.data(), (int)c.frames.size(), l.lv, c.cv, c.pix, c.work);
        pthread_barrier_wait(&g_block);                       // (the next block reuses the static LDS)
    }
}
template <typename E> static void reduce_lane_c(const Lane &l)
{
    switch (l.c->C) { case 1: reduce_lane<E, 1>(l); break; case 2: reduce_lane<E, 2>(l); break; case 3: reduce_lane<E, 3>(l); break; default: reduce_lane<E, 4>(l); }
}
static void *lane_main(void *arg)
{
    const Lane *l = (const Lane *)arg;
    threadIdx = {l->tx, l->ty, 0};
    if (l->c->elem == 0) reduce_lane_c<float>(*l); else reduce_lane_c<uint8_t>(*l);
    return nullptr;
}

static uint32_t tiles(int w, int h, uint32_t *tiles_x)
{
    *tiles_x = (uint32_t)((w + 63) / 64);
    return *tiles_x * (uint32_t)((h + 3) / 4);
}

template <typename E, int C> static void run(const Case &c)
{
    const MbCanvas &cv = c.cv;
    const MbFrame *fr = c.frames.empty() ? nullptr : c.frames.data();
    const int n = (int)c.frames.size();
    uint32_t tx = 0;
    const uint32_t nb = tiles(cv.cw, cv.ch, &tx);
    for (uint32_t b = 0; b < nb; b++) for (unsigned y = 0; y < 4; y++) for (unsigned x = 0; x < 64; x++) {
        gridDim = {nb, 1, 1}; blockIdx = {b, 0, 0}; threadIdx = {x, y, 0};
        k_mb_label(c.quads.empty() ? nullptr : c.quads.data(), (int)c.quads.size(), c.fld, c.W, c.H, c.feather, cv.cx, cv.cy, cv.cw, cv.ch, tx, c.labels);
    }
    for (uint32_t b = 0; b < c.blocks[0]; b++) for (unsigned x = 0; x < 256; x++) {
        gridDim = {c.blocks[0], 1, 1}; blockIdx = {b, 0, 0}; threadIdx = {x, 0, 0};
        k_mb_seed(fr, n, c.fld, cv, c.labels, c.work);
    }
    for (int lv = 1; lv < cv.L; lv++) {
        if (!c.blocks[lv]) continue;
        pthread_barrier_init(&g_block, nullptr, 256);
        std::vector<Lane> lanes(256);
        std::vector<pthread_t> th(256);
        for (unsigned t = 0; t < 256; t++) {
            lanes[t] = Lane{&c, t % kMbTileW, t / kMbTileW, lv};
            if (pthread_create(&th[t], nullptr, lane_main, &lanes[t])) { printf("cannot start a thread\n"); exit(2); }
        }
        for (unsigned t = 0; t < 256; t++) pthread_join(th[t], nullptr);
        pthread_barrier_destroy(&g_block);
    }
    for (int k = cv.L - 1; k >= 0; k--) {
        const uint32_t nk = k ? tiles(cv.pw >> k, cv.ph >> k, &tx) : tiles(cv.cw, cv.ch, &tx);
        for (uint32_t b = 0; b < nk; b++) for (unsigned y = 0; y < 4; y++) for (unsigned x = 0; x < 64; x++) {
            gridDim = {nk, 1, 1}; blockIdx = {b, 0, 0}; threadIdx = {x, y, 0};
            if (k) k_mb_blend<float, C, false>(fr, n, k, cv, c.pix, c.work, tx, c.canvas, c.weight);
            else k_mb_blend<E, C, true>(fr, n, k, cv, c.pix, c.work, tx, c.canvas, c.weight);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: multiband_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Case c;
    c.elem = get<int32_t>(f); c.C = get<int32_t>(f); c.W = get<int32_t>(f); c.H = get<int32_t>(f);
    MbCanvas &cv = c.cv;
    cv = MbCanvas{};
    cv.L = get<int32_t>(f);
    const int n_frames = get<int32_t>(f);
    cv.cx = get<int32_t>(f); cv.cy = get<int32_t>(f); cv.cw = get<int32_t>(f); cv.ch = get<int32_t>(f);
    const int pix_front = get<int32_t>(f), canvas_front = get<int32_t>(f), has_weight = get<int32_t>(f), own_labels = get<int32_t>(f), n_part = get<int32_t>(f);
    cv.pw = get<int32_t>(f); cv.ph = get<int32_t>(f);
    c.feather = get<float>(f);
    const uint64_t fld_bytes = get<uint64_t>(f), pix_bytes = get<uint64_t>(f), labels_off = get<uint64_t>(f), work_bytes = get<uint64_t>(f);
    for (int k = 0; k < kMbMaxBands; k++) cv.r_off[k] = get<uint64_t>(f);
    if (cv.cw < 1 || cv.ch < 1 || n_frames < 0 || n_frames > 4096 || n_part < 0 || n_part > n_frames || c.C < 1 || c.C > 4 || cv.L < 1 || cv.L > kMbMaxBands) { printf("bad case\n"); return 2; }
    cv.A = 1 << (cv.L - 1);
    const size_t px = (size_t)c.C * (c.elem == 0 ? 4 : 1), F = (size_t)n_frames;
    c.quads.assign((F + 3) / 4, MosaicFrame4{});
    std::vector<float> gains(F);
    for (size_t k = 0; k < F; k++) {
        MosaicFrame &r = c.quads[k / 4].f[k % 4];
        r.x_off = get<int32_t>(f); r.y_off = get<int32_t>(f); r.obj_w = get<int32_t>(f); r.obj_h = get<int32_t>(f);
        r.fld_off = get<uint64_t>(f); r.pix_off = get<uint64_t>(f);
        gains[k] = get<float>(f);
    }
    uint64_t blk[kMbMaxBands] = {0};
    for (int p = 0; p < n_part; p++) {
        MbFrame m{};
        m.index = get<int32_t>(f); m.gx = get<int32_t>(f); m.gy = get<int32_t>(f); m.gw = get<int32_t>(f); m.gh = get<int32_t>(f);
        m.flag_off = get<uint64_t>(f);
        for (int k = 0; k < kMbMaxBands; k++) m.img_off[k] = get<uint64_t>(f);
        for (int k = 0; k < kMbMaxBands; k++) m.msk_off[k] = get<uint64_t>(f);
        if (m.index < 0 || m.index >= n_frames) { printf("bad case\n"); return 2; }
        m.m = c.quads[(size_t)m.index / 4].f[m.index % 4];
        m.gain = gains[(size_t)m.index];
        m.blk0[0] = (uint32_t)blk[0];
        blk[0] += ((uint64_t)m.gw * m.gh + kMbSeedPx - 1) / kMbSeedPx;
        for (int k = 1; k < cv.L; k++) {
            m.blk0[k] = (uint32_t)blk[k];
            blk[k] += (uint64_t)(((m.gw >> k) + kMbTileW - 1) / kMbTileW) * (uint64_t)(((m.gh >> k) + kMbTileH - 1) / kMbTileH);
        }
        c.frames.push_back(m);
    }
    for (int k = 0; k < kMbMaxBands; k++) c.blocks[k] = (uint32_t)blk[k];
    std::vector<void *> owned;
    const size_t n_px = (size_t)cv.cw * cv.ch, canvas_bytes = n_px * px, weight_bytes = has_weight ? n_px * 4 : 0, label_bytes = own_labels ? n_px * 4 : 0;
    uint8_t *fld = block(0, fld_bytes, 0, owned), *pix = block((size_t)pix_front, pix_bytes, 0xEE, owned);
    c.canvas = block((size_t)canvas_front, canvas_bytes, 0xA5, owned);
    uint8_t *weight = block(0, weight_bytes, 0xA5, owned), *labels = block(0, label_bytes, 0xA5, owned);
    c.work = block(0, work_bytes, 0xA5, owned);
    if ((fld_bytes && fread(fld, 1, fld_bytes, f) != fld_bytes) || (pix_bytes && fread(pix, 1, pix_bytes, f) != pix_bytes)) { printf("short input\n"); return 2; }
    fclose(f);
    c.fld = fld; c.pix = pix;
    c.weight = has_weight ? reinterpret_cast<float *>(weight) : nullptr;
    c.labels = reinterpret_cast<int32_t *>(own_labels ? labels : c.work + labels_off);
#define RUN(E, CC) run<E, CC>(c)
#define RUNE(E) switch (c.C) { case 1: RUN(E, 1); break; case 2: RUN(E, 2); break; case 3: RUN(E, 3); break; default: RUN(E, 4); break; }
    if (c.elem == 0) RUNE(float) else RUNE(uint8_t)
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(c.canvas, 1, canvas_bytes, o); fwrite(weight, 1, weight_bytes, o); fwrite(c.labels, 1, n_px * 4, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: %d frames, %d take part, %d bands\n", n_frames, n_part, cv.L);
    return 0;
}
