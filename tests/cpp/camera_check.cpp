// camera_check.cpp -- host check of the camera kernels (homography.js_amd/csrc/hg_k_camera.hip): the kernel file itself is compiled for the CPU
// behind the thread-index shim (hip_host_shim.h; <hip/hip_runtime.h> resolves to tests/cpp/hip_stub) and runs under AddressSanitizer +
// UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside the records, the frame table, the point lists,
// the field or the point results is reported.  k_camera_field cooperates across lanes (the column and row terms go through LDS), so its
// workgroup runs as 256 real threads: __syncthreads is a barrier over the block, LDS is static storage.  The point kernels have no barrier:
// their lanes run one after the other.  The case comes from a file the test writes and the outputs go back into a file, which the test
// compares with the numpy model (tests/hgtest/camera.py).  A stand-alone program, no GPU.
//   in:  int32 n_frames, W, H, fmt, surface, n_pts, n_sets, 0; double scale, u0, v0; n_frames x 32 doubles; n_frames x 4 int32 windows;
//        n_sets x n_pts x 2 float32 positions
//   out: the field (frames packed at the 256-byte grain, filled with 0xA5 before), then n_frames x n_pts x 2 float32 canvas -> source
//        results, then as many source -> canvas results
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
#define __builtin_amdgcn_readfirstlane(x) (x)
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }

#include "hg_k_camera.hip"
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

struct Lane { const CamFieldArgs *a; unsigned t, gx, gy; int fmt, surface; };

template <int FMT> static void field_block(const CamFieldArgs &a, int surface)
{
    if (surface == kCamPlane) k_camera_field<FMT, kCamPlane>(a, a.records, a.frames, a.field);
    else if (surface == kCamCylinder) k_camera_field<FMT, kCamCylinder>(a, a.records, a.frames, a.field);
    else k_camera_field<FMT, kCamSphere>(a, a.records, a.frames, a.field);
}

static void *field_lane(void *arg)
{
    const Lane *l = (const Lane *)arg;
    threadIdx = {l->t, 0, 0};
    for (unsigned by = 0; by < l->gy; by++) for (unsigned bx = 0; bx < l->gx; bx++) {
        gridDim = {l->gx, l->gy, 1}; blockIdx = {bx, by, 0};
        if (l->fmt == 0) field_block<0>(*l->a, l->surface); else field_block<1>(*l->a, l->surface);
        pthread_barrier_wait(&g_block);                       // (the next block reuses the static LDS)
    }
    return nullptr;
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: camera_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t v[8];
    for (int k = 0; k < 8; k++) v[k] = get<int32_t>(f);
    const double scale = get<double>(f), u0 = get<double>(f), v0 = get<double>(f);
    const int F = v[0], W = v[1], H = v[2], fmt = v[3], surface = v[4], n_pts = v[5], n_sets = v[6];
    if (F < 1 || F > 16 || W < 1 || H < 1 || fmt < 0 || fmt > 1 || surface < 0 || surface > 2 || n_pts < 0 || n_pts > 4096 || n_sets < 1 || !(scale > 0.0)) {
        printf("bad case\n"); return 2;
    }
    std::vector<void *> owned;
    double *records = block<double>((size_t)F * kCamRecord, 0, owned);
    int32_t *win = block<int32_t>((size_t)F * 4, 0, owned);
    float *pts = block<float>((size_t)n_sets * n_pts * 2, 0, owned);
    if (fread(records, 8, (size_t)F * kCamRecord, f) != (size_t)F * kCamRecord || fread(win, 16, (size_t)F, f) != (size_t)F ||
        fread(pts, 8, (size_t)n_sets * n_pts, f) != (size_t)n_sets * n_pts) { printf("short input\n"); return 2; }
    fclose(f);

    // the field
    const size_t px = fmt == 0 ? 4 : 8;
    CamFrame *frames = block<CamFrame>((size_t)F, 0, owned);
    size_t foff = 0;
    int mw = 0, mh = 0;
    for (int k = 0; k < F; k++) {
        const int w = win[4 * k + 2], h = win[4 * k + 3];
        frames[k] = CamFrame{win[4 * k], win[4 * k + 1], w, h, foff, 0};
        if (w > 0 && h > 0) { foff += ((size_t)w * h * px + 255) & ~(size_t)255; mw = std::max(mw, w); mh = std::max(mh, h); }
    }
    // (the packed total ends on the 256-byte grain: cut the last frame's padding off, so that a write behind its last pixel is caught)
    size_t fbytes = 0;
    for (int k = 0; k < F; k++) if (frames[k].obj_w > 0 && frames[k].obj_h > 0) fbytes = frames[k].out_off + (size_t)frames[k].obj_w * frames[k].obj_h * px;
    uint8_t *field = block<uint8_t>(fbytes, 0xA5, owned);
    CamFieldArgs fa{records, frames, F, mw, mh, cam_pieces(mw), W, H, scale, u0, v0, field};
    if (mw > 0) {
        const unsigned B = kCamPiece, gx = (unsigned)(cam_pieces(mw) * cam_bands(mh));
        pthread_barrier_init(&g_block, nullptr, B);
        std::vector<Lane> lanes(B);
        std::vector<pthread_t> th(B);
        for (unsigned t = 0; t < B; t++) {
            lanes[t] = Lane{&fa, t, gx, (unsigned)F, fmt, surface};
            if (pthread_create(&th[t], nullptr, field_lane, &lanes[t])) { printf("cannot start a thread\n"); return 2; }
        }
        for (unsigned t = 0; t < B; t++) pthread_join(th[t], nullptr);
    }

    // the point lists, both directions
    float *to_src = block<float>((size_t)F * n_pts * 2, 0xA5, owned), *to_cnv = block<float>((size_t)F * n_pts * 2, 0xA5, owned);
    for (int dir = 0; dir < 2; dir++) {
        CamPointArgs pa{records, F, surface, scale, u0, v0, pts, n_pts, n_sets, dir == 0 ? to_src : to_cnv};
        for (unsigned fr = 0; fr < (unsigned)F && n_pts > 0; fr++) for (unsigned bx = 0; bx < (unsigned)(n_pts + 255) / 256; bx++) for (unsigned t = 0; t < 256; t++) {
            gridDim = {(unsigned)(n_pts + 255) / 256, (unsigned)F, 1}; blockIdx = {bx, fr, 0}; threadIdx = {t, 0, 0};
            if (dir == 0) k_camera_points<true>(pa, pa.records, pa.points, pa.out); else k_camera_points<false>(pa, pa.records, pa.points, pa.out);
        }
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    if (fbytes) fwrite(field, 1, fbytes, o);
    if (n_pts) { fwrite(to_src, 8, (size_t)F * n_pts, o); fwrite(to_cnv, 8, (size_t)F * n_pts, o); }
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: %d frames, format %d, surface %d, %zu field bytes, %d positions\n", F, fmt, surface, fbytes, n_pts);
    return 0;
}
