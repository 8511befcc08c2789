// detect_check.cpp -- host check of the keypoint kernels (homography.js_amd/csrc/hg_k_detect.hip): the kernel file itself is compiled for the
// CPU behind the thread-index shim (hip_host_shim.h; <hip/hip_runtime.h> resolves to tests/cpp/hip_stub) and runs under AddressSanitizer +
// UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside the planes, the scratch, the table or an output is
// reported.  All three kernels cooperate across lanes through LDS and barriers only, so a workgroup runs as real threads (256 for
// k_detect_cells and k_detect_compact, 64 for k_detect_describe): __syncthreads is a barrier over the block, LDS is static storage.  The
// table comes from the rule of hg_detect_dev.h, as hg_describe_pattern builds it.  The case comes from a file the test writes and the outputs
// go back into a file, which the test compares with the numpy model.  A stand-alone program, no GPU.
//   in:  int32 W, H, n_planes, channels, cell, per_cell, desc_stride, want (bit 0 points, 1 desc, 2 info), slack (bytes between planes), pad;
//        int64 min_response; the planes, each followed by `slack` bytes except the last
//   out: n_planes int32 d_counts, n_planes x n_slots x 8 bytes d_points, x desc_stride bytes d_desc, x 16 bytes d_info (each filled with 0xA5
//        before; an output that is not wanted stays so, and so do the bytes 32..desc_stride of every descriptor row)
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
static pthread_barrier_t g_block;
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }

#include "hg_k_detect.hip"
using namespace hg;

template <typename T> static T get(FILE *f) { T v; if (fread(&v, sizeof v, 1, f) != 1) { printf("short input\n"); exit(2); } return v; }
template <typename T> static T *block(size_t n, int fill, std::vector<void *> &owned)      // exactly n elements, 16-byte aligned; nullptr for none
{
    if (!n) return nullptr;
    const size_t bytes = n * sizeof(T);
    void *p = bytes % 16 ? malloc(bytes) : aligned_alloc(16, bytes);          // (the size stays exact)
    owned.push_back(p);
    memset(p, fill, bytes);
    return static_cast<T *>(p);
}

struct Case {
    int W, H, P, channels, cell, per_cell, cells_x, cells_y;
    size_t plane_stride, desc_stride;
    int64_t min_response;
    const uint8_t *planes; const int8_t *table;
    DetectRec *rec; int32_t *cnt, *list;
    int32_t *out_counts; uint2 *out_points; uint8_t *out_desc; DetectRec *out_info;
};
struct Lane { const Case *c; unsigned t; int phase; };

static void *lane_main(void *arg)
{
    const Lane *l = (const Lane *)arg;
    const Case &c = *l->c;
    threadIdx = {l->t, 0, 0};
    const unsigned cells = (unsigned)(c.cells_x * c.cells_y), slots = cells * (unsigned)c.per_cell;
    if (l->phase == 0) {
        for (unsigned p = 0; p < (unsigned)c.P; p++) for (unsigned b = 0; b < cells; b++) {
            gridDim = {cells, (unsigned)c.P, 1}; blockIdx = {b, p, 0};
            k_detect_cells(c.planes, c.W, c.H, c.plane_stride, c.channels, c.cell, c.per_cell, c.cells_x, c.min_response, c.rec, c.cnt);
            pthread_barrier_wait(&g_block);                       // (the next block reuses the static LDS)
        }
    } else if (l->phase == 1) {
        for (unsigned p = 0; p < (unsigned)c.P; p++) {
            gridDim = {(unsigned)c.P, 1, 1}; blockIdx = {p, 0, 0};
            k_detect_compact(c.W, (int)cells, c.per_cell, c.desc_stride, c.rec, c.cnt, c.list, c.out_counts, c.out_points, c.out_desc, c.out_info);
            pthread_barrier_wait(&g_block);
        }
    } else {
        for (unsigned p = 0; p < (unsigned)c.P; p++) for (unsigned k = 0; k < slots; k++) {
            if (c.list[(size_t)p * slots + k] < 0) break;        // (every lane sees the same list: the padding launches nothing worth a barrier)
            gridDim = {slots, (unsigned)c.P, 1}; blockIdx = {k, p, 0};
            k_detect_describe(c.planes, c.W, c.plane_stride, c.channels, slots, c.desc_stride, c.list, c.table, c.out_desc, c.out_info);
            pthread_barrier_wait(&g_block);
        }
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

// The helpers on their own: the float words against the compiler's conversion, the direction table against its symmetries.
static int helpers_ok()
{
    for (uint32_t v = 0; v < 40000; v++) if (detect_float_bits(v) != __float_as_uint((float)v)) { printf("float word of %u differs\n", v); return 0; }
    for (int k = 0; k <= 16; k++) if (detect_cos(16 - k) != -detect_cos(k) || detect_cos(32 - k) != detect_cos(k) || detect_sin(k) != detect_cos(k + 24)) {
        printf("direction table asymmetric at %d\n", k); return 0;
    }
    return detect_bin(0, 0) == 0 && detect_bin(5, 0) == 0 && detect_bin(0, 5) == 8 && detect_bin(-5, 0) == 16 && detect_bin(0, -5) == 24 && detect_bin(7, 7) == 4;
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: detect_check IN OUT\n"); return 2; }
    if (!helpers_ok()) return 3;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Case c;
    c.W = get<int32_t>(f); c.H = get<int32_t>(f); c.P = get<int32_t>(f); c.channels = get<int32_t>(f); c.cell = get<int32_t>(f); c.per_cell = get<int32_t>(f);
    c.desc_stride = (size_t)get<int32_t>(f);
    const int want = get<int32_t>(f), slack = get<int32_t>(f);
    (void)get<int32_t>(f);
    c.min_response = get<int64_t>(f);
    if (c.W < 1 || c.W > 4096 || c.H < 1 || c.H > 4096 || c.P < 1 || c.P > 16 || (c.channels != 1 && c.channels != 4) || c.cell < 8 || c.cell > 256 || c.per_cell < 1 ||
        c.per_cell > 16 || c.desc_stride % 16 || c.desc_stride < 32 || c.desc_stride > 256 || slack < 0 || slack > 4096 || c.min_response < 1) { printf("bad case\n"); return 2; }
    c.cells_x = (c.W + c.cell - 1) / c.cell; c.cells_y = (c.H + c.cell - 1) / c.cell;
    const size_t P = (size_t)c.P, plane = (size_t)c.W * c.H * c.channels, cells = (size_t)c.cells_x * c.cells_y, slots = cells * c.per_cell;
    c.plane_stride = plane + (size_t)slack;
    std::vector<void *> owned;
    uint8_t *planes = block<uint8_t>((P - 1) * c.plane_stride + plane, 0, owned);
    if (fread(planes, 1, (P - 1) * c.plane_stride + plane, f) != (P - 1) * c.plane_stride + plane) { printf("short input\n"); return 2; }
    fclose(f);
    int8_t *table = block<int8_t>((size_t)kDetectBins * kDetectTests * 4, 0, owned);
    for (int b = 0; b < kDetectTests; b++) {
        int8_t t[4];
        detect_base_test(b, t);
        for (int k = 0; k < kDetectBins; k++) {
            int8_t *o = table + ((size_t)k * kDetectTests + b) * 4;
            detect_rotate(t[0], t[1], k, o[0], o[1]);
            detect_rotate(t[2], t[3], k, o[2], o[3]);
        }
    }
    c.planes = planes; c.table = table;
    c.rec = block<DetectRec>(P * slots, 0xEE, owned); c.cnt = block<int32_t>(P * cells, 0xEE, owned); c.list = block<int32_t>(P * slots, 0xEE, owned);
    c.out_counts = block<int32_t>(P, 0xA5, owned);
    uint2 *pts = block<uint2>(P * slots, 0xA5, owned);
    uint8_t *desc = block<uint8_t>(P * slots * c.desc_stride, 0xA5, owned);
    DetectRec *info = block<DetectRec>(P * slots, 0xA5, owned);
    c.out_points = (want & 1) ? pts : nullptr; c.out_desc = (want & 2) ? desc : nullptr; c.out_info = (want & 4) ? info : nullptr;
    if (run_phase(c, 0, kDetectBlock) || run_phase(c, 1, kDetectBlock)) return 2;
    if ((c.out_desc || c.out_info) && run_phase(c, 2, kDescribeBlock)) return 2;
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(c.out_counts, 4, P, o);
    fwrite(pts, 8, P * slots, o); fwrite(desc, c.desc_stride, P * slots, o); fwrite(info, 16, P * slots, o);
    fclose(o);
    for (void *q : owned) free(q);
    printf("host check ran: %d x %d x %d, %d planes, cell %d, per_cell %d\n", c.W, c.H, c.channels, c.P, c.cell, c.per_cell);
    return 0;
}
