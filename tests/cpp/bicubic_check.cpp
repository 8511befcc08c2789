// bicubic_check.cpp -- host check of the bicubic remap kernel (k_remap_bicubic_frames; hg_k_bicubic.hip).  The kernel file itself is
// compiled for the CPU behind the thread-index shim (hip_host_shim.h) and run block by block, thread by thread, under AddressSanitizer +
// UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside a field, a plane, the table or the output is
// reported, so is a misaligned wide load or store, and so is a negative float converted to an unsigned byte (the cubic's negative lobes).
// The case comes from a file the test writes and the output goes back into a file, which the test compares with the numpy model -- x86 f32
// arithmetic with contraction off is the GPU's.  A stand-alone program: host code only, no GPU.
//   in:  int32 elem, C, W, H, n_planes, n_frames, plane_front, pad;  float p3, p2, p0, q3, q2, q1, q0, pad;
//        uint64 blk_px, plane_stride, fld_bytes, out_bytes;  n_frames x { int32 obj_w, obj_h; uint64 fld_off, out_off };
//        the field buffer;  the planes ((n_planes - 1) x plane_stride bytes + one plane)
//   out: the output buffer (filled with 0xA5 before the run)
#include "hip_host_shim.h"
#include "hg_k_bicubic.hip"
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

template <typename E, int C>
static void run(int W, int H, int n_frames, uint64_t blk_px, const CubicCoef &k, const std::vector<RemapFrame> &frames, uint32_t n_blocks,
                const uint8_t *fld, const uint8_t *planes, size_t plane_stride, uint8_t *out)
{
    std::vector<RemapFrame> fr = frames;                     // an exact-size table
    for (uint32_t b = 0; b < n_blocks; b++) for (unsigned t = 0; t < 256; t++) {
        gridDim = {n_blocks, 1, 1}; blockIdx = {b, 0, 0}; threadIdx = {t, 0, 0};
        k_remap_bicubic_frames<E, C>(fr.data(), n_frames, blk_px, k, fld, planes, plane_stride, W, H, out);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: bicubic_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int elem = get<int32_t>(f), C = get<int32_t>(f), W = get<int32_t>(f), H = get<int32_t>(f);
    const int n_planes = get<int32_t>(f), n_frames = get<int32_t>(f), plane_front = get<int32_t>(f);
    (void)get<int32_t>(f);
    CubicCoef k;
    k.p3 = get<float>(f); k.p2 = get<float>(f); k.p0 = get<float>(f); k.q3 = get<float>(f); k.q2 = get<float>(f); k.q1 = get<float>(f); k.q0 = get<float>(f);
    (void)get<float>(f);
    const uint64_t blk_px = get<uint64_t>(f), plane_stride = get<uint64_t>(f), fld_bytes = get<uint64_t>(f), out_bytes = get<uint64_t>(f);
    const size_t px = (size_t)C * (elem == 0 ? 4 : 1);
    std::vector<RemapFrame> frames((size_t)n_frames);
    uint64_t b = 0;
    for (int n = 0; n < n_frames; n++) {
        const int ow = get<int32_t>(f), oh = get<int32_t>(f);
        RemapFrame &r = frames[(size_t)n];
        r.fld_off = get<uint64_t>(f); r.out_off = get<uint64_t>(f);
        r.n_px = (ow > 0 && oh > 0) ? (uint64_t)ow * (uint64_t)oh : 0;
        r.blk0 = (uint32_t)b; r.plane = (uint32_t)(n % n_planes);
        b += (r.n_px + blk_px - 1) / blk_px;
    }
    std::vector<void *> owned;
    const size_t planes_bytes = (size_t)(n_planes - 1) * plane_stride + (size_t)W * H * px;          // exact: the last plane ends the block
    uint8_t *fld = block(0, fld_bytes, 0, owned), *planes = block((size_t)plane_front, planes_bytes, 0xEE, owned);
    uint8_t *out = block(0, out_bytes, 0xA5, owned);
    if ((fld_bytes && fread(fld, 1, fld_bytes, f) != fld_bytes) || fread(planes, 1, planes_bytes, f) != planes_bytes) { printf("short input\n"); return 2; }
    fclose(f);
#define RUN(E, CC) run<E, CC>(W, H, n_frames, blk_px, k, frames, (uint32_t)b, fld, planes, plane_stride, out)
#define RUNE(E) switch (C) { case 1: RUN(E, 1); break; case 2: RUN(E, 2); break; case 3: RUN(E, 3); break; case 4: RUN(E, 4); break; default: return 2; }
    if (elem == 0) RUNE(float) else RUNE(uint8_t)
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(out, 1, out_bytes, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: %d frames, %u blocks\n", n_frames, (unsigned)b);
    return 0;
}
