// trilinear_check.cpp -- host check of the pyramid and trilinear remap kernels (k_pyr_down, k_remap_trilinear_frames; hg_k_pyramid.hip).
// The kernel file itself is compiled for the CPU behind the thread-index shim (hip_host_shim.h) and run block by block, thread by thread,
// under AddressSanitizer + UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside a field, a plane, a pyramid,
// the tables or the output is reported, and so is a misaligned wide load or store.  The case comes from a file the test writes and the
// pyramids and the output go back into a file, which the test compares with the numpy model -- x86 f32 arithmetic with contraction off is
// the GPU's.  A stand-alone program: host code only, no GPU.
//   in:  int32 elem, C, W, H, levels, n_planes, n_frames, plane_front;  uint64 blk_px, plane_stride, pyr_front, pyr_stride, fld_bytes, out_bytes;
//        n_frames x { int32 obj_w, obj_h; uint64 fld_off, out_off };  the field buffer;  the planes (n_planes x plane_stride bytes)
//   out: the pyramid allocation behind pyr_front (n_planes x pyr_stride bytes), then the output buffer (filled with 0xA5 before the run)
#include "hip_host_shim.h"
#include "hg_k_pyramid.hip"
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
static void run(int W, int H, int levels, int n_planes, int n_frames, uint64_t blk_px, const std::vector<TriRemapFrame> &frames, uint32_t n_blocks,
                const uint8_t *fld, const uint8_t *planes, size_t plane_stride, uint8_t *pyr, size_t pyr_stride, const std::vector<uint64_t> &offs, uint8_t *out)
{
    const uint8_t *src = planes;
    size_t src_stride = plane_stride;
    int ws = W, hs = H;
    for (int k = 1; k < levels; k++) {
        const int wd = (ws + 1) >> 1, hd = (hs + 1) >> 1;
        // a grid smaller than the level in y and in planes, so that the strided loops run
        const dim3s grid = {(unsigned)((wd + 63) / 64), (unsigned)std::max(1, std::min((hd + 3) / 4, 3)), (unsigned)std::max(1, n_planes - 1)};
        for (unsigned bz = 0; bz < grid.z; bz++) for (unsigned by = 0; by < grid.y; by++) for (unsigned bx = 0; bx < grid.x; bx++)
            for (unsigned ty = 0; ty < 4; ty++) for (unsigned tx = 0; tx < 64; tx++) {
                gridDim = grid; blockIdx = {bx, by, bz}; threadIdx = {tx, ty, 0};
                k_pyr_down<E, C>(src, src_stride, ws, hs, pyr + offs[k], pyr_stride, wd, hd, n_planes);
            }
        src = pyr + offs[k]; src_stride = pyr_stride; ws = wd; hs = hd;
    }
    std::vector<uint64_t> tab(offs.begin(), offs.begin() + levels);      // exact-size tables
    std::vector<TriRemapFrame> fr = frames;
    for (uint32_t b = 0; b < n_blocks; b++) for (unsigned t = 0; t < 256; t++) {
        gridDim = {n_blocks, 1, 1}; blockIdx = {b, 0, 0}; threadIdx = {t, 0, 0};
        k_remap_trilinear_frames<E, C>(fr.data(), n_frames, blk_px, tab.data(), levels, fld, planes, pyr, W, H, out);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: trilinear_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int elem = get<int32_t>(f), C = get<int32_t>(f), W = get<int32_t>(f), H = get<int32_t>(f), levels = get<int32_t>(f);
    const int n_planes = get<int32_t>(f), n_frames = get<int32_t>(f), plane_front = get<int32_t>(f);
    const uint64_t blk_px = get<uint64_t>(f), plane_stride = get<uint64_t>(f), pyr_front = get<uint64_t>(f), pyr_stride = get<uint64_t>(f);
    const uint64_t fld_bytes = get<uint64_t>(f), out_bytes = get<uint64_t>(f);
    const size_t px = (size_t)C * (elem == 0 ? 4 : 1);
    std::vector<TriRemapFrame> frames((size_t)n_frames);
    uint64_t b = 0;
    for (int k = 0; k < n_frames; k++) {
        const int ow = get<int32_t>(f), oh = get<int32_t>(f);
        TriRemapFrame &r = frames[(size_t)k];
        r.fld_off = get<uint64_t>(f); r.out_off = get<uint64_t>(f);
        r.n_px = (ow > 0 && oh > 0) ? (uint64_t)ow * (uint64_t)oh : 0;
        r.plane_off = (uint64_t)(k % n_planes) * plane_stride; r.pyr_off = (uint64_t)(k % n_planes) * pyr_stride;
        r.blk0 = (uint32_t)b; r.obj_w = (uint32_t)std::max(ow, 0); r.obj_h = (uint32_t)std::max(oh, 0); r.pad = 0;
        b += (r.n_px + blk_px - 1) / blk_px;
    }
    std::vector<uint64_t> offs(32, 0);
    uint64_t off = 0;
    for (int k = 1, w = W, h = H; k < levels; k++) { w = (w + 1) >> 1; h = (h + 1) >> 1; offs[(size_t)k] = off; off += ((uint64_t)w * h * px + 255) & ~255ull; }
    if (n_planes > 1 && pyr_stride < off) { printf("pyr_stride too small\n"); return 2; }
    std::vector<void *> owned;
    const size_t planes_bytes = (size_t)(n_planes - 1) * plane_stride + (size_t)W * H * px;          // exact: the last plane ends the block
    const size_t pyr_bytes = levels > 1 ? (size_t)(n_planes - 1) * pyr_stride + off : 0;
    uint8_t *fld = block(0, fld_bytes, 0, owned), *planes = block((size_t)plane_front, planes_bytes, 0xEE, owned);
    uint8_t *pyr = block((size_t)pyr_front, pyr_bytes, 0xA5, owned), *out = block(0, out_bytes, 0xA5, owned);
    if ((fld_bytes && fread(fld, 1, fld_bytes, f) != fld_bytes) || fread(planes, 1, planes_bytes, f) != planes_bytes) { printf("short input\n"); return 2; }
    fclose(f);
#define RUN(E, CC) run<E, CC>(W, H, levels, n_planes, n_frames, blk_px, frames, (uint32_t)b, fld, planes, plane_stride, pyr, pyr_stride, offs, out)
#define RUNE(E) switch (C) { case 1: RUN(E, 1); break; case 2: RUN(E, 2); break; case 3: RUN(E, 3); break; case 4: RUN(E, 4); break; default: return 2; }
    if (elem == 0) RUNE(float) else RUNE(uint8_t)
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(pyr, 1, pyr_bytes, o); fwrite(out, 1, out_bytes, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: %d frames, %u blocks, %d levels\n", n_frames, (unsigned)b, levels);
    return 0;
}
