// mosaic_check.cpp -- host check of the mosaic kernel (k_mosaic_frames; hg_k_mosaic.hip).
// The kernel file itself is compiled for the CPU behind the thread-index shim (hip_host_shim.h) and run block by block, thread by thread,
// under AddressSanitizer + UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside a field, a frame, the table, the canvas or the weight plane is reported, and so is a
// misaligned wide load or store.  The case comes from a file the test writes and the canvas and the weights go back into a file, which the
// test compares with the numpy model -- x86 f32 arithmetic with contraction off is the GPU's.  A stand-alone program: host code only, no GPU.
//   in:  int32 elem, C, W, H, mode, n_frames, cx, cy, cw, ch, pix_front, canvas_front, has_weight, feather (the float's bits);
//        uint64 fld_bytes, pix_bytes;  n_frames x { int32 x_off, y_off, obj_w, obj_h; uint64 fld_off, pix_off };  the field buffer;  the pixel buffer
//   out: the canvas (cw x ch pixels), then the weight plane if has_weight (both filled with 0xA5 before the run)
#include "hip_host_shim.h"
#include "hg_k_mosaic.hip"
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
static unsigned run(const std::vector<MosaicFrame> &frames, const uint8_t *fld, const uint8_t *pix, int W, int H, int mode, float feather,
                    int cx, int cy, int cw, int ch, uint8_t *canvas, float *weight)
{
    std::vector<MosaicFrame4> fr((frames.size() + 3) / 4, MosaicFrame4{});      // an exact-size table: quads of records, the last one filled with empty frames
    for (size_t f = 0; f < frames.size(); f++) fr[f / 4].f[f % 4] = frames[f];
    const uint32_t tiles_x = (uint32_t)((cw + 63) / 64), n_blocks = tiles_x * (uint32_t)((ch + 3) / 4);
    for (uint32_t b = 0; b < n_blocks; b++) for (unsigned ty = 0; ty < 4; ty++) for (unsigned tx = 0; tx < 64; tx++) {
        gridDim = {n_blocks, 1, 1}; blockIdx = {b, 0, 0}; threadIdx = {tx, ty, 0};
        k_mosaic_frames<E, C>(fr.empty() ? nullptr : fr.data(), (int)fr.size(), fld, pix, W, H, mode, feather, cx, cy, cw, ch, tiles_x, canvas, weight);
    }
    return n_blocks;
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: mosaic_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int elem = get<int32_t>(f), C = get<int32_t>(f), W = get<int32_t>(f), H = get<int32_t>(f), mode = get<int32_t>(f), n_frames = get<int32_t>(f);
    const int cx = get<int32_t>(f), cy = get<int32_t>(f), cw = get<int32_t>(f), ch = get<int32_t>(f);
    const int pix_front = get<int32_t>(f), canvas_front = get<int32_t>(f), has_weight = get<int32_t>(f);
    const float feather = get<float>(f);
    const uint64_t fld_bytes = get<uint64_t>(f), pix_bytes = get<uint64_t>(f);
    if (cw < 1 || ch < 1 || n_frames < 0) { printf("bad case\n"); return 2; }
    const size_t px = (size_t)C * (elem == 0 ? 4 : 1);
    std::vector<MosaicFrame> frames((size_t)n_frames);
    for (MosaicFrame &r : frames) {
        r.x_off = get<int32_t>(f); r.y_off = get<int32_t>(f); r.obj_w = get<int32_t>(f); r.obj_h = get<int32_t>(f);
        r.fld_off = get<uint64_t>(f); r.pix_off = get<uint64_t>(f);
    }
    std::vector<void *> owned;
    const size_t canvas_bytes = (size_t)cw * ch * px, weight_bytes = has_weight ? (size_t)cw * ch * 4 : 0;
    uint8_t *fld = block(0, fld_bytes, 0, owned), *pix = block((size_t)pix_front, pix_bytes, 0xEE, owned);
    uint8_t *canvas = block((size_t)canvas_front, canvas_bytes, 0xA5, owned), *weight = block(0, weight_bytes, 0xA5, owned);
    if ((fld_bytes && fread(fld, 1, fld_bytes, f) != fld_bytes) || (pix_bytes && fread(pix, 1, pix_bytes, f) != pix_bytes)) { printf("short input\n"); return 2; }
    fclose(f);
    unsigned blocks = 0;
    float *wp = has_weight ? reinterpret_cast<float *>(weight) : nullptr;
#define RUN(E, CC) blocks = run<E, CC>(frames, fld, pix, W, H, mode, feather, cx, cy, cw, ch, canvas, wp)
#define RUNE(E) switch (C) { case 1: RUN(E, 1); break; case 2: RUN(E, 2); break; case 3: RUN(E, 3); break; case 4: RUN(E, 4); break; default: return 2; }
    if (elem == 0) RUNE(float) else RUNE(uint8_t)
    FILE *o = fopen(argv[2], "wb");
    if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
    fwrite(canvas, 1, canvas_bytes, o); fwrite(weight, 1, weight_bytes, o);
    fclose(o);
    for (void *p : owned) free(p);
    printf("host check ran: %d frames, %u blocks, mode %d\n", n_frames, blocks, mode);
    return 0;
}
