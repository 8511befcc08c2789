// hg_api_detect.hip -- the C ABI, part 10: detecting and describing keypoints of plane sets (hg_detect_layout, hg_describe_pattern,
// hg_detect_describe_frames_device).  Like a match, the call is work of its own: it needs no image, mesh or frame set, is independent of the
// sampling mode, and leaves the warp paths' taps (hg_last_*_kernel), the plan of the last warp, what the policy learned and every staged frame
// set as it found them.
#include "hg_ctx.h"
#include "hg_detect_dev.h"

static_assert(HG_DETECT_MARGIN == kDetectMargin && HG_DETECT_BINS == kDetectBins && HG_DETECT_DESC_BYTES * 8 == kDetectTests, "the header's constants are the kernels'");
constexpr int kDetectMaxSide = 32768, kDetectMaxSlots = 65536, kDetectMaxPlanes = 4096;

// The shape checks of a plane and its cells, in the order of the header's list; the layout comes back through the pointers.
static int check_detect_layout(hg_ctx *c, int W, int H, int cell, int per_cell, int *cells_x, int *cells_y, int *n_slots)
{
    if (W < 1 || W > kDetectMaxSide || H < 1 || H > kDetectMaxSide || (int64_t)W * H > ((int64_t)1 << 30))
        return fail(c, HG_ERR_INVALID, "detect: W and H must be 1..32768 and W * H <= 2^30");
    if (cell < 8 || cell > 256) return fail(c, HG_ERR_INVALID, "detect: cell must be 8..256");
    if (per_cell < 1 || per_cell > kDetectMaxPerCell) return fail(c, HG_ERR_INVALID, "detect: per_cell must be 1..16");
    const int64_t cx = (W + cell - 1) / cell, cy = (H + cell - 1) / cell, slots = cx * cy * per_cell;
    if (slots > kDetectMaxSlots) return fail(c, HG_ERR_INVALID, "detect: n_slots = cells_x * cells_y * per_cell must be <= 65536 (the matcher's row limit)");
    *cells_x = (int)cx; *cells_y = (int)cy; *n_slots = (int)slots;
    return HG_OK;
}

extern "C" int hg_detect_layout(int W, int H, int cell, int per_cell, int *cells_x, int *cells_y, int *n_slots)
{
    int cx = 0, cy = 0, slots = 0;
    HG_TRY(check_detect_layout(nullptr, W, H, cell, per_cell, &cx, &cy, &slots));
    if (!cells_x || !cells_y || !n_slots) return fail(nullptr, HG_ERR_INVALID, "hg_detect_layout: cells_x / cells_y / n_slots is NULL");
    *cells_x = cx; *cells_y = cy; *n_slots = slots;
    return HG_OK;
}

extern "C" int hg_describe_pattern(int8_t *out)
{
    if (!out) return fail(nullptr, HG_ERR_INVALID, "hg_describe_pattern: out is NULL");
    for (int b = 0; b < kDetectTests; b++) {
        int8_t t[4];
        detect_base_test(b, t);
        for (int k = 0; k < kDetectBins; k++) {
            int8_t *o = out + ((size_t)k * kDetectTests + b) * 4;
            detect_rotate(t[0], t[1], k, o[0], o[1]);
            detect_rotate(t[2], t[3], k, o[2], o[3]);
        }
    }
    return HG_OK;
}

extern "C" int hg_detect_describe_frames_device(hg_ctx *c, const void *d_planes, int W, int H, int n_planes, size_t plane_stride_bytes, int channels, int cell,
                                                int per_cell, int64_t min_response, size_t desc_stride, int32_t *d_counts, void *d_points, void *d_desc,
                                                void *d_info)
{
    // (the shape: needs no device)
    if (W < 1 || W > kDetectMaxSide || H < 1 || H > kDetectMaxSide || (int64_t)W * H > ((int64_t)1 << 30))
        return fail(c, HG_ERR_INVALID, "detect: W and H must be 1..32768 and W * H <= 2^30");
    if (channels != 1 && channels != 4) return fail(c, HG_ERR_INVALID, "detect: channels must be 1 or 4");
    int cells_x = 0, cells_y = 0, n_slots = 0;
    HG_TRY(check_detect_layout(c, W, H, cell, per_cell, &cells_x, &cells_y, &n_slots));
    if (n_planes < 0 || n_planes > kDetectMaxPlanes) return fail(c, HG_ERR_INVALID, "detect: n_planes must be 0..4096");
    if (min_response < 1) return fail(c, HG_ERR_INVALID, "detect: min_response must be >= 1");
    if ((desc_stride & 15) != 0 || desc_stride < (size_t)HG_DETECT_DESC_BYTES) return fail(c, HG_ERR_INVALID, "detect: desc_stride must be a multiple of 16 and >= 32");
    if (plane_stride_bytes < (size_t)W * (size_t)H * (size_t)channels) return fail(c, HG_ERR_INVALID, "detect: plane_stride_bytes must be >= W * H * channels");
    HG_TRY(bind(c));
    if (n_planes == 0) return HG_OK;
    if (!d_planes || !d_counts) return fail(c, HG_ERR_INVALID, "hg_detect_describe_frames_device: d_planes / d_counts is NULL");
    if (misaligned(d_counts, 4)) return fail(c, HG_ERR_INVALID, "hg_detect_describe_frames_device: d_counts must be aligned to 4 bytes");
    if (misaligned(d_points, 8) || misaligned(d_info, 8)) return fail(c, HG_ERR_INVALID, "hg_detect_describe_frames_device: d_points / d_info must be aligned to 8 bytes");
    if (misaligned(d_desc, 16)) return fail(c, HG_ERR_INVALID, "hg_detect_describe_frames_device: d_desc must be aligned to 16 bytes");
    HG_TRY(hg_sync(c));                                      // queued runs: settled first, as the matcher does
    const size_t P = (size_t)n_planes, cells = (size_t)cells_x * (size_t)cells_y;
    if (!c->d_detect_table.p) {                              // the turned pattern: once per context
        std::vector<int8_t> table((size_t)kDetectBins * kDetectTests * 4);
        HG_TRY(hg_describe_pattern(table.data()));
        HG_TRY(ensure(c, c->d_detect_table, table.size()));
        HIP_TRY(c, hipMemcpyAsync(c->d_detect_table.p, table.data(), table.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));         // (the vector goes away)
    }
    HG_TRY(ensure(c, c->d_detect_rec, P * cells * (size_t)per_cell));
    HG_TRY(ensure(c, c->d_detect_cnt, P * cells));
    HG_TRY(ensure(c, c->d_detect_list, P * (size_t)n_slots));
    hg::DetectArgs a{static_cast<const uint8_t *>(d_planes), W, H, n_planes, plane_stride_bytes, channels, cell, per_cell, cells_x, cells_y, min_response, desc_stride,
                     c->d_detect_rec.p, c->d_detect_cnt.p, c->d_detect_list.p, c->d_detect_table.p, d_counts, d_points, d_desc, d_info};
    hg::launch_detect(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return HG_OK;
}
