// hg_span_start.h -- the flat start of the span cache's use kernel (k_pw_rows_cached<.., SELF = 3>): the compact argument block that is
// the kernel's first parameter, the per-frame block the cache keeps beside its directory, and the division-free decode of a block id into (frame,
// row group).  Plain C++ apart from the function attributes: tests/cpp/span_start_check.cpp drives the decode on the host against frame_group (hg_dev.h).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_SS_FN __host__ __device__ inline
#else
#define HG_SS_FN inline
#endif

namespace hg {

// ------------------------------------------------------------------------------------------------ exact division by a launch constant
// n / d for 0 <= n < 2^31 and 1 <= d < 2^31 as one 32 x 32 -> 64 bit product and a shift.  With l = ceil(log2 d), shift = 31 + l and
// mul = ceil(2^shift / d):  mul * d = 2^shift + e with 0 <= e < d <= 2^l, so n * mul / 2^shift = n / d + n * e / (d * 2^shift), and the error term is
// below 1 / d because n * e < 2^31 * 2^l = 2^shift: the floor cannot reach the next integer.  mul < 2^32 because 2^l < 2 d.  Powers of two (d = 1
// among them) come out as mul = 2^31, shift = 31 + l: no special case.
struct SpanDiv { uint32_t mul, shift; };
HG_SS_FN SpanDiv span_div_make(uint32_t d)
{
    uint32_t l = 0;
    while (l < 31 && (1u << l) < d) l++;
    SpanDiv v;
    v.shift = 31 + l;
    v.mul = (uint32_t)((((uint64_t)1 << v.shift) + d - 1) / d);
    return v;
}
HG_SS_FN uint32_t span_div(uint32_t n, SpanDiv v) { return (uint32_t)(((uint64_t)n * v.mul) >> v.shift); }

// ------------------------------------------------------------------------------------------------ block id -> (frame, row group)
// frame_group (hg_dev.h) with its divisions replaced: the launcher knows the three divisors.  Same three layouts: bands, rotating bands, dealt sub-bands.
struct SpanStartDecode {
    int32_t xcc_log2, xcc_rotate;
    int32_t sub_groups, n_frames, per_sub, groups_per_xcd;      // per_sub = sub_groups * n_frames
    SpanDiv by_per_sub, by_sub, by_gpx;                         // (by_per_sub, by_sub: only read when sub_groups > 0)
};
HG_SS_FN SpanStartDecode span_start_decode_make(int xcc_log2, int xcc_rotate, int sub_groups, int n_frames, int groups_per_xcd)
{
    SpanStartDecode d;
    d.xcc_log2 = xcc_log2; d.xcc_rotate = xcc_rotate ? 1 : 0;
    d.sub_groups = sub_groups; d.n_frames = n_frames; d.per_sub = sub_groups * n_frames; d.groups_per_xcd = groups_per_xcd;
    d.by_per_sub = span_div_make((uint32_t)(d.per_sub > 0 ? d.per_sub : 1));
    d.by_sub = span_div_make((uint32_t)(sub_groups > 0 ? sub_groups : 1));
    d.by_gpx = span_div_make((uint32_t)(groups_per_xcd > 0 ? groups_per_xcd : 1));
    return d;
}
HG_SS_FN bool span_start_decode(const SpanStartDecode &d, int bid, int &f, int &g)
{
    const int xcd = bid & ((1 << d.xcc_log2) - 1), bi = bid >> d.xcc_log2;
    if (d.sub_groups > 0) {
        const int sb = (int)span_div((uint32_t)bi, d.by_per_sub), rem = bi - sb * d.per_sub;
        f = (int)span_div((uint32_t)rem, d.by_sub);
        g = ((sb << d.xcc_log2) + xcd) * d.sub_groups + (rem - f * d.sub_groups);
        return g < (d.groups_per_xcd << d.xcc_log2);
    }
    f = (int)span_div((uint32_t)bi, d.by_gpx);
    g = ((xcd + (d.xcc_rotate ? f : 0)) & ((1 << d.xcc_log2) - 1)) * d.groups_per_xcd + (bi - f * d.groups_per_xcd);
    return true;
}

// ------------------------------------------------------------------------------------------------ the per-frame block
// One per frame, written once per build (k_span_frame_blocks) from what the build launch itself reads: everything the use kernel's start fetched or
// rebuilt per workgroup that depends on the frame set and the plan key alone.  The first 64 bytes serve the high-dword bounds form; the fp64 form
// reads the four limits behind them.  What it holds is covered by the cache's two guards: the frame record and the frame's source minima by the
// frame-set epoch, the source's size and the bounds form by SpanPlanKey (W, H, the minima's extremes, hi_bounds).
// The frame's record form is not here: it is the rec_words of every directory entry of the frame, which the start has in hand anyway.
struct alignas(64) SpanFrameBlock {
    int32_t x_off, y_off, obj_w, obj_h;
    uint64_t out_off;
    int32_t ms_x, ms_y;                         // the frame's source minima (groups the directory does not hold: the prologue's bounds)
    uint32_t hb_lox, hb_rx, hb_loy, hb_ry;      // HiBounds (hg_dev.h), finished
    uint32_t pad_[4];
    double bx_lo, bx_hi, by_lo, by_hi;          // the fp64 limits of :1047 on h = RTN(s + 0.5)
    uint32_t pad2_[8];
};
static_assert(sizeof(SpanFrameBlock) == 128, "one 64-byte line for the high-dword form, a second for the fp64 limits");

// ------------------------------------------------------------------------------------------------ the argument block
// First parameter of the use kernel: every scalar a valid group needs from its first instruction to its last -- the decode, the start and the
// housekeeping stores -- in the first 128 bytes of the kernarg segment, fetched whole in the entry block.  The compiler cuts that fetch into five
// scalar loads (8, 4, 2, 16 and 2 words) issued back to back and waited for ONCE; it is 128 bytes and not 64 because the
// housekeeping pointers and the three multiply-shift pairs travel in it too, so that a valid group never touches the structs behind it.
// Copied by the launcher from the structs it already has (PwMesh, PwFrames, RowLists, SpanCacheDev); those stay as further parameters for the
// groups the directory does not hold and for flagging a frame.
struct SpanStartArgs {
    const void *dir;                            // int4 SpanDirEnt, n_frames x groups_per_frame
    const void *rec;                            // 16-byte record words
    const SpanFrameBlock *fblk;                 // n_frames
    uint8_t *out;
    const uint8_t *img;                         // the shared source (the cache is not eligible with one source per frame)
    int32_t *status_next;                       // housekeeping: the next step's status set (block 0 clears it) ...
    int32_t *cnt_clear;                         // ... and the other counter set (RowLists)
    int32_t src_w, src_h;
    int32_t groups_per_frame, rows_per_group, safe_spans, row_stride;
    SpanStartDecode dec;
};
static_assert(sizeof(SpanStartArgs) == 128, "56 bytes of pointers, 24 of launch scalars, 48 of decode");

} // namespace hg
