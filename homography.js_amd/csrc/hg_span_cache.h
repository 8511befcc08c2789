// hg_span_cache.h -- the span cache of k_pw_rows<SELF>: what the self-span prologue leaves in LDS for a 4-row group, kept in device memory
// while the frame set stays the same, so that later warps of the set copy the slots instead of rasterising the triangles again.
// Here: the record / directory formats and the host's decision (Off, Build, Use).  Plain C++, no runtime: tests/cpp/span_cache_check.cpp drives it.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HG_SC_FN __host__ __device__ inline
#else
#define HG_SC_FN inline
#endif

namespace hg {

// ------------------------------------------------------------------------------------------------ formats
// Records are runs of 16-byte words; a group's records lie back to back, row after row.  Since hg_span_runs.h a record stands for a RUN of its
// row (disjoint, sorted by start, with its winner), not for a span as the prologue filed it: word 0 then begins with run_pack_start() in place of
// span_pack_lo_hi(), and a row's count in the directory is its number of runs (<= 64).  The span form of word 0 and its helpers stay for the host checks.
//   word 0: lo | hi << 16 (cells [lo, hi) of the row, hi <= 65535), id << 1 | unsafe bit, m0 and m1 as the f32 they were widened from
//   word 1: one-fma frame {A, B} = {(m2 y) + m4, (m3 y) + m5}; long form {m2 y, m3 y}: two f64
//   word 2: long form only: m4, m5 as f32, two unused words
// A record's LDS offset is a function of its place: run i of a row goes to slot i of the row's block.
constexpr int kSpanRecWordsFma = 2, kSpanRecWordsLong = 3;               // 32 / 48 bytes per slot
struct SpanRecHead { uint32_t lo_hi, id_flag; float m0, m1; };

HG_SC_FN uint32_t span_pack_lo_hi(int lo, int hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }
HG_SC_FN int span_lo(uint32_t lo_hi) { return (int)(lo_hi & 0xffffu); }
HG_SC_FN int span_hi(uint32_t lo_hi) { return (int)(lo_hi >> 16); }
HG_SC_FN uint32_t span_pack_id(int id, int unsafe) { return ((uint32_t)id << 1) | (uint32_t)(unsafe & 1); }
HG_SC_FN int span_id(uint32_t id_flag) { return (int)(id_flag >> 1); }
HG_SC_FN int span_unsafe_bit(uint32_t id_flag) { return (int)(id_flag & 1u); }

// Directory: one entry per (frame, 4-row group), index frame * groups_per_frame + group.
enum : int32_t { SPAN_DIR_NOT_CACHED = 0, SPAN_DIR_VALID = 1, SPAN_DIR_OVERFLOWED = 2 };
struct SpanDirEnt { int32_t state; uint32_t off16; uint32_t counts; uint32_t rec_words; };      // off16: first word of the group's records; counts: row j in bits 8j .. 8j + 7 (runs: <= 64); rec_words: 2 or 3
HG_SC_FN uint32_t span_pack_counts(int c0, int c1, int c2, int c3) { return (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16) | ((uint32_t)c3 << 24); }
HG_SC_FN int span_count(uint32_t counts, int row) { return (int)((counts >> (8 * row)) & 0xffu); }

// ------------------------------------------------------------------------------------------------ the decision
enum class SpanCacheMode { Off = 0, Build = 1, Use = 2 };

// What the cached slots depend on besides the frame set itself (which the epoch stands for): the plan's instantiation-selecting fields, the
// source's size and minima and the set-wide bounds form.  eligible: Rows + self-spans + packed 4-row groups on a shared source.
struct SpanPlanKey {
    bool eligible = false;
    int32_t W = 0, H = 0;                       // source
    int32_t ms_lo_x = 0, ms_hi_x = 0, ms_lo_y = 0, ms_hi_y = 0;     // extremes of the source minima over the set
    int32_t hi_bounds = 0;                      // option "hi_bounds": with W, H and the minima it decides between the high-dword and the fp64 bounds form
    int32_t safe_spans = 0;                     // the unsafe bit of a key is only computed with it
    int32_t bands = 0, n_bands = 0;             // candidate bands in front of the prologue
    int32_t n_frames = 0, max_h = 0;            // directory layout
};
inline bool span_key_equal(const SpanPlanKey &a, const SpanPlanKey &b)
{
    return a.eligible == b.eligible && a.W == b.W && a.H == b.H && a.ms_lo_x == b.ms_lo_x && a.ms_hi_x == b.ms_hi_x && a.ms_lo_y == b.ms_lo_y &&
           a.ms_hi_y == b.ms_hi_y && a.hi_bounds == b.hi_bounds && a.safe_spans == b.safe_spans && a.bands == b.bands && a.n_bands == b.n_bands &&
           a.n_frames == b.n_frames && a.max_h == b.max_h;
}

struct SpanCacheState {
    uint64_t epoch = 0;                         // the frame-set epoch `calls` and `built` belong to
    uint32_t calls = 0;                         // eligible warps seen on it (saturating)
    bool built = false;                         // a build ran on it ...
    SpanPlanKey key;                            // ... under this key
};

// option: -1 default (first call as ever, second builds, third onwards uses), 0 off, 1 eager (first call builds).
// budget_bytes / estimate_bytes: the build is not started when the host's estimate exceeds the budget, unless force_budget (the kernel then
// caches what fits).  Pure: span_cache_commit applies the answer once the launch is queued.
inline SpanCacheMode span_cache_decide(const SpanCacheState &st, uint64_t epoch, const SpanPlanKey &key, int option, uint64_t budget_bytes,
                                       uint64_t estimate_bytes, bool force_budget)
{
    if (option == 0 || !key.eligible) return SpanCacheMode::Off;
    const bool same_epoch = st.epoch == epoch;                  // (any difference counts: a wrapped counter is a new epoch like any other)
    if (same_epoch && st.built && span_key_equal(st.key, key)) return SpanCacheMode::Use;
    // calls this one would be on its (epoch, key): a key that changed under a build starts over like a new epoch
    const uint32_t calls = same_epoch && !st.built ? (st.calls == UINT32_MAX ? st.calls : st.calls + 1) : 1;
    const uint32_t build_at = option == 1 ? 1 : 2;
    if (calls < build_at) return SpanCacheMode::Off;
    if (budget_bytes == 0 || (!force_budget && estimate_bytes > budget_bytes)) return SpanCacheMode::Off;
    return SpanCacheMode::Build;
}

inline void span_cache_commit(SpanCacheState &st, uint64_t epoch, const SpanPlanKey &key, int option, SpanCacheMode mode)
{
    if (option == 0 || !key.eligible) return;                   // (ineligible warps neither count nor drop a build: the next eligible plan is compared with its key)
    const bool same_epoch = st.epoch == epoch;
    if (mode == SpanCacheMode::Use) return;
    if (!same_epoch || st.built) { st.epoch = epoch; st.calls = 0; st.built = false; }
    if (st.calls != UINT32_MAX) st.calls++;
    if (mode == SpanCacheMode::Build) { st.built = true; st.key = key; }
}

} // namespace hg
