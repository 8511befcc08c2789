// span_cache_check.cpp -- the span cache's host decision and its record / directory packing (hg_span_cache.h), table-driven.  Stand-alone:
// tests/test_span_cache_cpu.py builds it under AddressSanitizer + UndefinedBehaviorSanitizer and runs it.
#include "hg_span_cache.h"

#include <cstdio>
#include <vector>

using namespace hg;

static long g_checks = 0, g_bad = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_bad++; std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static SpanPlanKey base_key()
{
    SpanPlanKey k;
    k.eligible = true; k.W = 3840; k.H = 2160; k.hi_bounds = 1; k.safe_spans = 1; k.n_frames = 64; k.max_h = 2160;
    return k;
}

// one warp as the host makes it: decide, then commit
static SpanCacheMode step(SpanCacheState &st, uint64_t epoch, const SpanPlanKey &k, int option, uint64_t budget = 1 << 20, uint64_t estimate = 1 << 10,
                          bool force = false)
{
    const SpanCacheMode m = span_cache_decide(st, epoch, k, option, budget, estimate, force);
    span_cache_commit(st, epoch, k, option, m);
    return m;
}

int main()
{
    const SpanCacheMode Off = SpanCacheMode::Off, Build = SpanCacheMode::Build, Use = SpanCacheMode::Use;
    const SpanPlanKey k0 = base_key();

    {   // default policy: Off, Build, Use, Use, ...
        SpanCacheState st;
        CHECK(step(st, 7, k0, -1) == Off);
        CHECK(step(st, 7, k0, -1) == Build);
        for (int i = 0; i < 100; i++) CHECK(step(st, 7, k0, -1) == Use);
    }
    {   // eager: Build, Use
        SpanCacheState st;
        CHECK(step(st, 7, k0, 1) == Build);
        CHECK(step(st, 7, k0, 1) == Use);
    }
    {   // off: never, and the state is not touched
        SpanCacheState st;
        for (int i = 0; i < 5; i++) CHECK(step(st, 7, k0, 0) == Off);
        CHECK(st.calls == 0 && !st.built);
        CHECK(step(st, 7, k0, -1) == Off);                   // switched on: counts from here
        CHECK(step(st, 7, k0, -1) == Build);
        CHECK(step(st, 7, k0, 0) == Off);                    // switched off under a build: today's launch
    }
    {   // a new epoch on every call (fresh points per step): never builds under the default, builds every time when eager
        SpanCacheState st;
        for (uint64_t e = 1; e < 50; e++) CHECK(step(st, e, k0, -1) == Off);
        CHECK(!st.built);
        SpanCacheState se;
        for (uint64_t e = 1; e < 5; e++) CHECK(step(se, e, k0, 1) == Build);
    }
    {   // every invalidation edge: an epoch bump after Use starts the sequence over
        SpanCacheState st;
        step(st, 1, k0, -1); step(st, 1, k0, -1);
        CHECK(step(st, 1, k0, -1) == Use);
        CHECK(step(st, 2, k0, -1) == Off);
        CHECK(step(st, 2, k0, -1) == Build);
        CHECK(step(st, 2, k0, -1) == Use);
        CHECK(step(st, 1, k0, -1) == Off);                   // (going "back" is a change like any other)
    }
    {   // epoch wrap: the counter's largest value, then 0
        SpanCacheState st;
        const uint64_t top = ~(uint64_t)0;
        CHECK(step(st, top, k0, 1) == Build);
        CHECK(step(st, top, k0, 1) == Use);
        CHECK(step(st, top + 1, k0, 1) == Build);            // (0: a fresh state's own epoch value must not read as "same set, built")
        CHECK(step(st, 0, k0, 1) == Use);
        SpanCacheState fresh;                                // epoch 0 on a fresh state: not built, so no Use
        CHECK(step(fresh, 0, k0, -1) == Off);
        CHECK(step(fresh, 0, k0, -1) == Build);
    }
    {   // a change in each selecting field of the key under a build: no Use with the old records; the sequence starts over on the new key
        struct Edit { const char *name; void (*apply)(SpanPlanKey &); };
        const Edit edits[] = {
            {"W", [](SpanPlanKey &k) { k.W++; }}, {"H", [](SpanPlanKey &k) { k.H--; }},
            {"ms_lo_x", [](SpanPlanKey &k) { k.ms_lo_x = -3; }}, {"ms_hi_x", [](SpanPlanKey &k) { k.ms_hi_x = 5; }},
            {"ms_lo_y", [](SpanPlanKey &k) { k.ms_lo_y = -1; }}, {"ms_hi_y", [](SpanPlanKey &k) { k.ms_hi_y = 2; }},
            {"hi_bounds", [](SpanPlanKey &k) { k.hi_bounds ^= 1; }}, {"safe_spans", [](SpanPlanKey &k) { k.safe_spans ^= 1; }},
            {"bands", [](SpanPlanKey &k) { k.bands ^= 1; }}, {"n_bands", [](SpanPlanKey &k) { k.n_bands += 3; }},
            {"n_frames", [](SpanPlanKey &k) { k.n_frames++; }}, {"max_h", [](SpanPlanKey &k) { k.max_h += 4; }},
        };
        for (const Edit &e : edits) {
            for (int option = -1; option <= 1; option += 2) {
                SpanCacheState st;
                step(st, 3, k0, 1);
                CHECK(step(st, 3, k0, option) == Use);
                SpanPlanKey k1 = k0;
                e.apply(k1);
                CHECK(!span_key_equal(k0, k1));
                if (option == 1) CHECK(step(st, 3, k1, 1) == Build);
                else { CHECK(step(st, 3, k1, -1) == Off); CHECK(step(st, 3, k1, -1) == Build); }
                CHECK(step(st, 3, k1, option) == Use);
                CHECK(step(st, 3, k0, option) != Use);       // and back: the records are k1's now
            }
        }
    }
    {   // ineligible plans: Off whatever the option; they neither count nor drop a build
        SpanPlanKey bad = k0;
        bad.eligible = false;
        SpanCacheState st;
        for (int option = -1; option <= 1; option++) CHECK(step(st, 9, bad, option) == Off);
        CHECK(st.calls == 0);
        CHECK(step(st, 9, k0, -1) == Off);
        CHECK(step(st, 9, bad, -1) == Off);
        CHECK(step(st, 9, k0, -1) == Build);
        CHECK(step(st, 9, bad, -1) == Off);
        CHECK(step(st, 9, k0, -1) == Use);
    }
    {   // budget below the estimate: no build at all; forced: build (the kernel caches what fits); a zero budget: never
        SpanCacheState st;
        for (int i = 0; i < 4; i++) CHECK(step(st, 4, k0, -1, 1000, 1001) == Off);
        CHECK(!st.built);
        CHECK(step(st, 4, k0, -1, 1001, 1001) == Build);     // (equal fits)
        SpanCacheState sf;
        CHECK(step(sf, 4, k0, 1, 1000, 1 << 30, true) == Build);
        CHECK(step(sf, 4, k0, 1, 1000, 1 << 30, true) == Use);
        SpanCacheState sz;
        CHECK(step(sz, 4, k0, 1, 0, 0, true) == Off);
        CHECK(step(sz, 4, k0, 1, 0, 0, false) == Off);
    }
    {   // the call counter saturates
        SpanCacheState st;
        st.epoch = 5; st.calls = UINT32_MAX;
        CHECK(step(st, 5, k0, -1, 10, 11) == Off);
        CHECK(st.calls == UINT32_MAX);
        CHECK(step(st, 5, k0, -1) == Build);
    }

    // ---- packing: corners and a sweep
    {
        const int los[] = {0, 1, 255, 256, 65534}, his[] = {1, 2, 256, 4095, 65535};
        for (int lo : los) for (int hi : his) {
            if (lo >= hi) continue;
            const uint32_t w = span_pack_lo_hi(lo, hi);
            CHECK(span_lo(w) == lo && span_hi(w) == hi);
        }
        CHECK(span_lo(span_pack_lo_hi(0, 65535)) == 0 && span_hi(span_pack_lo_hi(0, 65535)) == 65535);
        const int ids[] = {0, 1, 2, 255, 16383, 16384, 32766, 32767};
        for (int id : ids) for (int u = 0; u < 2; u++) {
            const uint32_t w = span_pack_id(id, u);
            CHECK(span_id(w) == id && span_unsafe_bit(w) == u);
        }
        for (int c0 = 0; c0 < 64; c0 += 9) for (int c1 = 0; c1 < 64; c1 += 7) for (int c2 = 63; c2 >= 0; c2 -= 21) for (int c3 = 0; c3 < 64; c3 += 63) {
            const uint32_t w = span_pack_counts(c0, c1, c2, c3);
            CHECK(span_count(w, 0) == c0 && span_count(w, 1) == c1 && span_count(w, 2) == c2 && span_count(w, 3) == c3);
        }
        CHECK(span_count(span_pack_counts(63, 63, 63, 63), 3) == 63);
        // records as the kernel lays them out: one-fma 2 words, long form 3 words of 16 bytes; f32 entries survive their round trip through
        // the f64 the LDS record holds
        static_assert(sizeof(SpanRecHead) == 16 && sizeof(SpanDirEnt) == 16, "16-byte words");
        CHECK(kSpanRecWordsFma * 16 == 32 && kSpanRecWordsLong * 16 == 48);
        const float ms[] = {0.f, -0.f, 1.f, -1.5f, 1.17549435e-38f, 3.4028235e38f, 1.0f / 3.0f, 1048576.f + 0.125f};
        for (float m : ms) {
            const double wide = (double)m;
            SpanRecHead h{span_pack_lo_hi(0, 65535), span_pack_id(32767, 1), (float)wide, (float)wide};
            std::vector<unsigned char> bytes(sizeof h);
            memcpy(bytes.data(), &h, sizeof h);
            SpanRecHead g;
            memcpy(&g, bytes.data(), sizeof g);
            CHECK(memcmp(&g.m0, &m, 4) == 0 && (double)g.m1 == wide && span_id(g.id_flag) == 32767 && span_unsafe_bit(g.id_flag) == 1);
        }
    }
    std::printf("span_cache_check: checks %ld failures %ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
