// ctx_mem_check -- the ownership types of the context (hg_mem.h: DevBuf / ensure, PinnedBuf, StageRing; hg_ctx.h: PwSolve, hg_ctx itself)
// against a fake HIP runtime.  Host only, no device: this program defines the runtime entry points the memory code calls (they take precedence over
// the HIP library's) as malloc-backed fakes that log every call in order and can be told to fail the next allocation.
//   ensure: the growth rule, nothing at all when the buffer is large enough, stream sync -> free -> malloc when it regrows, a failed hipMalloc;
//   StageRing<4>, StageRing<64>: when a slot waits, when it regrows, acquire without commit, where commit records;
//   upload_filled / upload_copied (hg_ctx.h) on a StageRing<4>: acquire, fill, upload, commit in that order; what a failed allocation and a failed
//   upload leave behind; the bytes that arrive, from one block and from two;
//   PwSolve: the six sizes, the six pointers;  hg_ctx: deleting it behind a stream synchronisation frees everything but a borrowed image.
// Built and run by tests/test_ctx_mem_cpu.py with -fsanitize=address,undefined (the leak check at exit covers the fakes' own blocks).
#include "hg_ctx.h"

#include <set>

thread_local std::string g_err;

// ------------------------------------------------------------------------------------------------ the fake runtime
enum Op { SYNC, MALLOC, FREE, HOST_MALLOC, HOST_FREE, EV_CREATE, EV_RECORD, EV_SYNC, EV_DESTROY, UPLOAD, MEMCPY };
struct Call { Op op; const void *p; size_t bytes; const void *stream; };
static std::vector<Call> g_log;
static std::set<const void *> g_dev, g_host, g_events;
static bool g_fail_next = false;                    // the next hipMalloc / hipHostMalloc fails
static bool g_fail_upload = false;                  // the next hipGetLastError / hipMemcpyAsync reports a failure
static long g_bad = 0, g_checks = 0;

#define CHECK(cond) do { g_checks++; if (!(cond)) { g_bad++; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static hipError_t fake_alloc(Op op, std::set<const void *> &live, void **p, size_t n)
{
    if (g_fail_next) { g_fail_next = false; *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(n ? n : 1);
    live.insert(*p);
    g_log.push_back({op, *p, n, nullptr});
    return hipSuccess;
}
static hipError_t fake_free(Op op, std::set<const void *> &live, void *p)
{
    g_log.push_back({op, p, 0, nullptr});
    if (!live.erase(p)) return hipErrorInvalidValue;           // (not ours: the callers below look for such frees in the log)
    std::free(p);
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return fake_alloc(MALLOC, g_dev, p, n); }
hipError_t hipFree(void *p) { return fake_free(FREE, g_dev, p); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int flags) { CHECK(flags == hipHostMallocDefault); return fake_alloc(HOST_MALLOC, g_host, p, n); }
hipError_t hipHostFree(void *p) { return fake_free(HOST_FREE, g_host, p); }
hipError_t hipStreamSynchronize(hipStream_t s) { g_log.push_back({SYNC, nullptr, 0, s}); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    CHECK(flags == hipEventDisableTiming);
    *e = reinterpret_cast<hipEvent_t>(std::malloc(1));
    g_events.insert(*e);
    g_log.push_back({EV_CREATE, *e, 0, nullptr});
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { g_log.push_back({EV_RECORD, e, 0, s}); return g_events.count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventSynchronize(hipEvent_t e) { g_log.push_back({EV_SYNC, e, 0, nullptr}); return g_events.count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventDestroy(hipEvent_t e)
{
    g_log.push_back({EV_DESTROY, e, 0, nullptr});
    if (!g_events.erase(e)) return hipErrorInvalidHandle;
    std::free(e);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
    CHECK(kind == hipMemcpyHostToDevice);
    g_log.push_back({MEMCPY, dst, n, s});
    if (g_fail_upload) { g_fail_upload = false; return hipErrorInvalidValue; }
    std::memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { const bool f = g_fail_upload; g_fail_upload = false; return f ? hipErrorLaunchFailure : hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory (fake)" : "error (fake)"; }
}

// k_upload's launch: the segments are copied at once; one log entry with the first destination and the bytes of all three
void hg::launch_upload(const UploadSegs &sg, hipStream_t s)
{
    for (int k = 0; k < 3; k++) if (sg.n8[k]) std::memcpy(sg.dst[k], sg.src[k], sg.n8[k] * 8);
    g_log.push_back({UPLOAD, sg.dst[0], (sg.n8[0] + sg.n8[1] + sg.n8[2]) * 8, s});
}

static size_t count(Op op) { size_t n = 0; for (const Call &c : g_log) n += c.op == op; return n; }
static hipStream_t const kStream = reinterpret_cast<hipStream_t>(0x5eed);

// ------------------------------------------------------------------------------------------------ ensure
template <typename T>
static void check_ensure(hg_ctx *c)
{
    static const size_t table[][2] = { {0, 1}, {0, 100}, {100, 100}, {100, 50}, {100, 0}, {100, 101}, {100, 150}, {100, 151}, {100, 400}, {7, 8}, {1, 2}, {3, 4} };
    for (const auto &row : table) {
        const size_t old = row[0], need = row[1];
        DevBuf<T> b;
        if (old) CHECK(ensure(c, b, old) == HG_OK && b.cap == old);
        T *const before = b;
        g_log.clear();
        CHECK(ensure(c, b, need) == HG_OK);
        if (need <= old) { CHECK(g_log.empty() && b.p == before && b.cap == old); continue; }
        const size_t want = std::max(need, old + old / 2);
        CHECK(b.cap == want && b.p != nullptr);
        if (old) {                                              // regrow: stream sync, then free, then malloc
            CHECK(g_log.size() == 3);
            if (g_log.size() != 3) continue;
            CHECK(g_log[0].op == SYNC && g_log[0].stream == kStream);
            CHECK(g_log[1].op == FREE && g_log[1].p == before);
            CHECK(g_log[2].op == MALLOC && g_log[2].bytes == want * sizeof(T) && g_log[2].p == b.p);
        } else CHECK(g_log.size() == 1 && g_log[0].op == MALLOC && g_log[0].bytes == want * sizeof(T));
    }
    // a failed hipMalloc, on an empty buffer and on one that holds memory
    for (size_t old : {(size_t)0, (size_t)10}) {
        DevBuf<T> b;
        if (old) CHECK(ensure(c, b, old) == HG_OK);
        g_fail_next = true; c->err.clear();
        CHECK(ensure(c, b, 64) == HG_ERR_NOMEM);
        CHECK(b.p == nullptr && b.cap == 0 && static_cast<T *>(b) == nullptr);
        CHECK(c->err.rfind("hipMalloc:", 0) == 0 && g_err == c->err);
        CHECK(g_dev.empty());                                   // (the old block went before the attempt)
        g_log.clear();
        CHECK(ensure(c, b, 5) == HG_OK && b.cap == 5 && g_log.size() == 1 && g_log[0].op == MALLOC && g_log[0].bytes == 5 * sizeof(T));
    }
    CHECK(g_dev.empty());                                       // every DevBuf above freed its block when it went out of scope
}

// ------------------------------------------------------------------------------------------------ staging rings
template <int N>
static void check_ring(hg_ctx *c)
{
    {
        StageRing<N> ring;
        StageSlot *s = nullptr, *first = nullptr;
        g_log.clear();
        for (int i = 0; i < N; i++) {                           // the first lap: nothing to wait for
            CHECK(ring.next() == i);
            CHECK(ring.acquire(c, 100, "frame-set staging", &s) == HG_OK && s == &ring.slot[i] && s->cap == 125 && s->h && !s->used);
            if (i == 0) first = s;
            CHECK(ring.next() == i);                            // acquire alone moves nothing
            const size_t at = g_log.size();
            CHECK(ring.commit(c, s) == HG_OK && s->used && ring.cur == i);
            CHECK(g_log.size() == at + 1 && g_log[at].op == EV_RECORD && g_log[at].p == s->done && g_log[at].stream == kStream);
        }
        CHECK(count(EV_SYNC) == 0 && count(EV_CREATE) == (size_t)N && count(HOST_MALLOC) == (size_t)N && count(HOST_FREE) == 0);
        for (size_t i = 0; i < g_log.size(); i++) if (g_log[i].op == HOST_MALLOC) CHECK(g_log[i].bytes == 125);
        g_log.clear();                                          // acquisition N + 1: one wait, on slot 0's event; 125 bytes fit
        CHECK(ring.next() == 0 && ring.acquire(c, 125, "frame-set staging", &s) == HG_OK && s == first);
        CHECK(g_log.size() == 1 && g_log[0].op == EV_SYNC && g_log[0].p == first->done);
        g_log.clear();                                          // not committed: the same slot again, now too small -> bytes + bytes / 4
        uint8_t *const old = s->h;
        CHECK(ring.next() == 0 && ring.acquire(c, 126, "frame-set staging", &s) == HG_OK && s == first && s->cap == 157);
        CHECK(g_log.size() == 3 && g_log[0].op == EV_SYNC && g_log[1].op == HOST_FREE && g_log[1].p == old && g_log[2].op == HOST_MALLOC && g_log[2].bytes == 157);
        CHECK(ring.commit(c, s) == HG_OK && ring.cur == 0 && ring.next() == 1 % N);
        g_fail_next = true; c->err.clear();                     // a failed regrow: message, empty slot, cursor where it was; the slot is taken again
        CHECK(ring.acquire(c, 1000, "field frame staging", &s) == HG_ERR_NOMEM && c->err.rfind("hipHostMalloc (field frame staging): ", 0) == 0);
        CHECK(ring.slot[1 % N].h == nullptr && ring.slot[1 % N].cap == 0 && ring.next() == 1 % N);
        CHECK(ring.acquire(c, 1000, "field frame staging", &s) == HG_OK && s == &ring.slot[1 % N] && s->cap == 1250);
    }
    CHECK(g_host.empty() && g_events.empty());                  // the ring's destructor
}

// ------------------------------------------------------------------------------------------------ staged uploads
static std::vector<uint8_t> pattern(size_t n, unsigned seed)
{
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint8_t)(seed * 37u + i * 11u + 1u);
    return v;
}
static size_t find(Op op, size_t from = 0) { for (size_t i = from; i < g_log.size(); i++) if (g_log[i].op == op) return i; return g_log.size(); }

static void check_staged_upload(hg_ctx *c)
{
    {
        StageRing<4> ring;
        DevBuf<uint8_t> d;
        CHECK(ensure(c, d, 4096) == HG_OK);
        // five uploads in a row: (create, allocate, upload, record) x 4, then ONE wait, on slot 0's event, before the fifth fill
        g_log.clear();
        for (unsigned i = 0; i < 4; i++) {
            const std::vector<uint8_t> src = pattern(64, i);
            CHECK(upload_copied(c, ring, "table staging", d.p, src.data(), src.size()) == HG_OK && ring.cur == (int)i);
            CHECK(std::memcmp(d.p, src.data(), 64) == 0);
        }
        CHECK(g_log.size() == 16);
        for (size_t i = 0; i + 3 < g_log.size() && i < 16; i += 4) {
            const StageSlot &sl = ring.slot[i / 4];
            CHECK(g_log[i].op == EV_CREATE && g_log[i].p == sl.done);
            CHECK(g_log[i + 1].op == HOST_MALLOC && g_log[i + 1].bytes == 80 && g_log[i + 1].p == sl.h);
            CHECK(g_log[i + 2].op == UPLOAD && g_log[i + 2].p == d.p && g_log[i + 2].bytes == 64 && g_log[i + 2].stream == kStream);
            CHECK(g_log[i + 3].op == EV_RECORD && g_log[i + 3].p == sl.done && g_log[i + 3].stream == kStream);
        }
        g_log.clear();
        size_t at_fill = 0; uint8_t *filled = nullptr;
        const std::vector<uint8_t> fifth = pattern(72, 5);
        CHECK(upload_filled(c, ring, "table staging", d.p, fifth.size(), [&](uint8_t *h) { at_fill = g_log.size(); filled = h; std::memcpy(h, fifth.data(), fifth.size()); }) == HG_OK);
        CHECK(filled == ring.slot[0].h && ring.cur == 0 && at_fill == 1 && std::memcmp(d.p, fifth.data(), 72) == 0);
        CHECK(g_log.size() == 3 && g_log[0].op == EV_SYNC && g_log[0].p == ring.slot[0].done && g_log[1].op == UPLOAD && g_log[1].bytes == 72 && g_log[2].op == EV_RECORD && g_log[2].p == ring.slot[0].done);
        // larger than the slot: wait, free the old host block, allocate bytes + bytes / 4, upload, record
        g_log.clear();
        uint8_t *const old = ring.slot[1].h;
        const std::vector<uint8_t> big = pattern(200, 6);
        CHECK(upload_copied(c, ring, "table staging", d.p, big.data(), big.size()) == HG_OK && ring.cur == 1 && ring.slot[1].cap == 250);
        CHECK(g_log.size() == 5 && g_log[0].op == EV_SYNC && g_log[0].p == ring.slot[1].done && g_log[1].op == HOST_FREE && g_log[1].p == old);
        CHECK(g_log.size() == 5 && g_log[2].op == HOST_MALLOC && g_log[2].bytes == 250 && g_log[3].op == UPLOAD && g_log[3].bytes == 200 && g_log[4].op == EV_RECORD);
        CHECK(std::memcmp(d.p, big.data(), 200) == 0);
        // a failed host allocation: its message, nothing filled, uploaded or recorded, the cursor where it was; the next call takes the same slot
        g_log.clear(); g_fail_next = true; c->err.clear();
        bool called = false;
        CHECK(upload_filled(c, ring, "table staging", d.p, 1000, [&](uint8_t *) { called = true; }) == HG_ERR_NOMEM);
        CHECK(c->err.rfind("hipHostMalloc (table staging): ", 0) == 0 && !called && ring.cur == 1 && ring.next() == 2);
        CHECK(count(UPLOAD) == 0 && count(MEMCPY) == 0 && count(EV_RECORD) == 0);
        CHECK(std::memcmp(d.p, big.data(), 200) == 0);           // (the device block is as the last upload left it)
        g_log.clear();
        const std::vector<uint8_t> again = pattern(1000, 7);
        CHECK(upload_filled(c, ring, "table staging", d.p, 1000, [&](uint8_t *h) { filled = h; std::memcpy(h, again.data(), 1000); }) == HG_OK);
        CHECK(filled == ring.slot[2].h && ring.cur == 2 && ring.slot[2].cap == 1250 && std::memcmp(d.p, again.data(), 1000) == 0);
        CHECK(find(UPLOAD) < find(EV_RECORD) && count(UPLOAD) == 1 && count(EV_RECORD) == 1);
        // a failed upload, by the kernel and by the copy engine: no commit -- nothing recorded, the cursor where it was, the same slot next
        for (size_t bytes : {(size_t)64, (size_t)12}) {             // (12 bytes: no multiple of 8, so the copy engine takes it)
            g_log.clear(); g_fail_upload = true; c->err.clear();
            const std::vector<uint8_t> src = pattern(bytes, 8);
            CHECK(upload_copied(c, ring, "table staging", d.p, src.data(), bytes) == HG_ERR_HIP && !c->err.empty());
            CHECK(count(EV_RECORD) == 0 && ring.cur == 2 && ring.next() == 3);
            CHECK(count(bytes == 64 ? UPLOAD : MEMCPY) == 1);
        }
        // the bytes that arrive: one block and two blocks back to back, by the kernel and by the copy engine; the record is behind the upload
        struct { size_t a, b; Op how; } const shapes[] = { {64, 0, UPLOAD}, {24, 40, UPLOAD}, {8, 8, UPLOAD}, {12, 0, MEMCPY}, {6, 6, MEMCPY}, {24, 4, MEMCPY} };
        unsigned seed = 20;
        for (const auto &sh : shapes) {
            const std::vector<uint8_t> a = pattern(sh.a, seed++), b = pattern(sh.b, seed++);
            std::memset(d.p, 0, 128);
            g_log.clear();
            const int before = ring.cur;
            CHECK(upload_copied(c, ring, "table staging", d.p, a.data(), sh.a, sh.b ? b.data() : nullptr, sh.b) == HG_OK && ring.cur == (before + 1) % 4);
            CHECK(std::memcmp(d.p, a.data(), sh.a) == 0 && (sh.b == 0 || std::memcmp(d.p + sh.a, b.data(), sh.b) == 0) && d.p[sh.a + sh.b] == 0);
            CHECK(std::memcmp(ring.slot[ring.cur].h, d.p, sh.a + sh.b) == 0);
            const size_t up = find(sh.how), rec = find(EV_RECORD);
            CHECK(count(UPLOAD) + count(MEMCPY) == 1 && count(EV_RECORD) == 1 && up < rec && rec == g_log.size() - 1);
            CHECK(up < g_log.size() && g_log[up].p == d.p && g_log[up].bytes == sh.a + sh.b && g_log[up].stream == kStream);
        }
        // option "upload_kernel" 0: the copy engine for every size
        c->opt_upload_kernel = 0;
        g_log.clear();
        const std::vector<uint8_t> src = pattern(64, 40);
        CHECK(upload_copied(c, ring, "table staging", d.p, src.data(), 64) == HG_OK && count(UPLOAD) == 0 && count(MEMCPY) == 1 && find(MEMCPY) < find(EV_RECORD));
        c->opt_upload_kernel = -1;
    }
    CHECK(g_host.empty() && g_events.empty() && g_dev.empty());
}

// ------------------------------------------------------------------------------------------------ PwSolve
static void check_solve(hg_ctx *c)
{
    static const int shapes[][2] = { {1, 1}, {3, 7}, {1, 0} };
    for (const auto &sh : shapes) {
        const size_t F = (size_t)sh[0], T = (size_t)std::max(sh[1], 1);      // (the callers' max(T, 1))
        PwSolve s;
        g_log.clear();
        CHECK(s.ensure(c, F, T) == HG_OK);
        const size_t want[6] = { F * T * sizeof(TriRange), F * T * sizeof(int2), F * T * 3 * sizeof(Seg), F * T * 6 * sizeof(float), F * T * kInvStride * sizeof(float), F * sizeof(int32_t) };
        const void *ptr[6] = { s.trir.p, s.trix.p, s.segs.p, s.fwd.p, s.inv.p, s.status.p };
        CHECK(g_log.size() == 6);
        for (size_t k = 0; k < 6 && k < g_log.size(); k++) CHECK(g_log[k].op == MALLOC && g_log[k].bytes == want[k] && g_log[k].p == ptr[k]);
        PwFrames a, b;
        std::memset(&a, 0xAB, sizeof a);
        std::memcpy(&b, &a, sizeof a);
        s.point(b);
        CHECK(b.trir == s.trir.p && b.trix == s.trix.p && b.segs == s.segs.p && b.fwd == s.fwd.p && b.inv == s.inv.p && b.status == s.status.p);
        b.trir = a.trir; b.trix = a.trix; b.segs = a.segs; b.fwd = a.fwd; b.inv = a.inv; b.status = a.status;
        CHECK(std::memcmp(&a, &b, sizeof a) == 0);             // ... and nothing else
        g_log.clear();
        CHECK(s.ensure(c, F, T) == HG_OK && g_log.empty());
    }
    CHECK(g_dev.empty());
}

// ------------------------------------------------------------------------------------------------ the context's lifetime
static void check_lifetime()
{
    static uint8_t callers_image[64];                           // not the fake's: must never reach hipFree
    hg_ctx *c = new hg_ctx();
    c->stream = kStream;
    CHECK(ensure(c, c->d_img, 4096) == HG_OK && c->d_img.cap == 4096);         // hg_set_image
    g_log.clear();
    c->d_img.borrow(callers_image);                             // hg_set_image_device: the context's own image goes, the caller's is borrowed
    CHECK(g_log.size() == 1 && g_log[0].op == FREE && c->d_img == callers_image && c->d_img.cap == 0);
    g_log.clear();
    CHECK(ensure(c, c->d_img, 100) == HG_OK && c->d_img.cap == 100 && count(FREE) == 0 && count(SYNC) == 0);   // hg_set_image again: dropped, not freed
    c->d_img.borrow(callers_image);
    CHECK(ensure(c, c->d_src, 10) == HG_OK && ensure(c, c->d_tris, 30) == HG_OK && ensure(c, c->d_set, 1000) == HG_OK && ensure(c, c->d_set, 3000) == HG_OK);
    CHECK(c->solve.ensure(c, 5, 18) == HG_OK && c->solve.ensure(c, 2, 2) == HG_OK && ensure(c, c->d_two_round, 5) == HG_OK);
    CHECK(ensure(c, c->d_rowcnt, 500) == HG_OK && ensure(c, c->d_rowent, 700) == HG_OK && ensure(c, c->d_bands, 64) == HG_OK);
    CHECK(ensure(c, c->d_redo_frame, 1) == HG_OK && ensure(c, c->d_redo_dst, 20) == HG_OK && ensure(c, c->d_redo_src, 20) == HG_OK && ensure(c, c->d_redo_min, 1) == HG_OK);
    CHECK(c->redo.ensure(c, 1, 18) == HG_OK && ensure(c, c->d_st_pts, 8) == HG_OK && ensure(c, c->d_st_tris, 6) == HG_OK && ensure(c, c->d_st_mats, 16) == HG_OK);
    CHECK(ensure(c, c->d_geo_frames, 3) == HG_OK && ensure(c, c->d_mats, 24) == HG_OK && ensure(c, c->d_geo_pts, 48) == HG_OK && ensure(c, c->d_geo_plain, 3) == HG_OK);
    CHECK(ensure(c, c->d_field_frames, 3) == HG_OK && ensure(c, c->d_field_tmp, 8) == HG_OK && ensure(c, c->d_remap_frames, 3) == HG_OK);
    CHECK(ensure(c, c->d_map32, 99) == HG_OK && ensure(c, c->d_fmap, 99) == HG_OK && ensure(c, c->d_win32, 99) == HG_OK && ensure(c, c->d_fwd_par, 99) == HG_OK);
    CHECK(ensure(c, c->d_fbbox, 8) == HG_OK && ensure(c, c->d_frowoff, 2) == HG_OK && ensure(c, c->d_frowext, 8) == HG_OK && ensure(c, c->d_ftile_cnt, 9) == HG_OK);
    CHECK(ensure(c, c->d_fwd_status, 16) == HG_OK && ensure(c, c->d_ftile_ent, 99) == HG_OK && ensure(c, c->d_ffield_status, 2) == HG_OK);
    CHECK(ensure(c, c->d_map16, 99) == HG_OK && ensure(c, c->d_out_tmp, 99) == HG_OK);
    CHECK(c->h_flag.alloc(c, 16, "flag word") == HG_OK && c->h_status.alloc(c, 64, "status words") == HG_OK && c->h_status.alloc(c, 320, "status words") == HG_OK);
    c->h_flag[0] = 0; c->h_status[319] = 7;                     // (the blocks are writable through the owners)
    for (int i = 0; i < 70; i++) {                              // the piecewise ring laps once, the geometric ring eight times, the field ring seventeen
        hg_ctx::Stage *st = nullptr;
        StageSlot *gs = nullptr, *fs = nullptr;
        CHECK(c->stage.acquire(c, 64 + (size_t)i, "frame-set staging", &st) == HG_OK && c->stage.commit(c, st) == HG_OK);
        st->n = i; st->n_pts = 4; st->moving = (i & 1) != 0;
        CHECK(c->geo_stage.acquire(c, 48 + (size_t)(i % 3) * 100, "frame-set staging", &gs) == HG_OK && c->geo_stage.commit(c, gs) == HG_OK);
        CHECK(c->field_stage.acquire(c, 32, "field frame staging", &fs) == HG_OK && c->field_stage.commit(c, fs) == HG_OK);
    }
    CHECK(c->stage.cur == 69 % 64 && c->geo_stage.cur == 69 % 8 && c->field_stage.cur == 69 % 4);
    const size_t events = g_events.size();
    CHECK(events == 64 + 8 + 4 && !g_dev.empty() && !g_host.empty());
    // as hg_destroy does: the stream is synchronised, then the context is deleted
    g_log.clear();
    (void)hipStreamSynchronize(c->stream);
    delete c;
    CHECK(g_log.size() > 1 && g_log[0].op == SYNC && g_log[0].stream == kStream);     // every free below is behind it
    CHECK(g_dev.empty() && g_host.empty() && g_events.empty());
    CHECK(count(EV_DESTROY) == events);
    for (const Call &k : g_log) CHECK(!((k.op == FREE || k.op == HOST_FREE) && k.p == callers_image));
}

int main()
{
    {
        hg_ctx ctx;                                             // (only its stream and its error text are used by the checks above the lifetime one)
        ctx.stream = kStream;
        check_ensure<uint8_t>(&ctx);
        check_ensure<float>(&ctx);
        check_ensure<Seg>(&ctx);
        check_ring<4>(&ctx);
        check_ring<64>(&ctx);
        check_staged_upload(&ctx);
        check_solve(&ctx);
    }
    check_lifetime();
    std::printf("ctx_mem_check: checks %ld failures %ld live %zu\n", g_checks, g_bad, g_dev.size() + g_host.size() + g_events.size());
    return g_bad == 0 ? 0 : 1;
}
