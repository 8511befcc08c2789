// hg_mem.h -- who owns the context's memory: device buffers (DevBuf), page-locked blocks (PinnedBuf) and the rings of page-locked staging
// slots frame sets are uploaded through (StageRing).  Each frees what it holds in its destructor, so deleting the context frees everything;
// hg_destroy synchronises the stream first.  Needs the HIP runtime API, the HG_* codes and fail() only (tests/cpp/ctx_mem_check.cpp drives it
// against a fake runtime).  Internal: nothing here is exported.
#pragma once
#include "../../include/hgwarp.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>

inline int fail(hg_ctx *c, int code, const std::string &msg);       // hg_ctx.h: records the message, returns the code
inline hipStream_t stream_of(const hg_ctx *c);                      // hg_ctx.h: the context's warp stream

#define HIP_TRY(c, expr)                                                                                     \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail((c), HG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

#define HG_TRY(expr) do { int s_ = (expr); if (s_ != HG_OK) return s_; } while (0)

struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };

// ------------------------------------------------------------------------------------------------ device buffers
// cap elements at p, owned while cap > 0.  Reads like the T * it holds.  borrow(): caller memory, never freed (capacity 0).
template <typename T>
struct DevBuf : NoCopy {
    T *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (cap) (void)hipFree(p); p = nullptr; cap = 0; }      // (the caller has waited for whatever used the block)
    void borrow(T *q) { release(); p = q; }
};

// Room for `need` elements; the contents are not kept.  A block in use is only replaced after the stream has drained.
template <typename T>
inline int ensure(hg_ctx *c, DevBuf<T> &b, size_t need)
{
    if (need <= b.cap) return HG_OK;
    const size_t n = std::max(need, b.cap + b.cap / 2);      // geometric growth from the OLD capacity
    if (b.cap) { HIP_TRY(c, hipStreamSynchronize(stream_of(c))); HIP_TRY(c, hipFree(b.p)); }
    b.p = nullptr; b.cap = 0;                                // (a borrowed pointer is dropped, not freed)
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T));
    if (e != hipSuccess) return fail(c, HG_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    b.p = static_cast<T *>(q); b.cap = n;
    return HG_OK;
}

// ------------------------------------------------------------------------------------------------ page-locked memory
template <typename T>
struct PinnedBuf : NoCopy {
    T *h = nullptr;
    size_t cap = 0;                                          // elements
    ~PinnedBuf() { if (h) (void)hipHostFree(h); }
    operator T *() const { return h; }
    // A fresh block of n elements in place of the old one (contents not kept; the caller has waited for whatever used it).
    int alloc(hg_ctx *c, size_t n, const char *what)
    {
        if (h) { HIP_TRY(c, hipHostFree(h)); h = nullptr; cap = 0; }
        void *q = nullptr;
        hipError_t e = hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return fail(c, HG_ERR_NOMEM, std::string("hipHostMalloc (") + what + "): " + hipGetErrorString(e));
        h = static_cast<T *>(q); cap = n;
        return HG_OK;
    }
};

// ------------------------------------------------------------------------------------------------ staging rings
// Frame sets and frame tables go up through a ring of page-locked slots: the caller's arrays are copied into the next slot and uploaded
// stream-ordered, so a call neither waits for the GPU nor keeps caller memory.  `done` is recorded behind the slot's upload: its bytes are not
// rewritten before the copy that reads them has run -- the only wait, and only once the ring has lapped an upload that is still queued.
struct StageSlot : PinnedBuf<uint8_t> {
    hipEvent_t done = nullptr;
    bool used = false;
    ~StageSlot() { if (done) (void)hipEventDestroy(done); }
};

template <int N, typename Slot = StageSlot>
struct StageRing {
    Slot slot[N];
    int cur = -1;                                            // the slot of the last committed upload
    int next() const { return (cur + 1) % N; }               // the slot the next acquire() hands out
    // The next slot with room for `bytes`, free to be written.  Nothing changes hands until commit(): after a failure the slot is taken again.
    int acquire(hg_ctx *c, size_t bytes, const char *what, Slot **out)
    {
        Slot &s = slot[next()];
        if (!s.done) HIP_TRY(c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        if (s.used) HIP_TRY(c, hipEventSynchronize(s.done));
        if (bytes > s.cap) HG_TRY(s.alloc(c, bytes + bytes / 4, what));
        *out = &s;
        return HG_OK;
    }
    // Behind the upload out of `s` (the slot acquire() returned).
    int commit(hg_ctx *c, Slot *s)
    {
        HIP_TRY(c, hipEventRecord(s->done, stream_of(c)));
        s->used = true;
        cur = (int)(s - slot);
        return HG_OK;
    }
};
