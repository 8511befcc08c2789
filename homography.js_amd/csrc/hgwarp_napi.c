/*
 * hgwarp_napi.c -- thin N-API addon over the C ABI (include/hgwarp.h) for the drop-in JS class js/Homography.mjs.
 *
 * It only unwraps TypedArrays, calls libhgwarp.so on the main JS thread (the reference's warp() is synchronous too)
 * and creates the result arrays; failures are thrown as bare strings like the reference does (`throw("...")`).
 * Built with plain gcc against /usr/include/node (Makefile target lib/hgwarp.node); no node-gyp, no C++.
 */
#define _GNU_SOURCE
#include <node_api.h>
#include <sys/mman.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hgwarp.h"

#define NAPI_OK(call) do { if ((call) != napi_ok) { napi_throw_error(env, NULL, "hgwarp: N-API call failed: " #call); return NULL; } } while (0)

static napi_value throw_str(napi_env env, const char *msg)
{
    napi_value s;
    napi_create_string_utf8(env, msg, NAPI_AUTO_LENGTH, &s);
    napi_throw(env, s);                       /* bare string, like the reference's throw("...") */
    return NULL;
}

static napi_value throw_hg(napi_env env, hg_ctx *ctx, const char *what, int code)
{
    char buf[512];
    snprintf(buf, sizeof buf, "hgwarp %s failed (%d): %s", what, code, hg_last_error(ctx));
    return throw_str(env, buf);
}

#define HG_CALL(ctx, what, call) do { int rc_ = (call); if (rc_ != HG_OK) return throw_hg(env, (ctx), (what), rc_); } while (0)

/* d_batch: device buffer the frames of warpInversePiecewiseBatch are produced in (kept between calls, grown as needed) */
/* n_pts / n_tris: the mesh last set, so that point-set and matrix buffers can be checked before the C ABI reads / fills them */
/* d_imgs: device buffer of the per-frame sources of setImages() (kept, grown as needed) */
/* d_remap: device scratch of the remap* functions: the field, the plane and the result; of mosaic*: the fields, the canvas, the weights (kept, grown as needed) */
/* slab: page-locked memory behind ONE external ArrayBuffer whose views are the frames of a batch (see "batches" below) */
typedef struct { void *ptr; size_t cap; napi_ref ab; } slab_t;
typedef struct { hg_ctx *ctx; int obj_w, obj_h; void *d_batch; size_t d_batch_cap; size_t n_pts, n_tris; void *d_imgs; size_t d_imgs_cap; slab_t slab[2]; void *d_remap; size_t d_remap_cap; } handle_t;

static void release_ctx(handle_t *h)
{
    if (h->ctx) {
        if (h->d_batch) hg_device_free(h->ctx, h->d_batch);
        if (h->d_remap) hg_device_free(h->ctx, h->d_remap);
        if (h->d_imgs) hg_device_free(h->ctx, h->d_imgs);      /* (waits for the stream; the context that aliases it goes next) */
        hg_destroy(h->ctx);
    }
    h->ctx = NULL; h->d_batch = NULL; h->d_batch_cap = 0; h->d_imgs = NULL; h->d_imgs_cap = 0; h->d_remap = NULL; h->d_remap_cap = 0;
}

static void slab_drop(napi_env env, slab_t *sl, int detach);

static void handle_finalize(napi_env env, void *data, void *hint)
{
    (void)hint;
    handle_t *h = (handle_t *)data;
    if (h) { for (int k = 0; k < 2; k++) slab_drop(env, &h->slab[k], 0); release_ctx(h); free(h); }
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv)
{
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) { throw_str(env, "hgwarp: wrong number of arguments"); return 0; }
    return 1;
}

static handle_t *get_handle(napi_env env, napi_value v)
{
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((handle_t *)p)->ctx) { throw_str(env, "hgwarp: invalid or destroyed context handle"); return NULL; }
    return (handle_t *)p;
}

/* typed array of an exact element type; returns data pointer and element count */
static void *get_typed(napi_env env, napi_value v, napi_typedarray_type want, size_t *len, const char *name)
{
    bool is = false;
    napi_typedarray_type t; size_t n = 0; void *data = NULL; napi_value ab; size_t off = 0;
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is || napi_get_typedarray_info(env, v, &t, &n, &data, &ab, &off) != napi_ok ||
        (t != want && !(want == napi_uint8_clamped_array && t == napi_uint8_array))) {
        char buf[160]; snprintf(buf, sizeof buf, "hgwarp: argument '%s' has the wrong TypedArray type", name);
        throw_str(env, buf); return NULL;
    }
    *len = n;
    return data ? data : (void *)"";          /* zero-length arrays may report a NULL pointer */
}

static int get_i32(napi_env env, napi_value v, int *out)
{
    double d;
    if (napi_get_value_double(env, v, &d) != napi_ok) { throw_str(env, "hgwarp: expected a number"); return 0; }
    /* NaN, +-Infinity and anything outside int32 would be undefined behaviour in the conversion (degenerate matrices give
     * such window sizes; the reference then dies with a RangeError on its allocation) */
    if (!(d >= -2147483648.0 && d <= 2147483647.0)) { throw_str(env, "hgwarp: number is not finite or does not fit an int32 (Invalid typed array length)"); return 0; }
    *out = (int)d;
    return 1;
}

static napi_value make_typed(napi_env env, napi_typedarray_type t, size_t n, size_t elem, void **data)
{
    napi_value ab, ta;
    NAPI_OK(napi_create_arraybuffer(env, n * elem, data, &ab));
    NAPI_OK(napi_create_typedarray(env, t, n, ab, 0, &ta));
    return ta;
}

/* ---------------------------------------------------------------- pinned frame pool
 * A fresh 34 MB Uint8ClampedArray per 4K frame is what the reference's contract asks for (:991, :1040), and in V8 that is a
 * calloc -> mmap -> ~8 400 first-touch page faults (8-9 ms, far more than the 1.3 ms of PCIe traffic).  Frames of 1 MiB and
 * more therefore come from a pool of page-locked buffers (hg_host_alloc) handed to JavaScript as EXTERNAL ArrayBuffers: the
 * GPU DMAs straight into them and a buffer returns to the pool when its ArrayBuffer is collected.  Node 12 runs N-API
 * finalizers from the event loop only, so a loop that never yields gets no buffer back: the pool then grows up to
 * `pin_limit` bytes (default 2 GiB, setPinnedLimit()) and after that warp() falls back to plain V8 arrays (slower, still
 * correct).  To get buffers back inside such a loop anyway, every pooled frame also carries a WEAK reference to its ArrayBuffer:
 * V8 clears it during the collection itself, so pin_acquire() can see synchronously that a frame is dead and reuse its
 * buffer long before the deferred finalizer runs (and the JS class asks for a collection when poolPressure() says the pool is
 * starving: see there).  release(typedArray) hands a frame back at once (its ArrayBuffer is detached). */
typedef struct { void *ptr; size_t cap; int in_use; int zombie; unsigned gen; napi_ref weak; } pin_t;
typedef struct { int idx; unsigned gen; } pin_ref_t;
#define PIN_MAX 512
#define PIN_GC_EVERY 32
static const size_t PIN_MIN_FRAME = (size_t)1 << 20;
/* The pool is PER ENVIRONMENT (napi_set_instance_data): its napi_refs belong to one env and its buffers are handed out on that
 * env's thread only, so a second env (worker_threads, or the addon loaded into two contexts) gets a pool of its own instead of
 * racing on -- and dereferencing references of -- somebody else's. */
typedef struct {
    pin_t pins[PIN_MAX];
    int npins;
    size_t pin_bytes, pin_limit;
    int since_gc;                                            /* pooled frames handed out since the last requested collection */
    int pool_malloc;                                         /* _poolTestFrames(): plain malloc instead of pinned memory (no GPU needed) */
    /* May a buffer whose ArrayBuffer is dead (weak reference cleared) or detached (release()) back a NEW external ArrayBuffer
     * before the old one's finalizer has run?  Under Node 12 (V8 7.x) yes, and that is what lets a synchronous loop get frames
     * back at all (finalizers only run from the event loop there).  From V8 8 on (Node >= 14) two ArrayBuffers over one backing
     * pointer abort the process (nodejs/node#32463): there a buffer is recycled only once its finalizer HAS run. */
    int early_reuse;
    double stat_hit, stat_new, stat_fallback, stat_reaped, stat_finalized, stat_forced_gc;   /* poolStats() */
} pool_t;

static pool_t *pool_of(napi_env env)
{
    void *p = NULL;
    if (napi_get_instance_data(env, &p) != napi_ok || !p) { throw_str(env, "hgwarp: addon instance data is missing"); return NULL; }
    return (pool_t *)p;
}

static void pin_drop(pool_t *P, int i)
{
    if (P->pins[i].ptr) { if (P->pool_malloc) free(P->pins[i].ptr); else hg_host_free(P->pins[i].ptr); P->pin_bytes -= P->pins[i].cap; }
    P->pins[i].ptr = NULL; P->pins[i].cap = 0; P->pins[i].in_use = 0; P->pins[i].zombie = 0;
}

/* frames whose ArrayBuffer has been collected (weak reference cleared) although their finalizer has not run yet */
static void pin_reap(napi_env env, pool_t *P)
{
    for (int i = 0; i < P->npins; i++) {
        if (!P->pins[i].ptr || !P->pins[i].in_use || !P->pins[i].weak) continue;
        napi_value v = NULL;
        if (napi_get_reference_value(env, P->pins[i].weak, &v) == napi_ok && v == NULL) {
            napi_delete_reference(env, P->pins[i].weak);
            P->pins[i].weak = NULL;
            P->stat_reaped++;
            int64_t adj; napi_adjust_external_memory(env, -(int64_t)P->pins[i].cap, &adj);
            if (P->early_reuse) { P->pins[i].in_use = 0; P->pins[i].gen++; }   /* the late finalizer will not match */
            else P->pins[i].zombie = 1;                                        /* V8 >= 8: stays out of circulation until pin_finalize */
        }
    }
}

static int pin_acquire(napi_env env, pool_t *P, size_t bytes)
{
    if (bytes < PIN_MIN_FRAME || P->pin_limit == 0) return -1;
    int best = -1, empty = -1;
    for (int pass = 0; pass < 2 && best < 0; pass++) {
        if (pass == 1) pin_reap(env, P);
        for (int i = 0; i < P->npins; i++) {
            if (!P->pins[i].ptr) continue;
            if (!P->pins[i].in_use && P->pins[i].cap >= bytes && P->pins[i].cap <= bytes + bytes / 2 && (best < 0 || P->pins[i].cap < P->pins[best].cap)) best = i;
        }
    }
    P->since_gc++;
    if (best >= 0) { P->pins[best].in_use = 1; P->stat_hit++; return best; }
    for (int i = 0; i < P->npins; i++) if (!P->pins[i].ptr) { empty = i; break; }
    /* make room: idle buffers of the wrong size go first */
    for (int i = 0; i < P->npins && P->pin_bytes + bytes > P->pin_limit; i++) if (P->pins[i].ptr && !P->pins[i].in_use) { pin_drop(P, i); if (empty < 0) empty = i; }
    if (P->pin_bytes + bytes > P->pin_limit) { P->stat_fallback++; return -1; }
    if (empty < 0) { if (P->npins == PIN_MAX) { P->stat_fallback++; return -1; } empty = P->npins++; }
    void *p = NULL;
    if (P->pool_malloc) p = malloc(bytes);
    else if (hg_host_alloc(bytes, &p) != HG_OK) p = NULL;
    if (!p) { P->stat_fallback++; return -1; }
    P->stat_new++;
    P->pins[empty].ptr = p; P->pins[empty].cap = bytes; P->pins[empty].in_use = 1; P->pins[empty].gen++;
    P->pin_bytes += bytes;
    return empty;
}

static void pin_finalize(napi_env env, void *data, void *hint)
{
    (void)data;
    pin_ref_t *r = (pin_ref_t *)hint;
    pool_t *P = NULL;
    if (napi_get_instance_data(env, (void **)&P) != napi_ok || !P) { free(r); return; }      /* (the env is going away: pool_free owns the buffers) */
    if (r && r->idx >= 0 && r->idx < P->npins && P->pins[r->idx].gen == r->gen && P->pins[r->idx].in_use) {
        if (P->pins[r->idx].weak) { napi_delete_reference(env, P->pins[r->idx].weak); P->pins[r->idx].weak = NULL; }
        P->stat_finalized++;
        P->pins[r->idx].in_use = 0;
        if (P->pins[r->idx].zombie) P->pins[r->idx].zombie = 0;               /* (its external-memory accounting went when it was reaped / released) */
        else { int64_t adj; napi_adjust_external_memory(env, -(int64_t)P->pins[r->idx].cap, &adj); }
    }
    free(r);
}

/* a Uint8ClampedArray of `bytes` bytes over a pooled pinned buffer, or NULL (pool exhausted / small frame) */
static napi_value make_pinned(napi_env env, size_t bytes, void **data)
{
    pool_t *P = pool_of(env);
    if (!P) return NULL;
    const int i = pin_acquire(env, P, bytes);
    if (i < 0) return NULL;
    pin_ref_t *r = (pin_ref_t *)malloc(sizeof *r);
    napi_value ab, ta;
    if (!r) { P->pins[i].in_use = 0; return NULL; }
    r->idx = i; r->gen = P->pins[i].gen;
    if (napi_create_external_arraybuffer(env, P->pins[i].ptr, bytes, pin_finalize, r, &ab) != napi_ok) { P->pins[i].in_use = 0; free(r); return NULL; }
    int64_t adj; napi_adjust_external_memory(env, (int64_t)P->pins[i].cap, &adj);     /* V8 learns about the memory pressure */
    P->pins[i].weak = NULL;
    if (napi_create_reference(env, ab, 0, &P->pins[i].weak) != napi_ok) P->pins[i].weak = NULL;
    if (napi_create_typedarray(env, napi_uint8_clamped_array, bytes, ab, 0, &ta) != napi_ok) return NULL;
    *data = P->pins[i].ptr;
    return ta;
}

/* RGBA outputs.  Default: a fresh, V8-owned Uint8ClampedArray per call like the reference (:991, :1040).  If the caller
 * passes its own Uint8ClampedArray of at least `bytes` bytes as the optional last argument, the frame is written there
 * and a view of exactly `bytes` bytes over the same memory is returned: no 34 MB allocation, first-touch page faults and
 * garbage per 4K frame (that, not PCIe, is most of the host time of a frame on this platform).  Measured and rejected:
 * pooled external ArrayBuffers -- Node 12 runs their finalizers only from the event loop, so a synchronous warp() loop
 * would hold every frame it ever produced. */
static napi_value make_pixels(napi_env env, size_t bytes, napi_value reuse, int have_reuse, void **data)
{
    if (have_reuse) {
        bool is = false;
        napi_typedarray_type t; size_t n = 0, off = 0; void *p = NULL; napi_value ab, ta;
        if (napi_is_typedarray(env, reuse, &is) == napi_ok && is &&
            napi_get_typedarray_info(env, reuse, &t, &n, &p, &ab, &off) == napi_ok &&
            (t == napi_uint8_clamped_array || t == napi_uint8_array) && n >= bytes && p) {
            NAPI_OK(napi_create_typedarray(env, napi_uint8_clamped_array, bytes, ab, off, &ta));
            *data = p;
            return ta;
        }
    }
    napi_value pinned = make_pinned(env, bytes, data);        /* fresh frame, pooled page-locked memory (see above) */
    if (pinned) return pinned;
    napi_value ta = make_typed(env, napi_uint8_clamped_array, bytes, 1, data);
    /* Pool exhausted (or switched off): a plain V8 array.  Its memory is a fresh anonymous mapping nobody has touched yet;
     * asking for transparent huge pages BEFORE the first write turns ~8 400 4-KiB page faults of a 4K frame into ~17 (where
     * the kernel runs THP in `madvise` mode, as on the MI355X hosts).  Advice only: failure changes nothing. */
    if (ta && bytes >= ((size_t)4 << 20) && *data) {
        const uintptr_t lo = ((uintptr_t)*data + 4095) & ~(uintptr_t)4095, hi = ((uintptr_t)*data + bytes) & ~(uintptr_t)4095;
        if (hi > lo) (void)madvise((void *)lo, hi - lo, MADV_HUGEPAGE);
    }
    return ta;
}

/* release(typedArray): a frame produced by warp() goes back to the pool now; its ArrayBuffer is detached (length 0). */
static napi_value fn_release(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    bool is = false;
    napi_typedarray_type t; size_t n = 0, off = 0; void *p = NULL; napi_value ab;
    napi_value res; napi_get_boolean(env, false, &res);
    pool_t *P = pool_of(env); if (!P) return NULL;
    if (napi_is_typedarray(env, a[0], &is) != napi_ok || !is || napi_get_typedarray_info(env, a[0], &t, &n, &p, &ab, &off) != napi_ok || !p) return res;
    for (int i = 0; i < P->npins; i++)
        if (P->pins[i].ptr == (char *)p - off && P->pins[i].in_use) {
            if (napi_detach_arraybuffer(env, ab) != napi_ok) return res;
            if (P->pins[i].weak) { napi_delete_reference(env, P->pins[i].weak); P->pins[i].weak = NULL; }
            if (P->early_reuse) { P->pins[i].in_use = 0; P->pins[i].gen++; }   /* the pending finalizer of this ArrayBuffer no longer matches */
            else P->pins[i].zombie = 1;                                        /* V8 >= 8: recycled once the detached buffer's finalizer has run */
            int64_t adj; napi_adjust_external_memory(env, -(int64_t)P->pins[i].cap, &adj);
            napi_get_boolean(env, true, &res);
            break;
        }
    return res;
}

/* _poolTestFrames(n, bytes): n frames of `bytes` bytes through the very allocation path warp() / warpBatch() use, without any
 * GPU work (tests of the pool's life cycle on machines without a GPU; the pool is switched to plain malloc memory). */
static napi_value fn_pool_test_frames(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    int n; double bytes;
    if (!get_i32(env, a[0], &n) || napi_get_value_double(env, a[1], &bytes) != napi_ok || n < 0 || !(bytes >= 0)) return throw_str(env, "hgwarp: _poolTestFrames(n, bytes)");
    pool_t *P = pool_of(env); if (!P) return NULL;
    if (!P->pool_malloc) { for (int i = 0; i < P->npins; i++) if (P->pins[i].ptr && !P->pins[i].in_use) pin_drop(P, i); P->pool_malloc = 1; }
    napi_value arr;
    NAPI_OK(napi_create_array_with_length(env, n, &arr));
    for (int f = 0; f < n; f++) {
        void *out; napi_value ta = make_pixels(env, (size_t)bytes, NULL, 0, &out);
        if (!ta) return NULL;
        if (bytes > 0) ((uint8_t *)out)[0] = (uint8_t)f;
        napi_set_element(env, arr, f, ta);
    }
    return arr;
}

/* pinnedBuffer(bytes): a zeroed Uint8ClampedArray in pooled page-locked memory (a plain V8 array when the pool is off, exhausted, or the
 * buffer is small): for SOURCE images the caller fills itself (decoded video frames ...) -- uploads out of page-locked memory are true
 * asynchronous DMA at the full PCIe rate, uploads out of V8's pageable memory are staged by the runtime (~20 % slower and host-blocking). */
static napi_value fn_pinned_buffer(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    double bytes;
    if (napi_get_value_double(env, a[0], &bytes) != napi_ok || !(bytes >= 0) || bytes > 4.0e9) return throw_str(env, "hgwarp: pinnedBuffer(bytes)");
    void *out = NULL;
    napi_value ta = make_pixels(env, (size_t)bytes, NULL, 0, &out);
    if (ta && out && bytes > 0) memset(out, 0, (size_t)bytes);
    return ta;
}

/* poolPressure(bytes, n): should the caller run a collection before asking for n frames of `bytes` bytes?  True when the pool
 * cannot serve them from free (or already collected) buffers AND at least `g_next_gc_live` pooled frames are alive or the
 * cap would be exceeded.  A loop that allocates little JavaScript (warpBatch: 8 frames per call) can go a long time without
 * a collection although dozens of 34 MB frames are garbage; V8's own external-memory heuristics start incremental cycles
 * that treat everything allocated meanwhile as live.  The JS class then calls a real collector (js/Homography.mjs) and
 * poolCollected(), which reaps and restarts the count: the next collection is due after another PIN_GC_EVERY pooled frames
 * (a caller that really keeps all its frames alive pays one useless collection per PIN_GC_EVERY frames), or when the cap is hit. */

static napi_value fn_pool_pressure(napi_env env, napi_callback_info info)
{
    napi_value a[2], res;
    if (!get_args(env, info, 2, a)) return NULL;
    double bytes; int n;
    napi_get_boolean(env, false, &res);
    pool_t *P = pool_of(env); if (!P) return NULL;
    if (napi_get_value_double(env, a[0], &bytes) != napi_ok || !get_i32(env, a[1], &n)) return res;
    if (!(bytes >= (double)PIN_MIN_FRAME) || P->pin_limit == 0 || n <= 0) return res;
    pin_reap(env, P);
    int fit = 0, live = 0;
    for (int i = 0; i < P->npins; i++) {
        if (!P->pins[i].ptr) continue;
        if (P->pins[i].in_use) live++;
        else if (P->pins[i].cap >= (size_t)bytes && P->pins[i].cap <= (size_t)bytes + (size_t)bytes / 2) fit++;
    }
    if (fit >= n) return res;
    (void)live;
    if (P->since_gc >= PIN_GC_EVERY || (double)P->pin_bytes + (n - fit) * bytes > (double)P->pin_limit) napi_get_boolean(env, true, &res);
    return res;
}

static napi_value fn_pool_collected(napi_env env, napi_callback_info info)
{
    (void)info;
    pool_t *P = pool_of(env); if (!P) return NULL;
    const double before = P->stat_reaped;
    pin_reap(env, P);
    P->since_gc = 0;
    P->stat_forced_gc++;
    napi_value v; NAPI_OK(napi_create_double(env, P->stat_reaped - before, &v));
    return v;
}

/* poolStats(): counters of the pinned frame pool since the addon was loaded */
static napi_value fn_pool_stats(napi_env env, napi_callback_info info)
{
    (void)info;
    napi_value o, v;
    pool_t *P = pool_of(env); if (!P) return NULL;
    NAPI_OK(napi_create_object(env, &o));
    int in_use = 0, total = 0;
    for (int i = 0; i < P->npins; i++) if (P->pins[i].ptr) { total++; in_use += P->pins[i].in_use; }
    const struct { const char *k; double x; } kv[] = { {"pinnedBytes", (double)P->pin_bytes}, {"buffers", total}, {"inUse", in_use}, {"reused", P->stat_hit},
        {"allocated", P->stat_new}, {"fallbackToV8", P->stat_fallback}, {"reapedByWeakRef", P->stat_reaped}, {"forcedCollections", P->stat_forced_gc}, {"finalized", P->stat_finalized}, {"earlyReuse", P->early_reuse} };
    for (size_t i = 0; i < sizeof kv / sizeof kv[0]; i++) { NAPI_OK(napi_create_double(env, kv[i].x, &v)); NAPI_OK(napi_set_named_property(env, o, kv[i].k, v)); }
    return o;
}

/* setPinnedLimit(bytes): cap of the pinned frame pool (0 disables it: every frame is a plain V8 array); returns bytes in use */
static napi_value fn_set_pinned_limit(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    double d;
    if (napi_get_value_double(env, a[0], &d) != napi_ok || !(d >= 0)) return throw_str(env, "hgwarp: setPinnedLimit needs a non-negative number of bytes");
    pool_t *P = pool_of(env); if (!P) return NULL;
    P->pin_limit = d > 1e15 ? (size_t)1e15 : (size_t)d;
    for (int i = 0; i < P->npins; i++) if (P->pins[i].ptr && !P->pins[i].in_use && P->pin_bytes > P->pin_limit) pin_drop(P, i);
    napi_value v;
    NAPI_OK(napi_create_double(env, (double)P->pin_bytes, &v));
    return v;
}

/* optional trailing argument: argv[want] if present and not undefined/null */
static int get_args_opt(napi_env env, napi_callback_info info, size_t want, napi_value *argv, int *have_opt)
{
    size_t argc = want + 1;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) { throw_str(env, "hgwarp: wrong number of arguments"); return 0; }
    *have_opt = 0;
    if (argc > want) {
        napi_valuetype vt;
        if (napi_typeof(env, argv[want], &vt) == napi_ok && vt != napi_undefined && vt != napi_null) *have_opt = 1;
    }
    return 1;
}

/* ---------------------------------------------------------------- context */
static napi_value fn_create(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    int dev = 0;
    if (!get_i32(env, a[0], &dev)) return NULL;
    handle_t *h = (handle_t *)calloc(1, sizeof *h);
    int rc = hg_create(dev, &h->ctx);
    if (rc != HG_OK) { free(h); return throw_hg(env, NULL, "hg_create", rc); }
    napi_value ext;
    NAPI_OK(napi_create_external(env, h, handle_finalize, NULL, &ext));
    return ext;
}

static napi_value fn_destroy(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    void *p = NULL;
    if (napi_get_value_external(env, a[0], &p) == napi_ok && p) {
        handle_t *h = (handle_t *)p;
        if (h->ctx) (void)hg_sync(h->ctx);
        for (int k = 0; k < 2; k++) slab_drop(env, &h->slab[k], 0);      /* (frames the caller still holds keep their memory: the ArrayBuffer owns it) */
        release_ctx(h);
    }
    return NULL;
}

static napi_value fn_device_count(napi_env env, napi_callback_info info)
{
    (void)info;
    int n = 0;
    hg_device_count(&n);
    napi_value v;
    NAPI_OK(napi_create_int32(env, n, &v));
    return v;
}

/* ---------------------------------------------------------------- host solves */
static napi_value fn_solve_affine(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    size_t n0, n1;
    float *s = (float *)get_typed(env, a[0], napi_float32_array, &n0, "src"); if (!s) return NULL;
    float *d = (float *)get_typed(env, a[1], napi_float32_array, &n1, "dst"); if (!d) return NULL;
    if (n0 < 6 || n1 < 6) return throw_str(env, "hgwarp: solveAffine needs 6 values per point set");
    void *out; napi_value r = make_typed(env, napi_float32_array, 6, 4, &out); if (!r) return NULL;
    HG_CALL(NULL, "hg_solve_affine", hg_solve_affine(s, d, (float *)out));
    return r;
}

static napi_value fn_invert_affine(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    size_t n;
    float *m = (float *)get_typed(env, a[0], napi_float32_array, &n, "matrix"); if (!m) return NULL;
    if (n < 6) return throw_str(env, "hgwarp: invertAffine needs 6 values");
    void *out; napi_value r = make_typed(env, napi_float32_array, 6, 4, &out); if (!r) return NULL;
    HG_CALL(NULL, "hg_invert_affine", hg_invert_affine(m, (float *)out));
    return r;
}

static napi_value fn_solve_projective(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    size_t n0, n1;
    float *s = (float *)get_typed(env, a[0], napi_float32_array, &n0, "src"); if (!s) return NULL;
    float *d = (float *)get_typed(env, a[1], napi_float32_array, &n1, "dst"); if (!d) return NULL;
    if (n0 < 8 || n1 < 8) return throw_str(env, "hgwarp: solveProjective needs 8 values per point set");
    void *out; napi_value r = make_typed(env, napi_float64_array, 8, 8, &out); if (!r) return NULL;
    HG_CALL(NULL, "hg_solve_projective", hg_solve_projective(s, d, (double *)out));
    return r;
}

static napi_value fn_transform_limits(napi_env env, napi_callback_info info)
{
    napi_value a[4];
    if (!get_args(env, info, 4, a)) return NULL;
    int kind; size_t n; double w, h;
    if (!get_i32(env, a[0], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[1], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (napi_get_value_double(env, a[2], &w) != napi_ok || napi_get_value_double(env, a[3], &h) != napi_ok) return throw_str(env, "hgwarp: width/height must be numbers");
    void *out; napi_value r = make_typed(env, napi_float64_array, 4, 8, &out); if (!r) return NULL;
    HG_CALL(NULL, "hg_transform_limits", hg_transform_limits(kind, m, w, h, (double *)out));
    return r;
}

static napi_value fn_minmax_xy(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    size_t n;
    float *p = (float *)get_typed(env, a[0], napi_float32_array, &n, "points"); if (!p) return NULL;
    void *out; napi_value r = make_typed(env, napi_float64_array, 4, 8, &out); if (!r) return NULL;
    HG_CALL(NULL, "hg_minmax_xy", hg_minmax_xy(p, (int)n, (double *)out));
    return r;
}

static napi_value fn_triangulate(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    size_t n;
    float *p = (float *)get_typed(env, a[0], napi_float32_array, &n, "points"); if (!p) return NULL;
    int count = 0;
    HG_CALL(NULL, "hg_triangulate", hg_triangulate(p, (int)(n / 2), NULL, 0, &count));
    void *out; napi_value r = make_typed(env, napi_uint32_array, (size_t)count * 3, 4, &out); if (!r) return NULL;
    if (count) HG_CALL(NULL, "hg_triangulate", hg_triangulate(p, (int)(n / 2), (uint32_t *)out, count, &count));
    return r;
}

/* ---------------------------------------------------------------- image + warps */
static napi_value fn_set_image(napi_env env, napi_callback_info info)
{
    napi_value a[4];
    if (!get_args(env, info, 4, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t n; int w, hh;
    uint8_t *px = (uint8_t *)get_typed(env, a[1], napi_uint8_clamped_array, &n, "image.data"); if (!px) return NULL;
    if (!get_i32(env, a[2], &w) || !get_i32(env, a[3], &hh)) return NULL;
    if (w <= 0 || hh <= 0 || n < (size_t)w * (size_t)hh * 4) return throw_str(env, "hgwarp: image.data is smaller than width*height*4");
    HG_CALL(h->ctx, "hg_set_image", hg_set_image(h->ctx, px, w, hh));
    return NULL;
}

/* setImages(ctx, [Uint8ClampedArray, ...], w, h): one source per frame of the next batch (`warp(image_f)` per frame in the
 * reference: setImage :290 on every call).  The images are copied into one device buffer; frame f reads image f % n. */
static napi_value fn_set_images(napi_env env, napi_callback_info info)
{
    napi_value a[4];
    if (!get_args(env, info, 4, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    bool is_arr = false; uint32_t n = 0; int w, hh;
    if (napi_is_array(env, a[1], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, a[1], &n) != napi_ok || n == 0)
        return throw_str(env, "hgwarp: setImages needs a non-empty array of image data arrays");
    if (!get_i32(env, a[2], &w) || !get_i32(env, a[3], &hh)) return NULL;
    if (w <= 0 || hh <= 0) return throw_str(env, "hgwarp: bad image size");
    const size_t bytes = (size_t)w * (size_t)hh * 4, stride = (bytes + 255) & ~(size_t)255;
    if (stride * n > h->d_imgs_cap) {
        /* grow: new buffer first, the context's alias moves to it, only then the old one is freed (never a dangling alias) */
        void *q = NULL;
        HG_CALL(h->ctx, "hg_device_alloc", hg_device_alloc(h->ctx, stride * n, &q));
        int rc = hg_set_images_device(h->ctx, q, w, hh, (int)n, stride);
        if (rc != HG_OK) { hg_device_free(h->ctx, q); return throw_hg(env, h->ctx, "hg_set_images_device", rc); }
        if (h->d_imgs) hg_device_free(h->ctx, h->d_imgs);
        h->d_imgs = q; h->d_imgs_cap = stride * n;
    }
    for (uint32_t k = 0; k < n; k++) {
        napi_value el; size_t len;
        NAPI_OK(napi_get_element(env, a[1], k, &el));
        uint8_t *px = (uint8_t *)get_typed(env, el, napi_uint8_clamped_array, &len, "images[k]"); if (!px) return NULL;
        if (len < bytes) return throw_str(env, "hgwarp: an image is smaller than width*height*4");
        HG_CALL(h->ctx, "hg_copy_to_device", hg_copy_to_device(h->ctx, (uint8_t *)h->d_imgs + stride * k, px, bytes));
    }
    HG_CALL(h->ctx, "hg_set_images_device", hg_set_images_device(h->ctx, h->d_imgs, w, hh, (int)n, stride));
    return NULL;
}

static int get_geom(napi_env env, napi_value *a, hg_geom *g)
{
    int v[4];
    for (int i = 0; i < 4; i++) if (!get_i32(env, a[i], &v[i])) return 0;
    g->x_off = v[0]; g->y_off = v[1]; g->obj_w = v[2]; g->obj_h = v[3];
    return 1;
}

static napi_value fn_warp_inverse_geometric(napi_env env, napi_callback_info info)
{
    napi_value a[8]; int reuse = 0;
    if (!get_args_opt(env, info, 7, a, &reuse)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind; size_t n; hg_geom g;
    if (!get_i32(env, a[1], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[2], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (!get_geom(env, a + 3, &g)) return NULL;
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    void *out; napi_value r = make_pixels(env, px * 4, a[7], reuse, &out); if (!r) return NULL;
    if (px) HG_CALL(h->ctx, "hg_warp_inverse_geometric", hg_warp_inverse_geometric(h->ctx, kind, m, g, (uint8_t *)out));
    return r;
}

static napi_value fn_piecewise_set_mesh(napi_env env, napi_callback_info info)
{
    napi_value a[5];
    if (!get_args(env, info, 5, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t np, nt; int msx, msy;
    float *src = (float *)get_typed(env, a[1], napi_float32_array, &np, "srcPoints"); if (!src) return NULL;
    uint32_t *tris = (uint32_t *)get_typed(env, a[2], napi_uint32_array, &nt, "triangles"); if (!tris) return NULL;
    if (!get_i32(env, a[3], &msx) || !get_i32(env, a[4], &msy)) return NULL;
    HG_CALL(h->ctx, "hg_piecewise_set_mesh", hg_piecewise_set_mesh(h->ctx, src, (int)(np / 2), tris, (int)(nt / 3), msx, msy));
    h->n_pts = np / 2; h->n_tris = nt / 3;
    return NULL;
}

static napi_value fn_piecewise_prepare(napi_env env, napi_callback_info info)
{
    napi_value a[6];
    if (!get_args(env, info, 6, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t n; hg_geom g;
    float *dst = (float *)get_typed(env, a[1], napi_float32_array, &n, "dstPoints"); if (!dst) return NULL;
    if (!get_geom(env, a + 2, &g)) return NULL;
    if (h->n_pts == 0 || n < 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold one x,y pair per mesh point (piecewiseSetMesh first)");
    HG_CALL(h->ctx, "hg_piecewise_prepare", hg_piecewise_prepare(h->ctx, dst, g));
    h->obj_w = g.obj_w; h->obj_h = g.obj_h;
    return NULL;
}

static napi_value fn_warp_inverse_piecewise(napi_env env, napi_callback_info info)
{
    napi_value a[2]; int reuse = 0;
    if (!get_args_opt(env, info, 1, a, &reuse)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    const size_t px = (h->obj_w > 0 && h->obj_h > 0) ? (size_t)h->obj_w * h->obj_h : 0;
    void *out; napi_value r = make_pixels(env, px * 4, a[1], reuse, &out); if (!r) return NULL;
    if (px) HG_CALL(h->ctx, "hg_warp_inverse_piecewise", hg_warp_inverse_piecewise(h->ctx, (uint8_t *)out));
    return r;
}

static napi_value fn_warp_forward_geometric(napi_env env, napi_callback_info info)
{
    napi_value a[7];
    if (!get_args(env, info, 7, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind; size_t n; hg_geom g;
    if (!get_i32(env, a[1], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[2], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (!get_geom(env, a + 3, &g)) return NULL;
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    void *out; napi_value r = make_pixels(env, px * 4, NULL, 0, &out); if (!r) return NULL;
    if (px) HG_CALL(h->ctx, "hg_warp_forward_geometric", hg_warp_forward_geometric(h->ctx, kind, m, g, (uint8_t *)out));
    return r;
}

static napi_value fn_warp_forward_piecewise(napi_env env, napi_callback_info info)
{
    napi_value a[8];
    if (!get_args(env, info, 8, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t n; int mx, my; hg_geom g;
    float *dst = (float *)get_typed(env, a[1], napi_float32_array, &n, "dstPoints"); if (!dst) return NULL;
    if (!get_i32(env, a[2], &mx) || !get_i32(env, a[3], &my)) return NULL;
    if (!get_geom(env, a + 4, &g)) return NULL;
    if (h->n_pts == 0 || n < 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold one x,y pair per mesh point (piecewiseSetMesh first)");
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    void *out; napi_value r = make_pixels(env, px * 4, NULL, 0, &out); if (!r) return NULL;
    if (px) HG_CALL(h->ctx, "hg_warp_forward_piecewise", hg_warp_forward_piecewise(h->ctx, dst, mx, my, g, (uint8_t *)out));
    return r;
}

/* ---------------------------------------------------------------- reference-state forms (stale matrices / stale map) */
/* solveAffineTriangles(src, dst, triangles) -> Float32Array(6 T): affineMatrixFromTriangles per triangle (:785-804), on the host */
static napi_value fn_solve_affine_triangles(napi_env env, napi_callback_info info)
{
    napi_value a[3];
    if (!get_args(env, info, 3, a)) return NULL;
    size_t ns, nd, nt;
    float *s = (float *)get_typed(env, a[0], napi_float32_array, &ns, "src"); if (!s) return NULL;
    float *d = (float *)get_typed(env, a[1], napi_float32_array, &nd, "dst"); if (!d) return NULL;
    uint32_t *t = (uint32_t *)get_typed(env, a[2], napi_uint32_array, &nt, "triangles"); if (!t) return NULL;
    const size_t np = (ns < nd ? ns : nd) / 2, T = nt / 3;
    void *out; napi_value r = make_typed(env, napi_float32_array, 6 * T, 4, &out); if (!r) return NULL;
    HG_CALL(NULL, "hg_solve_affine_triangles", hg_solve_affine_triangles(s, d, (int)np, t, (int)T, (float *)out));
    return r;
}

/* a map id without a matrix: the reference's loop throws a TypeError at that pixel (`matrix[0]` of undefined, :1383) */
static napi_value throw_state(napi_env env, hg_ctx *ctx, const char *what, int code)
{
    if (code == HG_ERR_RANGE) { napi_throw_type_error(env, NULL, "Cannot read property '0' of undefined"); return NULL; }
    return throw_hg(env, ctx, what, code);
}

/* warpInversePiecewiseState(ctx, fwdMats, dstPoints, triangles, minSrcX, minSrcY, xOff, yOff, objW, objH) */
static napi_value fn_warp_inverse_piecewise_state(napi_env env, napi_callback_info info)
{
    napi_value a[10];
    if (!get_args(env, info, 10, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t nm, np, nt; int msx, msy; hg_geom g;
    float *m = (float *)get_typed(env, a[1], napi_float32_array, &nm, "matrices"); if (!m) return NULL;
    float *p = (float *)get_typed(env, a[2], napi_float32_array, &np, "dstPoints"); if (!p) return NULL;
    uint32_t *t = (uint32_t *)get_typed(env, a[3], napi_uint32_array, &nt, "triangles"); if (!t) return NULL;
    if (!get_i32(env, a[4], &msx) || !get_i32(env, a[5], &msy)) return NULL;
    if (!get_geom(env, a + 6, &g)) return NULL;
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    void *out; napi_value r = make_pixels(env, px * 4, NULL, 0, &out); if (!r) return NULL;
    hg_tri_map_def def = { p, (int)(np / 2), t, (int)(nt / 3), g.obj_w, g.obj_h, g.y_off };
    if (px) { int rc = hg_warp_inverse_piecewise_state(h->ctx, m, (int)(nm / 6), &def, msx, msy, g, (uint8_t *)out);
              if (rc != HG_OK) return throw_state(env, h->ctx, "hg_warp_inverse_piecewise_state", rc); }
    return r;
}

/* warpForwardPiecewiseState(ctx, fwdMats, mapPoints, mapTriangles, mapWidth, mapHeight, mapYOff, minSrcX, minSrcY, maxSrcX, maxSrcY, xOff, yOff, objW, objH) */
static napi_value fn_warp_forward_piecewise_state(napi_env env, napi_callback_info info)
{
    napi_value a[15];
    if (!get_args(env, info, 15, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t nm, np, nt; int mw, mh, myo, msx, msy, mxx, mxy; hg_geom g;
    float *m = (float *)get_typed(env, a[1], napi_float32_array, &nm, "matrices"); if (!m) return NULL;
    float *p = (float *)get_typed(env, a[2], napi_float32_array, &np, "mapPoints"); if (!p) return NULL;
    uint32_t *t = (uint32_t *)get_typed(env, a[3], napi_uint32_array, &nt, "mapTriangles"); if (!t) return NULL;
    if (!get_i32(env, a[4], &mw) || !get_i32(env, a[5], &mh) || !get_i32(env, a[6], &myo)) return NULL;
    if (!get_i32(env, a[7], &msx) || !get_i32(env, a[8], &msy) || !get_i32(env, a[9], &mxx) || !get_i32(env, a[10], &mxy)) return NULL;
    if (!get_geom(env, a + 11, &g)) return NULL;
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    void *out; napi_value r = make_pixels(env, px * 4, NULL, 0, &out); if (!r) return NULL;
    hg_tri_map_def def = { p, (int)(np / 2), t, (int)(nt / 3), mw, mh, myo };
    uint8_t none[4];                                          /* a blank window still gets the held map's ids checked (the reference's loop runs and may throw) */
    if (!px) { g.x_off = g.y_off = g.obj_w = g.obj_h = 0; }
    int rc = hg_warp_forward_piecewise_state(h->ctx, m, (int)(nm / 6), &def, msx, msy, mxx, mxy, g, px ? (uint8_t *)out : none);
    if (rc != HG_OK) return throw_state(env, h->ctx, "hg_warp_forward_piecewise_state", rc);
    return r;
}

/* parity taps */
static napi_value fn_get_tri_map(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    bool fused = false;
    napi_get_value_bool(env, a[1], &fused);
    const size_t n = (h->obj_w > 0 && h->obj_h > 0) ? (size_t)h->obj_w * h->obj_h : 0;
    void *out; napi_value r = make_typed(env, napi_int16_array, n, 2, &out); if (!r) return NULL;
    if (n) HG_CALL(h->ctx, "hg_get_tri_map", fused ? hg_get_tri_map_fused(h->ctx, (int16_t *)out, n) : hg_get_tri_map(h->ctx, (int16_t *)out, n));
    return r;
}

/* fieldInverseGeometric(handle, kind, matrix, xOff, yOff, objW, objH, format) / fieldInversePiecewise(handle, format): the source field of
 * the inverse warp (hg_field_*): an Int32Array of objW * objH pixel indices (format 0) or a Float32Array of objW * objH (sx, sy) pairs (1). */
static napi_value make_field(napi_env env, int fmt, size_t px, void **out)
{
    if (fmt == HG_FIELD_INDEX) return make_typed(env, napi_int32_array, px, 4, out);
    if (fmt == HG_FIELD_COORDS) return make_typed(env, napi_float32_array, 2 * px, 4, out);
    return throw_str(env, "hgwarp: unknown field format");
}

static napi_value fn_field_inverse_geometric(napi_env env, napi_callback_info info)
{
    napi_value a[8];
    if (!get_args(env, info, 8, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind, fmt; size_t n; hg_geom g;
    if (!get_i32(env, a[1], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[2], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (!get_geom(env, a + 3, &g) || !get_i32(env, a[7], &fmt)) return NULL;
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    void *out; napi_value r = make_field(env, fmt, px, &out); if (!r) return NULL;
    if (px) HG_CALL(h->ctx, "hg_field_inverse_geometric", hg_field_inverse_geometric(h->ctx, kind, m, g, fmt, out));
    return r;
}

static napi_value fn_field_inverse_piecewise(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int fmt;
    if (!get_i32(env, a[1], &fmt)) return NULL;
    const size_t px = (h->obj_w > 0 && h->obj_h > 0) ? (size_t)h->obj_w * h->obj_h : 0;
    void *out; napi_value r = make_field(env, fmt, px, &out); if (!r) return NULL;
    if (px) HG_CALL(h->ctx, "hg_field_inverse_piecewise", hg_field_inverse_piecewise(h->ctx, fmt, out));
    return r;
}

/* fieldForwardGeometric(handle, kind, forwardMatrix, xOff, yOff, objW, objH) / fieldForwardPiecewise(handle, dstPoints, maxSrcX, maxSrcY, xOff,
 * yOff, objW, objH): the source field of the FORWARD warp (hg_field_forward_*): an Int32Array of objW * objH flat source pixel indices, -1
 * where the forward loop leaves a hole or its last writer reads outside the source. */
static napi_value fn_field_forward_geometric(napi_env env, napi_callback_info info)
{
    napi_value a[7];
    if (!get_args(env, info, 7, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind; size_t n; hg_geom g;
    if (!get_i32(env, a[1], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[2], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (!get_geom(env, a + 3, &g)) return NULL;
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    void *out; napi_value r = make_field(env, HG_FIELD_INDEX, px, &out); if (!r) return NULL;
    if (px) HG_CALL(h->ctx, "hg_field_forward_geometric", hg_field_forward_geometric(h->ctx, kind, m, g, out));
    return r;
}

static napi_value fn_field_forward_piecewise(napi_env env, napi_callback_info info)
{
    napi_value a[8];
    if (!get_args(env, info, 8, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t n; int mx, my; hg_geom g;
    float *dst = (float *)get_typed(env, a[1], napi_float32_array, &n, "dstPoints"); if (!dst) return NULL;
    if (!get_i32(env, a[2], &mx) || !get_i32(env, a[3], &my)) return NULL;
    if (!get_geom(env, a + 4, &g)) return NULL;
    if (h->n_pts == 0 || n < 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold one x,y pair per mesh point (piecewiseSetMesh first)");
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    void *out; napi_value r = make_field(env, HG_FIELD_INDEX, px, &out); if (!r) return NULL;
    if (px) HG_CALL(h->ctx, "hg_field_forward_piecewise", hg_field_forward_piecewise(h->ctx, dst, mx, my, g, out));
    return r;
}

/* remapInverseGeometric(<fieldInverseGeometric's arguments>, plane, channels, W, H) / remapInversePiecewise(handle, format, plane, channels, W, H) /
 * remapForwardGeometric(<fieldForwardGeometric's>, plane, channels, W, H) / remapForwardPiecewise(<fieldForwardPiecewise's>, plane, channels, W, H):
 * one plane of the W x H source (W * H * channels elements of any TypedArray class) through the field the field* twin would return, on the
 * device.  The field is computed into device scratch by the _device forms (forward: the _batch_device forms with one frame) and never comes
 * to the host: the plane goes up, hg_remap_index_device (format 0: pixels are opaque blocks of channels * BYTES_PER_ELEMENT = 1, 2, 4, 8 or 16
 * bytes) or hg_remap_bilinear_f32_device / _u8_device (format 1: Float32Array / Uint8Array / Uint8ClampedArray, 1..4 channels) runs, and the
 * result comes down as a TypedArray of the plane's class with objW * objH * channels elements. */
typedef struct { napi_typedarray_type type; void *data; size_t len, elem; int channels, W, H; void *d_field, *d_plane, *d_out, *out; size_t px; napi_value result;
                 int levels, max_aniso; void *d_pyr; size_t pyr_bytes; hg_geom geom;
                 int cubic; float cubic_b, cubic_c; } remap_job;      /* levels > 0: the trilinear remap, its pyramid behind the result; max_aniso > 0: the anisotropic one; cubic: the bicubic one */

static int remap_begin(napi_env env, handle_t *h, napi_value *a, int fmt, size_t px, int mip, remap_job *j)      /* mip: 0 none, 1 trilinear, 2 anisotropic (a[4] = maxAniso), 3 bicubic (a[4] = B, a[5] = C; no pyramid) */
{
    static const size_t elem_of[] = { 1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8 };       /* napi_int8_array .. napi_biguint64_array */
    bool is = false; napi_value ab; size_t off = 0;
    memset(j, 0, sizeof *j);
    if (napi_is_typedarray(env, a[0], &is) != napi_ok || !is || napi_get_typedarray_info(env, a[0], &j->type, &j->len, &j->data, &ab, &off) != napi_ok ||
        (size_t)j->type >= sizeof elem_of / sizeof elem_of[0]) { throw_str(env, "hgwarp: argument 'plane' must be a TypedArray"); return 0; }
    j->elem = elem_of[j->type];
    if (!get_i32(env, a[1], &j->channels) || !get_i32(env, a[2], &j->W) || !get_i32(env, a[3], &j->H)) return 0;
    if (fmt != HG_FIELD_INDEX && fmt != HG_FIELD_COORDS) { throw_str(env, "hgwarp: unknown field format"); return 0; }
    const size_t pb = (size_t)(j->channels > 0 ? j->channels : 0) * j->elem;
    if (fmt == HG_FIELD_INDEX ? !(pb == 1 || pb == 2 || pb == 4 || pb == 8 || pb == 16)
                              : !(j->channels >= 1 && j->channels <= 4 && (j->type == napi_float32_array || j->type == napi_uint8_array || j->type == napi_uint8_clamped_array))) {
        throw_str(env, "hgwarp: this plane class and channel count cannot be remapped in this format"); return 0;
    }
    if (j->W < 1 || j->H < 1 || j->len != (size_t)j->W * (size_t)j->H * (size_t)j->channels) { throw_str(env, "hgwarp: plane must hold W * H * channels elements"); return 0; }
    if (mip == 2) {
        if (!get_i32(env, a[4], &j->max_aniso)) return 0;
        if (j->max_aniso < 1 || j->max_aniso > 16) { throw_str(env, "hgwarp: maxAniso must lie in 1..16"); return 0; }
    }
    if (mip == 3) {
        double b, c;
        if (napi_get_value_double(env, a[4], &b) != napi_ok || napi_get_value_double(env, a[5], &c) != napi_ok) { throw_str(env, "hgwarp: expected a number"); return 0; }
        if (!(b >= 0.0 && b <= 1.0) || !(c >= 0.0 && c <= 1.0)) { throw_str(env, "hgwarp: the cubic's B and C must lie in [0, 1]"); return 0; }
        if (fmt != HG_FIELD_COORDS) { throw_str(env, "hgwarp: a bicubic remap needs the coords format"); return 0; }
        j->cubic = 1; j->cubic_b = (float)b; j->cubic_c = (float)c;
        mip = 0;
    }
    j->px = px;
    j->result = make_typed(env, j->type, px * (size_t)j->channels, j->elem, &j->out);
    if (!j->result) return 0;
    if (!px) return 1;
    size_t fb = (px * (fmt == HG_FIELD_INDEX ? 4 : 8) + 255) & ~(size_t)255, pl = (j->len * j->elem + 255) & ~(size_t)255, ob = px * pb;
    if (mip) {                                                 /* the full pyramid, all hg_pyramid_levels(W, H) levels */
        size_t offs[32];
        j->levels = hg_pyramid_levels(j->W, j->H);
        if (fmt != HG_FIELD_COORDS || hg_pyramid_layout(j->W, j->H, j->type == napi_float32_array ? HG_ELEM_F32 : HG_ELEM_U8, j->channels, j->levels, offs, &j->pyr_bytes) != HG_OK) {
            throw_str(env, mip == 2 ? "hgwarp: an anisotropic remap needs the coords format" : "hgwarp: a trilinear remap needs the coords format"); return 0;
        }
        ob = (ob + 255) & ~(size_t)255;
    }
    if (fb + pl + ob + j->pyr_bytes > h->d_remap_cap) {
        if (h->d_remap) { hg_device_free(h->ctx, h->d_remap); h->d_remap = NULL; h->d_remap_cap = 0; }
        int rc = hg_device_alloc(h->ctx, fb + pl + ob + j->pyr_bytes, &h->d_remap);
        if (rc != HG_OK) { throw_hg(env, h->ctx, "hg_device_alloc", rc); return 0; }
        h->d_remap_cap = fb + pl + ob + j->pyr_bytes;
    }
    j->d_field = h->d_remap; j->d_plane = (uint8_t *)h->d_remap + fb; j->d_out = (uint8_t *)h->d_remap + fb + pl; j->d_pyr = (uint8_t *)j->d_out + ob;
    int rc = hg_copy_to_device(h->ctx, j->d_plane, j->data, j->len * j->elem);
    if (rc != HG_OK) { throw_hg(env, h->ctx, "hg_copy_to_device", rc); return 0; }
    return 1;
}

static napi_value remap_finish(napi_env env, handle_t *h, int fmt, const remap_job *j)
{
    if (!j->px) return j->result;
    const size_t pb = (size_t)j->channels * j->elem;
    if (j->levels > 0) {
        const int elem = j->type == napi_float32_array ? HG_ELEM_F32 : HG_ELEM_U8;
        const size_t zero = 0;
        HG_CALL(h->ctx, "hg_pyramid_build_device", hg_pyramid_build_device(h->ctx, j->d_plane, j->W, j->H, 1, 0, elem, j->channels, j->levels, j->d_pyr, j->pyr_bytes));
        if (j->max_aniso > 0)
            HG_CALL(h->ctx, "hg_remap_aniso_frames_device", hg_remap_aniso_frames_device(h->ctx, &j->geom, 1, j->d_field, &zero, j->d_plane, j->W, j->H, 1, 0, elem,
                                                                                         j->channels, j->d_out, &zero, j->d_pyr, j->pyr_bytes, j->levels, j->max_aniso));
        else
        HG_CALL(h->ctx, "hg_remap_trilinear_frames_device", hg_remap_trilinear_frames_device(h->ctx, &j->geom, 1, j->d_field, &zero, j->d_plane, j->W, j->H, 1, 0, elem,
                                                                                             j->channels, j->d_out, &zero, j->d_pyr, j->pyr_bytes, j->levels));
    } else if (j->cubic) {
        const size_t zero = 0;
        HG_CALL(h->ctx, "hg_remap_bicubic_frames_device", hg_remap_bicubic_frames_device(h->ctx, &j->geom, 1, j->d_field, &zero, j->d_plane, j->W, j->H, 1, 0,
                                                                                         j->type == napi_float32_array ? HG_ELEM_F32 : HG_ELEM_U8, j->channels, j->d_out, &zero,
                                                                                         j->cubic_b, j->cubic_c));
    } else if (fmt == HG_FIELD_INDEX)
        HG_CALL(h->ctx, "hg_remap_index_device", hg_remap_index_device(h->ctx, j->d_field, j->px, j->d_plane, (size_t)j->W * (size_t)j->H, (int)pb, j->d_out));
    else if (j->type == napi_float32_array)
        HG_CALL(h->ctx, "hg_remap_bilinear_f32_device", hg_remap_bilinear_f32_device(h->ctx, j->d_field, j->px, (const float *)j->d_plane, j->W, j->H, j->channels, (float *)j->d_out));
    else
        HG_CALL(h->ctx, "hg_remap_bilinear_u8_device", hg_remap_bilinear_u8_device(h->ctx, j->d_field, j->px, (const uint8_t *)j->d_plane, j->W, j->H, j->channels, (uint8_t *)j->d_out));
    HG_CALL(h->ctx, "hg_copy_to_host", hg_copy_to_host(h->ctx, j->out, j->d_out, j->px * pb));
    return j->result;
}

static napi_value remap_inverse_geometric(napi_env env, napi_callback_info info, int mip)
{
    napi_value a[14];
    if (!get_args(env, info, mip == 3 ? 14 : mip == 2 ? 13 : 12, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind, fmt; size_t n; hg_geom g; remap_job j;
    if (!get_i32(env, a[1], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[2], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (!get_geom(env, a + 3, &g) || !get_i32(env, a[7], &fmt)) return NULL;
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0;
    if (!remap_begin(env, h, a + 8, fmt, px, mip, &j)) return NULL;
    j.geom = g;
    if (px) HG_CALL(h->ctx, "hg_field_inverse_geometric_device", hg_field_inverse_geometric_device(h->ctx, kind, m, g, fmt, j.d_field));
    return remap_finish(env, h, fmt, &j);
}

static napi_value remap_inverse_piecewise(napi_env env, napi_callback_info info, int mip)
{
    napi_value a[8];
    if (!get_args(env, info, mip == 3 ? 8 : mip == 2 ? 7 : 6, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int fmt; remap_job j;
    if (!get_i32(env, a[1], &fmt)) return NULL;
    const size_t px = (h->obj_w > 0 && h->obj_h > 0) ? (size_t)h->obj_w * h->obj_h : 0, zero = 0;
    if (!remap_begin(env, h, a + 2, fmt, px, mip, &j)) return NULL;
    j.geom.x_off = 0; j.geom.y_off = 0; j.geom.obj_w = h->obj_w; j.geom.obj_h = h->obj_h;
    if (px) HG_CALL(h->ctx, "hg_field_inverse_piecewise_frames_device", hg_field_inverse_piecewise_frames_device(h->ctx, fmt, &zero, j.d_field));
    return remap_finish(env, h, fmt, &j);
}

/* remapTrilinearInverseGeometric / remapTrilinearInversePiecewise: the arguments of remapInverseGeometric / remapInversePiecewise (format 1),
 * the plane through hg_pyramid_build_device (all levels, in device scratch) and hg_remap_trilinear_frames_device with the window as one frame.
 * remapAnisoInverseGeometric / remapAnisoInversePiecewise: the same arguments followed by maxAniso (1..16), through hg_remap_aniso_frames_device.
 * remapBicubicInverseGeometric / remapBicubicInversePiecewise: the remap* arguments (format 1) followed by the cubic's B and C (numbers in
 * [0, 1]), through hg_remap_bicubic_frames_device with the window as one frame; no pyramid. */
static napi_value fn_remap_inverse_geometric(napi_env env, napi_callback_info info) { return remap_inverse_geometric(env, info, 0); }
static napi_value fn_remap_inverse_piecewise(napi_env env, napi_callback_info info) { return remap_inverse_piecewise(env, info, 0); }
static napi_value fn_remap_trilinear_inverse_geometric(napi_env env, napi_callback_info info) { return remap_inverse_geometric(env, info, 1); }
static napi_value fn_remap_trilinear_inverse_piecewise(napi_env env, napi_callback_info info) { return remap_inverse_piecewise(env, info, 1); }
static napi_value fn_remap_aniso_inverse_geometric(napi_env env, napi_callback_info info) { return remap_inverse_geometric(env, info, 2); }
static napi_value fn_remap_aniso_inverse_piecewise(napi_env env, napi_callback_info info) { return remap_inverse_piecewise(env, info, 2); }
static napi_value fn_remap_bicubic_inverse_geometric(napi_env env, napi_callback_info info) { return remap_inverse_geometric(env, info, 3); }
static napi_value fn_remap_bicubic_inverse_piecewise(napi_env env, napi_callback_info info) { return remap_inverse_piecewise(env, info, 3); }

static napi_value fn_remap_forward_geometric(napi_env env, napi_callback_info info)
{
    napi_value a[11];
    if (!get_args(env, info, 11, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind; size_t n; hg_geom g; remap_job j;
    if (!get_i32(env, a[1], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[2], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (!get_geom(env, a + 3, &g)) return NULL;
    double m8[8] = { 0 };
    for (int k = 0; k < (kind == HG_AFFINE ? 6 : 8); k++) m8[k] = m[k];
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0, zero = 0;
    if (!remap_begin(env, h, a + 7, HG_FIELD_INDEX, px, 0, &j)) return NULL;
    if (px) HG_CALL(h->ctx, "hg_field_forward_geometric_batch_device", hg_field_forward_geometric_batch_device(h->ctx, kind, m8, &g, &zero, 1, j.d_field));
    return remap_finish(env, h, HG_FIELD_INDEX, &j);
}

static napi_value fn_remap_forward_piecewise(napi_env env, napi_callback_info info)
{
    napi_value a[12];
    if (!get_args(env, info, 12, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t n; int mx, my; hg_geom g; remap_job j;
    float *dst = (float *)get_typed(env, a[1], napi_float32_array, &n, "dstPoints"); if (!dst) return NULL;
    if (!get_i32(env, a[2], &mx) || !get_i32(env, a[3], &my)) return NULL;
    if (!get_geom(env, a + 4, &g)) return NULL;
    if (h->n_pts == 0 || n < 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold one x,y pair per mesh point (piecewiseSetMesh first)");
    const size_t px = (g.obj_w > 0 && g.obj_h > 0) ? (size_t)g.obj_w * g.obj_h : 0, zero = 0;
    if (!remap_begin(env, h, a + 8, HG_FIELD_INDEX, px, 0, &j)) return NULL;
    if (px) HG_CALL(h->ctx, "hg_field_forward_piecewise_batch_device", hg_field_forward_piecewise_batch_device(h->ctx, dst, mx, my, &g, &zero, 1, j.d_field));
    return remap_finish(env, h, HG_FIELD_INDEX, &j);
}

/* pointsInverseGeometric(<fieldInverseGeometric's arguments>, points) / pointsInversePiecewise(handle, format, points) /
 * pointsForwardGeometric(<fieldForwardGeometric's>, points) / pointsForwardPiecewise(<fieldForwardPiecewise's>, points): a list of x,y pairs
 * (Float32Array) through the geometry the field* twin would export, one frame (hg_points_*): Inverse = to source (window positions ->
 * source coordinates), Forward = to output (source positions -> window-relative output positions).  The format argument of the inverse
 * twins is accepted and ignored.  The points go up into device scratch, the _device form runs, the results come down as a Float32Array of
 * the same length, NaN (0x7fc00000) in both words of an unmapped point.
 * Unlike its twin fieldInverseGeometric, which has a single-frame C entry point, pointsInverseGeometric STAGES the frame as a one-frame
 * geometric set (hg_geometric_set_frames; the C ABI has no single-frame points form): a geometric frame set the context held before is
 * replaced.  Every batch function of this addon stages its own set inside the call, so nothing here depends on one surviving.
 * pointsForwardPiecewise stages its frame as the piecewise set, as fieldForwardPiecewise does. */
typedef struct { float *pts; size_t n; void *d_pts, *d_out, *out; napi_value result; } points_job;

static int points_begin(napi_env env, handle_t *h, napi_value arg, points_job *j)
{
    size_t len = 0;
    memset(j, 0, sizeof *j);
    j->pts = (float *)get_typed(env, arg, napi_float32_array, &len, "points");
    if (!j->pts) return 0;
    if (len & 1) { throw_str(env, "hgwarp: points must hold x,y pairs"); return 0; }
    if (len / 2 > ((size_t)1 << 24)) { throw_str(env, "hgwarp: more than 2^24 points"); return 0; }
    j->n = len / 2;
    j->result = make_typed(env, napi_float32_array, len, 4, &j->out);
    if (!j->result) return 0;
    if (!j->n) return 1;
    const size_t pb = (len * 4 + 255) & ~(size_t)255;
    if (2 * pb > h->d_remap_cap) {
        if (h->d_remap) { hg_device_free(h->ctx, h->d_remap); h->d_remap = NULL; h->d_remap_cap = 0; }
        int rc = hg_device_alloc(h->ctx, 2 * pb, &h->d_remap);
        if (rc != HG_OK) { throw_hg(env, h->ctx, "hg_device_alloc", rc); return 0; }
        h->d_remap_cap = 2 * pb;
    }
    j->d_pts = h->d_remap; j->d_out = (uint8_t *)h->d_remap + pb;
    int rc = hg_copy_to_device(h->ctx, j->d_pts, j->pts, len * 4);
    if (rc != HG_OK) { throw_hg(env, h->ctx, "hg_copy_to_device", rc); return 0; }
    return 1;
}

static napi_value points_finish(napi_env env, handle_t *h, const points_job *j)
{
    if (j->n) HG_CALL(h->ctx, "hg_copy_to_host", hg_copy_to_host(h->ctx, j->out, j->d_out, j->n * 8));
    return j->result;
}

static napi_value fn_points_inverse_geometric(napi_env env, napi_callback_info info)
{
    napi_value a[9];
    if (!get_args(env, info, 9, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind; size_t n; hg_geom g; points_job j;
    if (!get_i32(env, a[1], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[2], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (!get_geom(env, a + 3, &g)) return NULL;
    double m8[8] = { 0 };
    for (int k = 0; k < (kind == HG_AFFINE ? 6 : 8); k++) m8[k] = m[k];
    const size_t zero = 0;
    if (!points_begin(env, h, a[8], &j)) return NULL;
    if (j.n) {
        HG_CALL(h->ctx, "hg_geometric_set_frames", hg_geometric_set_frames(h->ctx, kind, m8, &g, &zero, 1));
        HG_CALL(h->ctx, "hg_points_to_source_geometric_frames_device", hg_points_to_source_geometric_frames_device(h->ctx, j.d_pts, (int)j.n, 1, j.d_out));
    }
    return points_finish(env, h, &j);
}

static napi_value fn_points_inverse_piecewise(napi_env env, napi_callback_info info)
{
    napi_value a[3];
    if (!get_args(env, info, 3, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    points_job j;
    if (!points_begin(env, h, a[2], &j)) return NULL;
    if (j.n) HG_CALL(h->ctx, "hg_points_to_source_piecewise_frames_device", hg_points_to_source_piecewise_frames_device(h->ctx, j.d_pts, (int)j.n, 1, j.d_out));
    return points_finish(env, h, &j);
}

static napi_value fn_points_forward_geometric(napi_env env, napi_callback_info info)
{
    napi_value a[8];
    if (!get_args(env, info, 8, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind; size_t n; hg_geom g; points_job j;
    if (!get_i32(env, a[1], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[2], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n < (size_t)(kind == HG_AFFINE ? 6 : 8)) return throw_str(env, "hgwarp: matrix too short");
    if (!get_geom(env, a + 3, &g)) return NULL;
    double m8[8] = { 0 };
    for (int k = 0; k < (kind == HG_AFFINE ? 6 : 8); k++) m8[k] = m[k];
    if (!points_begin(env, h, a[7], &j)) return NULL;
    if (j.n) HG_CALL(h->ctx, "hg_points_to_output_geometric_batch_device", hg_points_to_output_geometric_batch_device(h->ctx, kind, m8, &g, 1, j.d_pts, (int)j.n, 1, j.d_out));
    return points_finish(env, h, &j);
}

static napi_value fn_points_forward_piecewise(napi_env env, napi_callback_info info)
{
    napi_value a[9];
    if (!get_args(env, info, 9, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t n; int mx, my; hg_geom g; points_job j;
    float *dst = (float *)get_typed(env, a[1], napi_float32_array, &n, "dstPoints"); if (!dst) return NULL;
    if (!get_i32(env, a[2], &mx) || !get_i32(env, a[3], &my)) return NULL;
    if (!get_geom(env, a + 4, &g)) return NULL;
    if (h->n_pts == 0 || n < 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold one x,y pair per mesh point (piecewiseSetMesh first)");
    if (!points_begin(env, h, a[8], &j)) return NULL;
    if (j.n) HG_CALL(h->ctx, "hg_points_to_output_piecewise_batch_device", hg_points_to_output_piecewise_batch_device(h->ctx, dst, mx, my, &g, 1, j.d_pts, (int)j.n, 1, j.d_out));
    return points_finish(env, h, &j);
}

/* fitMatches(handle, kind, matches, nPoints, counts, threshold, nHyp, seed, samples | null, refit): one transform per frame from point matches
 * (hg_fit_matches_frames_device).  matches: Float32Array of F x nPoints x 4 (x, y, u, v), F = counts.length; counts: Int32Array; samples: Int32Array
 * of F x nHyp x 4 or null (the device draws them from `seed`).  Everything goes up into device memory of the call's own, the entry runs, and
 * { matrices, minimal: Float64Array(8 F), counts, best: Int32Array(F), mask: Uint8Array(F x nPoints) } come down.  Needs no image. */
static napi_value fn_fit_matches(napi_env env, napi_callback_info info)
{
    napi_value a[10];
    if (!get_args(env, info, 10, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind, n_points, n_hyp, refit; size_t n_m = 0, n_c = 0, n_s = 0; double thr, seed_d;
    if (!get_i32(env, a[1], &kind)) return NULL;
    float *m = (float *)get_typed(env, a[2], napi_float32_array, &n_m, "matches"); if (!m) return NULL;
    if (!get_i32(env, a[3], &n_points)) return NULL;
    int32_t *counts = (int32_t *)get_typed(env, a[4], napi_int32_array, &n_c, "counts"); if (!counts) return NULL;
    if (napi_get_value_double(env, a[5], &thr) != napi_ok) return throw_str(env, "hgwarp: threshold must be a number");
    if (!get_i32(env, a[6], &n_hyp)) return NULL;
    if (napi_get_value_double(env, a[7], &seed_d) != napi_ok || !(seed_d >= 0 && seed_d <= 4294967295.0)) return throw_str(env, "hgwarp: seed must be a uint32");
    napi_valuetype vt;
    NAPI_OK(napi_typeof(env, a[8], &vt));
    int32_t *samples = NULL;
    if (vt != napi_null && vt != napi_undefined) { samples = (int32_t *)get_typed(env, a[8], napi_int32_array, &n_s, "samples"); if (!samples) return NULL; }
    if (!get_i32(env, a[9], &refit)) return NULL;
    if (n_points < 0 || n_points > 65536 || n_hyp < 0 || n_hyp > 65536 || n_c > 4096) return throw_str(env, "hgwarp: fitMatches: nPoints, nHyp or the number of frames is out of range");
    const size_t F = n_c, N = (size_t)n_points, H = (size_t)n_hyp;
    if (n_m != F * N * 4) return throw_str(env, "hgwarp: matches must hold counts.length x nPoints x 4 floats");
    if (samples && n_s != F * H * 4) return throw_str(env, "hgwarp: samples must hold counts.length x nHyp x 4 indices");
    void *p_mats, *p_min, *p_cnt, *p_best, *p_mask;
    napi_value out, v_mats, v_min, v_cnt, v_best, v_mask;
    if (!(v_mats = make_typed(env, napi_float64_array, F * 8, 8, &p_mats)) || !(v_min = make_typed(env, napi_float64_array, F * 8, 8, &p_min)) ||
        !(v_cnt = make_typed(env, napi_int32_array, F, 4, &p_cnt)) || !(v_best = make_typed(env, napi_int32_array, F, 4, &p_best)) ||
        !(v_mask = make_typed(env, napi_uint8_array, F * N, 1, &p_mask))) return NULL;
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "matrices", v_mats)); NAPI_OK(napi_set_named_property(env, out, "minimal", v_min));
    NAPI_OK(napi_set_named_property(env, out, "counts", v_cnt)); NAPI_OK(napi_set_named_property(env, out, "best", v_best));
    NAPI_OK(napi_set_named_property(env, out, "mask", v_mask));
    if (!F) return out;
#define FIT_PAD(b) (((size_t)(b) + 255) & ~(size_t)255)
    const size_t o_m = 0, o_s = o_m + FIT_PAD(F * N * 16), o_mats = o_s + FIT_PAD(samples ? F * H * 16 : 0), o_min = o_mats + FIT_PAD(F * 64),
                 o_cnt = o_min + FIT_PAD(F * 64), o_best = o_cnt + FIT_PAD(F * 4), o_mask = o_best + FIT_PAD(F * 4), total = o_mask + FIT_PAD(F * N);
#undef FIT_PAD
    void *d = NULL;
    HG_CALL(h->ctx, "hg_device_alloc", hg_device_alloc(h->ctx, total, &d));
    uint8_t *b = (uint8_t *)d;
    int rc = HG_OK;
    const char *what = "hg_copy_to_device";
    if (F * N) rc = hg_copy_to_device(h->ctx, b + o_m, m, F * N * 16);
    if (rc == HG_OK && samples && F * H) rc = hg_copy_to_device(h->ctx, b + o_s, samples, F * H * 16);
    if (rc == HG_OK) {
        what = "hg_fit_matches_frames_device";
        rc = hg_fit_matches_frames_device(h->ctx, kind, F * N ? b + o_m : NULL, n_points, counts, (int)F, thr, n_hyp, (uint32_t)seed_d,
                                          samples ? (const int32_t *)(b + o_s) : NULL, refit, (double *)(b + o_mats), (double *)(b + o_min),
                                          (int32_t *)(b + o_cnt), (int32_t *)(b + o_best), (uint8_t *)(b + o_mask));
    }
    if (rc == HG_OK) { what = "hg_copy_to_host"; rc = hg_copy_to_host(h->ctx, p_mats, b + o_mats, F * 64); }
    if (rc == HG_OK) rc = hg_copy_to_host(h->ctx, p_min, b + o_min, F * 64);
    if (rc == HG_OK) rc = hg_copy_to_host(h->ctx, p_cnt, b + o_cnt, F * 4);
    if (rc == HG_OK) rc = hg_copy_to_host(h->ctx, p_best, b + o_best, F * 4);
    if (rc == HG_OK && F * N) rc = hg_copy_to_host(h->ctx, p_mask, b + o_mask, F * N);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); hg_device_free(h->ctx, d); return e; }
    HG_CALL(h->ctx, "hg_device_free", hg_device_free(h->ctx, d));
    return out;
}

/* bundleAdjust(handle, kind, W, H, fixed, pairs, matches, nPoints, counts, mask | null, nIter, eps, lambda0, huber, matrices): the frame -> canvas
 * matrices of a frame set adjusted over all pairs (hg_bundle_adjust_frames_device).  fixed: Uint8Array(F); pairs: Int32Array(2 P); matches:
 * Float32Array of P x nPoints x 4 (x, y, u, v); counts: Int32Array(P); mask: Uint8Array(P x nPoints) or null; matrices: Float64Array(8 F).
 * Everything goes up into device memory of the call's own, beside the scratch of hg_bundle_layout, the entry runs, and { matrices:
 * Float64Array(8 F), info: Uint8Array (the bytes of d_info: the call's record, one int32 per frame padded to 8 bytes, 24 bytes per pair) }
 * come down.  Needs no image. */
static napi_value fn_bundle_adjust(napi_env env, napi_callback_info info)
{
    napi_value a[15];
    if (!get_args(env, info, 15, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind, W, H, n_points, n_iter; size_t n_fx = 0, n_pr = 0, n_m = 0, n_c = 0, n_k = 0, n_mat = 0; double eps, lambda0, huber;
    if (!get_i32(env, a[1], &kind) || !get_i32(env, a[2], &W) || !get_i32(env, a[3], &H)) return NULL;
    uint8_t *fixed = (uint8_t *)get_typed(env, a[4], napi_uint8_array, &n_fx, "fixed"); if (!fixed) return NULL;
    int32_t *pairs = (int32_t *)get_typed(env, a[5], napi_int32_array, &n_pr, "pairs"); if (!pairs) return NULL;
    float *m = (float *)get_typed(env, a[6], napi_float32_array, &n_m, "matches"); if (!m) return NULL;
    if (!get_i32(env, a[7], &n_points)) return NULL;
    int32_t *counts = (int32_t *)get_typed(env, a[8], napi_int32_array, &n_c, "counts"); if (!counts) return NULL;
    napi_valuetype vt;
    NAPI_OK(napi_typeof(env, a[9], &vt));
    uint8_t *mask = NULL;
    if (vt != napi_null && vt != napi_undefined) { mask = (uint8_t *)get_typed(env, a[9], napi_uint8_array, &n_k, "mask"); if (!mask) return NULL; }
    if (!get_i32(env, a[10], &n_iter)) return NULL;
    if (napi_get_value_double(env, a[11], &eps) != napi_ok || napi_get_value_double(env, a[12], &lambda0) != napi_ok || napi_get_value_double(env, a[13], &huber) != napi_ok)
        return throw_str(env, "hgwarp: eps, lambda and huber must be numbers");
    double *mats = (double *)get_typed(env, a[14], napi_float64_array, &n_mat, "matrices"); if (!mats) return NULL;
    const size_t F = n_fx, P = n_c, N = (size_t)(n_points > 0 ? n_points : 0);
    if (n_points < 0 || n_points > 65536 || F > HG_BUNDLE_MAX_FRAMES || P > HG_BUNDLE_MAX_PAIRS) return throw_str(env, "hgwarp: bundleAdjust: nPoints, the number of frames or the number of pairs is out of range");
    if (n_mat != F * 8) return throw_str(env, "hgwarp: matrices must hold fixed.length x 8 numbers");
    if (n_pr != P * 2) return throw_str(env, "hgwarp: pairs must hold counts.length x 2 indices");
    if (n_m != P * N * 4) return throw_str(env, "hgwarp: matches must hold counts.length x nPoints x 4 floats");
    if (mask && n_k != P * N) return throw_str(env, "hgwarp: mask must hold counts.length x nPoints bytes");
    const size_t info_bytes = 48 + ((4 * F + 7) & ~(size_t)7) + 24 * P;
    void *p_mats, *p_info;
    napi_value out, v_mats, v_info;
    if (!(v_mats = make_typed(env, napi_float64_array, F * 8, 8, &p_mats)) || !(v_info = make_typed(env, napi_uint8_array, F ? info_bytes : 0, 1, &p_info))) return NULL;
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "matrices", v_mats)); NAPI_OK(napi_set_named_property(env, out, "info", v_info));
    size_t scratch = 0;
    HG_CALL(h->ctx, "hg_bundle_layout", hg_bundle_layout(kind, (int)F, (int)P, n_points, &scratch));
    if (!F) {
        HG_CALL(h->ctx, "hg_bundle_adjust_frames_device", hg_bundle_adjust_frames_device(h->ctx, kind, W, H, 0, fixed, pairs, (int)P, NULL, n_points, counts, NULL, n_iter, eps, lambda0,
                                                                                         huber, NULL, NULL, NULL, NULL, NULL, 0));
        return out;
    }
#define BUNDLE_PAD(b) (((size_t)(b) + 255) & ~(size_t)255)
    const size_t o_m = 0, o_k = o_m + BUNDLE_PAD(P * N * 16), o_in = o_k + BUNDLE_PAD(mask ? P * N : 0), o_out = o_in + BUNDLE_PAD(F * 64), o_info = o_out + BUNDLE_PAD(F * 64),
                 o_s = o_info + BUNDLE_PAD(info_bytes), total = o_s + BUNDLE_PAD(scratch);
#undef BUNDLE_PAD
    void *d = NULL;
    HG_CALL(h->ctx, "hg_device_alloc", hg_device_alloc(h->ctx, total, &d));
    uint8_t *b = (uint8_t *)d;
    int rc = HG_OK;
    const char *what = "hg_copy_to_device";
    if (P * N) rc = hg_copy_to_device(h->ctx, b + o_m, m, P * N * 16);
    if (rc == HG_OK && mask && P * N) rc = hg_copy_to_device(h->ctx, b + o_k, mask, P * N);
    if (rc == HG_OK) rc = hg_copy_to_device(h->ctx, b + o_in, mats, F * 64);
    if (rc == HG_OK) {
        what = "hg_bundle_adjust_frames_device";
        rc = hg_bundle_adjust_frames_device(h->ctx, kind, W, H, (int)F, fixed, pairs, (int)P, P * N ? b + o_m : NULL, n_points, counts, mask && P * N ? b + o_k : NULL, n_iter, eps,
                                            lambda0, huber, (const double *)(b + o_in), (double *)(b + o_out), b + o_info, NULL, b + o_s, scratch);
    }
    if (rc == HG_OK) { what = "hg_copy_to_host"; rc = hg_copy_to_host(h->ctx, p_mats, b + o_out, F * 64); }
    if (rc == HG_OK) rc = hg_copy_to_host(h->ctx, p_info, b + o_info, info_bytes);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); hg_device_free(h->ctx, d); return e; }
    HG_CALL(h->ctx, "hg_device_free", hg_device_free(h->ctx, d));
    return out;
}

/* bundleChain(kind, nFrames, pairs: Int32Array(2 P), pairMatrices: Float64Array(8 P), anchor) -> Float64Array(8 nFrames): hg_bundle_chain_from_pairs.
 * bundleInvert(kind, matrix: Float64Array(8)) -> Float64Array(8): hg_bundle_invert_matrix.  Host only: no handle. */
static napi_value fn_bundle_chain(napi_env env, napi_callback_info info)
{
    napi_value a[5];
    if (!get_args(env, info, 5, a)) return NULL;
    int kind, n_frames, anchor; size_t n_pr = 0, n_pm = 0;
    if (!get_i32(env, a[0], &kind) || !get_i32(env, a[1], &n_frames)) return NULL;
    int32_t *pairs = (int32_t *)get_typed(env, a[2], napi_int32_array, &n_pr, "pairs"); if (!pairs) return NULL;
    double *pm = (double *)get_typed(env, a[3], napi_float64_array, &n_pm, "pairMatrices"); if (!pm) return NULL;
    if (!get_i32(env, a[4], &anchor)) return NULL;
    if (n_frames < 0 || n_frames > HG_BUNDLE_MAX_FRAMES || n_pr % 2 != 0 || n_pr / 2 > HG_BUNDLE_MAX_PAIRS) return throw_str(env, "hgwarp: bundleChain: the number of frames or of pairs is out of range");
    if (n_pm != (n_pr / 2) * 8) return throw_str(env, "hgwarp: pairMatrices must hold 8 numbers per pair");
    void *p; napi_value out;
    if (!(out = make_typed(env, napi_float64_array, (size_t)n_frames * 8, 8, &p))) return NULL;
    HG_CALL(NULL, "hg_bundle_chain_from_pairs", hg_bundle_chain_from_pairs(kind, n_frames, pairs, (int)(n_pr / 2), pm, anchor, (double *)p));
    return out;
}

static napi_value fn_bundle_invert(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    int kind; size_t n = 0;
    if (!get_i32(env, a[0], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[1], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n != 8) return throw_str(env, "hgwarp: bundleInvert: a matrix is 8 numbers");
    void *p; napi_value out;
    if (!(out = make_typed(env, napi_float64_array, 8, 8, &p))) return NULL;
    HG_CALL(NULL, "hg_bundle_invert_matrix", hg_bundle_invert_matrix(kind, m, (double *)p));
    return out;
}

/* The alignment of the drop-in class (refineAlignment): the planes and their pyramids stay in device memory of a JOB between the calls of
 * a coarse-to-fine walk; only the matrices travel.
 *   alignBegin(handle, from, Wf, Hf, nFrames, to, Wt, Ht, nToSets, channels, levels) -> job: from / to are Uint8Arrays of nFrames resp.
 *     nToSets planes of W x H x channels; they go up, and with levels > 1 hg_pyramid_build_device builds both pyramids.
 *   alignLevel(handle, job, kind, level, rect: Int32Array(4), step, photometric, nIter, eps, minValid, matrices: Float64Array(8 F)) ->
 *     { matrices, status, updates: Int32Array(F), nValid: Int32Array(2 F), rms, gains: Float64Array(2 F) }: hg_align_refine_frames_device on
 *     that level of both pyramids (matrices and rect in the level's pixels); nValid and rms hold (first, last), gains (gain, bias) per frame.
 *   alignScaleMatrix(kind, matrices: Float64Array(8 F), levelIn, levelOut) -> Float64Array(8 F): hg_align_scale_matrix row by row; a row with
 *     an entry that is not finite is copied.  Host only.
 *   alignEnd(handle, job): frees the job's device memory. */
typedef struct { void *d; int Wf, Hf, F, Wt, Ht, S, channels, levels; size_t o_from, o_to, o_fpyr, o_tpyr, o_mats, o_info, fpyr_bytes, tpyr_bytes; size_t foffs[32], toffs[32]; } align_job_t;

static void align_job_finalize(napi_env env, void *data, void *hint) { (void)env; (void)hint; free(data); }      /* (the device block is alignEnd's) */

static napi_value fn_align_begin(napi_env env, napi_callback_info info)
{
    napi_value a[11];
    if (!get_args(env, info, 11, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int Wf, Hf, F, Wt, Ht, S, ch, levels; size_t n_f = 0, n_t = 0;
    uint8_t *from = (uint8_t *)get_typed(env, a[1], napi_uint8_array, &n_f, "from"); if (!from) return NULL;
    if (!get_i32(env, a[2], &Wf) || !get_i32(env, a[3], &Hf) || !get_i32(env, a[4], &F)) return NULL;
    uint8_t *to = (uint8_t *)get_typed(env, a[5], napi_uint8_array, &n_t, "to"); if (!to) return NULL;
    if (!get_i32(env, a[6], &Wt) || !get_i32(env, a[7], &Ht) || !get_i32(env, a[8], &S) || !get_i32(env, a[9], &ch) || !get_i32(env, a[10], &levels)) return NULL;
    if (Wf < 1 || Hf < 1 || Wt < 1 || Ht < 1 || Wf > 32768 || Hf > 32768 || Wt > 32768 || Ht > 32768 || F < 1 || F > 4096 || S < 1 || S > F || (ch != 1 && ch != 4))
        return throw_str(env, "hgwarp: alignBegin: sizes, frame counts or channels are out of range");
    const size_t fb = (size_t)Wf * Hf * ch, tb = (size_t)Wt * Ht * ch;
    if (n_f != fb * F || n_t != tb * S) return throw_str(env, "hgwarp: alignBegin: from / to must hold nFrames resp. nToSets planes of W x H x channels bytes");
    if (levels < 1 || levels > 31 || levels > hg_pyramid_levels(Wf, Hf) || levels > hg_pyramid_levels(Wt, Ht)) return throw_str(env, "hgwarp: alignBegin: levels must exist on both sides");
    align_job_t *j = (align_job_t *)calloc(1, sizeof *j);
    if (!j) return throw_str(env, "hgwarp: out of memory");
    j->Wf = Wf; j->Hf = Hf; j->F = F; j->Wt = Wt; j->Ht = Ht; j->S = S; j->channels = ch; j->levels = levels;
    if (hg_pyramid_layout(Wf, Hf, HG_ELEM_U8, ch, levels, j->foffs, &j->fpyr_bytes) != HG_OK || hg_pyramid_layout(Wt, Ht, HG_ELEM_U8, ch, levels, j->toffs, &j->tpyr_bytes) != HG_OK) {
        free(j); return throw_str(env, "hgwarp: alignBegin: hg_pyramid_layout failed");
    }
#define ALIGN_PAD(b) (((size_t)(b) + 255) & ~(size_t)255)
    j->o_from = 0; j->o_to = j->o_from + ALIGN_PAD(fb * F); j->o_fpyr = j->o_to + ALIGN_PAD(tb * S); j->o_tpyr = j->o_fpyr + ALIGN_PAD(j->fpyr_bytes * F);
    j->o_mats = j->o_tpyr + ALIGN_PAD(j->tpyr_bytes * S); j->o_info = j->o_mats + ALIGN_PAD((size_t)F * 64);
    const size_t total = j->o_info + ALIGN_PAD((size_t)F * 48);
#undef ALIGN_PAD
    int rc = hg_device_alloc(h->ctx, total, &j->d);
    const char *what = "hg_device_alloc";
    uint8_t *b = (uint8_t *)j->d;
    if (rc == HG_OK) { what = "hg_copy_to_device"; rc = hg_copy_to_device(h->ctx, b + j->o_from, from, fb * F); }
    if (rc == HG_OK) rc = hg_copy_to_device(h->ctx, b + j->o_to, to, tb * S);
    if (rc == HG_OK && levels > 1) {
        what = "hg_pyramid_build_device";
        rc = hg_pyramid_build_device(h->ctx, b + j->o_from, Wf, Hf, F, fb, HG_ELEM_U8, ch, levels, b + j->o_fpyr, j->fpyr_bytes);
        if (rc == HG_OK) rc = hg_pyramid_build_device(h->ctx, b + j->o_to, Wt, Ht, S, tb, HG_ELEM_U8, ch, levels, b + j->o_tpyr, j->tpyr_bytes);
    }
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); if (j->d) hg_device_free(h->ctx, j->d); free(j); return e; }
    napi_value ext;
    if (napi_create_external(env, j, align_job_finalize, NULL, &ext) != napi_ok) { hg_device_free(h->ctx, j->d); free(j); return throw_str(env, "hgwarp: cannot wrap the alignment job"); }
    return ext;
}

static align_job_t *get_align_job(napi_env env, napi_value v)
{
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((align_job_t *)p)->d) { throw_str(env, "hgwarp: invalid or ended alignment job"); return NULL; }
    return (align_job_t *)p;
}

static napi_value fn_align_level(napi_env env, napi_callback_info info)
{
    napi_value a[11];
    if (!get_args(env, info, 11, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    align_job_t *j = get_align_job(env, a[1]); if (!j) return NULL;
    int kind, level, step, photo, n_iter, min_valid; double eps; size_t n_r = 0, n_m = 0;
    if (!get_i32(env, a[2], &kind) || !get_i32(env, a[3], &level)) return NULL;
    int32_t *rect = (int32_t *)get_typed(env, a[4], napi_int32_array, &n_r, "rect"); if (!rect) return NULL;
    if (!get_i32(env, a[5], &step) || !get_i32(env, a[6], &photo) || !get_i32(env, a[7], &n_iter)) return NULL;
    if (napi_get_value_double(env, a[8], &eps) != napi_ok) return throw_str(env, "hgwarp: eps must be a number");
    if (!get_i32(env, a[9], &min_valid)) return NULL;
    double *m = (double *)get_typed(env, a[10], napi_float64_array, &n_m, "matrices"); if (!m) return NULL;
    const size_t F = (size_t)j->F;
    if (n_r != 4 || n_m != F * 8 || level < 0 || level >= j->levels) return throw_str(env, "hgwarp: alignLevel: rect must hold 4 numbers, matrices 8 per frame, level must exist");
    int Wf = j->Wf, Hf = j->Hf, Wt = j->Wt, Ht = j->Ht;
    for (int k = 0; k < level; k++) { Wf = (Wf + 1) >> 1; Hf = (Hf + 1) >> 1; Wt = (Wt + 1) >> 1; Ht = (Ht + 1) >> 1; }
    void *p_m, *p_st, *p_up, *p_nv, *p_rms, *p_g;
    napi_value out, v_m, v_st, v_up, v_nv, v_rms, v_g;
    if (!(v_m = make_typed(env, napi_float64_array, F * 8, 8, &p_m)) || !(v_st = make_typed(env, napi_int32_array, F, 4, &p_st)) ||
        !(v_up = make_typed(env, napi_int32_array, F, 4, &p_up)) || !(v_nv = make_typed(env, napi_int32_array, F * 2, 4, &p_nv)) ||
        !(v_rms = make_typed(env, napi_float64_array, F * 2, 8, &p_rms)) || !(v_g = make_typed(env, napi_float64_array, F * 2, 8, &p_g))) return NULL;
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "matrices", v_m)); NAPI_OK(napi_set_named_property(env, out, "status", v_st));
    NAPI_OK(napi_set_named_property(env, out, "updates", v_up)); NAPI_OK(napi_set_named_property(env, out, "nValid", v_nv));
    NAPI_OK(napi_set_named_property(env, out, "rms", v_rms)); NAPI_OK(napi_set_named_property(env, out, "gains", v_g));
    uint8_t *b = (uint8_t *)j->d;
    const size_t px = (size_t)j->channels;
    const uint8_t *d_from = level == 0 ? b + j->o_from : b + j->o_fpyr + j->foffs[level], *d_to = level == 0 ? b + j->o_to : b + j->o_tpyr + j->toffs[level];
    const size_t fs = level == 0 ? (size_t)j->Wf * j->Hf * px : j->fpyr_bytes, ts = level == 0 ? (size_t)j->Wt * j->Ht * px : j->tpyr_bytes;
    HG_CALL(h->ctx, "hg_copy_to_device", hg_copy_to_device(h->ctx, b + j->o_mats, m, F * 64));
    HG_CALL(h->ctx, "hg_align_refine_frames_device", hg_align_refine_frames_device(h->ctx, kind, d_from, Wf, Hf, j->F, fs, d_to, Wt, Ht, j->S, ts, j->channels,
            rect[0], rect[1], rect[2], rect[3], step, photo, n_iter, eps, min_valid, (const double *)(b + j->o_mats), (double *)(b + j->o_mats), b + j->o_info, NULL));
    HG_CALL(h->ctx, "hg_copy_to_host", hg_copy_to_host(h->ctx, p_m, b + j->o_mats, F * 64));
    uint8_t *raw = (uint8_t *)malloc(F * 48);
    if (!raw) return throw_str(env, "hgwarp: out of memory");
    int rc = hg_copy_to_host(h->ctx, raw, b + j->o_info, F * 48);
    if (rc != HG_OK) { free(raw); return throw_hg(env, h->ctx, "hg_copy_to_host", rc); }
    for (size_t f = 0; f < F; f++) {
        const uint8_t *r = raw + f * 48;
        memcpy((int32_t *)p_st + f, r, 4); memcpy((int32_t *)p_up + f, r + 4, 4); memcpy((int32_t *)p_nv + 2 * f, r + 8, 8);
        memcpy((double *)p_rms + 2 * f, r + 16, 16); memcpy((double *)p_g + 2 * f, r + 32, 16);
    }
    free(raw);
    return out;
}

static napi_value fn_align_scale_matrix(napi_env env, napi_callback_info info)
{
    napi_value a[4];
    if (!get_args(env, info, 4, a)) return NULL;
    int kind, li, lo; size_t n = 0;
    if (!get_i32(env, a[0], &kind)) return NULL;
    double *m = (double *)get_typed(env, a[1], napi_float64_array, &n, "matrices"); if (!m) return NULL;
    if (!get_i32(env, a[2], &li) || !get_i32(env, a[3], &lo)) return NULL;
    if (n % 8 != 0) return throw_str(env, "hgwarp: alignScaleMatrix: matrices must hold 8 numbers per frame");
    void *p; napi_value out;
    if (!(out = make_typed(env, napi_float64_array, n, 8, &p))) return NULL;
    for (size_t f = 0; f < n / 8; f++) {
        const double *r = m + 8 * f; double *o = (double *)p + 8 * f;
        int fin = 1;
        for (int k = 0; k < 8; k++) fin = fin && r[k] - r[k] == 0.0;
        if (!fin) { memcpy(o, r, 64); continue; }
        HG_CALL(NULL, "hg_align_scale_matrix", hg_align_scale_matrix(kind, r, li, lo, o));
    }
    return out;
}

static napi_value fn_align_end(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    void *p = NULL;
    if (napi_get_value_external(env, a[1], &p) != napi_ok || !p) return throw_str(env, "hgwarp: invalid alignment job");
    align_job_t *j = (align_job_t *)p;
    if (j->d) { void *d = j->d; j->d = NULL; HG_CALL(h->ctx, "hg_device_free", hg_device_free(h->ctx, d)); }
    napi_value u;
    NAPI_OK(napi_get_undefined(env, &u));
    return u;
}

/* warpThinPlate(handle, from, nFromSets, to, nToSets, nPoints, windows, smoothing, step, output, images | null, W, H, nImages): thin-plate
 * splines through landmark pairs, one per window (hg_tps_solve_frames_device -> hg_field_tps_frames_device -> a remap), all on the device.
 * from / to: Float32Arrays of nFromSets resp. nToSets lists of nPoints x,y pairs (from = output space, to = source space); windows:
 * Int32Array of F x (x, y, width, height); output: 0 = picture by the index field (hg_remap_index_frames_device, 4-byte pixels), 1 = picture
 * by the coords field (hg_remap_bilinear_frames_device, u8 x 4), 2 = the index field, 3 = the coords field; images: Uint8Array of nImages
 * RGBA pictures of W x H (outputs 0 and 1; frame f reads picture f % nImages), else null.  Returns { data: Uint8Array, the frames packed at
 * the 256-byte grain, status: Int32Array(F) }.  Only the results come down. */
static napi_value fn_warp_thin_plate(napi_env env, napi_callback_info info)
{
    napi_value a[14];
    if (!get_args(env, info, 14, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int n_fs, n_ts, N, step, output, W, H, n_img; size_t n_f = 0, n_t = 0, n_w = 0, n_i = 0; double lambda;
    float *from = (float *)get_typed(env, a[1], napi_float32_array, &n_f, "from"); if (!from) return NULL;
    if (!get_i32(env, a[2], &n_fs)) return NULL;
    float *to = (float *)get_typed(env, a[3], napi_float32_array, &n_t, "to"); if (!to) return NULL;
    if (!get_i32(env, a[4], &n_ts) || !get_i32(env, a[5], &N)) return NULL;
    int32_t *win = (int32_t *)get_typed(env, a[6], napi_int32_array, &n_w, "windows"); if (!win && n_w) return NULL;
    if (napi_get_value_double(env, a[7], &lambda) != napi_ok) return throw_str(env, "hgwarp: smoothing must be a number");
    if (!get_i32(env, a[8], &step) || !get_i32(env, a[9], &output)) return NULL;
    napi_valuetype vt;
    NAPI_OK(napi_typeof(env, a[10], &vt));
    uint8_t *img = NULL;
    if (vt != napi_null && vt != napi_undefined) { img = (uint8_t *)get_typed(env, a[10], napi_uint8_array, &n_i, "images"); if (!img) return NULL; }
    if (!get_i32(env, a[11], &W) || !get_i32(env, a[12], &H) || !get_i32(env, a[13], &n_img)) return NULL;
    if (N < 3 || N > HG_TPS_MAX_POINTS || n_fs < 1 || n_ts < 1 || n_w % 4 != 0 || n_w / 4 > 4096 || output < 0 || output > 3 || W < 1 || H < 1)
        return throw_str(env, "hgwarp: warpThinPlate: nPoints, set counts, windows, output or the source size is out of range");
    const size_t F = n_w / 4;
    if (n_f != (size_t)n_fs * N * 2 || n_t != (size_t)n_ts * N * 2) return throw_str(env, "hgwarp: warpThinPlate: from / to must hold their sets of nPoints x,y pairs");
    const int picture = output < 2, fmt = (output == 0 || output == 2) ? HG_FIELD_INDEX : HG_FIELD_COORDS;
    const size_t plane = (size_t)W * (size_t)H * 4;
    if (picture && (!img || n_img < 1 || n_i != plane * (size_t)n_img)) return throw_str(env, "hgwarp: warpThinPlate: images must hold nImages RGBA pictures of W x H");
    hg_geom *g = (hg_geom *)calloc(F ? F : 1, sizeof *g);
    if (!g) return throw_str(env, "hgwarp: out of memory");
    for (size_t f = 0; f < F; f++) { g[f].x_off = win[4 * f]; g[f].y_off = win[4 * f + 1]; g[f].obj_w = win[4 * f + 2]; g[f].obj_h = win[4 * f + 3]; }
    size_t fld_total = 0, out_total = 0, rec_b = 0, scr_b = 0, node_b = 0;
    int rc = hg_tps_layout(N, (int)F, &rec_b, &scr_b);
    const char *what = "hg_tps_layout";
    if (rc == HG_OK) { what = "hg_tps_field_layout"; rc = hg_tps_field_layout(g, (int)F, step, &node_b); }
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); free(g); return e; }
    for (size_t f = 0; f < F; f++) {
        const size_t px = (g[f].obj_w > 0 && g[f].obj_h > 0) ? (size_t)g[f].obj_w * (size_t)g[f].obj_h : 0;
        fld_total += (px * (fmt == HG_FIELD_INDEX ? 4 : 8) + 255) & ~(size_t)255;
        out_total += (px * 4 + 255) & ~(size_t)255;
    }
    const size_t res_total = picture ? out_total : fld_total;
    void *p_data, *p_status;
    napi_value out, v_data, v_status;
    if (!(v_data = make_typed(env, napi_uint8_array, res_total, 1, &p_data)) || !(v_status = make_typed(env, napi_int32_array, F, 4, &p_status))) { free(g); return NULL; }
    if (napi_create_object(env, &out) != napi_ok || napi_set_named_property(env, out, "data", v_data) != napi_ok ||
        napi_set_named_property(env, out, "status", v_status) != napi_ok) { free(g); return throw_str(env, "hgwarp: N-API call failed"); }
    if (!F) { free(g); return out; }
#define TPS_PAD(b) (((size_t)(b) + 255) & ~(size_t)255)
    const size_t o_from = 0, o_to = o_from + TPS_PAD(n_f * 4), o_rec = o_to + TPS_PAD(n_t * 4), o_st = o_rec + TPS_PAD(rec_b * F), o_scr = o_st + TPS_PAD(F * 4),
                 o_node = o_scr + TPS_PAD(scr_b), o_fld = o_node + TPS_PAD(node_b), o_img = o_fld + TPS_PAD(fld_total), o_out = o_img + TPS_PAD(picture ? n_i : 0),
                 total = o_out + TPS_PAD(picture ? out_total : 0);
#undef TPS_PAD
    void *d = NULL;
    rc = hg_device_alloc(h->ctx, total, &d);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, "hg_device_alloc", rc); free(g); return e; }
    uint8_t *b = (uint8_t *)d;
    what = "hg_copy_to_device";
    rc = hg_copy_to_device(h->ctx, b + o_from, from, n_f * 4);
    if (rc == HG_OK) rc = hg_copy_to_device(h->ctx, b + o_to, to, n_t * 4);
    if (rc == HG_OK && picture) rc = hg_copy_to_device(h->ctx, b + o_img, img, n_i);
    if (rc == HG_OK) {
        what = "hg_tps_solve_frames_device";
        rc = hg_tps_solve_frames_device(h->ctx, b + o_from, n_fs, b + o_to, n_ts, N, (int)F, lambda, (double *)(b + o_rec), (int32_t *)(b + o_st), scr_b ? b + o_scr : NULL);
    }
    if (rc == HG_OK) {
        what = "hg_field_tps_frames_device";
        rc = hg_field_tps_frames_device(h->ctx, (const double *)(b + o_rec), N, g, (int)F, W, H, fmt, step, NULL, b + o_fld, node_b ? b + o_node : NULL);
    }
    if (rc == HG_OK && output == 0) {
        what = "hg_remap_index_frames_device";
        rc = hg_remap_index_frames_device(h->ctx, g, (int)F, b + o_fld, NULL, b + o_img, (size_t)W * (size_t)H, n_img, plane, 4, b + o_out, NULL);
    }
    if (rc == HG_OK && output == 1) {
        what = "hg_remap_bilinear_frames_device";
        rc = hg_remap_bilinear_frames_device(h->ctx, g, (int)F, b + o_fld, NULL, b + o_img, W, H, n_img, plane, HG_ELEM_U8, 4, b + o_out, NULL);
    }
    if (rc == HG_OK && res_total) { what = "hg_copy_to_host"; rc = hg_copy_to_host(h->ctx, p_data, picture ? b + o_out : b + o_fld, res_total); }
    if (rc == HG_OK) { what = "hg_copy_to_host"; rc = hg_copy_to_host(h->ctx, p_status, b + o_st, F * 4); }
    free(g);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); hg_device_free(h->ctx, d); return e; }
    HG_CALL(h->ctx, "hg_device_free", hg_device_free(h->ctx, d));
    return out;
}

/* The camera models ("camera models" in include/hgwarp.h).  Host only, no handle:
 *   cameraPackRecord(R: Float64Array(9), fx, fy, cx, cy, dist: Float64Array(5) | null, W, H) -> Float64Array(32): hg_camera_pack_record.
 *   cameraLimits(record: Float64Array(32), W, H, surface, scale, u0, v0) -> Int32Array(4) {x, y, width, height}: hg_camera_limits.
 *   cameraFocals(H: Float64Array(9)) -> Float64Array(4) {fFrom, fTo, okFrom, okTo}: hg_camera_focals_from_matrix.
 *   cameraRotation(H: Float64Array(9), kFrom: Float64Array(4), kTo: Float64Array(4)) -> Float64Array(9): hg_camera_rotation_from_matrix. */
static int get_f64(napi_env env, napi_value v, double *out)
{
    if (napi_get_value_double(env, v, out) != napi_ok) { throw_str(env, "hgwarp: expected a number"); return 0; }
    return 1;
}

static napi_value fn_camera_pack_record(napi_env env, napi_callback_info info)
{
    napi_value a[8];
    if (!get_args(env, info, 8, a)) return NULL;
    size_t n_r = 0, n_d = 0; double fx, fy, cx, cy; int W, H;
    double *R = (double *)get_typed(env, a[0], napi_float64_array, &n_r, "rotation"); if (!R) return NULL;
    if (!get_f64(env, a[1], &fx) || !get_f64(env, a[2], &fy) || !get_f64(env, a[3], &cx) || !get_f64(env, a[4], &cy)) return NULL;
    napi_valuetype vt;
    NAPI_OK(napi_typeof(env, a[5], &vt));
    double *dist = NULL;
    if (vt != napi_null && vt != napi_undefined) { dist = (double *)get_typed(env, a[5], napi_float64_array, &n_d, "distortion"); if (!dist) return NULL; }
    if (!get_i32(env, a[6], &W) || !get_i32(env, a[7], &H)) return NULL;
    if (n_r != 9 || (dist && n_d != 5)) return throw_str(env, "hgwarp: cameraPackRecord: a rotation is 9 numbers, a distortion 5");
    void *p; napi_value out;
    if (!(out = make_typed(env, napi_float64_array, HG_CAMERA_RECORD_DOUBLES, 8, &p))) return NULL;
    HG_CALL(NULL, "hg_camera_pack_record", hg_camera_pack_record(R, fx, fy, cx, cy, dist, W, H, (double *)p));
    return out;
}

static napi_value fn_camera_limits(napi_env env, napi_callback_info info)
{
    napi_value a[7];
    if (!get_args(env, info, 7, a)) return NULL;
    size_t n = 0; int W, H, surface; double scale, u0, v0;
    double *rec = (double *)get_typed(env, a[0], napi_float64_array, &n, "record"); if (!rec) return NULL;
    if (!get_i32(env, a[1], &W) || !get_i32(env, a[2], &H) || !get_i32(env, a[3], &surface)) return NULL;
    if (!get_f64(env, a[4], &scale) || !get_f64(env, a[5], &u0) || !get_f64(env, a[6], &v0)) return NULL;
    if (n != HG_CAMERA_RECORD_DOUBLES) return throw_str(env, "hgwarp: cameraLimits: a record is 32 numbers");
    void *p; napi_value out;
    if (!(out = make_typed(env, napi_int32_array, 4, 4, &p))) return NULL;
    HG_CALL(NULL, "hg_camera_limits", hg_camera_limits(rec, W, H, surface, scale, u0, v0, (int32_t *)p));
    return out;
}

static napi_value fn_camera_focals(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    size_t n = 0;
    double *m = (double *)get_typed(env, a[0], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    if (n != 9) return throw_str(env, "hgwarp: cameraFocals: a matrix is 9 numbers");
    void *p; napi_value out;
    if (!(out = make_typed(env, napi_float64_array, 4, 8, &p))) return NULL;
    double *o = (double *)p; int ok_from = 0, ok_to = 0;
    HG_CALL(NULL, "hg_camera_focals_from_matrix", hg_camera_focals_from_matrix(m, &o[0], &o[1], &ok_from, &ok_to));
    o[2] = ok_from; o[3] = ok_to;
    return out;
}

static napi_value fn_camera_rotation(napi_env env, napi_callback_info info)
{
    napi_value a[3];
    if (!get_args(env, info, 3, a)) return NULL;
    size_t n = 0, n_a = 0, n_b = 0;
    double *m = (double *)get_typed(env, a[0], napi_float64_array, &n, "matrix"); if (!m) return NULL;
    double *ka = (double *)get_typed(env, a[1], napi_float64_array, &n_a, "kFrom"); if (!ka) return NULL;
    double *kb = (double *)get_typed(env, a[2], napi_float64_array, &n_b, "kTo"); if (!kb) return NULL;
    if (n != 9 || n_a != 4 || n_b != 4) return throw_str(env, "hgwarp: cameraRotation: a matrix is 9 numbers, an intrinsic 4");
    void *p; napi_value out;
    if (!(out = make_typed(env, napi_float64_array, 9, 8, &p))) return NULL;
    HG_CALL(NULL, "hg_camera_rotation_from_matrix", hg_camera_rotation_from_matrix(m, ka, kb, (double *)p));
    return out;
}

/* warpCamera(handle, records, windows, surface, scale, u0, v0, output, images | null, W, H, nImages): the frames of a camera set on a plane,
 * a cylinder or a sphere (hg_field_camera_frames_device -> a remap), all on the device.  records: Float64Array of F x 32 doubles
 * (cameraPackRecord); windows: Int32Array of F x (x, y, width, height) of the canvas; output, images, W, H, nImages and the result's data
 * as for warpThinPlate.  Returns { data: Uint8Array, the frames packed at the 256-byte grain }.  Only the results come down. */
static napi_value fn_warp_camera(napi_env env, napi_callback_info info)
{
    napi_value a[12];
    if (!get_args(env, info, 12, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int surface, output, W, H, n_img; size_t n_r = 0, n_w = 0, n_i = 0; double scale, u0, v0;
    double *rec = (double *)get_typed(env, a[1], napi_float64_array, &n_r, "records"); if (!rec && n_r) return NULL;
    int32_t *win = (int32_t *)get_typed(env, a[2], napi_int32_array, &n_w, "windows"); if (!win && n_w) return NULL;
    if (!get_i32(env, a[3], &surface) || !get_f64(env, a[4], &scale) || !get_f64(env, a[5], &u0) || !get_f64(env, a[6], &v0) || !get_i32(env, a[7], &output)) return NULL;
    napi_valuetype vt;
    NAPI_OK(napi_typeof(env, a[8], &vt));
    uint8_t *img = NULL;
    if (vt != napi_null && vt != napi_undefined) { img = (uint8_t *)get_typed(env, a[8], napi_uint8_array, &n_i, "images"); if (!img) return NULL; }
    if (!get_i32(env, a[9], &W) || !get_i32(env, a[10], &H) || !get_i32(env, a[11], &n_img)) return NULL;
    if (n_w % 4 != 0 || n_w / 4 > 4096 || n_r != (n_w / 4) * HG_CAMERA_RECORD_DOUBLES || output < 0 || output > 3 || W < 1 || H < 1)
        return throw_str(env, "hgwarp: warpCamera: records, windows, output or the source size is out of range");
    const size_t F = n_w / 4;
    const int picture = output < 2, fmt = (output == 0 || output == 2) ? HG_FIELD_INDEX : HG_FIELD_COORDS;
    const size_t plane = (size_t)W * (size_t)H * 4;
    if (picture && (!img || n_img < 1 || n_i != plane * (size_t)n_img)) return throw_str(env, "hgwarp: warpCamera: images must hold nImages RGBA pictures of W x H");
    hg_geom *g = (hg_geom *)calloc(F ? F : 1, sizeof *g);
    if (!g) return throw_str(env, "hgwarp: out of memory");
    size_t fld_total = 0, out_total = 0;
    for (size_t f = 0; f < F; f++) {
        g[f].x_off = win[4 * f]; g[f].y_off = win[4 * f + 1]; g[f].obj_w = win[4 * f + 2]; g[f].obj_h = win[4 * f + 3];
        const size_t px = (g[f].obj_w > 0 && g[f].obj_h > 0) ? (size_t)g[f].obj_w * (size_t)g[f].obj_h : 0;
        fld_total += (px * (fmt == HG_FIELD_INDEX ? 4 : 8) + 255) & ~(size_t)255;
        out_total += (px * 4 + 255) & ~(size_t)255;
    }
    const size_t res_total = picture ? out_total : fld_total;
    void *p_data;
    napi_value out, v_data;
    if (!(v_data = make_typed(env, napi_uint8_array, res_total, 1, &p_data))) { free(g); return NULL; }
    if (napi_create_object(env, &out) != napi_ok || napi_set_named_property(env, out, "data", v_data) != napi_ok) { free(g); return throw_str(env, "hgwarp: N-API call failed"); }
    if (!F) { free(g); return out; }
#define CAM_PAD(b) (((size_t)(b) + 255) & ~(size_t)255)
    const size_t o_rec = 0, o_fld = o_rec + CAM_PAD(n_r * 8), o_img = o_fld + CAM_PAD(fld_total), o_out = o_img + CAM_PAD(picture ? n_i : 0),
                 total = o_out + CAM_PAD(picture ? out_total : 0);
#undef CAM_PAD
    void *d = NULL;
    int rc = hg_device_alloc(h->ctx, total, &d);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, "hg_device_alloc", rc); free(g); return e; }
    uint8_t *b = (uint8_t *)d;
    const char *what = "hg_copy_to_device";
    rc = hg_copy_to_device(h->ctx, b + o_rec, rec, n_r * 8);
    if (rc == HG_OK && picture) rc = hg_copy_to_device(h->ctx, b + o_img, img, n_i);
    if (rc == HG_OK) {
        what = "hg_field_camera_frames_device";
        rc = hg_field_camera_frames_device(h->ctx, (const double *)(b + o_rec), g, (int)F, W, H, surface, scale, u0, v0, fmt, NULL, b + o_fld);
    }
    if (rc == HG_OK && output == 0) {
        what = "hg_remap_index_frames_device";
        rc = hg_remap_index_frames_device(h->ctx, g, (int)F, b + o_fld, NULL, b + o_img, (size_t)W * (size_t)H, n_img, plane, 4, b + o_out, NULL);
    }
    if (rc == HG_OK && output == 1) {
        what = "hg_remap_bilinear_frames_device";
        rc = hg_remap_bilinear_frames_device(h->ctx, g, (int)F, b + o_fld, NULL, b + o_img, W, H, n_img, plane, HG_ELEM_U8, 4, b + o_out, NULL);
    }
    if (rc == HG_OK && res_total) { what = "hg_copy_to_host"; rc = hg_copy_to_host(h->ctx, p_data, picture ? b + o_out : b + o_fld, res_total); }
    free(g);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); hg_device_free(h->ctx, d); return e; }
    HG_CALL(h->ctx, "hg_device_free", hg_device_free(h->ctx, d));
    return out;
}

/* denseFlow(handle, from, to, W, H, channels, nFrames, nToSets, levels, iterations, radius, minEig, maxUpdate, flags): dense optical flow
 * between nFrames pairs of u8 planes (hg_flow_dense_frames_device), all on the device.  from: Uint8Array of nFrames planes of W x H x
 * channels, to: Uint8Array of nToSets planes (frame f is registered onto plane f % nToSets).  flags: 1 = the field comes down, 2 = the
 * residual, 4 = the good flags, 8 = the FROM planes sent through the field by hg_remap_bilinear_frames_device (u8 x channels).  Returns
 * { field: Float32Array(F x W x H x 2) | null, residual: Uint8Array(F x W x H) | null, good: Uint8Array | null, images: Uint8Array(F x W x
 * H x channels) | null }, every frame tightly packed.  Only what was asked for comes down. */
static napi_value fn_dense_flow(napi_env env, napi_callback_info info)
{
    napi_value a[14];
    if (!get_args(env, info, 14, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int W, H, ch, F, S, levels, n_iter, radius, flags; size_t n_f = 0, n_t = 0; double min_eig, max_update;
    uint8_t *from = (uint8_t *)get_typed(env, a[1], napi_uint8_array, &n_f, "from"); if (!from && n_f) return NULL;
    uint8_t *to = (uint8_t *)get_typed(env, a[2], napi_uint8_array, &n_t, "to"); if (!to && n_t) return NULL;
    if (!get_i32(env, a[3], &W) || !get_i32(env, a[4], &H) || !get_i32(env, a[5], &ch) || !get_i32(env, a[6], &F) || !get_i32(env, a[7], &S) ||
        !get_i32(env, a[8], &levels) || !get_i32(env, a[9], &n_iter) || !get_i32(env, a[10], &radius)) return NULL;
    if (napi_get_value_double(env, a[11], &min_eig) != napi_ok || napi_get_value_double(env, a[12], &max_update) != napi_ok)
        return throw_str(env, "hgwarp: minEig and maxUpdate must be numbers");
    if (!get_i32(env, a[13], &flags)) return NULL;
    if (W < 1 || W > 32768 || H < 1 || H > 32768 || (ch != 1 && ch != 4) || F < 0 || F > 4096 || S < 1 || flags < 0 || flags > 15)
        return throw_str(env, "hgwarp: denseFlow: the size, channels, frame counts or flags are out of range");
    const size_t n_px = (size_t)W * (size_t)H, plane = n_px * (size_t)ch, NF = (size_t)F;
    if (n_f != plane * NF || n_t != plane * (size_t)S) return throw_str(env, "hgwarp: denseFlow: from / to must hold their planes of W x H x channels bytes");
    size_t scr_b = 0;
    int rc = hg_flow_layout(W, H, ch, F, S, levels, &scr_b);
    if (rc != HG_OK) return throw_hg(env, h->ctx, "hg_flow_layout", rc);
    void *p_fld = NULL, *p_res = NULL, *p_good = NULL, *p_img = NULL;
    napi_value out, v_fld, v_res, v_good, v_img;
    if (flags & 1) { if (!(v_fld = make_typed(env, napi_float32_array, NF * n_px * 2, 4, &p_fld))) return NULL; } else NAPI_OK(napi_get_null(env, &v_fld));
    if (flags & 2) { if (!(v_res = make_typed(env, napi_uint8_array, NF * n_px, 1, &p_res))) return NULL; } else NAPI_OK(napi_get_null(env, &v_res));
    if (flags & 4) { if (!(v_good = make_typed(env, napi_uint8_array, NF * n_px, 1, &p_good))) return NULL; } else NAPI_OK(napi_get_null(env, &v_good));
    if (flags & 8) { if (!(v_img = make_typed(env, napi_uint8_array, NF * plane, 1, &p_img))) return NULL; } else NAPI_OK(napi_get_null(env, &v_img));
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "field", v_fld)); NAPI_OK(napi_set_named_property(env, out, "residual", v_res));
    NAPI_OK(napi_set_named_property(env, out, "good", v_good)); NAPI_OK(napi_set_named_property(env, out, "images", v_img));
    if (!F) return out;
#define FLOW_PAD(b) (((size_t)(b) + 255) & ~(size_t)255)
    const size_t fld_frame = FLOW_PAD(n_px * 8), img_frame = FLOW_PAD(plane);
    const size_t o_from = 0, o_to = o_from + FLOW_PAD(n_f), o_scr = o_to + FLOW_PAD(n_t), o_fld = o_scr + FLOW_PAD(scr_b), o_res = o_fld + fld_frame * NF,
                 o_good = o_res + FLOW_PAD((flags & 2) ? NF * n_px : 0), o_img = o_good + FLOW_PAD((flags & 4) ? NF * n_px : 0),
                 total = o_img + ((flags & 8) ? img_frame * NF : 0);
#undef FLOW_PAD
    hg_geom *g = (hg_geom *)calloc(NF, sizeof *g);
    if (!g) return throw_str(env, "hgwarp: out of memory");
    for (size_t f = 0; f < NF; f++) { g[f].obj_w = W; g[f].obj_h = H; }
    void *d = NULL;
    rc = hg_device_alloc(h->ctx, total, &d);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, "hg_device_alloc", rc); free(g); return e; }
    uint8_t *b = (uint8_t *)d;
    const char *what = "hg_copy_to_device";
    rc = hg_copy_to_device(h->ctx, b + o_from, from, n_f);
    if (rc == HG_OK) rc = hg_copy_to_device(h->ctx, b + o_to, to, n_t);
    if (rc == HG_OK) {
        what = "hg_flow_dense_frames_device";
        rc = hg_flow_dense_frames_device(h->ctx, b + o_from, F, plane, b + o_to, S, plane, W, H, ch, levels, n_iter, radius, min_eig, max_update, NULL, b + o_fld,
                                         NULL, (flags & 2) ? b + o_res : NULL, (flags & 4) ? b + o_good : NULL, b + o_scr);
    }
    if (rc == HG_OK && (flags & 8)) {
        what = "hg_remap_bilinear_frames_device";
        rc = hg_remap_bilinear_frames_device(h->ctx, g, F, b + o_fld, NULL, b + o_from, W, H, F, plane, HG_ELEM_U8, ch, b + o_img, NULL);
    }
    free(g);
    what = rc == HG_OK ? "hg_copy_to_host" : what;
    for (size_t f = 0; f < NF && rc == HG_OK; f++) {
        if (flags & 1) rc = hg_copy_to_host(h->ctx, (uint8_t *)p_fld + f * n_px * 8, b + o_fld + f * fld_frame, n_px * 8);
        if (rc == HG_OK && (flags & 8)) rc = hg_copy_to_host(h->ctx, (uint8_t *)p_img + f * plane, b + o_img + f * img_frame, plane);
    }
    if (rc == HG_OK && (flags & 2)) rc = hg_copy_to_host(h->ctx, p_res, b + o_res, NF * n_px);
    if (rc == HG_OK && (flags & 4)) rc = hg_copy_to_host(h->ctx, p_good, b + o_good, NF * n_px);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); hg_device_free(h->ctx, d); return e; }
    HG_CALL(h->ctx, "hg_device_free", hg_device_free(h->ctx, d));
    return out;
}

/* matchDescriptors(handle, kind, descBytes, stride, query, nQuery, countsQ, train, nTrain, countsT, ratio, maxDistance, crossCheck,
 * queryPoints | null, trainPoints | null): the accepted nearest-neighbour pairs of every frame (hg_match_descriptors_frames_device).  query:
 * Uint8Array of F x nQuery x stride, F = countsQ.length; train: Uint8Array of S x nTrain x stride, S = countsT.length; the points: Float32Array
 * of F x nQuery x 2 resp. S x nTrain x 2, both or none.  Everything goes up into device memory of the call's own, the entry runs, and
 * { counts: Int32Array(F), pairs: Int32Array(F x nQuery x 2), matches: Float32Array(F x nQuery x 4) | null } come down.  Needs no image. */
static napi_value fn_match_descriptors(napi_env env, napi_callback_info info)
{
    napi_value a[15];
    if (!get_args(env, info, 15, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int kind, desc_bytes, stride, n_query, n_train, cross; size_t n_q = 0, n_t = 0, n_cq = 0, n_ct = 0, n_qp = 0, n_tp = 0; double ratio, maxd;
    if (!get_i32(env, a[1], &kind) || !get_i32(env, a[2], &desc_bytes) || !get_i32(env, a[3], &stride)) return NULL;
    uint8_t *q = (uint8_t *)get_typed(env, a[4], napi_uint8_array, &n_q, "query"); if (!q) return NULL;
    if (!get_i32(env, a[5], &n_query)) return NULL;
    int32_t *cq = (int32_t *)get_typed(env, a[6], napi_int32_array, &n_cq, "countsQ"); if (!cq) return NULL;
    uint8_t *t = (uint8_t *)get_typed(env, a[7], napi_uint8_array, &n_t, "train"); if (!t) return NULL;
    if (!get_i32(env, a[8], &n_train)) return NULL;
    int32_t *ct = (int32_t *)get_typed(env, a[9], napi_int32_array, &n_ct, "countsT"); if (!ct) return NULL;
    if (napi_get_value_double(env, a[10], &ratio) != napi_ok) return throw_str(env, "hgwarp: ratio must be a number");
    if (napi_get_value_double(env, a[11], &maxd) != napi_ok || !(maxd >= 0 && maxd <= 4294967295.0)) return throw_str(env, "hgwarp: maxDistance must be a uint32");
    if (!get_i32(env, a[12], &cross)) return NULL;
    napi_valuetype vq, vt;
    NAPI_OK(napi_typeof(env, a[13], &vq)); NAPI_OK(napi_typeof(env, a[14], &vt));
    const int has_q = vq != napi_null && vq != napi_undefined, has_t = vt != napi_null && vt != napi_undefined;
    if (has_q != has_t) return throw_str(env, "hgwarp: matchDescriptors: queryPoints and trainPoints come together");
    float *qp = NULL, *tp = NULL;
    if (has_q) {
        qp = (float *)get_typed(env, a[13], napi_float32_array, &n_qp, "queryPoints"); if (!qp) return NULL;
        tp = (float *)get_typed(env, a[14], napi_float32_array, &n_tp, "trainPoints"); if (!tp) return NULL;
    }
    if (stride < 16 || stride > 1024 || n_query < 0 || n_query > 65536 || n_train < 0 || n_train > 65536 || n_cq > 4096 || n_ct > 4096)
        return throw_str(env, "hgwarp: matchDescriptors: stride, nQuery, nTrain or the number of sets is out of range");
    const size_t F = n_cq, S = n_ct, NQ = (size_t)n_query, NT = (size_t)n_train, ST = (size_t)stride;
    if (n_q != F * NQ * ST || n_t != S * NT * ST) return throw_str(env, "hgwarp: query / train must hold sets x rows x stride bytes");
    if (has_q && (n_qp != F * NQ * 2 || n_tp != S * NT * 2)) return throw_str(env, "hgwarp: queryPoints / trainPoints must hold sets x rows x 2 floats");
    void *p_cnt, *p_pairs, *p_m = NULL;
    napi_value out, v_cnt, v_pairs, v_m;
    if (!(v_cnt = make_typed(env, napi_int32_array, F, 4, &p_cnt)) || !(v_pairs = make_typed(env, napi_int32_array, F * NQ * 2, 4, &p_pairs))) return NULL;
    if (has_q) { if (!(v_m = make_typed(env, napi_float32_array, F * NQ * 4, 4, &p_m))) return NULL; }
    else NAPI_OK(napi_get_null(env, &v_m));
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_set_named_property(env, out, "counts", v_cnt)); NAPI_OK(napi_set_named_property(env, out, "pairs", v_pairs));
    NAPI_OK(napi_set_named_property(env, out, "matches", v_m));
    if (!F) return out;
#define MATCH_PAD(b) (((size_t)(b) + 255) & ~(size_t)255)
    const size_t o_q = 0, o_t = o_q + MATCH_PAD(F * NQ * ST), o_qp = o_t + MATCH_PAD(S * NT * ST), o_tp = o_qp + MATCH_PAD(has_q ? F * NQ * 8 : 0),
                 o_cnt = o_tp + MATCH_PAD(has_q ? S * NT * 8 : 0), o_pairs = o_cnt + MATCH_PAD(F * 4), o_m = o_pairs + MATCH_PAD(F * NQ * 8),
                 total = o_m + MATCH_PAD(has_q ? F * NQ * 16 : 0);
#undef MATCH_PAD
    void *d = NULL;
    HG_CALL(h->ctx, "hg_device_alloc", hg_device_alloc(h->ctx, total, &d));
    uint8_t *b = (uint8_t *)d;
    int rc = HG_OK;
    const char *what = "hg_copy_to_device";
    if (F * NQ) rc = hg_copy_to_device(h->ctx, b + o_q, q, F * NQ * ST);
    if (rc == HG_OK && S * NT) rc = hg_copy_to_device(h->ctx, b + o_t, t, S * NT * ST);
    if (rc == HG_OK && has_q && F * NQ) rc = hg_copy_to_device(h->ctx, b + o_qp, qp, F * NQ * 8);
    if (rc == HG_OK && has_q && S * NT) rc = hg_copy_to_device(h->ctx, b + o_tp, tp, S * NT * 8);
    if (rc == HG_OK) {
        what = "hg_match_descriptors_frames_device";
        rc = hg_match_descriptors_frames_device(h->ctx, kind, desc_bytes, ST, b + o_q, n_query, cq, (int)F, b + o_t, n_train, ct, (int)S, ratio, (uint32_t)maxd, cross,
                                                has_q ? b + o_qp : NULL, has_q ? b + o_tp : NULL, (int32_t *)(b + o_cnt), has_q ? b + o_m : NULL,
                                                (int32_t *)(b + o_pairs), NULL);
    }
    if (rc == HG_OK) { what = "hg_copy_to_host"; rc = hg_copy_to_host(h->ctx, p_cnt, b + o_cnt, F * 4); }
    if (rc == HG_OK && F * NQ) rc = hg_copy_to_host(h->ctx, p_pairs, b + o_pairs, F * NQ * 8);
    if (rc == HG_OK && has_q && F * NQ) rc = hg_copy_to_host(h->ctx, p_m, b + o_m, F * NQ * 16);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); hg_device_free(h->ctx, d); return e; }
    HG_CALL(h->ctx, "hg_device_free", hg_device_free(h->ctx, d));
    return out;
}

/* detectAndDescribe(handle, planes, nPlanes, width, height, channels, cell, perCell, minResponse): the keypoints of nPlanes planes
 * (hg_detect_describe_frames_device).  planes: Uint8Array of nPlanes x width x height x channels; minResponse: an integer number in 1..2^53.
 * Everything goes up into device memory of the call's own, the entry runs, and { nSlots, counts: Int32Array(nPlanes), points:
 * Float32Array(nPlanes x nSlots x 2), descriptors: Uint8Array(nPlanes x nSlots x 32) } come down.  Needs no image. */
static napi_value fn_detect_describe(napi_env env, napi_callback_info info)
{
    napi_value a[9];
    if (!get_args(env, info, 9, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int n_planes, W, H, channels, cell, per_cell; size_t n_p = 0; double thr;
    uint8_t *planes = (uint8_t *)get_typed(env, a[1], napi_uint8_array, &n_p, "planes"); if (!planes) return NULL;
    if (!get_i32(env, a[2], &n_planes) || !get_i32(env, a[3], &W) || !get_i32(env, a[4], &H) || !get_i32(env, a[5], &channels) || !get_i32(env, a[6], &cell) ||
        !get_i32(env, a[7], &per_cell)) return NULL;
    if (napi_get_value_double(env, a[8], &thr) != napi_ok || !(thr >= 1.0 && thr <= 9007199254740992.0) || thr != (double)(int64_t)thr)
        return throw_str(env, "hgwarp: minResponse must be an integer in 1..2^53");
    int cx = 0, cy = 0, n_slots = 0;
    if (hg_detect_layout(W, H, cell, per_cell, &cx, &cy, &n_slots) != HG_OK) return throw_str(env, hg_last_error(NULL));
    if (n_planes < 0 || n_planes > 4096 || (channels != 1 && channels != 4)) return throw_str(env, "hgwarp: detectAndDescribe: nPlanes or channels is out of range");
    const size_t P = (size_t)n_planes, NS = (size_t)n_slots, plane = (size_t)W * (size_t)H * (size_t)channels;
    if (n_p != P * plane) return throw_str(env, "hgwarp: planes must hold nPlanes x width x height x channels bytes");
    void *p_cnt, *p_pts, *p_desc;
    napi_value out, v_cnt, v_pts, v_desc, v_slots;
    if (!(v_cnt = make_typed(env, napi_int32_array, P, 4, &p_cnt)) || !(v_pts = make_typed(env, napi_float32_array, P * NS * 2, 4, &p_pts)) ||
        !(v_desc = make_typed(env, napi_uint8_array, P * NS * 32, 1, &p_desc))) return NULL;
    NAPI_OK(napi_create_object(env, &out));
    NAPI_OK(napi_create_int32(env, n_slots, &v_slots));
    NAPI_OK(napi_set_named_property(env, out, "nSlots", v_slots)); NAPI_OK(napi_set_named_property(env, out, "counts", v_cnt));
    NAPI_OK(napi_set_named_property(env, out, "points", v_pts)); NAPI_OK(napi_set_named_property(env, out, "descriptors", v_desc));
    if (!P) return out;
#define DETECT_PAD(b) (((size_t)(b) + 255) & ~(size_t)255)
    const size_t o_p = 0, o_cnt = o_p + DETECT_PAD(P * plane), o_pts = o_cnt + DETECT_PAD(P * 4), o_desc = o_pts + DETECT_PAD(P * NS * 8),
                 total = o_desc + DETECT_PAD(P * NS * 32);
#undef DETECT_PAD
    void *d = NULL;
    HG_CALL(h->ctx, "hg_device_alloc", hg_device_alloc(h->ctx, total, &d));
    uint8_t *b = (uint8_t *)d;
    const char *what = "hg_copy_to_device";
    int rc = hg_copy_to_device(h->ctx, b + o_p, planes, P * plane);
    if (rc == HG_OK) {
        what = "hg_detect_describe_frames_device";
        rc = hg_detect_describe_frames_device(h->ctx, b + o_p, W, H, n_planes, plane, channels, cell, per_cell, (int64_t)thr, 32, (int32_t *)(b + o_cnt), b + o_pts,
                                              b + o_desc, NULL);
    }
    if (rc == HG_OK) { what = "hg_copy_to_host"; rc = hg_copy_to_host(h->ctx, p_cnt, b + o_cnt, P * 4); }
    if (rc == HG_OK) rc = hg_copy_to_host(h->ctx, p_pts, b + o_pts, P * NS * 8);
    if (rc == HG_OK) rc = hg_copy_to_host(h->ctx, p_desc, b + o_desc, P * NS * 32);
    if (rc != HG_OK) { napi_value e = throw_hg(env, h->ctx, what, rc); hg_device_free(h->ctx, d); return e; }
    HG_CALL(h->ctx, "hg_device_free", hg_device_free(h->ctx, d));
    return out;
}

/* redoneFrames(ctx): frames the fused kernels flagged and hg_sync redid through the map so far (hg_redone_frames; tests) */
static napi_value fn_redone_frames(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    napi_value out;
    NAPI_OK(napi_create_double(env, (double)hg_redone_frames(h->ctx), &out));
    return out;
}

/* spanCacheStats(ctx): hg_span_cache_stats as an array of six numbers -- builds, warps that ran from the cache, groups valid, groups not cached,
 * bytes held, state of the last inverse piecewise warp (0 off, 1 build, 2 use); null if the call failed */
static napi_value fn_span_cache_stats(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int64_t st[6] = { 0, 0, 0, 0, 0, 0 };
    napi_value out, v;
    if (hg_span_cache_stats(h->ctx, st) != HG_OK) { NAPI_OK(napi_get_null(env, &out)); return out; }
    NAPI_OK(napi_create_array_with_length(env, 6, &out));
    for (uint32_t i = 0; i < 6; i++) {
        NAPI_OK(napi_create_double(env, (double)st[i], &v));
        NAPI_OK(napi_set_element(env, out, i, v));
    }
    return out;
}

/* setSampling(handle, mode): HG_SAMPLE_NEAREST (0) / HG_SAMPLE_BILINEAR (1) for the inverse warps called from now on */
static napi_value fn_set_sampling(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int mode;
    if (!get_i32(env, a[1], &mode)) return NULL;
    HG_CALL(h->ctx, "hg_set_sampling", hg_set_sampling(h->ctx, mode));
    return NULL;
}

static napi_value fn_get_matrices(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    int T; if (!get_i32(env, a[1], &T)) return NULL;
    T = (int)h->n_tris;                                      /* the C ABI fills n_triangles x 6 floats: size by the mesh, not by the caller */
    void *fwd, *inv;
    napi_value rf = make_typed(env, napi_float32_array, (size_t)T * 6, 4, &fwd); if (!rf) return NULL;
    napi_value ri = make_typed(env, napi_float32_array, (size_t)T * 6, 4, &inv); if (!ri) return NULL;
    if (T) HG_CALL(h->ctx, "hg_get_matrices", hg_get_matrices(h->ctx, (float *)fwd, (float *)inv));
    napi_value obj;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_set_named_property(env, obj, "forward", rf));
    NAPI_OK(napi_set_named_property(env, obj, "inverse", ri));
    return obj;
}

/* ---------------------------------------------------------------- batches: the caller loop `setDestinyPoints(dst_f); warp()` as device passes
 * Frames come back as views of ONE page-locked slab owned by the context handle (two of them: slot 0 for the frames warp() sends down
 * the inverse loops, slot 1 for the forward loops): one external ArrayBuffer per slab, created once and reused by the NEXT batch of the
 * same kind on this instance -- frames of a batch are valid until then (or releaseBatch()), like `reuseOutput` for warp().  Nothing
 * depends on the garbage collector: no per-frame ArrayBuffer, no finalizer has to run before memory comes back, no fall-back to V8
 * arrays.  `ownFrames` (optional argument) = the old behaviour: every frame its own pooled buffer with a GC-bound life time.
 * With per-frame sources ({images}: the video loop warp(image_f), README.md:121-137) the pass is pipelined frame by frame:
 * H2D(f + 1) on the context's copy stream runs while D2H(f) travels the other way on the warp stream. */
static void slab_finalize(napi_env env, void *data, void *hint)
{
    const size_t bytes = hint ? *(size_t *)hint : 0;          /* (the hint is the slab's size: what was added to V8's external-memory counter and to the pinned total) */
    free(hint);
    if (data) hg_host_free(data);
    pool_t *P = NULL;
    if (!bytes || napi_get_instance_data(env, (void **)&P) != napi_ok || !P) return;        /* (the env is going away) */
    P->pin_bytes -= bytes < P->pin_bytes ? bytes : P->pin_bytes;
    int64_t adj; napi_adjust_external_memory(env, -(int64_t)bytes, &adj);
}

static void slab_drop(napi_env env, slab_t *sl, int detach)
{
    if (sl->ab) {
        if (detach) { napi_value ab = NULL; if (napi_get_reference_value(env, sl->ab, &ab) == napi_ok && ab) (void)napi_detach_arraybuffer(env, ab); }
        napi_delete_reference(env, sl->ab);                   /* the ArrayBuffer's own finalizer frees the page-locked memory once no view is left */
    }
    sl->ab = NULL; sl->ptr = NULL; sl->cap = 0;
}

/* JS array of F Uint8ClampedArray views, frame f at byte offs[f] of slab `slot` (grown to `total` bytes if needed) */
/* The slab is page-locked memory like the pooled frames and counts against the same cap (setPinnedLimit): when it does not fit -- or the
 * cap is 0, or the allocation fails -- *fallback is set, NULL is returned WITHOUT a pending exception, and the batch gets own frames. */
static napi_value slab_frames(napi_env env, handle_t *h, int slot, const hg_geom *g, const size_t *offs, int F, size_t total, uint8_t **base, int *fallback)
{
    slab_t *sl = &h->slab[slot];
    *fallback = 0;
    pool_t *P = pool_of(env); if (!P) return NULL;
    if (sl->ab && (P->pin_limit == 0 || P->pin_bytes > P->pin_limit)) {      /* the cap was lowered since this slab was made: it goes (its views keep their memory until collected) */
        slab_drop(env, sl, 0);
        if (P->pin_limit == 0) { P->stat_fallback++; *fallback = 1; return NULL; }
    }
    if (total > sl->cap || !sl->ab) {
        slab_drop(env, sl, 0);
        const size_t want = total + total / 8 + 4096;
        for (int i = 0; i < P->npins && P->pin_bytes + want > P->pin_limit; i++) if (P->pins[i].ptr && !P->pins[i].in_use) pin_drop(P, i);   /* idle pooled frames make room */
        if (P->pin_limit == 0 || P->pin_bytes + want > P->pin_limit) { P->stat_fallback++; *fallback = 1; return NULL; }
        void *p = NULL; napi_value ab;
        size_t *hint = (size_t *)malloc(sizeof *hint);
        if (!hint || hg_host_alloc(want, &p) != HG_OK) { free(hint); P->stat_fallback++; *fallback = 1; return NULL; }
        *hint = want;
        if (napi_create_external_arraybuffer(env, p, want, slab_finalize, hint, &ab) != napi_ok) { hg_host_free(p); free(hint); return throw_str(env, "hgwarp: cannot wrap the frame slab"); }
        P->pin_bytes += want;                                 /* (slab_finalize takes both back) */
        int64_t adj; napi_adjust_external_memory(env, (int64_t)want, &adj);
        if (napi_create_reference(env, ab, 1, &sl->ab) != napi_ok) return throw_str(env, "hgwarp: cannot keep the frame slab");
        sl->ptr = p; sl->cap = want;
    }
    napi_value ab, arr;
    NAPI_OK(napi_get_reference_value(env, sl->ab, &ab));
    NAPI_OK(napi_create_array_with_length(env, F, &arr));
    for (int f = 0; f < F; f++) {
        const size_t px = (g[f].obj_w > 0 && g[f].obj_h > 0) ? (size_t)g[f].obj_w * g[f].obj_h : 0;
        napi_value ta;
        NAPI_OK(napi_create_typedarray(env, napi_uint8_clamped_array, px * 4, ab, px ? offs[f] : 0, &ta));
        NAPI_OK(napi_set_element(env, arr, f, ta));
    }
    *base = (uint8_t *)sl->ptr;
    return arr;
}

/* releaseBatch(ctx): the frames of the last batches become empty (their ArrayBuffers are detached), the slabs go */
static napi_value fn_release_batch(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    (void)hg_sync(h->ctx);
    for (int k = 0; k < 2; k++) slab_drop(env, &h->slab[k], 1);
    return NULL;
}

enum { JOB_PW_INV, JOB_GEO_INV, JOB_PW_FWD, JOB_GEO_FWD, JOB_PW_INV_SRC };
/* src / min_src (JOB_PW_INV_SRC): the frames' own source points (F x 2N) and source minima (F x 2) */
typedef struct { int type, kind; const float *dst, *from, *to; const double *m; int mx, my; size_t per; const float *src; const int32_t *min_src; } batch_job;

/* frames [f0, f0 + n) of the job into d_out at offs[f0 ..] */
static int job_launch(handle_t *h, const batch_job *j, const hg_geom *g, const size_t *offs, int f0, int n, void *d_out)
{
    switch (j->type) {
    case JOB_PW_INV:  return hg_warp_inverse_piecewise_batch_device(h->ctx, j->dst + (size_t)f0 * 2 * h->n_pts, g + f0, offs + f0, n, d_out);
    case JOB_PW_INV_SRC:
        return hg_warp_inverse_piecewise_src_batch_device(h->ctx, j->src + (size_t)f0 * 2 * h->n_pts, j->min_src + (size_t)f0 * 2, j->dst + (size_t)f0 * 2 * h->n_pts,
                                                          g + f0, offs + f0, n, d_out);
    case JOB_PW_FWD:  return hg_warp_forward_piecewise_batch_device(h->ctx, j->dst + (size_t)f0 * 2 * h->n_pts, j->mx, j->my, g + f0, offs + f0, n, d_out);
    case JOB_GEO_FWD: return hg_warp_forward_geometric_batch_device(h->ctx, j->kind, j->m + (size_t)f0 * 8, g + f0, offs + f0, n, d_out);
    default: {
        int rc = hg_geometric_set_frames_points(h->ctx, j->kind, j->from + (size_t)f0 * j->per, j->to + (size_t)f0 * j->per, g + f0, offs + f0, n);
        return rc == HG_OK ? hg_warp_inverse_geometric_frames_device(h->ctx, d_out) : rc;
    }
    }
}

/* opt[0] = ownFrames (boolean), opt[1] = images (Array of Uint8ClampedArray) or null / undefined, opt[2], opt[3] = their width, height */
static napi_value run_batch(napi_env env, handle_t *h, const batch_job *job, const int32_t *gv, int F, int slot, const napi_value *opt, size_t n_opt, const char *what)
{
    const hg_geom *g = (const hg_geom *)gv;
    bool own = false;
    if (n_opt > 0) { napi_valuetype vt; if (napi_typeof(env, opt[0], &vt) == napi_ok && vt == napi_boolean) napi_get_value_bool(env, opt[0], &own); }
    uint32_t n_img = 0;
    int iw = 0, ih = 0;
    if (n_opt > 1) {
        bool is_arr = false;
        if (napi_is_array(env, opt[1], &is_arr) == napi_ok && is_arr) {
            NAPI_OK(napi_get_array_length(env, opt[1], &n_img));
            if (n_img == 0 || n_opt < 4 || !get_i32(env, opt[2], &iw) || !get_i32(env, opt[3], &ih) || iw <= 0 || ih <= 0)
                return throw_str(env, "hgwarp: a batch with per-frame sources needs a non-empty image list and their width, height");
        }
    }
    size_t *offs = (size_t *)malloc(sizeof(size_t) * F);
    if (!offs) return throw_str(env, "hgwarp: out of memory (frame offsets)");
    size_t total = 0;
    hg_pack_offsets(g, F, offs, &total);
    int rc = HG_OK;
    if (total > h->d_batch_cap) {
        if (h->d_batch) hg_device_free(h->ctx, h->d_batch);
        h->d_batch = NULL; h->d_batch_cap = 0;
        rc = hg_device_alloc(h->ctx, total, &h->d_batch);
        if (rc == HG_OK) h->d_batch_cap = total;
    }
    if (rc != HG_OK) { free(offs); return throw_hg(env, h->ctx, what, rc); }
    /* where the frames go */
    napi_value arr = NULL;
    uint8_t *base = NULL;
    uint8_t **outs = NULL;
    if (!own) {
        int fallback = 0;
        arr = slab_frames(env, h, slot, g, offs, F, total, &base, &fallback);
        if (!arr && !fallback) { free(offs); return NULL; }
        if (!arr) own = true;                                 /* no room under the pinned cap (or no page-locked memory): own frames, as without the option */
    }
    if (own) {
        outs = (uint8_t **)calloc((size_t)F, sizeof *outs);
        if (!outs || napi_create_array_with_length(env, F, &arr) != napi_ok) { free(offs); free(outs); return throw_str(env, "hgwarp: out of memory (frames)"); }
        for (int f = 0; f < F; f++) {
            const size_t px = (g[f].obj_w > 0 && g[f].obj_h > 0) ? (size_t)g[f].obj_w * g[f].obj_h : 0;
            void *out; napi_value ta = make_pixels(env, px * 4, NULL, 0, &out);
            if (!ta) { free(offs); free(outs); return NULL; }
            outs[f] = (uint8_t *)out;
            napi_set_element(env, arr, f, ta);
        }
    }
    const uint8_t *d_out = (const uint8_t *)h->d_batch;
    if (n_img == 0) {
        /* one source for all frames: one pass; the copies queue behind the kernels on the warp stream (page-locked memory: asynchronous DMA) */
        rc = job_launch(h, job, g, offs, 0, F, h->d_batch);
        if (rc == HG_OK && !own) rc = hg_copy_to_host_async(h->ctx, base, d_out, total);       /* (the slab has the device layout: one copy) */
        for (int f = 0; f < F && rc == HG_OK && own; f++) {
            const size_t px = (g[f].obj_w > 0 && g[f].obj_h > 0) ? (size_t)g[f].obj_w * g[f].obj_h : 0;
            if (px) rc = hg_copy_to_host_async(h->ctx, outs[f], d_out + offs[f], px * 4);
        }
    } else {
        /* one source per frame (frame f reads images[f % n]): upload(f + 1) on the copy stream while frame f's pixels come down */
        const size_t bytes = (size_t)iw * (size_t)ih * 4, stride = (bytes + 255) & ~(size_t)255;
        const uint8_t **src = (const uint8_t **)calloc(n_img, sizeof *src);
        if (!src) rc = HG_ERR_NOMEM;
        for (uint32_t k = 0; k < n_img && rc == HG_OK; k++) {
            napi_value el; size_t len;
            if (napi_get_element(env, opt[1], k, &el) != napi_ok) { rc = HG_ERR_INVALID; break; }
            src[k] = (const uint8_t *)get_typed(env, el, napi_uint8_clamped_array, &len, "images[k]");
            if (!src[k]) { free(src); free(offs); free(outs); return NULL; }
            if (len < bytes) { free(src); free(offs); free(outs); return throw_str(env, "hgwarp: an image is smaller than width*height*4"); }
        }
        if (rc == HG_OK && stride * n_img > h->d_imgs_cap) {
            void *q = NULL;
            rc = hg_device_alloc(h->ctx, stride * n_img, &q);
            if (rc == HG_OK) rc = hg_set_images_device(h->ctx, q, iw, ih, 1, stride);      /* (the context's alias moves first: never dangling) */
            if (rc == HG_OK) { if (h->d_imgs) hg_device_free(h->ctx, h->d_imgs); h->d_imgs = q; h->d_imgs_cap = stride * n_img; }
            else if (q) hg_device_free(h->ctx, q);
        }
        /* Three streams: image f + 1 goes up (copy stream) and frame f - 1 comes down (download stream) while frame f is warped; the host
         * only ever waits for warps.  A frame comes down unsettled: if the settlement that precedes the next image binding (or the final
         * hg_sync) redid it -- hg_redone_frames moved --, it comes down again. */
        if (rc == HG_OK) rc = hg_upload_on_copy_stream(h->ctx, h->d_imgs, src[0], bytes);
        long redone = hg_redone_frames(h->ctx);
        for (int f = 0; f <= F && rc == HG_OK; f++) {
            if (f < F) rc = hg_set_images_device(h->ctx, (uint8_t *)h->d_imgs + stride * ((uint32_t)f % n_img), iw, ih, 1, stride);   /* (settles frame f - 1) */
            else rc = hg_sync(h->ctx);
            if (rc == HG_OK && f > 0) {
                const long now = hg_redone_frames(h->ctx);
                const size_t ppx = (g[f - 1].obj_w > 0 && g[f - 1].obj_h > 0) ? (size_t)g[f - 1].obj_w * g[f - 1].obj_h : 0;
                if (now != redone && ppx) rc = hg_download_behind_warps(h->ctx, own ? outs[f - 1] : base + offs[f - 1], d_out + offs[f - 1], ppx * 4);
                redone = now;
            } else if (rc == HG_OK) redone = hg_redone_frames(h->ctx);      /* f == 0: that binding settled runs queued BEFORE this batch; their redos are not frame 0's */
            if (f == F || rc != HG_OK) break;
            const size_t px = (g[f].obj_w > 0 && g[f].obj_h > 0) ? (size_t)g[f].obj_w * g[f].obj_h : 0;
            rc = hg_fence_copies(h->ctx);                                                   /* the warp stream waits for image f */
            if (rc == HG_OK) rc = job_launch(h, job, g, offs, f, 1, h->d_batch);
            if (rc == HG_OK && px) rc = hg_download_behind_warps(h->ctx, own ? outs[f] : base + offs[f], d_out + offs[f], px * 4);
            if (rc == HG_OK && (uint32_t)(f + 1) < n_img && f + 1 < F)                      /* ... and image f + 1 goes up meanwhile */
                rc = hg_upload_on_copy_stream(h->ctx, (uint8_t *)h->d_imgs + stride * (uint32_t)(f + 1), src[f + 1], bytes);
        }
        free(src);
        { const int rcd = hg_fence_downloads(h->ctx); if (rc == HG_OK) rc = rcd; }
    }
    const int rc2 = hg_sync(h->ctx);
    if (rc == HG_OK) rc = rc2;
    free(offs); free(outs);
    if (rc != HG_OK) return throw_hg(env, h->ctx, what, rc);
    return arr;
}

/* warpInversePiecewiseBatch(ctx, dstPoints F x 2N float32, geoms Int32Array F x 4 [, ownFrames, images, width, height]) */
static napi_value fn_warp_inverse_piecewise_batch(napi_env env, napi_callback_info info)
{
    napi_value a[7]; size_t argc = 7;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 3) return throw_str(env, "hgwarp: wrong number of arguments");
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t nd, ng; batch_job job = { JOB_PW_INV, 0, NULL, NULL, NULL, NULL, 0, 0, 0 };
    job.dst = (const float *)get_typed(env, a[1], napi_float32_array, &nd, "dstPoints"); if (!job.dst) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[2], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (h->n_pts == 0 || nd < (size_t)F * 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold frames x mesh points x,y pairs (piecewiseSetMesh first)");
    return run_batch(env, h, &job, gv, F, 0, a + 3, argc - 3, "warpInversePiecewiseBatch");
}

/* warpInversePiecewiseSrcBatch(ctx, srcPoints F x 2N float32, minSrc Int32Array F x 2, dstPoints F x 2N float32, geoms Int32Array F x 4
 * [, ownFrames, images, width, height]): warpInversePiecewiseBatch for frames that bring their own source points and source minima
 * (hg_warp_inverse_piecewise_src_batch_device; triangles and point count are those of piecewiseSetMesh); same frames, pooling and {images} pipeline */
static napi_value fn_warp_inverse_piecewise_src_batch(napi_env env, napi_callback_info info)
{
    napi_value a[9]; size_t argc = 9;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 5) return throw_str(env, "hgwarp: wrong number of arguments");
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t ns, nm, nd, ng; batch_job job = { JOB_PW_INV_SRC, 0, NULL, NULL, NULL, NULL, 0, 0, 0, NULL, NULL };
    job.src = (const float *)get_typed(env, a[1], napi_float32_array, &ns, "srcPoints"); if (!job.src) return NULL;
    job.min_src = (const int32_t *)get_typed(env, a[2], napi_int32_array, &nm, "minSrc"); if (!job.min_src) return NULL;
    job.dst = (const float *)get_typed(env, a[3], napi_float32_array, &nd, "dstPoints"); if (!job.dst) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[4], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (h->n_pts == 0 || nd < (size_t)F * 2 * h->n_pts || ns < (size_t)F * 2 * h->n_pts)
        return throw_str(env, "hgwarp: srcPoints and dstPoints must hold frames x mesh points x,y pairs (piecewiseSetMesh first)");
    if (nm < (size_t)F * 2) return throw_str(env, "hgwarp: minSrc must hold 2 integers per frame");
    return run_batch(env, h, &job, gv, F, 0, a + 5, argc - 5, "warpInversePiecewiseSrcBatch");
}

/* warpInverseGeometricBatch(ctx, kind, from, to, geoms [, ownFrames, images, width, height]): from / to = F point sets each (3 or 4 points
 * x,y float32; the matrix of frame f maps from[f] -> to[f]: pass dst, src for the inverse warp, the solves run on the GPU like the
 * reference's :994 runs per warp) */
static napi_value fn_warp_inverse_geometric_batch(napi_env env, napi_callback_info info)
{
    napi_value a[9]; size_t argc = 9;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 5) return throw_str(env, "hgwarp: wrong number of arguments");
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t nf, nt, ng; batch_job job = { JOB_GEO_INV, 0, NULL, NULL, NULL, NULL, 0, 0, 0 };
    if (!get_i32(env, a[1], &job.kind)) return NULL;
    if (job.kind != HG_AFFINE && job.kind != HG_PROJECTIVE) return throw_str(env, "hgwarp: kind must be 0 (affine) or 1 (projective)");
    job.from = (const float *)get_typed(env, a[2], napi_float32_array, &nf, "fromPoints"); if (!job.from) return NULL;
    job.to = (const float *)get_typed(env, a[3], napi_float32_array, &nt, "toPoints"); if (!job.to) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[4], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    job.per = job.kind == HG_AFFINE ? 6 : 8;
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (nf < (size_t)F * job.per || nt < (size_t)F * job.per) return throw_str(env, "hgwarp: point sets must hold frames x points x,y pairs");
    return run_batch(env, h, &job, gv, F, 0, a + 5, argc - 5, "warpInverseGeometricBatch");
}

/* mosaicInverseGeometric(ctx, kind, from, to, geoms, mode, feather, canvas, wantWeight, W, H) /
 * mosaicInversePiecewise(ctx, dstPoints, geoms, mode, feather, canvas, wantWeight, W, H): the inverse batch of warpInverseGeometricBatch /
 * warpInversePiecewiseBatch (the bound source(s): setImage / setImages) blended into ONE picture on the device.  The set is staged and warped
 * into device scratch, its coords fields are exported beside it, hg_sync settles both, hg_mosaic_frames_device (mode: HG_MOSAIC_*; W x H: the
 * source's size) blends them over `canvas` (Int32Array x, y, width, height) and only the canvas comes down: { data: Uint8ClampedArray
 * [, weight: Float32Array] }.
 * One more argument, `exposure`, equalises the frames' exposures first (hg_mosaic_frames_gain_device): a Float32Array of one gain per frame
 * is applied as given; a Float64Array [sigmaN, sigmaG] has the gains fitted on the overlaps -- hg_mosaic_overlap_stats_device, 16 F^2 bytes
 * down, hg_mosaic_solve_gains on the host -- and the frames still never leave the device.  The result then carries gains: Float32Array.
 * mosaicMultibandInverseGeometric(ctx, kind, from, to, geoms, bands, feather, canvas, wantWeight, W, H, wantLabels [, exposure]) /
 * mosaicMultibandInversePiecewise(ctx, dstPoints, geoms, bands, feather, canvas, wantWeight, W, H, wantLabels [, exposure]): the same with
 * hg_mosaic_multiband_device as the blend (`bands` in the place of the mode, feather ranks the frames).  The work area is allocated for the
 * call and freed behind it; with wantLabels the result carries labels: Int32Array, the owner of every canvas pixel or -1.
 * mosaicRobustInverseGeometric(ctx, kind, from, to, geoms, mode, trim, canvas, wantWeight, W, H [, exposure]) /
 * mosaicRobustInversePiecewise(ctx, dstPoints, geoms, mode, trim, canvas, wantWeight, W, H [, exposure]): the plain mosaic's arguments with
 * hg_mosaic_robust_device as the blend (mode: HG_ROBUST_*, `trim` in the place of the feather; W and H are not read). */
static napi_value run_mosaic(napi_env env, handle_t *h, const batch_job *job, const int32_t *gv, int F, const napi_value *a, napi_value exposure, const char *what,
                             napi_value multiband_labels, int robust)
{
    const hg_geom *g = (const hg_geom *)gv;
    int mode, W, H; double feather; size_t nc; bool want_weight = false, want_labels = false;
    const int multiband = multiband_labels != NULL;         /* then a[0] is the band count */
    if (!get_i32(env, a[0], &mode)) return NULL;
    if (multiband && napi_get_value_bool(env, multiband_labels, &want_labels) != napi_ok) return throw_str(env, "hgwarp: wantLabels must be a boolean");
    if (napi_get_value_double(env, a[1], &feather) != napi_ok) return throw_str(env, robust ? "hgwarp: trim must be a number" : "hgwarp: feather must be a number");
    const int32_t *cv = (const int32_t *)get_typed(env, a[2], napi_int32_array, &nc, "canvas"); if (!cv) return NULL;
    if (nc != 4) return throw_str(env, "hgwarp: canvas must hold x, y, width, height");
    if (napi_get_value_bool(env, a[3], &want_weight) != napi_ok) return throw_str(env, "hgwarp: wantWeight must be a boolean");
    if (!get_i32(env, a[4], &W) || !get_i32(env, a[5], &H)) return NULL;
    const hg_geom canvas = { cv[0], cv[1], cv[2], cv[3] };
    const size_t n = (canvas.obj_w > 0 && canvas.obj_h > 0) ? (size_t)canvas.obj_w * (size_t)canvas.obj_h : 0;
    int fit = 0; double sigma_n = 0.0, sigma_g = 0.0; void *gdata = NULL;      /* fit: the gains are solved for here */
    napi_value gains_out = NULL;
    if (exposure) {
        napi_typedarray_type tt; size_t len = 0; void *ed = NULL; bool is_ta = false;
        if (napi_is_typedarray(env, exposure, &is_ta) != napi_ok || !is_ta || napi_get_typedarray_info(env, exposure, &tt, &len, &ed, NULL, NULL) != napi_ok ||
            !((tt == napi_float32_array && len == (size_t)F) || (tt == napi_float64_array && len == 2)))
            return throw_str(env, "hgwarp: exposure must be a Float32Array of one gain per frame or a Float64Array [sigmaN, sigmaG]");
        if (!(gains_out = make_typed(env, napi_float32_array, (size_t)F, 4, &gdata))) return NULL;
        if (tt == napi_float64_array) { fit = 1; sigma_n = ((const double *)ed)[0]; sigma_g = ((const double *)ed)[1]; for (int f = 0; f < F; f++) ((float *)gdata)[f] = 1.0f; }
        else memcpy(gdata, ed, sizeof(float) * (size_t)F);
    }
    void *data = NULL, *wdata = NULL, *ldata = NULL;
    napi_value result, pixels = make_typed(env, napi_uint8_clamped_array, n * 4, 1, &data), weights = NULL, labels = NULL;
    if (!pixels) return NULL;
    if (want_weight && !(weights = make_typed(env, napi_float32_array, n, 4, &wdata))) return NULL;
    if (want_labels && !(labels = make_typed(env, napi_int32_array, n, 4, &ldata))) return NULL;
    NAPI_OK(napi_create_object(env, &result));
    NAPI_OK(napi_set_named_property(env, result, "data", pixels));
    if (want_weight) NAPI_OK(napi_set_named_property(env, result, "weight", weights));
    if (exposure) NAPI_OK(napi_set_named_property(env, result, "gains", gains_out));
    if (want_labels) NAPI_OK(napi_set_named_property(env, result, "labels", labels));
    if (!n) return result;
    if (fit && F > 256) {                                   /* before anything is staged or warped: the library's own refusal, no pointer involved */
        int rc0 = hg_mosaic_overlap_stats_device(h->ctx, g, F, NULL, NULL, NULL, NULL, 4, canvas, NULL);
        return rc0 != HG_OK ? throw_hg(env, h->ctx, what, rc0) : throw_str(env, "hgwarp: exposure 'gain' takes at most 256 frames");
    }
    size_t *offs = (size_t *)malloc(sizeof(size_t) * 2 * (size_t)F);
    if (!offs) return throw_str(env, "hgwarp: out of memory (frame offsets)");
    size_t *foffs = offs + F, total = 0, ftotal = 0;
    hg_pack_offsets(g, F, offs, &total);
    int rc = hg_pack_field_offsets(g, F, HG_FIELD_COORDS, foffs, &ftotal);
    if (rc == HG_OK && total > h->d_batch_cap) {
        if (h->d_batch) hg_device_free(h->ctx, h->d_batch);
        h->d_batch = NULL; h->d_batch_cap = 0;
        rc = hg_device_alloc(h->ctx, total, &h->d_batch);
        if (rc == HG_OK) h->d_batch_cap = total;
    }
    /* the statistics lie behind the weights (8-byte aligned: the parts before them are multiples of 256, 256 and 8) */
    const size_t cb = (n * 4 + 255) & ~(size_t)255, wb = want_weight ? ((n * 4 + 7) & ~(size_t)7) : 0;
    const size_t sb = fit ? (size_t)F * (size_t)F * 16 : 0, need = ftotal + cb + wb + sb;
    if (rc == HG_OK && need > h->d_remap_cap) {
        if (h->d_remap) hg_device_free(h->ctx, h->d_remap);
        h->d_remap = NULL; h->d_remap_cap = 0;
        rc = hg_device_alloc(h->ctx, need, &h->d_remap);
        if (rc == HG_OK) h->d_remap_cap = need;
    }
    uint8_t *d_field = (uint8_t *)h->d_remap, *d_canvas = d_field + ftotal;
    float *d_weight = want_weight ? (float *)(d_canvas + cb) : NULL;
    if (rc == HG_OK) rc = job_launch(h, job, g, offs, 0, F, h->d_batch);
    if (rc == HG_OK) rc = job->type == JOB_PW_INV ? hg_field_inverse_piecewise_frames_device(h->ctx, HG_FIELD_COORDS, foffs, d_field)
                                                  : hg_field_inverse_geometric_frames_device(h->ctx, HG_FIELD_COORDS, foffs, d_field);
    if (rc == HG_OK) rc = hg_sync(h->ctx);
    int host_rc = HG_OK;                                    /* a refusal of the host solve: its text is not the context's */
    if (rc == HG_OK && fit) {
        uint64_t *d_stats = (uint64_t *)(d_canvas + cb + wb), *stats = (uint64_t *)malloc(sb);
        rc = hg_mosaic_overlap_stats_device(h->ctx, g, F, d_field, foffs, h->d_batch, offs, 4, canvas, d_stats);
        if (rc == HG_OK && !stats) { free(offs); return throw_str(env, "hgwarp: out of memory (overlap statistics)"); }
        if (rc == HG_OK) rc = hg_copy_to_host(h->ctx, stats, d_stats, sb);
        if (rc == HG_OK) rc = host_rc = hg_mosaic_solve_gains(stats, F, 4, sigma_n, sigma_g, (float *)gdata);
        free(stats);
    }
    void *d_mb = NULL;                                      /* a multi-band blend: the labels, then the work area; this call's own */
    if (rc == HG_OK && multiband) {
        size_t work = 0;
        const size_t lb = want_labels ? ((n * 4 + 255) & ~(size_t)255) : 0;
        rc = host_rc = hg_mosaic_multiband_layout(g, F, canvas, 4, mode, &work);
        if (rc == HG_OK) { host_rc = HG_OK; rc = hg_device_alloc(h->ctx, lb + work + 256, &d_mb); }
        if (rc == HG_OK) rc = hg_mosaic_multiband_device(h->ctx, g, F, d_field, foffs, h->d_batch, offs, HG_ELEM_U8, 4, W, H, (float)feather, mode, canvas, d_canvas,
                                                         d_weight, want_labels ? (int32_t *)d_mb : NULL, exposure ? (const float *)gdata : NULL,
                                                         (uint8_t *)d_mb + lb, work);
        if (rc == HG_OK && want_labels) rc = hg_copy_to_host(h->ctx, ldata, d_mb, n * 4);
    } else if (rc == HG_OK && robust)
        rc = hg_mosaic_robust_device(h->ctx, g, F, d_field, foffs, h->d_batch, offs, 4, mode, (float)feather, exposure ? (const float *)gdata : NULL, canvas, d_canvas,
                                     d_weight);
    else if (rc == HG_OK)
        rc = hg_mosaic_frames_gain_device(h->ctx, g, F, d_field, foffs, h->d_batch, offs, HG_ELEM_U8, 4, W, H, mode, (float)feather, canvas, d_canvas, d_weight,
                                          exposure ? (const float *)gdata : NULL);
    if (rc == HG_OK) rc = hg_copy_to_host(h->ctx, data, d_canvas, n * 4);
    if (rc == HG_OK && want_weight) rc = hg_copy_to_host(h->ctx, wdata, d_weight, n * 4);
    if (d_mb) { if (rc != HG_OK) hg_sync(h->ctx); hg_device_free(h->ctx, d_mb); }
    free(offs);
    if (rc != HG_OK) return throw_hg(env, host_rc != HG_OK ? NULL : h->ctx, what, rc);
    return result;
}

static napi_value mosaic_inverse_geometric(napi_env env, napi_callback_info info, int multiband, int robust)
{
    napi_value a[13]; int have_exposure = 0;
    if (!get_args_opt(env, info, 11 + (size_t)multiband, a, &have_exposure)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t nf, nt, ng; batch_job job = { JOB_GEO_INV, 0, NULL, NULL, NULL, NULL, 0, 0, 0 };
    if (!get_i32(env, a[1], &job.kind)) return NULL;
    if (job.kind != HG_AFFINE && job.kind != HG_PROJECTIVE) return throw_str(env, "hgwarp: kind must be 0 (affine) or 1 (projective)");
    job.from = (const float *)get_typed(env, a[2], napi_float32_array, &nf, "fromPoints"); if (!job.from) return NULL;
    job.to = (const float *)get_typed(env, a[3], napi_float32_array, &nt, "toPoints"); if (!job.to) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[4], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    job.per = job.kind == HG_AFFINE ? 6 : 8;
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (nf < (size_t)F * job.per || nt < (size_t)F * job.per) return throw_str(env, "hgwarp: point sets must hold frames x points x,y pairs");
    return run_mosaic(env, h, &job, gv, F, a + 5, have_exposure ? a[11 + multiband] : NULL, multiband ? "mosaicMultibandInverseGeometric" : robust ? "mosaicRobustInverseGeometric" : "mosaicInverseGeometric",
                      multiband ? a[11] : NULL, robust);
}
static napi_value fn_mosaic_inverse_geometric(napi_env env, napi_callback_info info) { return mosaic_inverse_geometric(env, info, 0, 0); }
static napi_value fn_mosaic_robust_inverse_geometric(napi_env env, napi_callback_info info) { return mosaic_inverse_geometric(env, info, 0, 1); }
static napi_value fn_mosaic_multiband_inverse_geometric(napi_env env, napi_callback_info info) { return mosaic_inverse_geometric(env, info, 1, 0); }

static napi_value mosaic_inverse_piecewise(napi_env env, napi_callback_info info, int multiband, int robust)
{
    napi_value a[11]; int have_exposure = 0;
    if (!get_args_opt(env, info, 9 + (size_t)multiband, a, &have_exposure)) return NULL;
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t nd, ng; batch_job job = { JOB_PW_INV, 0, NULL, NULL, NULL, NULL, 0, 0, 0 };
    job.dst = (const float *)get_typed(env, a[1], napi_float32_array, &nd, "dstPoints"); if (!job.dst) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[2], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (h->n_pts == 0 || nd < (size_t)F * 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold frames x mesh points x,y pairs (piecewiseSetMesh first)");
    return run_mosaic(env, h, &job, gv, F, a + 3, have_exposure ? a[9 + multiband] : NULL, multiband ? "mosaicMultibandInversePiecewise" : robust ? "mosaicRobustInversePiecewise" : "mosaicInversePiecewise",
                      multiband ? a[9] : NULL, robust);
}
static napi_value fn_mosaic_inverse_piecewise(napi_env env, napi_callback_info info) { return mosaic_inverse_piecewise(env, info, 0, 0); }
static napi_value fn_mosaic_robust_inverse_piecewise(napi_env env, napi_callback_info info) { return mosaic_inverse_piecewise(env, info, 0, 1); }
static napi_value fn_mosaic_multiband_inverse_piecewise(napi_env env, napi_callback_info info) { return mosaic_inverse_piecewise(env, info, 1, 0); }

/* warpForwardPiecewiseBatch(ctx, dstPoints, maxSrcX, maxSrcY, geoms [, ownFrames, images, width, height]): the frames warp() sends down the
 * FORWARD piecewise path (:421-422: output not larger than the input and at least input / 1.2) */
static napi_value fn_warp_forward_piecewise_batch(napi_env env, napi_callback_info info)
{
    napi_value a[9]; size_t argc = 9;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 5) return throw_str(env, "hgwarp: wrong number of arguments");
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t nd, ng; batch_job job = { JOB_PW_FWD, 0, NULL, NULL, NULL, NULL, 0, 0, 0 };
    job.dst = (const float *)get_typed(env, a[1], napi_float32_array, &nd, "dstPoints"); if (!job.dst) return NULL;
    if (!get_i32(env, a[2], &job.mx) || !get_i32(env, a[3], &job.my)) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[4], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (h->n_pts == 0 || nd < (size_t)F * 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold frames x mesh points x,y pairs (piecewiseSetMesh first)");
    return run_batch(env, h, &job, gv, F, 1, a + 5, argc - 5, "warpForwardPiecewiseBatch");
}

/* warpForwardGeometricBatch(ctx, kind, mats Float64Array F x 8 (the FORWARD matrices, 6 used), geoms [, ownFrames, images, width, height]): the
 * affine frames warp() sends forward (:426-427: output of the source's size) */
static napi_value fn_warp_forward_geometric_batch(napi_env env, napi_callback_info info)
{
    napi_value a[8]; size_t argc = 8;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 4) return throw_str(env, "hgwarp: wrong number of arguments");
    handle_t *h = get_handle(env, a[0]); if (!h) return NULL;
    size_t nm, ng; batch_job job = { JOB_GEO_FWD, 0, NULL, NULL, NULL, NULL, 0, 0, 0 };
    if (!get_i32(env, a[1], &job.kind)) return NULL;
    if (job.kind != HG_AFFINE && job.kind != HG_PROJECTIVE) return throw_str(env, "hgwarp: kind must be 0 (affine) or 1 (projective)");
    job.m = (const double *)get_typed(env, a[2], napi_float64_array, &nm, "matrices"); if (!job.m) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[3], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (nm < (size_t)F * 8) return throw_str(env, "hgwarp: matrices must hold 8 doubles per frame");
    return run_batch(env, h, &job, gv, F, 1, a + 4, argc - 4, "warpForwardGeometricBatch");
}

/* ---------------------------------------------------------------- several GPUs (hg_multi_*) */
typedef struct { hg_multi *m; size_t n_pts; } mhandle_t;

static void mhandle_finalize(napi_env env, void *data, void *hint)
{
    (void)env; (void)hint;
    mhandle_t *h = (mhandle_t *)data;
    if (h) { if (h->m) hg_multi_destroy(h->m); free(h); }
}

static mhandle_t *get_mhandle(napi_env env, napi_value v)
{
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((mhandle_t *)p)->m) { throw_str(env, "hgwarp: invalid or destroyed multi-device handle"); return NULL; }
    return (mhandle_t *)p;
}

static napi_value throw_multi(napi_env env, hg_multi *m, const char *what, int code)
{
    char buf[512];
    snprintf(buf, sizeof buf, "hgwarp %s failed (%d): %s", what, code, hg_multi_last_error(m));
    return throw_str(env, buf);
}

static napi_value fn_multi_create(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    size_t n;
    int32_t *ids = (int32_t *)get_typed(env, a[0], napi_int32_array, &n, "devices"); if (!ids) return NULL;
    if (n == 0) return throw_str(env, "hgwarp: multiCreate needs at least one device id");
    mhandle_t *h = (mhandle_t *)calloc(1, sizeof *h);
    int rc = hg_multi_create((const int *)ids, (int)n, &h->m);
    if (rc != HG_OK) { free(h); return throw_multi(env, NULL, "hg_multi_create", rc); }
    napi_value ext;
    NAPI_OK(napi_create_external(env, h, mhandle_finalize, NULL, &ext));
    return ext;
}

static napi_value fn_multi_destroy(napi_env env, napi_callback_info info)
{
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    void *p = NULL;
    if (napi_get_value_external(env, a[0], &p) == napi_ok && p && ((mhandle_t *)p)->m) { hg_multi_destroy(((mhandle_t *)p)->m); ((mhandle_t *)p)->m = NULL; }
    return NULL;
}

static napi_value fn_multi_set_sampling(napi_env env, napi_callback_info info)
{
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    mhandle_t *h = get_mhandle(env, a[0]); if (!h) return NULL;
    int mode;
    if (!get_i32(env, a[1], &mode)) return NULL;
    int rc = hg_multi_set_sampling(h->m, mode);
    if (rc != HG_OK) return throw_multi(env, h->m, "hg_multi_set_sampling", rc);
    return NULL;
}

static napi_value fn_multi_set_image(napi_env env, napi_callback_info info)
{
    napi_value a[4];
    if (!get_args(env, info, 4, a)) return NULL;
    mhandle_t *h = get_mhandle(env, a[0]); if (!h) return NULL;
    size_t n; int w, hh;
    uint8_t *px = (uint8_t *)get_typed(env, a[1], napi_uint8_clamped_array, &n, "image.data"); if (!px) return NULL;
    if (!get_i32(env, a[2], &w) || !get_i32(env, a[3], &hh)) return NULL;
    if (w <= 0 || hh <= 0 || n < (size_t)w * (size_t)hh * 4) return throw_str(env, "hgwarp: image.data is smaller than width*height*4");
    int rc = hg_multi_set_image(h->m, px, w, hh);
    if (rc != HG_OK) return throw_multi(env, h->m, "hg_multi_set_image", rc);
    return NULL;
}

static napi_value fn_multi_set_mesh(napi_env env, napi_callback_info info)
{
    napi_value a[5];
    if (!get_args(env, info, 5, a)) return NULL;
    mhandle_t *h = get_mhandle(env, a[0]); if (!h) return NULL;
    size_t np, nt; int msx, msy;
    float *src = (float *)get_typed(env, a[1], napi_float32_array, &np, "srcPoints"); if (!src) return NULL;
    uint32_t *tris = (uint32_t *)get_typed(env, a[2], napi_uint32_array, &nt, "triangles"); if (!tris) return NULL;
    if (!get_i32(env, a[3], &msx) || !get_i32(env, a[4], &msy)) return NULL;
    int rc = hg_multi_piecewise_set_mesh(h->m, src, (int)(np / 2), tris, (int)(nt / 3), msx, msy);
    if (rc != HG_OK) return throw_multi(env, h->m, "hg_multi_piecewise_set_mesh", rc);
    h->n_pts = np / 2;
    return NULL;
}

/* Optional per-frame sources of a multi-device batch: a JS array of n Uint8ClampedArray (width*height*4 each) -> F host pointers,
 * frame f reads images[f % n] (the rule of setImages).  Returns 1 with *out = NULL when `v` is undefined / null (shared source). */
static int get_frame_images(napi_env env, napi_value v, napi_value vw, napi_value vh, int F, const uint8_t ***out, int *w, int *hh)
{
    *out = NULL;
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return 0;
    if (t == napi_undefined || t == napi_null) return 1;
    bool is_arr = false; uint32_t n = 0;
    if (napi_is_array(env, v, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, v, &n) != napi_ok || n == 0) {
        throw_str(env, "hgwarp: images must be a non-empty array of image data arrays"); return 0;
    }
    if (!get_i32(env, vw, w) || !get_i32(env, vh, hh)) return 0;
    if (*w <= 0 || *hh <= 0) { throw_str(env, "hgwarp: bad image size"); return 0; }
    const size_t bytes = (size_t)*w * (size_t)*hh * 4;
    const uint8_t **ptrs = (const uint8_t **)calloc((size_t)F, sizeof *ptrs);
    if (!ptrs) { throw_str(env, "hgwarp: out of memory"); return 0; }
    for (int f = 0; f < F; f++) {
        napi_value el; size_t len;
        if (napi_get_element(env, v, (uint32_t)f % n, &el) != napi_ok) { free(ptrs); throw_str(env, "hgwarp: N-API call failed"); return 0; }
        const uint8_t *px = (const uint8_t *)get_typed(env, el, napi_uint8_clamped_array, &len, "images[k]");
        if (!px) { free(ptrs); return 0; }
        if (len < bytes) { free(ptrs); throw_str(env, "hgwarp: an image is smaller than width*height*4"); return 0; }
        ptrs[f] = px;
    }
    *out = ptrs;
    return 1;
}

/* warpBatch over the device list: dst = F x 2N float32, geoms = Int32Array F x 4 [, images, width, height: one source per frame,
 * every device uploads its own block]; returns an Array of F Uint8ClampedArray
 * (pooled pinned memory where possible, so that the D2H copies of different devices run at the same time). */
static napi_value fn_multi_warp_batch(napi_env env, napi_callback_info info)
{
    napi_value a[6];
    size_t argc = 6;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 3) return throw_str(env, "hgwarp: multiWarpBatch(multi, dstPoints, geoms[, images, width, height])");
    mhandle_t *h = get_mhandle(env, a[0]); if (!h) return NULL;
    size_t nd, ng;
    float *dst = (float *)get_typed(env, a[1], napi_float32_array, &nd, "dstPoints"); if (!dst) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[2], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (h->n_pts == 0 || nd < (size_t)F * 2 * h->n_pts) return throw_str(env, "hgwarp: dstPoints must hold frames x mesh points x,y pairs (multiSetMesh first)");
    napi_value arr;
    NAPI_OK(napi_create_array_with_length(env, F, &arr));
    uint8_t **outs = (uint8_t **)calloc((size_t)F, sizeof *outs);
    uint8_t dummy = 0;
    for (int f = 0; f < F; f++) {
        const hg_geom *g = (const hg_geom *)gv + f;
        const size_t px = (g->obj_w > 0 && g->obj_h > 0) ? (size_t)g->obj_w * g->obj_h : 0;
        void *out = NULL; napi_value ta = make_pixels(env, px * 4, NULL, 0, &out);
        if (!ta) { free(outs); return NULL; }
        outs[f] = px ? (uint8_t *)out : &dummy;
        napi_set_element(env, arr, f, ta);
    }
    const uint8_t **imgs = NULL; int iw = 0, ih = 0;
    if (argc >= 6 && !get_frame_images(env, a[3], a[4], a[5], F, &imgs, &iw, &ih)) { free(outs); return NULL; }
    int rc = imgs ? hg_multi_warp_piecewise_batch_images(h->m, dst, (const hg_geom *)gv, F, imgs, iw, ih, outs)
                  : hg_multi_warp_piecewise_batch(h->m, dst, (const hg_geom *)gv, F, outs);
    free(outs); free(imgs);
    if (rc != HG_OK) return throw_multi(env, h->m, imgs ? "hg_multi_warp_piecewise_batch_images" : "hg_multi_warp_piecewise_batch", rc);
    return arr;
}

static napi_value fn_multi_warp_geometric_batch(napi_env env, napi_callback_info info)
{
    napi_value a[8];
    size_t argc = 8;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 5) return throw_str(env, "hgwarp: multiWarpGeometricBatch(multi, kind, from, to, geoms[, images, width, height])");
    mhandle_t *h = get_mhandle(env, a[0]); if (!h) return NULL;
    int kind; size_t nf, nt, ng;
    if (!get_i32(env, a[1], &kind)) return NULL;
    if (kind != HG_AFFINE && kind != HG_PROJECTIVE) return throw_str(env, "hgwarp: kind must be 0 (affine) or 1 (projective)");
    float *from = (float *)get_typed(env, a[2], napi_float32_array, &nf, "fromPoints"); if (!from) return NULL;
    float *to = (float *)get_typed(env, a[3], napi_float32_array, &nt, "toPoints"); if (!to) return NULL;
    int32_t *gv = (int32_t *)get_typed(env, a[4], napi_int32_array, &ng, "geoms"); if (!gv) return NULL;
    const int F = (int)(ng / 4);
    const size_t per = kind == HG_AFFINE ? 6 : 8;
    if (F <= 0) return throw_str(env, "hgwarp: geoms must hold 4 integers per frame");
    if (nf < (size_t)F * per || nt < (size_t)F * per) return throw_str(env, "hgwarp: point sets must hold frames x points x,y pairs");
    napi_value arr;
    NAPI_OK(napi_create_array_with_length(env, F, &arr));
    uint8_t **outs = (uint8_t **)calloc((size_t)F, sizeof *outs);
    uint8_t dummy = 0;
    for (int f = 0; f < F; f++) {
        const hg_geom *g = (const hg_geom *)gv + f;
        const size_t px = (g->obj_w > 0 && g->obj_h > 0) ? (size_t)g->obj_w * g->obj_h : 0;
        void *out = NULL; napi_value ta = make_pixels(env, px * 4, NULL, 0, &out);
        if (!ta) { free(outs); return NULL; }
        outs[f] = px ? (uint8_t *)out : &dummy;
        napi_set_element(env, arr, f, ta);
    }
    const uint8_t **imgs = NULL; int iw = 0, ih = 0;
    if (argc >= 8 && !get_frame_images(env, a[5], a[6], a[7], F, &imgs, &iw, &ih)) { free(outs); return NULL; }
    int rc = imgs ? hg_multi_warp_geometric_batch_images(h->m, kind, from, to, (const hg_geom *)gv, F, imgs, iw, ih, outs)
                  : hg_multi_warp_geometric_batch(h->m, kind, from, to, (const hg_geom *)gv, F, outs);
    free(outs); free(imgs);
    if (rc != HG_OK) return throw_multi(env, h->m, imgs ? "hg_multi_warp_geometric_batch_images" : "hg_multi_warp_geometric_batch", rc);
    return arr;
}

/* ---------------------------------------------------------------- module */
static void pool_free(napi_env env, void *data, void *hint)
{
    (void)env; (void)hint;
    pool_t *P = (pool_t *)data;
    if (!P) return;
    /* the env is gone and every ArrayBuffer with it: the buffers go back to the driver */
    for (int i = 0; i < P->npins; i++) if (P->pins[i].ptr) { if (P->pool_malloc) free(P->pins[i].ptr); else hg_host_free(P->pins[i].ptr); }
    free(P);
}

static napi_value init(napi_env env, napi_value exports)
{
    pool_t *P = (pool_t *)calloc(1, sizeof *P);
    if (!P) return NULL;
    P->pin_limit = (size_t)2 << 30;
    const napi_node_version *nv = NULL;
    P->early_reuse = (napi_get_node_version(env, &nv) == napi_ok && nv && nv->major <= 12) ? 1 : 0;
    if (getenv("HGWARP_POOL_NO_EARLY_REUSE")) P->early_reuse = 0;           /* (tests: the V8 >= 8 life cycle under Node 12) */
    if (napi_set_instance_data(env, P, pool_free, NULL) != napi_ok) { free(P); return NULL; }
    static const struct { const char *name; napi_callback fn; } fns[] = {
        { "create", fn_create }, { "destroy", fn_destroy }, { "deviceCount", fn_device_count },
        { "solveAffine", fn_solve_affine }, { "invertAffine", fn_invert_affine }, { "solveProjective", fn_solve_projective },
        { "transformLimits", fn_transform_limits }, { "minmaxXY", fn_minmax_xy }, { "triangulate", fn_triangulate },
        { "setImage", fn_set_image }, { "setImages", fn_set_images }, { "warpInverseGeometric", fn_warp_inverse_geometric },
        { "piecewiseSetMesh", fn_piecewise_set_mesh }, { "piecewisePrepare", fn_piecewise_prepare },
        { "warpInversePiecewise", fn_warp_inverse_piecewise }, { "getTriMap", fn_get_tri_map }, { "getMatrices", fn_get_matrices },
        { "warpInversePiecewiseBatch", fn_warp_inverse_piecewise_batch }, { "warpInversePiecewiseSrcBatch", fn_warp_inverse_piecewise_src_batch }, { "warpInverseGeometricBatch", fn_warp_inverse_geometric_batch },
        { "warpForwardGeometric", fn_warp_forward_geometric }, { "warpForwardPiecewise", fn_warp_forward_piecewise },
        { "warpForwardPiecewiseBatch", fn_warp_forward_piecewise_batch }, { "warpForwardGeometricBatch", fn_warp_forward_geometric_batch },
        { "releaseBatch", fn_release_batch }, { "pinnedBuffer", fn_pinned_buffer },
        { "fieldInverseGeometric", fn_field_inverse_geometric }, { "fieldInversePiecewise", fn_field_inverse_piecewise },
        { "fieldForwardGeometric", fn_field_forward_geometric }, { "fieldForwardPiecewise", fn_field_forward_piecewise },
        { "remapInverseGeometric", fn_remap_inverse_geometric }, { "remapInversePiecewise", fn_remap_inverse_piecewise },
        { "remapForwardGeometric", fn_remap_forward_geometric }, { "remapForwardPiecewise", fn_remap_forward_piecewise },
        { "remapTrilinearInverseGeometric", fn_remap_trilinear_inverse_geometric }, { "remapTrilinearInversePiecewise", fn_remap_trilinear_inverse_piecewise },
        { "remapAnisoInverseGeometric", fn_remap_aniso_inverse_geometric }, { "remapAnisoInversePiecewise", fn_remap_aniso_inverse_piecewise },
        { "remapBicubicInverseGeometric", fn_remap_bicubic_inverse_geometric }, { "remapBicubicInversePiecewise", fn_remap_bicubic_inverse_piecewise },
        { "mosaicInverseGeometric", fn_mosaic_inverse_geometric }, { "mosaicInversePiecewise", fn_mosaic_inverse_piecewise },
        { "mosaicMultibandInverseGeometric", fn_mosaic_multiband_inverse_geometric }, { "mosaicMultibandInversePiecewise", fn_mosaic_multiband_inverse_piecewise },
        { "mosaicRobustInverseGeometric", fn_mosaic_robust_inverse_geometric }, { "mosaicRobustInversePiecewise", fn_mosaic_robust_inverse_piecewise },
        { "pointsInverseGeometric", fn_points_inverse_geometric }, { "pointsInversePiecewise", fn_points_inverse_piecewise },
        { "pointsForwardGeometric", fn_points_forward_geometric }, { "pointsForwardPiecewise", fn_points_forward_piecewise },
        { "fitMatches", fn_fit_matches },
        { "alignBegin", fn_align_begin }, { "alignLevel", fn_align_level }, { "alignScaleMatrix", fn_align_scale_matrix }, { "alignEnd", fn_align_end },
        { "bundleAdjust", fn_bundle_adjust }, { "bundleChain", fn_bundle_chain }, { "bundleInvert", fn_bundle_invert },
        { "warpThinPlate", fn_warp_thin_plate },
        { "cameraPackRecord", fn_camera_pack_record }, { "cameraLimits", fn_camera_limits }, { "cameraFocals", fn_camera_focals },
        { "cameraRotation", fn_camera_rotation }, { "warpCamera", fn_warp_camera },
        { "denseFlow", fn_dense_flow },
        { "matchDescriptors", fn_match_descriptors },
        { "detectAndDescribe", fn_detect_describe },
        { "solveAffineTriangles", fn_solve_affine_triangles }, { "warpInversePiecewiseState", fn_warp_inverse_piecewise_state },
        { "warpForwardPiecewiseState", fn_warp_forward_piecewise_state },
        { "release", fn_release }, { "setPinnedLimit", fn_set_pinned_limit }, { "poolStats", fn_pool_stats }, { "redoneFrames", fn_redone_frames }, { "spanCacheStats", fn_span_cache_stats }, { "setSampling", fn_set_sampling }, { "multiSetSampling", fn_multi_set_sampling }, { "_poolTestFrames", fn_pool_test_frames }, { "poolPressure", fn_pool_pressure }, { "poolCollected", fn_pool_collected },
        { "multiCreate", fn_multi_create }, { "multiDestroy", fn_multi_destroy }, { "multiSetImage", fn_multi_set_image },
        { "multiSetMesh", fn_multi_set_mesh }, { "multiWarpBatch", fn_multi_warp_batch }, { "multiWarpGeometricBatch", fn_multi_warp_geometric_batch },
    };
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
        if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
    }
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
