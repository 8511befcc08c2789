// hip_wave_shim.h -- what a host program needs beyond hip_host_shim.h to compile a kernel file whose lanes talk to each other (LDS, a
// barrier, a ballot, a shuffle): a block of 64 x 4 runs as 256 real threads.  __shared__ is static storage, __syncthreads a barrier over the
// block, and a ballot or a shuffle exchanges its values through one slot per lane between two barriers over the wave.  Include it after
// hip_host_shim.h and before the kernel files; wave_block_run starts the threads.  (tests/cpp/mosaic_gain_check.cpp carries the same
// construction in its own text.)
#pragma once
#include <pthread.h>
#include "hip_host_shim.h"

#define __shared__ static
static pthread_barrier_t g_block, g_wave[4];
static uint64_t g_slot[4][64];
static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
// every lane of the wave leaves its value, waits, reads what it needs, and waits again before the slots are reused
template <typename T, typename F> static inline T wave_exchange(T v, F pick)
{
    const unsigned w = threadIdx.y;
    uint64_t bits = 0;
    memcpy(&bits, &v, sizeof v);
    g_slot[w][threadIdx.x] = bits;
    pthread_barrier_wait(&g_wave[w]);
    const T r = pick(g_slot[w]);
    pthread_barrier_wait(&g_wave[w]);
    return r;
}
static inline uint64_t __ballot(int p)
{
    return wave_exchange<uint64_t>(p ? 1 : 0, [](const uint64_t *s) { uint64_t m = 0; for (int l = 0; l < 64; l++) m |= (s[l] & 1) << l; return m; });
}
template <typename T> static inline T __shfl(T v, int src) { return wave_exchange<T>(v, [=](const uint64_t *s) { T r; memcpy(&r, &s[src & 63], sizeof r); return r; }); }

// Runs body(block) for block = 0..n_blocks-1 on 256 threads, thread (x, y) with threadIdx = {x, y, 0} and blockIdx = {block, 0, 0}; the
// blocks run one after another (they share the static LDS).  False if a thread could not be started.
struct WaveRun { void (*body)(uint32_t, void *); void *arg; uint32_t n_blocks; unsigned tx, ty; };
static void *wave_lane_main(void *p)
{
    const WaveRun *r = (const WaveRun *)p;
    threadIdx = {r->tx, r->ty, 0};
    for (uint32_t b = 0; b < r->n_blocks; b++) {
        gridDim = {r->n_blocks, 1, 1}; blockIdx = {b, 0, 0};
        r->body(b, r->arg);
        pthread_barrier_wait(&g_block);                           // (the next block reuses the static LDS)
    }
    return nullptr;
}
static bool wave_block_run(uint32_t n_blocks, void (*body)(uint32_t, void *), void *arg)
{
    pthread_barrier_init(&g_block, nullptr, 256);
    for (int w = 0; w < 4; w++) pthread_barrier_init(&g_wave[w], nullptr, 64);
    std::vector<WaveRun> lanes(256);
    std::vector<pthread_t> th(256);
    pthread_attr_t at;
    pthread_attr_init(&at);
    pthread_attr_setstacksize(&at, 1 << 20);
    for (unsigned t = 0; t < 256; t++) {
        lanes[t] = WaveRun{body, arg, n_blocks, t % 64, t / 64};
        if (pthread_create(&th[t], &at, wave_lane_main, &lanes[t])) return false;      // (the started ones wait at a barrier: the caller exits)
    }
    for (unsigned t = 0; t < 256; t++) pthread_join(th[t], nullptr);
    pthread_attr_destroy(&at);
    pthread_barrier_destroy(&g_block);
    for (int w = 0; w < 4; w++) pthread_barrier_destroy(&g_wave[w]);
    return true;
}
