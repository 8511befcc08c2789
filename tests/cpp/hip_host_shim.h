// hip_host_shim.h -- what a host program needs to compile the remap family's kernel files (homography.js_amd/csrc/hg_k_remap.hip,
// hg_k_pyramid.hip, hg_k_aniso.hip, hg_k_mosaic.hip -- the files themselves, with -I homography.js_amd/csrc) with a plain C++ compiler: the
// HIP qualifiers as nothing, the thread indices as variables a check sets before every call of a kernel, and the few HIP types and
// conversions the kernels use.  Include it before the kernel files; their launchers are compiled under hipcc only.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct dim3s { unsigned x, y, z; };
static thread_local dim3s threadIdx, blockIdx, gridDim;
struct uint2 { uint32_t x, y; }; struct uint4 { uint32_t x, y, z, w; }; struct float2 { float x, y; };
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return {a, b}; }
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
static inline float2 make_float2(float a, float b) { return {a, b}; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
using std::min; using std::max;
