// common.h — shared host/device helpers for libmri3d_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <algorithm>
#include <initializer_list>
#include "../../include/mri3d.h"

namespace mri3d {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return MRI3D_ELAUNCH;
    }
    return MRI3D_OK;
}

#define MRI3D_REQUIRE(cond, code, ...)      \
    do {                                    \
        if (!(cond)) {                      \
            ::mri3d::set_error(__VA_ARGS__); \
            return (code);                  \
        }                                   \
    } while (0)

// A/B switches exist only in a tuning build (-DMRI3D_TUNING, tools/): the shipped library reads no environment variable, so a
// stray variable in a job's environment cannot change which kernel runs or what it computes.
#ifdef MRI3D_TUNING
inline int tuning_knob(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
#else
constexpr int tuning_knob(const char*, int dflt) { return dflt; }
#endif

inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Cap for grid-stride streaming kernels: 256 CUs x 8 blocks (cdna_hip_programming.md Guideline 11).
constexpr int kMaxStreamBlocks = 2048;

inline int stream_grid(int64_t work_items, int per_block) {
    int64_t b = cdiv64(work_items, per_block);
    if (b > kMaxStreamBlocks) b = kMaxStreamBlocks;
    if (b < 1) b = 1;
    return (int)b;
}

// ---------------------------------------------------------------- storage types
// Activations are stored as float (MRI3D_F32) or bfloat16 (MRI3D_BF16, BASELINE configs[3]); arithmetic, statistics,
// parameters and parameter gradients are always fp32.  gfx950 converts with v_cvt_pk_bf16_f32 (round-to-nearest-even).
typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;

template <typename T> __device__ __forceinline__ float ldf(const T* p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void stf(T* p, float v) { *p = (T)v; }

// 4 consecutive elements; p must be aligned to 4 elements (16 B for float, 8 B for bf16)
__device__ __forceinline__ float4 ldf4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ldf4(const bf16_t* p) {
    const bf16x4_t v = *reinterpret_cast<const bf16x4_t*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ void stf4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void stf4(bf16_t* p, float4 v) {
    bf16x4_t o;
    o[0] = (bf16_t)v.x, o[1] = (bf16_t)v.y, o[2] = (bf16_t)v.z, o[3] = (bf16_t)v.w;
    *reinterpret_cast<bf16x4_t*>(p) = o;
}

inline size_t dtype_size(int dtype) { return dtype == MRI3D_BF16 ? 2 : 4; }
// all pointers aligned for 4-element vector access in the given storage type
inline bool aligned_vec4(int dtype, const void* a, const void* b = nullptr, const void* c = nullptr) {
    const uintptr_t m = dtype == MRI3D_BF16 ? 7 : 15;
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & m) == 0;
}

// every given pointer 16-byte aligned (dwordx4 accesses, LDS-DMA pieces)
inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

// the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte (a null pointer overlaps nothing)
inline bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
    if (!a || !b) return false;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + bbytes && pb < pa + abytes;
}

// largest power of two <= 16 that divides every given address (a null pointer divides by everything): what the route query is
// told about a tensor instead of its pointer
inline int ptr_align(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
                           reinterpret_cast<uintptr_t>(d) | 16;
    return (int)(bits & (~bits + 1));
}
// aligned_vec4 / aligned16 of a tensor known by its ptr_align
inline bool align_vec4(int dtype, int align) { return align >= (dtype == MRI3D_BF16 ? 8 : 16); }
inline bool align16(int align) { return align >= 16; }

// Run `body` with `T` bound to the storage type of `dtype`.
#define MRI3D_DISPATCH_DTYPE(dtype, T, ...)  \
    do {                                     \
        if ((dtype) == MRI3D_BF16) {         \
            using T = ::mri3d::bf16_t;       \
            __VA_ARGS__                      \
        } else {                             \
            using T = float;                 \
            __VA_ARGS__                      \
        }                                    \
    } while (0)

// ---------------------------------------------------------------- pooling plans shared by resample.hip and norm.hip
// slab kernels: a block walks (n, depth, h-chunk) slabs of about 2048 (w, channel-vector) elements times hch rows
inline void slab_plan(int nd, int h, int w, int cv, int& hch, int& grid) {
    int64_t per_row = (int64_t)w * cv;
    hch = (int)std::max<int64_t>(1, std::min<int64_t>(h, 2048 / std::max<int64_t>(per_row, 1)));
    int64_t slabs = (int64_t)nd * ((h + hch - 1) / hch);
    grid = (int)std::min<int64_t>(slabs, 8192);
}

// MaxPool3d(2) on even extents, one sample below 2^31 elements: what the line-contiguous pool kernels serve
inline bool pool2_ok(const Mri3dPoolGeom& g, int vec) {
    const int cv = g.c / vec;
    return g.kd == 2 && g.kh == 2 && g.kw == 2 && g.sd == 2 && g.sh == 2 && g.sw == 2 && g.pd == 0 && g.ph == 0 && g.pw == 0 &&
           g.di == 2 * g.dout && g.hi == 2 * g.ho && g.wi == 2 * g.wo && cv >= 1 && cv <= 32 && (cv & (cv - 1)) == 0 &&
           (int64_t)g.di * g.hi * g.wi * g.x_ld < ((int64_t)1 << 31);
}

// channels per lane of a pooling pass: 8 (bf16 only: 16-byte accesses), 4 or 1.  A vector needs the channels and every pitch in
// whole vectors, every tensor (aligns: their ptr_align) aligned to one, and the index bytes (align_idx) to one byte per channel.
inline int pool_vec(int dtype, int c, std::initializer_list<int> pitches, std::initializer_list<int> aligns, int align_idx) {
    int lds = c, align = 16;
    for (int ld : pitches) lds |= ld;   // (a | b) % 2^k == 0 exactly when both are
    for (int a : aligns) align = std::min(align, a);
    if (lds % 4 != 0 || !align_vec4(dtype, align) || align_idx < 4) return 1;
    return dtype == MRI3D_BF16 && lds % 8 == 0 && align16(align) && align_idx >= 8 ? 8 : 4;
}

// forward of a pool: its vector width, whether the line-contiguous MaxPool3d(2) kernels serve it (lanes then walk input columns),
// and the slab plan that goes with the two
struct PoolFwdLanes { int vec; bool lines; int hch, grid; };
inline PoolFwdLanes pool_fwd_lanes(const Mri3dPoolGeom& g, std::initializer_list<int> pitches, std::initializer_list<int> aligns,
                                   int align_idx) {
    PoolFwdLanes p;
    p.vec = pool_vec(g.dtype, g.c, pitches, aligns, align_idx);
    p.lines = p.vec >= 4 && pool2_ok(g, p.vec);
    slab_plan(g.n * g.dout, g.ho, p.lines ? g.wi : g.wo, g.c / p.vec, p.hch, p.grid);
    return p;
}

// a workspace of 8-byte elements (double or 64-bit integer partials): present, large enough and 8-byte aligned
inline int ws_check8(const char* who, const void* workspace, size_t ws_bytes, size_t need) {
    MRI3D_REQUIRE(workspace && ws_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MRI3D_EWORKSPACE,
                  "%s: workspace %zu < %zu, or not 8-byte aligned", who, ws_bytes, need);
    return MRI3D_OK;
}

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float apply_act(float v, int act, float slope) {
    // act: MRI3D_ACT_*; for PReLU the caller passes alpha as `slope`.
    if (act == MRI3D_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == MRI3D_ACT_LEAKY || act == MRI3D_ACT_PRELU) return v > 0.f ? v : v * slope;
    return v;
}

}  // namespace mri3d
