// labels.hip — label maps on the device: raw label volume -> uint8 class map (id remap through a lookup table), and every exact
// count of two uint8 maps: the five overlap sums of two masks and the C x C confusion counts of two class maps.  (The softmax-Dice
// loss against a class map is in loss.hip, beside the float-target form.)
// Reference: prepare_batch (segmentation/routine.py:185-196), validate_dsc_asd's Dice / IoU (routine.py:198-235, metrics.py:312-329).
//
// HBM-bound streaming passes.  Algorithmic bytes per voxel:
//   remap                  sizeof(in) + sizeof(out); the table (<= 64 KiB) stays in the caches and is read through them
//   overlap / confusion    2
#include "common.h"
#include <math.h>
#include <algorithm>

namespace mri3d {

// ------------------------------------------------------------------ id remap
struct RemapRule {
    const uint8_t* lut;
    int lut_len;
    uint8_t above, other;
};

__device__ __forceinline__ uint8_t remap_int(int v, const RemapRule& r) {
    return v < 0 ? r.other : v >= r.lut_len ? r.above : r.lut[v];
}
__device__ __forceinline__ uint8_t remap_one(uint8_t v, const RemapRule& r) { return remap_int(v, r); }
__device__ __forceinline__ uint8_t remap_one(int16_t v, const RemapRule& r) { return remap_int(v, r); }
__device__ __forceinline__ uint8_t remap_one(int32_t v, const RemapRule& r) { return remap_int(v, r); }
__device__ __forceinline__ uint8_t remap_one(float v, const RemapRule& r) {
    if (v >= (float)r.lut_len) return r.above;                 // lut_len <= 65536 is exact in float; +inf counts, NaN does not
    if (v >= 0.f && truncf(v) == v) return r.lut[(int)v];      // -0.0 is the integer 0
    return r.other;
}

// V elements of TO in one store of up to 16 bytes, or several of 16; p is aligned to min(16, V * sizeof(TO))
template <typename TO, int V> __device__ __forceinline__ void remap_store(TO* p, const TO (&e)[V]) {
    constexpr int B = V * (int)sizeof(TO);
    if constexpr (B >= 16) {
        uint4 w[B / 16];
        __builtin_memcpy(w, e, B);
#pragma unroll
        for (int k = 0; k < B / 16; ++k) reinterpret_cast<uint4*>(p)[k] = w[k];
    } else if constexpr (B == 8) {
        uint2 w;
        __builtin_memcpy(&w, e, 8);
        *reinterpret_cast<uint2*>(p) = w;
    } else {
        static_assert(B == 4, "a whole dword");
        uint32_t w;
        __builtin_memcpy(&w, e, 4);
        *reinterpret_cast<uint32_t*>(p) = w;
    }
}

constexpr int kRemapLoads = 4;   // 16-byte loads a lane has in flight

// Elements [head, head + nvec * V) go V = 16 / sizeof(TI) at a time (in + head is 16-byte aligned, out + head aligned for
// remap_store); the head elements in front and the ragged rest behind go one at a time in the same launch.  A lane writes only
// what it has read, after reading it, so out == in of the same type is in place.  No __restrict__: in and out may be one buffer.
template <typename TI, typename TO>
__global__ void __launch_bounds__(256)
label_remap_kernel(const TI* in, TO* out, int64_t n, int64_t head, int64_t nvec, RemapRule r) {
    constexpr int V = 16 / (int)sizeof(TI), U = kRemapLoads;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    const uint4* in16 = reinterpret_cast<const uint4*>(in + head);
    TO* outv = out + head;
    for (int64_t i0 = tid; i0 < nvec; i0 += nth * U) {
        uint4 raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i0 + u * nth < nvec) raw[u] = in16[i0 + u * nth];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * nth;
            if (i < nvec) {
                TI e[V];
                TO o[V];
                __builtin_memcpy(e, &raw[u], 16);
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = (TO)remap_one(e[k], r);
                remap_store<TO, V>(outv + i * V, o);
            }
        }
    }
    const int64_t body = nvec * V, singles = n - body;
    for (int64_t i = tid; i < singles; i += nth) {
        const int64_t k = i < head ? i : body + i;
        out[k] = (TO)remap_one(in[k], r);
    }
}

// ------------------------------------------------------------------ exact counts of two uint8 maps
// All counts are integers, so any order of addition is exact.  One pass over the two maps (16 voxels per lane per load), the
// blocks' partial counts to the workspace, then one small kernel that adds them: only the counts leave the device.
//
// Mask overlap: validate_dsc_asd scores the arg-max mask against the label map (segmentation/routine.py:198-235,
// metrics.py:312-329): Dice = 2*sum(gt & pred) / (sum(gt) + sum(pred)), IoU = #(pred>0 and gt>0) / #(pred>0 or gt>0).
//   out[0] = sum(gt)  out[1] = sum(pred)  out[2] = sum(gt & pred)  out[3] = #(gt>0 & pred>0)  out[4] = #(gt>0 | pred>0)
// Confusion: key of a voxel = gt * C + pred, or C * C when either is no class; out[key] = #voxels.
constexpr int kConfMinC = 2, kConfMaxC = 32;
constexpr int kConfRegBlocks = 512;    // five counters in registers, 256 lanes: mask overlap, and confusion at C == 2
constexpr int kConfLdsBlocks = 256;    // C >= 3: bins in LDS, 1024 lanes sharing them
constexpr int kConfMaxBins = kConfMaxC * kConfMaxC + 1;

struct ConfSpan {   // [head, head + nvec * 16) in 16-byte loads (pred + head and gt + head aligned), the rest byte by byte
    int64_t head, nvec;
};

// the two accumulate steps of counts5_kernel
__device__ __forceinline__ void ovl_acc(unsigned g, unsigned p, unsigned long long (&c)[5]) {
    c[0] += g;
    c[1] += p;
    c[2] += g & p;
    c[3] += (g != 0u && p != 0u) ? 1u : 0u;
    c[4] += (g != 0u || p != 0u) ? 1u : 0u;
}
__device__ __forceinline__ void conf2_acc(unsigned g, unsigned p, unsigned long long (&c)[5]) {
    const unsigned key = (g > 1u || p > 1u) ? 4u : g * 2u + p;
#pragma unroll
    for (unsigned k = 0; k < 5; ++k) c[k] += key == k ? 1u : 0u;
}

// F(g, p) for every voxel this lane owns: 16 per load over the aligned span, single bytes elsewhere
template <typename F>
__device__ __forceinline__ void conf_walk(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t n, ConfSpan s,
                                          F&& f) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    const uint4* p4 = reinterpret_cast<const uint4*>(pred + s.head);
    const uint4* g4 = reinterpret_cast<const uint4*>(gt + s.head);
    for (int64_t i = tid; i < s.nvec; i += nth) {
        const uint4 pv = p4[i], gv = g4[i];
        const unsigned pw[4] = {pv.x, pv.y, pv.z, pv.w}, gw[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int b = 0; b < 4; ++b) f((gw[w] >> (8 * b)) & 0xffu, (pw[w] >> (8 * b)) & 0xffu);
    }
    const int64_t body = s.nvec * 16, singles = n - body;
    for (int64_t i = tid; i < singles; i += nth) {
        const int64_t k = i < s.head ? i : body + i;
        f((unsigned)gt[k], (unsigned)pred[k]);
    }
}

// five counters per lane -> part[blk][5]: wave shuffles, then the four waves through LDS
template <void (*Acc)(unsigned, unsigned, unsigned long long (&)[5])>
__global__ void __launch_bounds__(256)
counts5_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t n, ConfSpan s,
               unsigned long long* __restrict__ part) {
    __shared__ unsigned long long red[4][5];
    unsigned long long c[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    conf_walk(pred, gt, n, s, [&](unsigned g, unsigned p) { Acc(g, p, c); });
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        unsigned long long v = c[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 5)
        part[(size_t)blockIdx.x * 5 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// A lane adds a run of equal keys to its bin at once: in a label map neighbouring voxels mostly agree, so the 64 lanes of a wave
// meet at one LDS address once per run instead of once per voxel.
__global__ void __launch_bounds__(1024)
confusion_lds_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t n, ConfSpan s, int C,
                     unsigned long long* __restrict__ part) {
    __shared__ unsigned long long bins[kConfMaxBins];
    const int nb = C * C + 1;
    for (int k = threadIdx.x; k < nb; k += blockDim.x) bins[k] = 0ull;
    __syncthreads();
    unsigned prev = 0u, run = 0u;
    const unsigned uc = (unsigned)C;
    conf_walk(pred, gt, n, s, [&](unsigned g, unsigned p) {
        const unsigned key = (g >= uc || p >= uc) ? uc * uc : g * uc + p;
        if (key != prev && run != 0u) {
            atomicAdd(&bins[prev], (unsigned long long)run);
            run = 0u;
        }
        prev = key;
        ++run;
    });
    if (run != 0u) atomicAdd(&bins[prev], (unsigned long long)run);
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += blockDim.x) part[(size_t)blockIdx.x * nb + k] = bins[k];
}

__global__ void __launch_bounds__(256)
confusion_finalize_kernel(const unsigned long long* __restrict__ part, int nblk, int nb, int64_t* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    unsigned long long s = 0ull;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * nb + k];
    out[k] = (int64_t)s;
}

// the longest span of 16-byte loads that two byte arrays of n elements allow: none unless they are misaligned alike
static ConfSpan conf_span(const void* a, const void* b, int64_t n) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    ConfSpan s = {n, 0};
    const int64_t head = (int64_t)((16 - (pa & 15)) & 15);
    if (((pa ^ pb) & 15) == 0 && head <= n) {
        s.head = head;
        s.nvec = (n - head) / 16;
    }
    return s;
}

// counts5_kernel<Acc> over the two maps, then its five sums to counts
template <void (*Acc)(unsigned, unsigned, unsigned long long (&)[5])>
static void launch_counts5(const uint8_t* pred, const uint8_t* gt, int64_t nvox, int64_t* counts, void* workspace, hipStream_t s) {
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    const int nblk = (int)std::min<int64_t>(kConfRegBlocks, cdiv64(nvox, 256 * 16));
    hipLaunchKernelGGL(counts5_kernel<Acc>, dim3(nblk), dim3(256), 0, s, pred, gt, nvox, conf_span(pred, gt, nvox), part);
    hipLaunchKernelGGL(confusion_finalize_kernel, dim3(1), dim3(256), 0, s, part, nblk, 5, counts);
}

}  // namespace mri3d

using namespace mri3d;

static size_t label_size(int dtype) { return dtype == MRI3D_LABEL_U8 ? 1 : dtype == MRI3D_LABEL_I16 ? 2 : 4; }

extern "C" int mri3d_label_remap(const void* in, int32_t in_dtype, void* out, int32_t out_dtype, int64_t n, const uint8_t* lut,
                                 int32_t lut_len, int32_t above, int32_t other, mri3d_stream_t stream) {
    MRI3D_REQUIRE(in_dtype >= MRI3D_LABEL_U8 && in_dtype <= MRI3D_LABEL_F32, MRI3D_ENOTSUP, "label_remap: unknown input dtype %d",
                  in_dtype);
    MRI3D_REQUIRE(out_dtype == MRI3D_LABEL_U8 || out_dtype == MRI3D_LABEL_F32, MRI3D_ENOTSUP,
                  "label_remap: output dtype %d is neither uint8 nor float32", out_dtype);
    MRI3D_REQUIRE(in && out && lut, MRI3D_EINVAL, "label_remap: null pointer");
    MRI3D_REQUIRE(n > 0, MRI3D_EINVAL, "label_remap: n = %lld", (long long)n);
    MRI3D_REQUIRE(lut_len >= 1 && lut_len <= 65536, MRI3D_EINVAL, "label_remap: lut_len %d outside 1..65536", lut_len);
    MRI3D_REQUIRE(above >= 0 && above <= 255 && other >= 0 && other <= 255, MRI3D_EINVAL,
                  "label_remap: above %d / other %d outside 0..255", above, other);
    const size_t isz = label_size(in_dtype), osz = label_size(out_dtype);
    const uintptr_t pi = reinterpret_cast<uintptr_t>(in), po = reinterpret_cast<uintptr_t>(out);
    MRI3D_REQUIRE(pi % isz == 0 && po % osz == 0, MRI3D_EINVAL, "label_remap: a pointer is not aligned to its element");
    MRI3D_REQUIRE((in == out && in_dtype == out_dtype) || !overlaps(in, (size_t)n * isz, out, (size_t)n * osz), MRI3D_EINVAL,
                  "label_remap: output overlaps the input (only out == in of the same type is in place)");
    MRI3D_REQUIRE(!overlaps(lut, (size_t)lut_len, out, (size_t)n * osz), MRI3D_EINVAL, "label_remap: output overlaps the table");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the vector span: from the first 16-byte aligned input element, if the output is aligned for its stores there
    const int64_t v = 16 / (int64_t)isz;
    int64_t head = (int64_t)((16 - (pi & 15)) & 15) / (int64_t)isz, nvec = 0;
    const uintptr_t ostore = std::min<uintptr_t>(16, (uintptr_t)v * osz);
    if (head <= n && (po + (uintptr_t)head * osz) % ostore == 0) nvec = (n - head) / v;
    else head = n;
    if (nvec == 0) head = n;
    const RemapRule r = {lut, lut_len, (uint8_t)above, (uint8_t)other};
    const int grid = stream_grid(std::max<int64_t>(cdiv64(nvec, kRemapLoads), n - nvec * v), 256);
#define REMAP_OUT(TI)                                                                                                         \
    do {                                                                                                                      \
        if (out_dtype == MRI3D_LABEL_U8)                                                                                      \
            hipLaunchKernelGGL((label_remap_kernel<TI, uint8_t>), dim3(grid), dim3(256), 0, s, (const TI*)in, (uint8_t*)out, \
                               n, head, nvec, r);                                                                             \
        else                                                                                                                  \
            hipLaunchKernelGGL((label_remap_kernel<TI, float>), dim3(grid), dim3(256), 0, s, (const TI*)in, (float*)out, n,  \
                               head, nvec, r);                                                                                \
    } while (0)
    switch (in_dtype) {
        case MRI3D_LABEL_U8: REMAP_OUT(uint8_t); break;
        case MRI3D_LABEL_I16: REMAP_OUT(int16_t); break;
        case MRI3D_LABEL_I32: REMAP_OUT(int32_t); break;
        default: REMAP_OUT(float); break;
    }
#undef REMAP_OUT
    return check_launch("label_remap");
}

extern "C" size_t mri3d_mask_overlap_workspace_bytes(void) { return (size_t)kConfRegBlocks * 5 * sizeof(unsigned long long); }

extern "C" int mri3d_mask_overlap(const uint8_t* pred, const uint8_t* gt, int64_t nvox, int64_t* counts, void* workspace,
                                  size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(pred && gt && counts && nvox > 0, MRI3D_EINVAL, "mask_overlap: bad arguments");
    int rc = ws_check8("mask_overlap", workspace, ws_bytes, mri3d_mask_overlap_workspace_bytes());
    if (rc) return rc;
    launch_counts5<ovl_acc>(pred, gt, nvox, counts, workspace, static_cast<hipStream_t>(stream));
    return check_launch("mask_overlap");
}

extern "C" size_t mri3d_confusion_workspace_bytes(int32_t c) {
    if (c < kConfMinC || c > kConfMaxC) return 0;
    return (size_t)(c == 2 ? kConfRegBlocks : kConfLdsBlocks) * (size_t)(c * c + 1) * sizeof(unsigned long long);
}

extern "C" int mri3d_confusion_counts(const uint8_t* pred, const uint8_t* gt, int64_t nvox, int32_t c, int64_t* counts,
                                      void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(c >= kConfMinC && c <= kConfMaxC, MRI3D_ENOTSUP, "confusion_counts: classes must be in [%d,%d], got %d", kConfMinC,
                  kConfMaxC, c);
    MRI3D_REQUIRE(pred && gt && counts, MRI3D_EINVAL, "confusion_counts: null pointer");
    MRI3D_REQUIRE(nvox > 0, MRI3D_EINVAL, "confusion_counts: nvox = %lld", (long long)nvox);
    MRI3D_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, MRI3D_EINVAL, "confusion_counts: counts is not 8-byte aligned");
    int rc = ws_check8("confusion_counts", workspace, ws_bytes, mri3d_confusion_workspace_bytes(c));
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c == 2) {
        launch_counts5<conf2_acc>(pred, gt, nvox, counts, workspace, s);
    } else {
        unsigned long long* part = static_cast<unsigned long long*>(workspace);
        const int nb = c * c + 1;
        const int nblk = (int)std::min<int64_t>(kConfLdsBlocks, cdiv64(nvox, 1024 * 16));
        hipLaunchKernelGGL(confusion_lds_kernel, dim3(nblk), dim3(1024), 0, s, pred, gt, nvox, conf_span(pred, gt, nvox), c, part);
        hipLaunchKernelGGL(confusion_finalize_kernel, dim3(cdiv(nb, 256)), dim3(256), 0, s, part, nblk, nb, counts);
    }
    return check_launch("confusion_counts");
}
