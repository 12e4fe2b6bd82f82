// labels.hip — the label path on the device: raw label volume -> uint8 class map (id remap through a lookup table), the
// softmax-Dice loss against that class map for 2..32 classes, and exact C x C confusion counts of two class maps.
// Reference: prepare_batch (segmentation/routine.py:185-196), F.softmax + get_dice_loss + .mean() (routine.py:239-253, 272-274),
// validate_dsc_asd's Dice / IoU (routine.py:198-235, metrics.py:312-329).
//
// All three are HBM-bound streaming passes.  Algorithmic bytes per voxel:
//   remap        sizeof(in) + sizeof(out); the table (<= 64 KiB) stays in the caches and is read through them
//   index Dice   forward C * esz + 1;  backward 2 * C * esz + 1      (the float one-hot form: + 4 * C instead of + 1)
//   confusion    2
#include "common.h"
#include <math.h>

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

// ------------------------------------------------------------------ softmax-Dice against a class map
constexpr int kIdxMinC = 2, kIdxMaxC = 32;
constexpr int kIdxMaxBlocks = 2048;
// how a lane reads its logits: one element at a time; a voxel's classes in 4-element vectors (c, x_ld multiples of 4, aligned
// base); or, for two dense classes, 4 voxels = 8 logits per lane (16-byte aligned logits, 4-byte aligned labels)
enum { kIdxScalar = 0, kIdxRows4 = 1, kIdxVox4 = 2 };

// One instantiation per class bucket CB in {2, 4, 8, 16, 32}, serving CB/2 < C <= CB (C == 2: CB = 2).  Classes C..CB-1 read as
// -inf: their probability is exactly 0, and adding 0 leaves every float sum as the C-class computation has it.
template <typename T, int CB>
__device__ __forceinline__ void idx_load_row(const T* p, int C, int mode, float (&z)[CB]) {
    if constexpr (CB >= 4) {
        if (mode == kIdxRows4) {
#pragma unroll
            for (int j = 0; j < CB; j += 4) {
                float4 t = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                if (j < C) t = ldf4(p + j);
                z[j] = t.x, z[j + 1] = t.y, z[j + 2] = t.z, z[j + 3] = t.w;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) z[j] = j < C ? ldf(p + j) : -INFINITY;
}

// z -> softmax(z) in place; the arithmetic of softmax_c (loss.hip)
template <int CB> __device__ __forceinline__ void idx_softmax(float (&z)[CB]) {
    float m = z[0];
#pragma unroll
    for (int j = 1; j < CB; ++j) m = fmaxf(m, z[j]);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CB; ++j) { z[j] = expf(z[j] - m); s += z[j]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int j = 0; j < CB; ++j) z[j] *= inv;
}

// 8 consecutive elements (4 voxels of 2 classes), p 16-byte (bf16) / 32-byte (fp32) aligned
__device__ __forceinline__ void idx_ld8(const float* p, float (&r)[8]) {
    const float4 a = ldf4(p), b = ldf4(p + 4);
    r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w, r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w;
}
__device__ __forceinline__ void idx_ld8(const bf16_t* p, float (&r)[8]) {
    const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (float)v[k];
}
__device__ __forceinline__ void idx_st8(float* p, const float (&r)[8]) {
    stf4(p, make_float4(r[0], r[1], r[2], r[3]));
    stf4(p + 4, make_float4(r[4], r[5], r[6], r[7]));
}
__device__ __forceinline__ void idx_st8(bf16_t* p, const float (&r)[8]) {
    bf16x8_t o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (bf16_t)r[k];
    *reinterpret_cast<bf16x8_t*>(p) = o;
}

// The voxels of sample n as work items of the 4-voxel path: `head` single voxels up to the first one whose index in the whole
// batch is a multiple of 4 (there logits and labels are aligned), `groups` groups of 4, then the rest as single voxels.
struct IdxVox4Plan {
    int64_t head, groups, items;
    __device__ __forceinline__ IdxVox4Plan(int64_t n, int64_t vox) {
        head = (4 - ((n * vox) & 3)) & 3;
        if (head > vox) head = vox;
        groups = (vox - head) >> 2;
        items = groups + (vox - groups * 4);
    }
    // item i >= groups is a single voxel: which one
    __device__ __forceinline__ int64_t single(int64_t i) const {
        const int64_t s = i - groups;
        return s < head ? s : groups * 4 + s;
    }
};

// tp and sum_p of a lane in double (torch's CPU reductions, the oracle's arithmetic, accumulate float sums in double); sum_g is a
// count.  tp only receives p[label]: a select per class, no indexed registers.
template <int CB> struct IdxAcc {
    double tp[CB], sp[CB];
    unsigned sg[CB];
    __device__ __forceinline__ void add(const float (&p)[CB], unsigned lab) {
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            const bool hit = lab == (unsigned)j;
            tp[j] += (double)(hit ? p[j] : 0.f);
            sp[j] += (double)p[j];
            sg[j] += hit ? 1u : 0u;
        }
    }
};

// part[n][blk][c][3] = (tp, sum_p, sum_g), the layout dice_fwd_kernel (loss.hip) leaves and dice_finalize (common.h) reads
template <typename T, int CB>
__global__ void __launch_bounds__(256)
dice_index_fwd_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ labels, double* __restrict__ part, int64_t vox,
                      int C, int x_ld, int mode) {
    __shared__ double red[4][CB * 3];
    const int n = blockIdx.y;
    const T* zn = logits + (int64_t)n * vox * x_ld;
    const uint8_t* ln = labels + (int64_t)n * vox;
    IdxAcc<CB> a;
#pragma unroll
    for (int j = 0; j < CB; ++j) { a.tp[j] = 0.0; a.sp[j] = 0.0; a.sg[j] = 0u; }
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    if (CB == 2 && mode == kIdxVox4) {
        if constexpr (CB == 2) {
            const IdxVox4Plan plan(n, vox);
            for (int64_t i = tid; i < plan.items; i += nth) {
                if (i < plan.groups) {
                    const int64_t v0 = plan.head + i * 4;
                    float z[8];
                    idx_ld8(zn + v0 * 2, z);
                    const uint32_t lw = *reinterpret_cast<const uint32_t*>(ln + v0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float p[2] = {z[2 * k], z[2 * k + 1]};
                        idx_softmax<2>(p);
                        a.add(p, (lw >> (8 * k)) & 0xffu);
                    }
                } else {
                    const int64_t v = plan.single(i);
                    float p[2] = {ldf(zn + v * 2), ldf(zn + v * 2 + 1)};
                    idx_softmax<2>(p);
                    a.add(p, ln[v]);
                }
            }
        }
    } else {
#pragma unroll 1
        for (int64_t v = tid; v < vox; v += nth) {
            float p[CB];
            idx_load_row<T, CB>(zn + v * x_ld, C, mode, p);
            idx_softmax<CB>(p);
            a.add(p, ln[v]);
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < CB; ++j) {
        if (j < C) {
            const double t = wave_sum_d(a.tp[j]), s = wave_sum_d(a.sp[j]);
            unsigned cnt = a.sg[j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
            if (lane == 0) { red[wave][j * 3] = t; red[wave][j * 3 + 1] = s; red[wave][j * 3 + 2] = (double)cnt; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < C * 3) {
        const double s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        part[((size_t)n * gridDim.x + blockIdx.x) * C * 3 + threadIdx.x] = s;
    }
}

// d(1 - dice_c)/dp_c(v) = -(2 g den - 2 tp)/den^2 scaled by dloss/(N*C), g = [label == c]: kb, plus ka where the label hits
// (dice_bwd_kernel's fmaf(ka, g, kb) at g = 1 and g = 0), then the softmax Jacobian
template <int CB>
__device__ __forceinline__ void idx_grad(float (&p)[CB], unsigned lab, const float (&ka)[CB], const float (&kb)[CB]) {
    float dp[CB], dot = 0.f;
#pragma unroll
    for (int j = 0; j < CB; ++j) {
        dp[j] = lab == (unsigned)j ? ka[j] + kb[j] : kb[j];
        dot = fmaf(p[j], dp[j], dot);
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) p[j] *= dp[j] - dot;
}

template <typename T, int CB>
__global__ void __launch_bounds__(256)
dice_index_bwd_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ labels, const float* __restrict__ stats,
                      const float* __restrict__ dloss, T* __restrict__ dlogits, int64_t vox, int N, int C, int x_ld, int mode,
                      float eps) {
    const int n = blockIdx.y;
    const T* zn = logits + (int64_t)n * vox * x_ld;
    const uint8_t* ln = labels + (int64_t)n * vox;
    T* dn = dlogits + (int64_t)n * vox * x_ld;
    // the two coefficients of every class, one class per lane, then to every lane's registers through LDS
    __shared__ float ska[CB], skb[CB];
    if (threadIdx.x < CB) {
        const int j = threadIdx.x;
        float a = 0.f, b = 0.f;        // a class >= C has p = 0 and takes no part
        if (j < C) {
            const float scale = dloss[0] / (float)(N * C);
            const float tp = stats[(n * C + j) * 3], sp = stats[(n * C + j) * 3 + 1], sg = stats[(n * C + j) * 3 + 2];
            const float den = sp + sg + eps;
            a = -2.f * scale / den;
            b = 2.f * scale * tp / (den * den);
        }
        ska[j] = a, skb[j] = b;
    }
    __syncthreads();
    float ka[CB], kb[CB];
#pragma unroll
    for (int j = 0; j < CB; ++j) ka[j] = ska[j], kb[j] = skb[j];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    if (CB == 2 && mode == kIdxVox4) {
        if constexpr (CB == 2) {
            const IdxVox4Plan plan(n, vox);
            for (int64_t i = tid; i < plan.items; i += nth) {
                if (i < plan.groups) {
                    const int64_t v0 = plan.head + i * 4;
                    float z[8];
                    idx_ld8(zn + v0 * 2, z);
                    const uint32_t lw = *reinterpret_cast<const uint32_t*>(ln + v0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float p[2] = {z[2 * k], z[2 * k + 1]};
                        idx_softmax<2>(p);
                        idx_grad<2>(p, (lw >> (8 * k)) & 0xffu, ka, kb);
                        z[2 * k] = p[0], z[2 * k + 1] = p[1];
                    }
                    idx_st8(dn + v0 * 2, z);
                } else {
                    const int64_t v = plan.single(i);
                    float p[2] = {ldf(zn + v * 2), ldf(zn + v * 2 + 1)};
                    idx_softmax<2>(p);
                    idx_grad<2>(p, ln[v], ka, kb);
                    stf(dn + v * 2, p[0]);
                    stf(dn + v * 2 + 1, p[1]);
                }
            }
        }
        return;
    }
#pragma unroll 1      // one voxel's CB registers at a time: unrolled, the 32-class body does not fit the register file
    for (int64_t v = tid; v < vox; v += nth) {
        float p[CB];
        idx_load_row<T, CB>(zn + v * x_ld, C, mode, p);
        idx_softmax<CB>(p);
        idx_grad<CB>(p, ln[v], ka, kb);
        T* d = dn + v * x_ld;
        bool stored = false;
        if constexpr (CB >= 4) {
            if (mode == kIdxRows4) {
#pragma unroll
                for (int j = 0; j < CB; j += 4)
                    if (j < C) stf4(d + j, make_float4(p[j], p[j + 1], p[j + 2], p[j + 3]));
                stored = true;
            }
        }
        if (!stored) {
#pragma unroll
            for (int j = 0; j < CB; ++j)
                if (j < C) stf(d + j, p[j]);
        }
    }
}

// ------------------------------------------------------------------ confusion counts
// key of a voxel: gt * C + pred, or C * C when either is no class.  Integer counts: any order of addition is exact.
constexpr int kConfRegBlocks = 512;    // C == 2: five counters in registers, 256 lanes (mask_overlap_kernel's shape)
constexpr int kConfLdsBlocks = 256;    // C >= 3: bins in LDS, 1024 lanes sharing them
constexpr int kConfMaxBins = kIdxMaxC * kIdxMaxC + 1;

struct ConfSpan {   // [head, head + nvec * 16) in 16-byte loads (pred + head and gt + head aligned), the rest byte by byte
    int64_t head, nvec;
};

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

__global__ void __launch_bounds__(256)
confusion2_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t n, ConfSpan s,
                  unsigned long long* __restrict__ part) {
    __shared__ unsigned long long red[4][5];
    unsigned long long c[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    conf_walk(pred, gt, n, s, [&](unsigned g, unsigned p) { conf2_acc(g, p, c); });
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

static int idx_blocks_fwd(const Mri3dDiceIndexGeom& g, int mode) {
    const int64_t items = mode == kIdxVox4 ? g.vox / 4 + 6 : g.vox;
    const int64_t want = cdiv64(items, 256 * 4);
    int cap = kIdxMaxBlocks / g.n;
    if (cap < 1) cap = 1;
    const int b = (int)(want < cap ? want : cap);
    return b < 1 ? 1 : b;
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

static int idx_check(const Mri3dDiceIndexGeom* g, const char* who) {
    MRI3D_REQUIRE(g != nullptr, MRI3D_EINVAL, "%s: null geometry", who);
    MRI3D_REQUIRE(g->dtype == MRI3D_F32 || g->dtype == MRI3D_BF16, MRI3D_ENOTSUP, "%s: unknown dtype %d", who, g->dtype);
    MRI3D_REQUIRE(g->n > 0 && g->vox > 0, MRI3D_EINVAL, "%s: empty tensor", who);
    MRI3D_REQUIRE(g->c >= kIdxMinC && g->c <= kIdxMaxC, MRI3D_ENOTSUP, "%s: classes must be in [%d,%d], got %d", who, kIdxMinC,
                  kIdxMaxC, g->c);
    MRI3D_REQUIRE(g->x_ld >= g->c, MRI3D_EINVAL, "%s: pitch %d < classes %d", who, g->x_ld, g->c);
    return MRI3D_OK;
}

static int idx_mode(const Mri3dDiceIndexGeom& g, const void* logits, const void* labels, const void* dlogits = nullptr) {
    if (g.c == 2 && g.x_ld == 2 && aligned16(logits, dlogits) && (reinterpret_cast<uintptr_t>(labels) & 3) == 0) return kIdxVox4;
    if (g.c % 4 == 0 && g.x_ld % 4 == 0 && aligned_vec4(g.dtype, logits, dlogits)) return kIdxRows4;
    return kIdxScalar;
}

#define IDX_DISPATCH(CALL)           \
    do {                             \
        if (g->c <= 2) CALL(2);      \
        else if (g->c <= 4) CALL(4); \
        else if (g->c <= 8) CALL(8); \
        else if (g->c <= 16) CALL(16); \
        else CALL(32);               \
    } while (0)

extern "C" size_t mri3d_softmax_dice_index_workspace_bytes(const Mri3dDiceIndexGeom* g) {
    if (!g || g->n <= 0 || g->c < kIdxMinC || g->c > kIdxMaxC) return 0;
    return ((size_t)kIdxMaxBlocks + (size_t)g->n) * g->c * 3 * sizeof(double);
}

extern "C" int mri3d_softmax_dice_index_fwd(const Mri3dDiceIndexGeom* g, const void* logits, const uint8_t* labels, float* loss,
                                            float* stats, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = idx_check(g, "softmax_dice_index_fwd");
    if (rc) return rc;
    MRI3D_REQUIRE(logits && labels && loss && stats, MRI3D_EINVAL, "softmax_dice_index_fwd: null pointer");
    MRI3D_REQUIRE(workspace && ws_bytes >= mri3d_softmax_dice_index_workspace_bytes(g) &&
                      (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                  MRI3D_EWORKSPACE, "softmax_dice_index_fwd: workspace %zu < %zu, or not 8-byte aligned", ws_bytes,
                  mri3d_softmax_dice_index_workspace_bytes(g));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int mode = idx_mode(*g, logits, labels);
    const int nblk = idx_blocks_fwd(*g, mode);
    double* part = static_cast<double*>(workspace);
#define CALL(CB)                                                                                                    \
    hipLaunchKernelGGL((dice_index_fwd_kernel<T, CB>), dim3(nblk, g->n), dim3(256), 0, s, (const T*)logits, labels, \
                       part, g->vox, g->c, g->x_ld, mode)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { IDX_DISPATCH(CALL); });
#undef CALL
    dice_finalize(part, stats, loss, g->n, g->c, nblk, g->eps, s);
    return check_launch("softmax_dice_index_fwd");
}

extern "C" int mri3d_softmax_dice_index_bwd(const Mri3dDiceIndexGeom* g, const void* logits, const uint8_t* labels,
                                            const float* stats, const float* dloss, void* dlogits, mri3d_stream_t stream) {
    int rc = idx_check(g, "softmax_dice_index_bwd");
    if (rc) return rc;
    MRI3D_REQUIRE(logits && labels && stats && dloss && dlogits, MRI3D_EINVAL, "softmax_dice_index_bwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int mode = idx_mode(*g, logits, labels, dlogits);
    int nblk = stream_grid(mode == kIdxVox4 ? g->vox / 4 + 6 : g->vox, 256);
    if ((int64_t)nblk * g->n > 4096) nblk = 4096 / g->n > 0 ? 4096 / g->n : 1;
#define CALL(CB)                                                                                                    \
    hipLaunchKernelGGL((dice_index_bwd_kernel<T, CB>), dim3(nblk, g->n), dim3(256), 0, s, (const T*)logits, labels, \
                       stats, dloss, (T*)dlogits, g->vox, g->n, g->c, g->x_ld, mode, g->eps)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { IDX_DISPATCH(CALL); });
#undef CALL
    return check_launch("softmax_dice_index_bwd");
}

extern "C" size_t mri3d_confusion_workspace_bytes(int32_t c) {
    if (c < kIdxMinC || c > kIdxMaxC) return 0;
    return (size_t)(c == 2 ? kConfRegBlocks : kConfLdsBlocks) * (size_t)(c * c + 1) * sizeof(unsigned long long);
}

extern "C" int mri3d_confusion_counts(const uint8_t* pred, const uint8_t* gt, int64_t nvox, int32_t c, int64_t* counts,
                                      void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(c >= kIdxMinC && c <= kIdxMaxC, MRI3D_ENOTSUP, "confusion_counts: classes must be in [%d,%d], got %d", kIdxMinC,
                  kIdxMaxC, c);
    MRI3D_REQUIRE(pred && gt && counts, MRI3D_EINVAL, "confusion_counts: null pointer");
    MRI3D_REQUIRE(nvox > 0, MRI3D_EINVAL, "confusion_counts: nvox = %lld", (long long)nvox);
    MRI3D_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, MRI3D_EINVAL, "confusion_counts: counts is not 8-byte aligned");
    MRI3D_REQUIRE(workspace && ws_bytes >= mri3d_confusion_workspace_bytes(c) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                  MRI3D_EWORKSPACE, "confusion_counts: workspace %zu < %zu, or not 8-byte aligned", ws_bytes,
                  mri3d_confusion_workspace_bytes(c));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ConfSpan span = conf_span(pred, gt, nvox);
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    const int nb = c * c + 1;
    int nblk;
    if (c == 2) {
        nblk = (int)std::min<int64_t>(kConfRegBlocks, cdiv64(nvox, 256 * 16));
        hipLaunchKernelGGL(confusion2_kernel, dim3(nblk), dim3(256), 0, s, pred, gt, nvox, span, part);
    } else {
        nblk = (int)std::min<int64_t>(kConfLdsBlocks, cdiv64(nvox, 1024 * 16));
        hipLaunchKernelGGL(confusion_lds_kernel, dim3(nblk), dim3(1024), 0, s, pred, gt, nvox, span, c, part);
    }
    hipLaunchKernelGGL(confusion_finalize_kernel, dim3(cdiv(nb, 256)), dim3(256), 0, s, part, nblk, nb, counts);
    return check_launch("confusion_counts");
}
