// loss_index.h — what the class-map losses share: loss.hip (softmax-Dice) and ce_loss.hip (cross-entropy / focal, alone or fused
// with that Dice).  The device helpers stand here word for word as loss.hip had them: its kernels' code generation is sensitive to
// how they are written (tests/golden/loss_family_bits.json records their bits), so change nothing here without recomputing it.
#pragma once
#include "common.h"
#include <math.h>
#include <algorithm>

namespace mri3d {

constexpr int kIdxMinC = 2, kIdxMaxC = 32;
// blocks of one forward launch over all samples: the cap fixes the summation order
constexpr int kIdxMaxBlocks = 2048;

// A lane's sums of classes [0, C) -> the block's row part[n][blk = blockIdx.x][c][3] = (tp, sum_p, sum_g): wave shuffles, then the
// four waves through LDS (red, the kernel's) in a fixed order.  sum_g is a double sum (float target) or a count added as integers
// (class map).  The kernels' code is sensitive to how this tail is written (the 32-class forward's register allocation follows
// it): n, red and the two spellings of the sum_g reduction keep every forward kernel's loop as it was compiled before the two
// forms shared this function.
template <int K, typename G>
__device__ __forceinline__ void dice_block_row(const double (&tp)[K], const double (&sp)[K], const G (&sg)[K], int C, int n,
                                               double (&red)[4][K * 3], double* __restrict__ part) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < C) {
            const double a = wave_sum_d(tp[j]), b = wave_sum_d(sp[j]);
            G c = sg[j];
            if constexpr (sizeof(G) == sizeof(double)) {
                c = wave_sum_d(c);
            } else {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
            }
            if (lane == 0) { red[wave][j * 3] = a; red[wave][j * 3 + 1] = b; red[wave][j * 3 + 2] = (double)c; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < C * 3) {
        const double s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        part[((size_t)n * gridDim.x + blockIdx.x) * C * 3 + threadIdx.x] = s;
    }
}

// d(1 - dice_c)/dp_c(v) = -(2 g den - 2 tp)/den^2 scaled by dloss/(N*C) = ka * g + kb, from the (tp, sum_p, sum_g) of one (n, c)
__device__ __forceinline__ void dice_coeffs(const float* __restrict__ st, float scale, float eps, float& ka, float& kb) {
    const float tp = st[0], sp = st[1], sg = st[2];
    const float den = sp + sg + eps;
    ka = -2.f * scale / den;              // multiplies g
    kb = 2.f * scale * tp / (den * den);  // constant term
}

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

// ------------------------------------------------------------------ grid rules of the class-map kernels (host)
// forward: a lane takes about 4 items, and all samples together at most `cap` blocks
static int dice_fwd_blocks(int64_t items, int n, int cap) {
    const int64_t want = cdiv64(items, 256 * 4);
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, cap / n));
}

// backward: one item per lane up to the stream cap, and at most 4096 blocks over all samples
static int dice_bwd_blocks(int64_t items, int n) {
    int64_t b = stream_grid(items, 256);
    if (b * n > 4096) b = std::max(4096 / n, 1);
    return (int)b;
}

}  // namespace mri3d
