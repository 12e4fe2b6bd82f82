// loss_index.h — what the class-map losses are made of: loss.hip (softmax-Dice), ce_loss.hip (cross-entropy / focal, alone or
// fused with that Dice) and the boundary loss of distance.hip.  Every one of them reads softmax(logits) against a per-voxel target
// and is written as prologue + per-voxel body + epilogue around the pieces that stand here once:
//   device  idx_walk (the 4-voxel path with its head and tail singles, the row loop over idx_load_row and, in a backward, the
//           write-back through idx_store_row), dice_block_row / pair_block_row (a block's row of partials), dice_finalize_rows /
//           pair_finalize_sum (the single-block folds, every sum in a fixed order);
//   host    idx_check (the common head of the geometry checks), idx_plan (bucket, read mode, blocks, lanes, items, trips: the six
//           launches and mri3d_softmax_ce_index_plan_query all go by it), IDX_DISPATCH (the bucket -> instantiation switch).
// A class-map kernel supplies only its body: one voxel's logits in place plus its label.  The boundary kernels index a map by
// voxel and keep their two row loops, around the same idx_load_row and idx_store_row.  The bodies keep their arithmetic expression
// for expression: tests/golden/loss_family_bits.json records the bits of the whole family, and tests/test_loss_codegen.py holds
// every instantiation to 0 bytes of scratch and to the occupancy recorded before the walk was shared.
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

// p -> one voxel's C classes at d: 4-element vectors (rows-of-4 mode) or one element at a time
template <typename T, int CB>
__device__ __forceinline__ void idx_store_row(T* d, int C, int mode, const float (&p)[CB]) {
    if constexpr (CB >= 4) {
        if (mode == kIdxRows4) {
#pragma unroll
            for (int j = 0; j < CB; j += 4)
                if (j < C) stf4(d + j, make_float4(p[j], p[j + 1], p[j + 2], p[j + 3]));
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < CB; ++j)
        if (j < C) stf(d + j, p[j]);
}

// The voxels of sample blockIdx.y of a class-map loss: body(p, label, classes) gets one voxel's logits (classes >= C: -inf) and
// leaves in p what STORE writes to the gradient (which has the logits' pitch).  In the 4-voxel mode (two dense classes) a lane takes 8 logits and a 4-byte label word at a time, the head
// and tail as singles.
template <bool STORE, typename T, int CB, typename Body>
__device__ __forceinline__ void idx_walk(const T* logits, const uint8_t* labels, T* dlogits, int64_t vox, int C, int x_ld, int mode,
                                         Body&& body) {
    const int n = blockIdx.y;
    const T* zn = logits + (int64_t)n * vox * x_ld;
    const uint8_t* ln = labels + (int64_t)n * vox;
    T* dn = STORE ? dlogits + (int64_t)n * vox * x_ld : nullptr;
    if (CB == 2 && mode == kIdxVox4) {
        if constexpr (CB == 2) {
            const IdxVox4Plan plan(n, vox);
            for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < plan.items; i += (int64_t)gridDim.x * 256) {
                if (i < plan.groups) {
                    const int64_t v0 = plan.head + i * 4;
                    float z[8];
                    idx_ld8(zn + v0 * 2, z);
                    const uint32_t lw = *reinterpret_cast<const uint32_t*>(ln + v0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float p[2] = {z[2 * k], z[2 * k + 1]};
                        body(p, (lw >> (8 * k)) & 0xffu, 2);
                        if constexpr (STORE) z[2 * k] = p[0], z[2 * k + 1] = p[1];
                    }
                    if constexpr (STORE) idx_st8(dn + v0 * 2, z);
                } else {
                    const int64_t v = plan.single(i);
                    float p[2] = {ldf(zn + v * 2), ldf(zn + v * 2 + 1)};
                    body(p, ln[v], 2);
                    if constexpr (STORE) { stf(dn + v * 2, p[0]); stf(dn + v * 2 + 1, p[1]); }
                }
            }
        }
        return;
    }
#pragma unroll 1      // one voxel's CB registers at a time: unrolled, the 32-class bodies do not fit the register file
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < vox; v += (int64_t)gridDim.x * 256) {
        float p[CB];
        idx_load_row<T, CB>(zn + v * x_ld, C, mode, p);
        body(p, ln[v], C);
        if constexpr (STORE) idx_store_row<T, CB>(dn + v * x_ld, C, mode, p);
    }
}

// Two wave-reduced double sums of a block -> part[(n * gridDim.x + blockIdx.x) * 2]: the four waves through LDS in a fixed order
__device__ __forceinline__ void pair_block_row(double a, double b, int n, double* __restrict__ part) {
    __shared__ double red[4][2];
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2)
        part[((size_t)n * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// `rows` such rows -> (num, den), valid in thread 0 of a block of 256: lane t adds rows t, t + 256, ...; lane 0 adds the 256
// lane sums in order
__device__ __forceinline__ void pair_finalize_sum(const double* __restrict__ part, int rows, double& num, double& den) {
    __shared__ double r0[256], r1[256];
    double a = 0.0, b = 0.0;
    for (int q = threadIdx.x; q < rows; q += 256) { a += part[(size_t)q * 2]; b += part[(size_t)q * 2 + 1]; }
    r0[threadIdx.x] = a; r1[threadIdx.x] = b;
    __syncthreads();
    num = 0.0, den = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < 256; ++k) { num += r0[k]; den += r1[k]; }
}

// dice_block_row's rows -> stats[n][c][3] = (tp, sum_p, sum_g) and the mean over (n, c) of 1 - dice, valid in thread 0 of a block
// of 256: the pairs are handled 8 at a time by 32 partial lanes each (fixed-order double sums).  The float-target and the
// class-map loss are one expression of the three sums.
__device__ __forceinline__ float dice_finalize_rows(const double* __restrict__ part, float* __restrict__ stats, int N, int C, int nblk,
                                                    float eps) {
    __shared__ double r0[256], r1[256], r2[256];
    const int el = threadIdx.x >> 5, ql = threadIdx.x & 31;
    double acc_loss = 0.0;
    for (int base = 0; base < N * C; base += 8) {
        const int i = base + el;
        double tp = 0.0, sp = 0.0, sg = 0.0;
        if (i < N * C) {
            const int n = i / C, c = i - n * C;
            const double* p = part + ((size_t)n * nblk * C + c) * 3;
            for (int q = ql; q < nblk; q += 32) {
                tp += p[(size_t)q * C * 3];
                sp += p[(size_t)q * C * 3 + 1];
                sg += p[(size_t)q * C * 3 + 2];
            }
        }
        r0[threadIdx.x] = tp; r1[threadIdx.x] = sp; r2[threadIdx.x] = sg;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int e = 0; e < 8 && base + e < N * C; ++e) {
                double a = 0.0, b = 0.0, d = 0.0;
                for (int k = 0; k < 32; ++k) { a += r0[e * 32 + k]; b += r1[e * 32 + k]; d += r2[e * 32 + k]; }
                const int i2 = base + e;
                stats[i2 * 3] = (float)a;
                stats[i2 * 3 + 1] = (float)b;
                stats[i2 * 3 + 2] = (float)d;
                // float arithmetic from here mirrors the reference's fp32 tensors
                const float ftp = (float)a, den = 2.f * ftp + ((float)b - ftp) + ((float)d - ftp) + eps;
                acc_loss += 1.0 - (double)(2.f * ftp / den);
            }
        }
        __syncthreads();
    }
    return (float)(acc_loss / (double)(N * C));
}

// ------------------------------------------------------------------ host side of the class-map kernels
// The common head of every geometry check of the family (Geom: any of the loss geometries of mri3d.h); nmax: the most samples,
// 0 for none.  An operator adds its own clauses behind it.
template <typename Geom> static int idx_check(const Geom* g, const char* who, int cmax, int nmax) {
    MRI3D_REQUIRE(g != nullptr, MRI3D_EINVAL, "%s: null geometry", who);
    MRI3D_REQUIRE(g->dtype == MRI3D_F32 || g->dtype == MRI3D_BF16, MRI3D_ENOTSUP, "%s: unknown dtype %d", who, g->dtype);
    MRI3D_REQUIRE(g->n > 0 && g->vox > 0, MRI3D_EINVAL, "%s: empty tensor", who);
    MRI3D_REQUIRE(g->c >= kIdxMinC && g->c <= cmax, MRI3D_ENOTSUP, "%s: classes must be in [%d,%d], got %d", who, kIdxMinC, cmax, g->c);
    MRI3D_REQUIRE(g->x_ld >= g->c, MRI3D_EINVAL, "%s: pitch %d < classes %d", who, g->x_ld, g->c);
    MRI3D_REQUIRE(nmax == 0 || g->n <= nmax, MRI3D_ENOTSUP, "%s: at most %d samples, got %d", who, nmax, g->n);
    return MRI3D_OK;
}

// grid rules (blocks of 256).  Forward: a lane takes about 4 items, and all samples together at most `cap` blocks
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

// One decision per pass: the plan query reports it, every launch of the family goes by it.  dx_ld: the gradient's pitch (the
// logits' where there is none); align_logits: ptr_align of the logits (and, in a backward, of their gradient); align_labels:
// ptr_align of the class map, or 0 for an operator that reads no label bytes and so has no 4-voxel path (boundary).
struct IdxPlan { int bucket, mode, blocks, lanes, whole_trips, remainder; int64_t items; };

static IdxPlan idx_plan(int dtype, int n, int64_t vox, int c, int x_ld, int dx_ld, bool bwd, int align_logits, int align_labels) {
    IdxPlan p;
    p.bucket = c <= 2 ? 2 : c <= 4 ? 4 : c <= 8 ? 8 : c <= 16 ? 16 : 32;
    if (c == 2 && x_ld == 2 && dx_ld == 2 && align16(align_logits) && align_labels >= 4) p.mode = kIdxVox4;
    else if (c % 4 == 0 && x_ld % 4 == 0 && dx_ld % 4 == 0 && align_vec4(dtype, align_logits)) p.mode = kIdxRows4;
    else p.mode = kIdxScalar;
    // the grid is sized by the most items a sample can have (4-voxel path: groups and at most 6 single voxels)
    const int64_t grid_items = p.mode == kIdxVox4 ? vox / 4 + 6 : vox;
    p.blocks = bwd ? dice_bwd_blocks(grid_items, n) : dice_fwd_blocks(grid_items, n, kIdxMaxBlocks);
    p.lanes = p.blocks * 256;
    // the trips are those of sample 0, which starts aligned: groups of 4 and the voxels behind them
    p.items = p.mode == kIdxVox4 ? vox / 4 + vox % 4 : vox;
    p.whole_trips = (int)(p.items / p.lanes);
    p.remainder = (int)(p.items % p.lanes);
    return p;
}

}  // namespace mri3d

// CALL(CB) for the plan's class bucket
#define IDX_DISPATCH(BUCKET, CALL)          \
    do {                                    \
        switch (BUCKET) {                   \
            case 2: CALL(2); break;         \
            case 4: CALL(4); break;         \
            case 8: CALL(8); break;         \
            case 16: CALL(16); break;       \
            default: CALL(32); break;       \
        }                                   \
    } while (0)
