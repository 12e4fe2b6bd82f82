// ce_loss.hip — voxel-wise cross-entropy / focal loss of softmax(logits) against a uint8 class map, alone or fused with the
// class-map softmax-Dice of loss.hip in the same pass, and the gradient of the two in one pass.
//
//   m = max z, e_j = exp(z_j - m), s = sum e_j, p = e / s, pt = p_y, 1 - pt = (sum_{j != y} e_j) / s, logp_y = (z_y - m) - log s
//   l_v    = -w_y (1 - pt)^gamma logp_y                    (0 where the label is >= C: the voxel is ignored)
//   CE     = sum_v l_v / sum_v w_y                          (both sums over the non-ignored voxels of the whole batch; 0 / 0 = 0)
//   dCE/dz_j(v) = (w_y / sum w) [(1 - pt)^gamma - gamma pt (1 - pt)^(gamma - 1) logp_y] (p_j - [j == y])
//   loss   = dice_weight * Dice_index + ce_weight * CE      (Dice_index: loss.hip's class-map form, eps and ignored voxels included)
// logp_y never goes through log(pt) (pt underflows at a logit gap of about 88) and 1 - pt is never a subtraction; p_y - 1 in the
// gradient is -(1 - pt).  gamma is 0 or in [1, 8]: below 1, (1 - pt)^(gamma - 1) logp_y is inf * 0 once pt rounds to 1.
//
// The forward is one streaming pass over the plan of the index Dice (class buckets 2, 4, 8, 16, 32; three read modes; the same
// grid rules, loss_index.h), one instantiation per bucket x storage type x {CE only, CE + Dice}: the CE-only one carries two double
// accumulators per lane, the compound one the Dice triples besides.  A block leaves one row of partials in the workspace, a
// single-block kernel adds the rows in a fixed order: no float atomics, the same bits run to run.
//
// Bytes per voxel: the forward reads C * esz + 1, the backward moves 2 * C * esz + 1, CE only or compound — the index Dice's.  The
// forward is bound by its instructions (double sums, selects, a log per voxel), not by these bytes: DESIGN §4.18 has the figures.
#include "loss_index.h"

namespace mri3d {

// floats of `stats` in front of the Dice triples: CE value, 1 / sum_w (0 when nothing counts), sum of l_v, Dice value
constexpr int kCeStatsHead = 4;
enum { kCeVal = 0, kCeInvDen = 1, kCeNum = 2, kCeDice = 3 };

// (1 - pt)^(gamma - 1) for gamma >= 1: the focal weight is this times (1 - pt).  gamma = 1 and 2 need no pow; pow(0, 0) = 1.
__device__ __forceinline__ float focal_q(float omp, float gamma) {
    if (gamma == 1.f) return 1.f;
    if (gamma == 2.f) return omp;
    return powf(omp, gamma - 1.f);
}

// One voxel's softmax around its label.  z -> e = exp(z - m) in place (classes >= C hold -inf -> 0), s their sum.  A label that
// is no class hits nothing: zy = ey = 0, so = s, and the caller drops the voxel.
template <int K> struct CeVoxel {
    float m, s, zy, ey, so;
    __device__ __forceinline__ void run(float (&z)[K], unsigned lab) {
        m = z[0];
#pragma unroll
        for (int j = 1; j < K; ++j) m = fmaxf(m, z[j]);
        s = 0.f, zy = 0.f, ey = 0.f, so = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const bool hit = lab == (unsigned)j;
            zy = hit ? z[j] : zy;
            z[j] = expf(z[j] - m);
            s += z[j];                     // the order of softmax_inplace: the Dice part sees the index Dice's probabilities
            ey = hit ? z[j] : ey;
            so += hit ? 0.f : z[j];
        }
    }
    __device__ __forceinline__ float logp() const { return (zy - m) - logf(s); }
};

// l_v / w_y = -(1 - pt)^gamma logp_y
__device__ __forceinline__ float ce_voxel_loss(float pt, float omp, float logp, float gamma) {
    const float f = gamma == 0.f ? 1.f : focal_q(omp, gamma) * omp;
    return -f * logp;
}
// (1 - pt)^gamma - gamma pt (1 - pt)^(gamma - 1) logp_y
__device__ __forceinline__ float ce_voxel_slope(float pt, float omp, float logp, float gamma) {
    if (gamma == 0.f) return 1.f;
    const float q = focal_q(omp, gamma);
    return q * omp - gamma * pt * q * logp;
}

// the Dice accumulators exist only in the compound instance
template <int CB, bool DICE> struct CeDiceAcc;
template <int CB> struct CeDiceAcc<CB, true> : IdxAcc<CB> {
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int j = 0; j < CB; ++j) { this->tp[j] = 0.0; this->sp[j] = 0.0; this->sg[j] = 0u; }
    }
};
template <int CB> struct CeDiceAcc<CB, false> {
    __device__ __forceinline__ void zero() {}
};

template <int CB, bool DICE> struct CeFwdLane {
    CeDiceAcc<CB, DICE> dice;
    double num, den;
    // z: the voxel's logits (classes >= C: -inf); w: the class weights in LDS
    __device__ __forceinline__ void add(float (&z)[CB], unsigned lab, int C, const float* w, float gamma) {
        CeVoxel<CB> v;
        v.run(z, lab);
        const float inv = 1.f / v.s;
        if (lab < (unsigned)C) {
            const float wy = w[lab];
            num += (double)(wy * ce_voxel_loss(v.ey * inv, v.so * inv, v.logp(), gamma));
            den += (double)wy;
        }
        if constexpr (DICE) {
#pragma unroll
            for (int j = 0; j < CB; ++j) z[j] *= inv;
            dice.add(z, lab);
        }
    }
};

// part_ce[(n * gridDim.x + blockIdx.x) * 2] = the block's (sum l_v, sum w_y); part_dice: dice_block_row's rows
template <typename T, int CB, bool DICE>
__global__ void __launch_bounds__(256)
ce_index_fwd_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ labels, const float* __restrict__ weight,
                    double* __restrict__ part_dice, double* __restrict__ part_ce, int64_t vox, int C, int x_ld, int mode,
                    float gamma) {
    __shared__ double red[4][DICE ? CB * 3 : 1];
    __shared__ double redce[4][2];
    __shared__ float sw[kIdxMaxC];
    const int n = blockIdx.y;
    const T* zn = logits + (int64_t)n * vox * x_ld;
    const uint8_t* ln = labels + (int64_t)n * vox;
    if (threadIdx.x < kIdxMaxC) sw[threadIdx.x] = (int)threadIdx.x < C ? (weight ? weight[threadIdx.x] : 1.f) : 0.f;
    __syncthreads();
    CeFwdLane<CB, DICE> a;
    a.dice.zero();
    a.num = 0.0, a.den = 0.0;
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
                        a.add(p, (lw >> (8 * k)) & 0xffu, 2, sw, gamma);
                    }
                } else {
                    const int64_t v = plan.single(i);
                    float p[2] = {ldf(zn + v * 2), ldf(zn + v * 2 + 1)};
                    a.add(p, ln[v], 2, sw, gamma);
                }
            }
        }
    } else {
#pragma unroll 1
        for (int64_t v = tid; v < vox; v += nth) {
            float p[CB];
            idx_load_row<T, CB>(zn + v * x_ld, C, mode, p);
            a.add(p, ln[v], C, sw, gamma);
        }
    }
    // the two CE sums: wave shuffles, then the four waves through LDS in a fixed order
    const double bn = wave_sum_d(a.num), bd = wave_sum_d(a.den);
    if ((threadIdx.x & 63) == 0) { redce[threadIdx.x >> 6][0] = bn; redce[threadIdx.x >> 6][1] = bd; }
    if constexpr (DICE) {
        dice_block_row<CB>(a.dice.tp, a.dice.sp, a.dice.sg, C, n, red, part_dice);      // (its barrier orders redce too)
    } else {
        __syncthreads();
    }
    if (threadIdx.x < 2)
        part_ce[((size_t)n * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
            redce[0][threadIdx.x] + redce[1][threadIdx.x] + redce[2][threadIdx.x] + redce[3][threadIdx.x];
}

// The rows of partials -> stats and the loss, one block of 256 threads, every sum in a fixed order.
//   stats[0..4) = {CE, 1 / sum_w (0 when sum_w == 0), sum l_v, Dice};  with the Dice part, stats[4 + (n * C + c) * 3 ...] = (tp, sum_p,
//   sum_g) and the Dice value as loss.hip's dice_finalize_kernel computes it (8 (n, c) pairs at a time, 32 partial lanes each).
__global__ void __launch_bounds__(256)
ce_index_finalize_kernel(const double* __restrict__ part_dice, const double* __restrict__ part_ce, float* __restrict__ stats,
                         float* __restrict__ loss, int N, int C, int nblk, float eps, float dice_weight, float ce_weight,
                         int dice) {
    __shared__ double r0[256], r1[256], r2[256];
    __shared__ double acc_loss;
    const int el = threadIdx.x >> 5, ql = threadIdx.x & 31;
    if (threadIdx.x == 0) acc_loss = 0.0;
    // CE: lane t adds rows t, t + 256, ...; lane 0 adds the 256 lane sums in order
    double a = 0.0, b = 0.0;
    for (int q = threadIdx.x; q < N * nblk; q += 256) { a += part_ce[(size_t)q * 2]; b += part_ce[(size_t)q * 2 + 1]; }
    r0[threadIdx.x] = a; r1[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        double num = 0.0, den = 0.0;
        for (int k = 0; k < 256; ++k) { num += r0[k]; den += r1[k]; }
        stats[kCeVal] = den > 0.0 ? (float)(num / den) : 0.f;
        stats[kCeInvDen] = den > 0.0 ? (float)(1.0 / den) : 0.f;
        stats[kCeNum] = (float)num;
    }
    __syncthreads();
    if (dice) {
        float* dstats = stats + kCeStatsHead;
        for (int base = 0; base < N * C; base += 8) {
            const int i = base + el;
            double tp = 0.0, sp = 0.0, sg = 0.0;
            if (i < N * C) {
                const int n = i / C, c = i - n * C;
                const double* p = part_dice + ((size_t)n * nblk * C + c) * 3;
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
                    double x = 0.0, y = 0.0, d = 0.0;
                    for (int k = 0; k < 32; ++k) { x += r0[e * 32 + k]; y += r1[e * 32 + k]; d += r2[e * 32 + k]; }
                    const int i2 = base + e;
                    dstats[i2 * 3] = (float)x;
                    dstats[i2 * 3 + 1] = (float)y;
                    dstats[i2 * 3 + 2] = (float)d;
                    const float ftp = (float)x, den = 2.f * ftp + ((float)y - ftp) + ((float)d - ftp) + eps;
                    acc_loss += 1.0 - (double)(2.f * ftp / den);
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        const float dv = dice ? (float)(acc_loss / (double)(N * C)) : 0.f;
        stats[kCeDice] = dv;
        loss[0] = dice ? dice_weight * dv + ce_weight * stats[kCeVal] : ce_weight * stats[kCeVal];
    }
}

// what a block's lanes keep for the whole backward pass
template <int CB, bool DICE> struct CeBwdCoef;
template <int CB> struct CeBwdCoef<CB, true> { float ka[CB], kb[CB]; };
template <int CB> struct CeBwdCoef<CB, false> {};

// z (logits, classes >= C: -inf) -> dlogits in place.  kce = dloss * ce_weight / sum_w; the Dice coefficients are scaled by
// dloss * dice_weight / (N * C) already.
template <int CB, bool DICE>
__device__ __forceinline__ void ce_grad(float (&z)[CB], unsigned lab, int C, const float* w, float gamma, float kce,
                                        const CeBwdCoef<CB, DICE>& k) {
    CeVoxel<CB> v;
    v.run(z, lab);
    const float inv = 1.f / v.s;
    float a = 0.f;
    if (lab < (unsigned)C) a = kce * w[lab] * ce_voxel_slope(v.ey * inv, v.so * inv, v.logp(), gamma);
    const float my = -(v.so * inv);        // p_y - 1
    if constexpr (DICE) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            z[j] *= inv;
            dot = fmaf(z[j], lab == (unsigned)j ? k.ka[j] + k.kb[j] : k.kb[j], dot);
        }
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            const bool hit = lab == (unsigned)j;
            z[j] = fmaf(a, hit ? my : z[j], z[j] * ((hit ? k.ka[j] + k.kb[j] : k.kb[j]) - dot));
        }
    } else {
#pragma unroll
        for (int j = 0; j < CB; ++j) z[j] = a * (lab == (unsigned)j ? my : z[j] * inv);
    }
}

template <typename T, int CB, bool DICE>
__global__ void __launch_bounds__(256)
ce_index_bwd_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ labels, const float* __restrict__ weight,
                    const float* __restrict__ stats, const float* __restrict__ dloss, T* __restrict__ dlogits, int64_t vox, int N,
                    int C, int x_ld, int mode, float eps, float gamma, float dice_weight, float ce_weight) {
    const int n = blockIdx.y;
    const T* zn = logits + (int64_t)n * vox * x_ld;
    const uint8_t* ln = labels + (int64_t)n * vox;
    T* dn = dlogits + (int64_t)n * vox * x_ld;
    __shared__ float sw[kIdxMaxC], ska[kIdxMaxC], skb[kIdxMaxC];
    if (threadIdx.x < kIdxMaxC) {
        const int j = threadIdx.x;
        sw[j] = j < C ? (weight ? weight[j] : 1.f) : 0.f;
        float a = 0.f, b = 0.f;        // a class >= C has p = 0 and takes no part
        if (DICE && j < C)
            dice_coeffs(stats + kCeStatsHead + (n * C + j) * 3, dloss[0] * dice_weight / (float)(N * C), eps, a, b);
        ska[j] = a, skb[j] = b;
    }
    __syncthreads();
    CeBwdCoef<CB, DICE> k;
    if constexpr (DICE) {
#pragma unroll
        for (int j = 0; j < CB; ++j) k.ka[j] = ska[j], k.kb[j] = skb[j];
    }
    const float kce = dloss[0] * ce_weight * stats[kCeInvDen];
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
                    for (int q = 0; q < 4; ++q) {
                        float p[2] = {z[2 * q], z[2 * q + 1]};
                        ce_grad<2, DICE>(p, (lw >> (8 * q)) & 0xffu, 2, sw, gamma, kce, k);
                        z[2 * q] = p[0], z[2 * q + 1] = p[1];
                    }
                    idx_st8(dn + v0 * 2, z);
                } else {
                    const int64_t v = plan.single(i);
                    float p[2] = {ldf(zn + v * 2), ldf(zn + v * 2 + 1)};
                    ce_grad<2, DICE>(p, ln[v], 2, sw, gamma, kce, k);
                    stf(dn + v * 2, p[0]);
                    stf(dn + v * 2 + 1, p[1]);
                }
            }
        }
        return;
    }
#pragma unroll 1
    for (int64_t v = tid; v < vox; v += nth) {
        float p[CB];
        idx_load_row<T, CB>(zn + v * x_ld, C, mode, p);
        ce_grad<CB, DICE>(p, ln[v], C, sw, gamma, kce, k);
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

// ------------------------------------------------------------------ host
// One decision per pass: the query reports it, the launches go by it.
struct CePlan { int bucket, mode, dice, blocks, lanes, whole_trips, remainder; int64_t items; };

static int ce_check(const Mri3dCeIndexGeom* g, const char* who) {
    MRI3D_REQUIRE(g != nullptr, MRI3D_EINVAL, "%s: null geometry", who);
    MRI3D_REQUIRE(g->dtype == MRI3D_F32 || g->dtype == MRI3D_BF16, MRI3D_ENOTSUP, "%s: unknown dtype %d", who, g->dtype);
    MRI3D_REQUIRE(g->n > 0 && g->vox > 0, MRI3D_EINVAL, "%s: empty tensor", who);
    MRI3D_REQUIRE(g->c >= kIdxMinC && g->c <= kIdxMaxC, MRI3D_ENOTSUP, "%s: classes must be in [%d,%d], got %d", who, kIdxMinC,
                  kIdxMaxC, g->c);
    MRI3D_REQUIRE(g->x_ld >= g->c, MRI3D_EINVAL, "%s: pitch %d < classes %d", who, g->x_ld, g->c);
    MRI3D_REQUIRE(g->gamma == 0.f || (g->gamma >= 1.f && g->gamma <= 8.f), MRI3D_EINVAL,
                  "%s: gamma must be 0 or in [1, 8], got %g", who, (double)g->gamma);
    MRI3D_REQUIRE(g->dice_weight >= 0.f && g->ce_weight >= 0.f && g->dice_weight <= 3.0e38f && g->ce_weight <= 3.0e38f, MRI3D_EINVAL,
                  "%s: loss weights must be finite and not negative, got dice %g, ce %g", who, (double)g->dice_weight,
                  (double)g->ce_weight);
    MRI3D_REQUIRE(g->dice_weight > 0.f || g->ce_weight > 0.f, MRI3D_EINVAL, "%s: both loss weights are zero", who);
    MRI3D_REQUIRE(g->n <= kIdxMaxBlocks, MRI3D_ENOTSUP, "%s: at most %d samples, got %d", who, kIdxMaxBlocks, g->n);
    return MRI3D_OK;
}

// align_logits: ptr_align of the logits (and, in the backward, of their gradient); align_labels: of the class map
static CePlan ce_plan(const Mri3dCeIndexGeom& g, bool bwd, int align_logits, int align_labels) {
    CePlan p;
    p.bucket = g.c <= 2 ? 2 : g.c <= 4 ? 4 : g.c <= 8 ? 8 : g.c <= 16 ? 16 : 32;
    p.dice = g.dice_weight > 0.f;
    if (g.c == 2 && g.x_ld == 2 && align16(align_logits) && align_labels >= 4) p.mode = kIdxVox4;
    else if (g.c % 4 == 0 && g.x_ld % 4 == 0 && align_vec4(g.dtype, align_logits)) p.mode = kIdxRows4;
    else p.mode = kIdxScalar;
    // the grid is sized by the most items a sample can have (4-voxel path: groups and at most 6 single voxels), as the index Dice's
    const int64_t grid_items = p.mode == kIdxVox4 ? g.vox / 4 + 6 : g.vox;
    p.blocks = bwd ? dice_bwd_blocks(grid_items, g.n) : dice_fwd_blocks(grid_items, g.n, kIdxMaxBlocks);
    p.lanes = p.blocks * 256;
    // the trips are those of sample 0, which starts aligned: groups of 4 and the voxels behind them
    p.items = p.mode == kIdxVox4 ? g.vox / 4 + g.vox % 4 : g.vox;
    p.whole_trips = (int)(p.items / p.lanes);
    p.remainder = (int)(p.items % p.lanes);
    return p;
}

static size_t ce_ws_bytes(const Mri3dCeIndexGeom& g) {
    return ((size_t)kIdxMaxBlocks * 2 + (g.dice_weight > 0.f ? (size_t)kIdxMaxBlocks * g.c * 3 : 0)) * sizeof(double);
}

}  // namespace mri3d

using namespace mri3d;

#define CE_DISPATCH(CALL)                                       \
    do {                                                        \
        if (plan.dice) {                                        \
            switch (plan.bucket) {                              \
                case 2: CALL(2, true); break;                   \
                case 4: CALL(4, true); break;                   \
                case 8: CALL(8, true); break;                   \
                case 16: CALL(16, true); break;                 \
                default: CALL(32, true); break;                 \
            }                                                   \
        } else {                                                \
            switch (plan.bucket) {                              \
                case 2: CALL(2, false); break;                  \
                case 4: CALL(4, false); break;                  \
                case 8: CALL(8, false); break;                  \
                case 16: CALL(16, false); break;                \
                default: CALL(32, false); break;                \
            }                                                   \
        }                                                       \
    } while (0)

extern "C" size_t mri3d_softmax_ce_index_workspace_bytes(const Mri3dCeIndexGeom* g) {
    if (!g || g->n <= 0 || g->n > kIdxMaxBlocks || g->c < kIdxMinC || g->c > kIdxMaxC) return 0;
    return ce_ws_bytes(*g);
}

extern "C" int mri3d_softmax_ce_index_plan_query(const Mri3dCeIndexGeom* g, int32_t pass, int32_t align_logits, int32_t align_labels,
                                                 Mri3dCeIndexPlanInfo* out) {
    MRI3D_REQUIRE(out != nullptr, MRI3D_EINVAL, "softmax_ce_index_plan_query: null output");
    int rc = ce_check(g, "softmax_ce_index_plan_query");
    if (rc) return rc;
    MRI3D_REQUIRE(pass == MRI3D_PASS_FWD || pass == MRI3D_PASS_DGRAD, MRI3D_EINVAL, "softmax_ce_index_plan_query: pass %d", pass);
    MRI3D_REQUIRE(align_logits >= 1 && align_labels >= 1, MRI3D_EINVAL, "softmax_ce_index_plan_query: alignments %d, %d", align_logits,
                  align_labels);
    const CePlan p = ce_plan(*g, pass == MRI3D_PASS_DGRAD, align_logits, align_labels);
    out->bucket = p.bucket, out->mode = p.mode, out->dice = p.dice, out->blocks = p.blocks, out->lanes = p.lanes;
    out->whole_trips = p.whole_trips, out->remainder = p.remainder, out->items = p.items;
    return MRI3D_OK;
}

extern "C" int mri3d_softmax_ce_index_fwd(const Mri3dCeIndexGeom* g, const void* logits, const uint8_t* labels, const float* weight,
                                          float* loss, float* stats, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = ce_check(g, "softmax_ce_index_fwd");
    if (rc) return rc;
    MRI3D_REQUIRE(logits && labels && loss && stats, MRI3D_EINVAL, "softmax_ce_index_fwd: null pointer");
    rc = ws_check8("softmax_ce_index_fwd", workspace, ws_bytes, ce_ws_bytes(*g));
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CePlan plan = ce_plan(*g, false, ptr_align(logits), ptr_align(labels));
    double* part_ce = static_cast<double*>(workspace);
    double* part_dice = part_ce + (size_t)kIdxMaxBlocks * 2;
#define CALL(CB, DICE)                                                                                                        \
    hipLaunchKernelGGL((ce_index_fwd_kernel<T, CB, DICE>), dim3(plan.blocks, g->n), dim3(256), 0, s, (const T*)logits, labels, \
                       weight, part_dice, part_ce, g->vox, g->c, g->x_ld, plan.mode, g->gamma)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { CE_DISPATCH(CALL); });
#undef CALL
    rc = check_launch("softmax_ce_index_fwd");
    if (rc) return rc;
    hipLaunchKernelGGL(ce_index_finalize_kernel, dim3(1), dim3(256), 0, s, part_dice, part_ce, stats, loss, g->n, g->c, plan.blocks,
                       g->eps, g->dice_weight, g->ce_weight, plan.dice);
    return check_launch("softmax_ce_index_fwd");
}

extern "C" int mri3d_softmax_ce_index_bwd(const Mri3dCeIndexGeom* g, const void* logits, const uint8_t* labels, const float* weight,
                                          const float* stats, const float* dloss, void* dlogits, mri3d_stream_t stream) {
    int rc = ce_check(g, "softmax_ce_index_bwd");
    if (rc) return rc;
    MRI3D_REQUIRE(logits && labels && stats && dloss && dlogits, MRI3D_EINVAL, "softmax_ce_index_bwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CePlan plan = ce_plan(*g, true, ptr_align(logits, dlogits), ptr_align(labels));
#define CALL(CB, DICE)                                                                                                        \
    hipLaunchKernelGGL((ce_index_bwd_kernel<T, CB, DICE>), dim3(plan.blocks, g->n), dim3(256), 0, s, (const T*)logits, labels, \
                       weight, stats, dloss, (T*)dlogits, g->vox, g->n, g->c, g->x_ld, plan.mode, g->eps, g->gamma,           \
                       g->dice_weight, g->ce_weight)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { CE_DISPATCH(CALL); });
#undef CALL
    return check_launch("softmax_ce_index_bwd");
}
