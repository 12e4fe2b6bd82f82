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
// The forward is one streaming pass of loss_index.h's voxel walk, launched by its idx_plan exactly as the index Dice is (class
// buckets 2, 4, 8, 16, 32; three read modes; the same grid rules), one instantiation per bucket x storage type x {CE only, CE + Dice}: the CE-only one carries two double
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
    __shared__ float sw[kIdxMaxC];
    if (threadIdx.x < kIdxMaxC) sw[threadIdx.x] = (int)threadIdx.x < C ? (weight ? weight[threadIdx.x] : 1.f) : 0.f;
    __syncthreads();
    CeFwdLane<CB, DICE> a;
    a.dice.zero();
    a.num = 0.0, a.den = 0.0;
    idx_walk<false, T, CB>(logits, labels, (T*)nullptr, vox, C, x_ld, mode,
                           [&](float (&p)[CB], unsigned lab, int classes) { a.add(p, lab, classes, sw, gamma); });
    // the two CE sums: wave shuffles, then the four waves through LDS in a fixed order
    const double bn = wave_sum_d(a.num), bd = wave_sum_d(a.den);
    pair_block_row(bn, bd, blockIdx.y, part_ce);
    if constexpr (DICE) dice_block_row<CB>(a.dice.tp, a.dice.sp, a.dice.sg, C, blockIdx.y, red, part_dice);
}

// The rows of partials -> stats and the loss, one block of 256 threads, every sum in a fixed order.
//   stats[0..4) = {CE, 1 / sum_w (0 when sum_w == 0), sum l_v, Dice};  with the Dice part, stats[4 + (n * C + c) * 3 ...] = (tp, sum_p,
//   sum_g) and the Dice value: loss_index.h's dice_finalize_rows, which loss.hip's dice_finalize_kernel runs too.
__global__ void __launch_bounds__(256)
ce_index_finalize_kernel(const double* __restrict__ part_dice, const double* __restrict__ part_ce, float* __restrict__ stats,
                         float* __restrict__ loss, int N, int C, int nblk, float eps, float dice_weight, float ce_weight,
                         int dice) {
    double num, den;
    pair_finalize_sum(part_ce, N * nblk, num, den);
    const float dv = dice ? dice_finalize_rows(part_dice, stats + kCeStatsHead, N, C, nblk, eps) : 0.f;
    if (threadIdx.x == 0) {
        const float ce = den > 0.0 ? (float)(num / den) : 0.f;
        stats[kCeVal] = ce;
        stats[kCeInvDen] = den > 0.0 ? (float)(1.0 / den) : 0.f;
        stats[kCeNum] = (float)num;
        stats[kCeDice] = dv;
        loss[0] = dice ? dice_weight * dv + ce_weight * ce : ce_weight * ce;
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
    idx_walk<true, T, CB>(logits, labels, dlogits, vox, C, x_ld, mode, [&](float (&p)[CB], unsigned lab, int classes) {
        ce_grad<CB, DICE>(p, lab, classes, sw, gamma, kce, k);
    });
}

// ------------------------------------------------------------------ host
static int ce_check(const Mri3dCeIndexGeom* g, const char* who) {
    int rc = idx_check(g, who, kIdxMaxC, kIdxMaxBlocks);
    if (rc) return rc;
    MRI3D_REQUIRE(g->gamma == 0.f || (g->gamma >= 1.f && g->gamma <= 8.f), MRI3D_EINVAL,
                  "%s: gamma must be 0 or in [1, 8], got %g", who, (double)g->gamma);
    MRI3D_REQUIRE(g->dice_weight >= 0.f && g->ce_weight >= 0.f && g->dice_weight <= 3.0e38f && g->ce_weight <= 3.0e38f, MRI3D_EINVAL,
                  "%s: loss weights must be finite and not negative, got dice %g, ce %g", who, (double)g->dice_weight,
                  (double)g->ce_weight);
    MRI3D_REQUIRE(g->dice_weight > 0.f || g->ce_weight > 0.f, MRI3D_EINVAL, "%s: both loss weights are zero", who);
    return MRI3D_OK;
}

static size_t ce_ws_bytes(const Mri3dCeIndexGeom& g) {
    return ((size_t)kIdxMaxBlocks * 2 + (g.dice_weight > 0.f ? (size_t)kIdxMaxBlocks * g.c * 3 : 0)) * sizeof(double);
}

}  // namespace mri3d

using namespace mri3d;

// the bucket's instantiation with or without the Dice part
#define CE_CALL(CB)                          \
    do {                                     \
        if (g->dice_weight > 0.f) CE_LAUNCH(CB, true); \
        else CE_LAUNCH(CB, false);           \
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
    const IdxPlan p = idx_plan(g->dtype, g->n, g->vox, g->c, g->x_ld, g->x_ld, pass == MRI3D_PASS_DGRAD, align_logits, align_labels);
    out->bucket = p.bucket, out->mode = p.mode, out->dice = g->dice_weight > 0.f, out->blocks = p.blocks, out->lanes = p.lanes;
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
    const IdxPlan plan = idx_plan(g->dtype, g->n, g->vox, g->c, g->x_ld, g->x_ld, false, ptr_align(logits), ptr_align(labels));
    double* part_ce = static_cast<double*>(workspace);
    double* part_dice = part_ce + (size_t)kIdxMaxBlocks * 2;
#define CE_LAUNCH(CB, DICE)                                                                                                        \
    hipLaunchKernelGGL((ce_index_fwd_kernel<T, CB, DICE>), dim3(plan.blocks, g->n), dim3(256), 0, s, (const T*)logits, labels, \
                       weight, part_dice, part_ce, g->vox, g->c, g->x_ld, plan.mode, g->gamma)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { IDX_DISPATCH(plan.bucket, CE_CALL); });
#undef CE_LAUNCH
    rc = check_launch("softmax_ce_index_fwd");
    if (rc) return rc;
    hipLaunchKernelGGL(ce_index_finalize_kernel, dim3(1), dim3(256), 0, s, part_dice, part_ce, stats, loss, g->n, g->c, plan.blocks,
                       g->eps, g->dice_weight, g->ce_weight, g->dice_weight > 0.f);
    return check_launch("softmax_ce_index_fwd");
}

extern "C" int mri3d_softmax_ce_index_bwd(const Mri3dCeIndexGeom* g, const void* logits, const uint8_t* labels, const float* weight,
                                          const float* stats, const float* dloss, void* dlogits, mri3d_stream_t stream) {
    int rc = ce_check(g, "softmax_ce_index_bwd");
    if (rc) return rc;
    MRI3D_REQUIRE(logits && labels && stats && dloss && dlogits, MRI3D_EINVAL, "softmax_ce_index_bwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const IdxPlan plan = idx_plan(g->dtype, g->n, g->vox, g->c, g->x_ld, g->x_ld, true, ptr_align(logits, dlogits), ptr_align(labels));
#define CE_LAUNCH(CB, DICE)                                                                                                        \
    hipLaunchKernelGGL((ce_index_bwd_kernel<T, CB, DICE>), dim3(plan.blocks, g->n), dim3(256), 0, s, (const T*)logits, labels, \
                       weight, stats, dloss, (T*)dlogits, g->vox, g->n, g->c, g->x_ld, plan.mode, g->eps, g->gamma,           \
                       g->dice_weight, g->ce_weight)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { IDX_DISPATCH(plan.bucket, CE_CALL); });
#undef CE_LAUNCH
    return check_launch("softmax_ce_index_bwd");
}
