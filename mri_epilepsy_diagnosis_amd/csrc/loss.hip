// loss.hip — fused softmax(dim=C) + soft-Dice loss and its gradient for both target forms (float channels, 2..8 classes; a uint8
// class map, 2..32 classes), plus the argmax->uint8 mask used by validation.
// Reference: F.softmax(logits, dim=1) -> get_dice_loss(probabilities, targets) -> .mean()
// (segmentation/routine.py:239-253, 272-274); labels = logits.argmax(dim=1) (routine.py:226-227).
//
//   p = softmax(z);  tp_c = sum p_c g_c,  fp_c = sum p_c (1-g_c),  fn_c = sum (1-p_c) g_c
//   dice_c = 2 tp_c / (2 tp_c + fp_c + fn_c + eps) = 2 tp_c / (sum p_c + sum g_c + eps)
//   loss = mean_{n,c} (1 - dice_{n,c})
// Float target: the reference feeds a (N,1,...) target against (N,2,...) probabilities, i.e. g_c = g for every class (SURVEY
// Appendix C.1); ct == 1 reproduces that broadcast, ct == c is the per-class form.  Class map: g_c = [label == c], a label >= C
// belongs to no class.
//
// The float form has its own forward and backward loops; the class-map form is a body inside loss_index.h's voxel walk (4-voxel
// path, class buckets, integer sum_g) and launches by its idx_plan.  Both share what stands around them: the softmax, the block's
// row of partial sums, the finalize, the gradient's coefficients, the grid rules and the head of the host checks.
//
// HBM-bound.  Bytes per voxel: forward C * esz + target, backward 2 * C * esz + target; target = 4 * ct (float) or 1 (class map).
#include "loss_index.h"

namespace mri3d {

constexpr int kDiceMaxC = 8;
// blocks of one forward launch over all samples: the cap fixes the summation order, so each form keeps its own (kIdxMaxBlocks:
// loss_index.h)
constexpr int kDiceMaxBlocks = 1024;

// ------------------------------------------------------------------ shared by both target forms
// z -> softmax(z) in place
template <int K> __device__ __forceinline__ void softmax_inplace(float (&z)[K]) {
    float m = z[0];
#pragma unroll
    for (int j = 1; j < K; ++j) m = fmaxf(m, z[j]);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) { z[j] = expf(z[j] - m); s += z[j]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int j = 0; j < K; ++j) z[j] *= inv;
}

// part -> stats[n][c][3] and the mean loss, one block of 256 threads
__global__ void __launch_bounds__(256)
dice_finalize_kernel(const double* __restrict__ part, float* __restrict__ stats, float* __restrict__ loss, int N, int C,
                     int nblk, float eps) {
    const float dv = dice_finalize_rows(part, stats, N, C, nblk, eps);
    if (threadIdx.x == 0) loss[0] = dv;
}

// ------------------------------------------------------------------ float target
template <typename T, int C>
__global__ void __launch_bounds__(256)
dice_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ target, double* __restrict__ part,
                int64_t vox, int ct, int x_ld, int t_ld) {
    __shared__ double red[4][C * 3];
    const int n = blockIdx.y;
    const T* zn = logits + (int64_t)n * vox * x_ld;
    const float* tn = target + (int64_t)n * vox * t_ld;
    double tp[C], sp[C], sg[C];  // torch's CPU reductions (the oracle's arithmetic) accumulate float sums in double
#pragma unroll
    for (int j = 0; j < C; ++j) { tp[j] = 0.0; sp[j] = 0.0; sg[j] = 0.0; }
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < vox; v += (int64_t)gridDim.x * blockDim.x) {
        float p[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = ldf(zn + v * x_ld + j);
        softmax_inplace<C>(p);
#pragma unroll
        for (int j = 0; j < C; ++j) {
            float g = tn[v * t_ld + (ct == 1 ? 0 : j)];
            tp[j] += (double)(p[j] * g);
            sp[j] += (double)p[j];
            sg[j] += (double)g;
        }
    }
    dice_block_row<C>(tp, sp, sg, C, n, red, part);
}

template <typename T, int C>
__global__ void __launch_bounds__(256)
dice_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ target, const float* __restrict__ stats,
                const float* __restrict__ dloss, T* __restrict__ dlogits, int64_t vox, int N, int ct, int x_ld,
                int t_ld, float eps) {
    const int n = blockIdx.y;
    const T* zn = logits + (int64_t)n * vox * x_ld;
    const float* tn = target + (int64_t)n * vox * t_ld;
    T* dn = dlogits + (int64_t)n * vox * x_ld;
    float ka[C], kb[C];
    const float scale = dloss[0] / (float)(N * C);
#pragma unroll
    for (int j = 0; j < C; ++j) dice_coeffs(stats + (n * C + j) * 3, scale, eps, ka[j], kb[j]);
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < vox; v += (int64_t)gridDim.x * blockDim.x) {
        float p[C], dp[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = ldf(zn + v * x_ld + j);
        softmax_inplace<C>(p);
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            float g = tn[v * t_ld + (ct == 1 ? 0 : j)];
            dp[j] = fmaf(ka[j], g, kb[j]);
            dot = fmaf(p[j], dp[j], dot);
        }
#pragma unroll
        for (int j = 0; j < C; ++j) stf(dn + v * x_ld + j, p[j] * (dp[j] - dot));
    }
}

// ------------------------------------------------------------------ class-map target
template <typename T, int CB>
__global__ void __launch_bounds__(256)
dice_index_fwd_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ labels, double* __restrict__ part, int64_t vox,
                      int C, int x_ld, int mode) {
    __shared__ double red[4][CB * 3];
    IdxAcc<CB> a;
#pragma unroll
    for (int j = 0; j < CB; ++j) { a.tp[j] = 0.0; a.sp[j] = 0.0; a.sg[j] = 0u; }
    idx_walk<false, T, CB>(logits, labels, (T*)nullptr, vox, C, x_ld, mode, [&](float (&p)[CB], unsigned lab, int) {
        softmax_inplace<CB>(p);
        a.add(p, lab);
    });
    dice_block_row<CB>(a.tp, a.sp, a.sg, C, blockIdx.y, red, part);
}

// ka * [label == c] + kb (dice_bwd_kernel's fmaf(ka, g, kb) at g = 1 and g = 0), then the softmax Jacobian
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
    // the two coefficients of every class, one class per lane, then to every lane's registers through LDS
    __shared__ float ska[CB], skb[CB];
    if (threadIdx.x < CB) {
        const int j = threadIdx.x;
        float a = 0.f, b = 0.f;        // a class >= C has p = 0 and takes no part
        if (j < C) dice_coeffs(stats + (n * C + j) * 3, dloss[0] / (float)(N * C), eps, a, b);
        ska[j] = a, skb[j] = b;
    }
    __syncthreads();
    float ka[CB], kb[CB];
#pragma unroll
    for (int j = 0; j < CB; ++j) ka[j] = ska[j], kb[j] = skb[j];
    idx_walk<true, T, CB>(logits, labels, dlogits, vox, C, x_ld, mode, [&](float (&p)[CB], unsigned lab, int) {
        softmax_inplace<CB>(p);
        idx_grad<CB>(p, lab, ka, kb);
    });
}

// ------------------------------------------------------------------ arg-max
template <typename T>
__global__ void __launch_bounds__(256)
argmax_u8_kernel(const T* __restrict__ logits, uint8_t* __restrict__ out, int64_t nvox, int C, int ld) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
        const T* z = logits + v * ld;
        float best = ldf(z);
        int bi = 0;
        for (int j = 1; j < C; ++j) {
            float t = ldf(z + j);
            // torch.argmax: first maximal value; NaN counts as maximal
            if ((t > best && best == best) || (t != t && best == best)) { best = t; bi = j; }
        }
        out[v] = (uint8_t)bi;
    }
}

// ------------------------------------------------------------------ host side of both Dice forms
static size_t dice_ws_bytes(int cap, int n, int c) { return ((size_t)cap + (size_t)n) * c * 3 * sizeof(double); }

static int dice_float_check(const Mri3dDiceGeom* g, const char* who) {
    int rc = idx_check(g, who, kDiceMaxC, 0);
    if (rc) return rc;
    MRI3D_REQUIRE(g->ct == 1 || g->ct == g->c, MRI3D_EINVAL, "%s: target channels %d must be 1 or %d", who, g->ct, g->c);
    MRI3D_REQUIRE(g->t_ld >= g->ct, MRI3D_EINVAL, "%s: target pitch %d < target channels %d", who, g->t_ld, g->ct);
    return MRI3D_OK;
}

static int dice_finalize(const char* who, const double* part, float* stats, float* loss, int n, int c, int nblk, float eps,
                         hipStream_t s) {
    hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(256), 0, s, part, stats, loss, n, c, nblk, eps);
    return check_launch(who);
}

}  // namespace mri3d

using namespace mri3d;

#define DICE_DISPATCH(CALL)                 \
    switch (g->c) {                         \
        case 2: CALL(2); break;             \
        case 3: CALL(3); break;             \
        case 4: CALL(4); break;             \
        case 5: CALL(5); break;             \
        case 6: CALL(6); break;             \
        case 7: CALL(7); break;             \
        default: CALL(8); break;            \
    }

extern "C" size_t mri3d_softmax_dice_workspace_bytes(const Mri3dDiceGeom* g) {
    return g ? dice_ws_bytes(kDiceMaxBlocks, g->n, g->c) : 0;
}

extern "C" int mri3d_softmax_dice_fwd(const Mri3dDiceGeom* g, const void* logits, const void* target, float* loss,
                                      float* stats, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = dice_float_check(g, "softmax_dice_fwd");
    if (rc) return rc;
    MRI3D_REQUIRE(logits && target && loss && stats, MRI3D_EINVAL, "softmax_dice_fwd: null pointer");
    rc = ws_check8("softmax_dice_fwd", workspace, ws_bytes, mri3d_softmax_dice_workspace_bytes(g));
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = dice_fwd_blocks(g->vox, g->n, kDiceMaxBlocks);
    double* part = static_cast<double*>(workspace);
#define CALL(CC)                                                                                              \
    hipLaunchKernelGGL((dice_fwd_kernel<T, CC>), dim3(nblk, g->n), dim3(256), 0, s, (const T*)logits,         \
                       (const float*)target, part, g->vox, g->ct, g->x_ld, g->t_ld)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { DICE_DISPATCH(CALL) });
#undef CALL
    return dice_finalize("softmax_dice_fwd", part, stats, loss, g->n, g->c, nblk, g->eps, s);
}

extern "C" int mri3d_softmax_dice_bwd(const Mri3dDiceGeom* g, const void* logits, const void* target,
                                      const float* stats, const float* dloss, void* dlogits, mri3d_stream_t stream) {
    int rc = dice_float_check(g, "softmax_dice_bwd");
    if (rc) return rc;
    MRI3D_REQUIRE(logits && target && stats && dloss && dlogits, MRI3D_EINVAL, "softmax_dice_bwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = dice_bwd_blocks(g->vox, g->n);
#define CALL(CC)                                                                                              \
    hipLaunchKernelGGL((dice_bwd_kernel<T, CC>), dim3(nblk, g->n), dim3(256), 0, s, (const T*)logits,         \
                       (const float*)target, stats, dloss, (T*)dlogits, g->vox, g->n, g->ct, g->x_ld,        \
                       g->t_ld, g->eps)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { DICE_DISPATCH(CALL) });
#undef CALL
    return check_launch("softmax_dice_bwd");
}

extern "C" size_t mri3d_softmax_dice_index_workspace_bytes(const Mri3dDiceIndexGeom* g) {
    if (!g || g->n <= 0 || g->c < kIdxMinC || g->c > kIdxMaxC) return 0;
    return dice_ws_bytes(kIdxMaxBlocks, g->n, g->c);
}

extern "C" int mri3d_softmax_dice_index_fwd(const Mri3dDiceIndexGeom* g, const void* logits, const uint8_t* labels, float* loss,
                                            float* stats, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = idx_check(g, "softmax_dice_index_fwd", kIdxMaxC, 0);
    if (rc) return rc;
    MRI3D_REQUIRE(logits && labels && loss && stats, MRI3D_EINVAL, "softmax_dice_index_fwd: null pointer");
    rc = ws_check8("softmax_dice_index_fwd", workspace, ws_bytes, mri3d_softmax_dice_index_workspace_bytes(g));
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const IdxPlan plan = idx_plan(g->dtype, g->n, g->vox, g->c, g->x_ld, g->x_ld, false, ptr_align(logits), ptr_align(labels));
    double* part = static_cast<double*>(workspace);
#define CALL(CB)                                                                                                    \
    hipLaunchKernelGGL((dice_index_fwd_kernel<T, CB>), dim3(plan.blocks, g->n), dim3(256), 0, s, (const T*)logits, labels, \
                       part, g->vox, g->c, g->x_ld, plan.mode)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { IDX_DISPATCH(plan.bucket, CALL); });
#undef CALL
    return dice_finalize("softmax_dice_index_fwd", part, stats, loss, g->n, g->c, plan.blocks, g->eps, s);
}

extern "C" int mri3d_softmax_dice_index_bwd(const Mri3dDiceIndexGeom* g, const void* logits, const uint8_t* labels,
                                            const float* stats, const float* dloss, void* dlogits, mri3d_stream_t stream) {
    int rc = idx_check(g, "softmax_dice_index_bwd", kIdxMaxC, 0);
    if (rc) return rc;
    MRI3D_REQUIRE(logits && labels && stats && dloss && dlogits, MRI3D_EINVAL, "softmax_dice_index_bwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const IdxPlan plan = idx_plan(g->dtype, g->n, g->vox, g->c, g->x_ld, g->x_ld, true, ptr_align(logits, dlogits), ptr_align(labels));
#define CALL(CB)                                                                                                    \
    hipLaunchKernelGGL((dice_index_bwd_kernel<T, CB>), dim3(plan.blocks, g->n), dim3(256), 0, s, (const T*)logits, labels, \
                       stats, dloss, (T*)dlogits, g->vox, g->n, g->c, g->x_ld, plan.mode, g->eps)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { IDX_DISPATCH(plan.bucket, CALL); });
#undef CALL
    return check_launch("softmax_dice_index_bwd");
}

extern "C" int mri3d_argmax_u8(const void* logits, uint8_t* out, int64_t nvox, int32_t c, int32_t ld, int32_t dtype,
                               mri3d_stream_t stream) {
    MRI3D_REQUIRE(dtype == MRI3D_F32 || dtype == MRI3D_BF16, MRI3D_ENOTSUP, "argmax_u8: unknown dtype %d", dtype);
    MRI3D_REQUIRE(logits && out && nvox > 0 && c > 0 && c <= 256 && ld >= c, MRI3D_EINVAL, "argmax_u8: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MRI3D_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL(argmax_u8_kernel<T>, dim3(stream_grid(nvox, 256)), dim3(256), 0, s, (const T*)logits, out, nvox, c,
                           ld);
    });
    return check_launch("argmax_u8");
}
