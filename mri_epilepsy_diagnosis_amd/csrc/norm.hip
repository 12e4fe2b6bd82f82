// norm.hip — BatchNorm3d / InstanceNorm3d statistics, fused normalise+affine+activation forward, and the fused
// backward (activation' -> dgamma/dbeta/dalpha reductions -> dx), NDHWC with voxel pitch.
// Reference semantics: torch.nn.BatchNorm3d (eps 1e-5, momentum .1, biased var for normalisation, unbiased for the
// running estimate) + nn.PReLU / LeakyReLU / ReLU as used by unet.UNet blocks, AE_model.py:30-36, cnn_model.py,
// modified_3dunet.py:20-94 (InstanceNorm3d, affine=False).
//
// Roofline: pure streaming (HBM-bound).  Algorithmic bytes: stats = 1 read of x; fwd apply = 1 read + 1 write;
// bwd = 2 reads (x,dy) for the reductions + 2 reads + 1 write for dx.
//
// Thread mapping: a 256-thread block is a (VT voxels) x (CL channel-lanes) grid, each lane owning VEC consecutive
// channels, so a thread's channels never change across the grid-stride loop: per-channel partial sums live in
// registers, are combined across the VT voxel rows through LDS once per block, and one partial per block goes to
// the workspace.  A finalize kernel sums the partials in a fixed order in double precision (deterministic).
#include "common.h"
#include <algorithm>
#include <type_traits>

namespace mri3d {

struct NormPlan {
    int vec;     // channels per lane (8: bf16 only, 4 or 1)
    int CL;      // channel lanes per voxel row handled by one block (<= 256)
    int VT;      // voxel rows per block iteration
    int cy;      // grid.y = channel chunks
    int nblk;    // grid.x = blocks per group
    int groups;  // grid.z
    int64_t gvox;  // voxels per group
};

constexpr int kNormMaxBlocks = 1024;  // 4 blocks/CU of streaming work; keeps the finalize pass short
constexpr int kFinQL = 64;            // partial-sum lanes per channel in the finalize kernels: with 16 lanes (64 dependent
                                      // loads + adds each over 1024 partials) the two finalize passes took 20 us per launch

static NormPlan norm_plan(const Mri3dNormGeom& g, bool al, bool al16 = false) {
    NormPlan p;
    p.vec = (g.c % 4 == 0 && g.x_ld % 4 == 0 && g.y_ld % 4 == 0 && al) ? 4 : 1;
    // bf16: 8 channels per lane make the accesses 16 bytes wide (with 4 they are 8-byte loads and the streaming kernels sat at
    // 2.9 TB/s against 5.4 TB/s for the same kernels in fp32)
    if (p.vec == 4 && g.dtype == MRI3D_BF16 && g.c % 8 == 0 && g.x_ld % 8 == 0 && g.y_ld % 8 == 0 && al16) p.vec = 8;
    int lanes = g.c / p.vec;
    p.CL = lanes < 256 ? lanes : 256;
    p.cy = cdiv(lanes, p.CL);
    p.VT = 256 / p.CL;
    p.groups = g.instance ? g.n : 1;
    p.gvox = g.instance ? g.vox : (int64_t)g.n * g.vox;
    int64_t want = cdiv64(p.gvox, (int64_t)p.VT * 8);  // >= 8 voxel rows per thread
    int cap = kNormMaxBlocks / (p.groups * p.cy);
    if (cap < 1) cap = 1;
    p.nblk = (int)(want < cap ? want : cap);
    if (p.nblk < 1) p.nblk = 1;
    return p;
}

// The plan of one pass (MRI3D_NORM_PASS_*) over tensors known by their ptr_align: the one decision mri3d_norm_stats,
// mri3d_norm_act_fwd, mri3d_norm_act_bwd and the query mri3d_norm_plan_query all read.  The statistics pass reads x alone (y_ld
// takes no part); only the bf16 forward moves 8 channels per lane (the float64 accumulators of the other two measured slower).
static NormPlan norm_plan_for(const Mri3dNormGeom& g, int pass, int align) {
    if (pass == MRI3D_NORM_PASS_STATS) {
        Mri3dNormGeom gg = g;
        gg.y_ld = gg.x_ld;
        return norm_plan(gg, align_vec4(g.dtype, align));
    }
    return norm_plan(g, align_vec4(g.dtype, align), pass == MRI3D_NORM_PASS_FWD && align16(align));
}

size_t norm_workspace_floats(const Mri3dNormGeom& g) {
    // plan with worst-case (vec=1) block count is not needed: nblk <= kMaxStreamBlocks/groups always.
    int groups = g.instance ? g.n : 1;
    size_t part = (size_t)(kNormMaxBlocks + groups) * g.c * 3 * 2;  // per-block partials in double (groups*nblk <= kNormMaxBlocks, or nblk=1)
    part += (size_t)groups * g.c * 3;                           // bwd per-(group,channel) sums
    return part;
}

// Run `body` with `VEC` bound to a plan's channels per lane: 4 or 1, and 8 where `with8` (a constant expression: the bf16
// forward) allows it.  Only the branches written here are instantiated.
#define MRI3D_DISPATCH_VEC(vec, with8, VEC, ...)                      \
    do {                                                              \
        if constexpr (with8) {                                        \
            if ((vec) == 8) { constexpr int VEC = 8; __VA_ARGS__ }    \
        }                                                             \
        if ((vec) == 4) { constexpr int VEC = 4; __VA_ARGS__ }        \
        else if ((vec) == 1) { constexpr int VEC = 1; __VA_ARGS__ }   \
    } while (0)

template <int VEC>
struct Ld {
    template <typename T>
    static __device__ __forceinline__ void load(const T* p, float (&v)[VEC]) {
        if constexpr (VEC == 8) {   // bf16 only: one 16-byte load
            const bf16x8_t t = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
        } else if constexpr (VEC == 4) {
            float4 t = ldf4(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            v[0] = ldf(p);
        }
    }
    template <typename T>
    static __device__ __forceinline__ void store(T* p, const float (&v)[VEC]) {
        if constexpr (VEC == 8) {
            bf16x8_t o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (bf16_t)v[j];
            *reinterpret_cast<bf16x8_t*>(p) = o;
        } else if constexpr (VEC == 4) {
            stf4(p, make_float4(v[0], v[1], v[2], v[3]));
        } else {
            stf(p, v[0]);
        }
    }
};

// ------------------------------------------------------------------ statistics
// partial layout: part[((group*cy... flattened as [group][blk][c][2]
template <typename T, int VEC>
__global__ void __launch_bounds__(256)
norm_stats_kernel(const T* __restrict__ x, double* __restrict__ part, int C, int ld, int64_t gvox, int CL, int VT) {
    __shared__ double red[256 * 2 * VEC];
    const int tid = threadIdx.x;
    const int cl = tid % CL, vt = tid / CL;
    const int c0 = (blockIdx.y * CL + cl) * VEC;
    const bool active = vt < VT && c0 < C;
    const int group = blockIdx.z;
    const T* xg = x + (int64_t)group * gvox * ld;
    // double accumulators: torch's CPU batch-norm (the oracle's arithmetic) accumulates float sums in double
    double s[VEC], ss[VEC];
    float k[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { s[j] = 0.0; ss[j] = 0.0; k[j] = 0.f; }
    if (active) {
        Ld<VEC>::load(xg + c0, k);  // shift = first voxel of the group: removes E[x^2]-E[x]^2 cancellation
        // the differences are formed in double, where they are exact: a float subtraction rounds each by up to 2^-24 |x - k|, an
        // error in the mean that does not shrink with |mean| and shows wherever few voxels share a statistic
        // four voxel rows per trip: the loads are independent, so four 16-byte requests per lane are in flight (one at a
        // time left this read-only pass at 4.2 TB/s); the sums still run in voxel order
        const int64_t step = (int64_t)gridDim.x * VT;
        int64_t v = (int64_t)blockIdx.x * VT + vt;
        for (; v + 3 * step < gvox; v += 4 * step) {
            float xv[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; ++u) Ld<VEC>::load(xg + (v + u * step) * ld + c0, xv[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const double d = (double)xv[u][j] - (double)k[j];
                    s[j] += d;
                    ss[j] = fma(d, d, ss[j]);
                }
        }
        for (; v < gvox; v += step) {
            float xv[VEC];
            Ld<VEC>::load(xg + v * ld + c0, xv);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const double d = (double)xv[j] - (double)k[j];
                s[j] += d;
                ss[j] = fma(d, d, ss[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) { red[(tid * VEC + j) * 2] = s[j]; red[(tid * VEC + j) * 2 + 1] = ss[j]; }
    __syncthreads();
    if (vt == 0 && c0 < C) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            double a = 0.0, b = 0.0;
            for (int q = 0; q < VT; ++q) {
                a += red[((q * CL + cl) * VEC + j) * 2];
                b += red[((q * CL + cl) * VEC + j) * 2 + 1];
            }
            double* o = part + (((size_t)group * gridDim.x + blockIdx.x) * C + c0 + j) * 2;
            o[0] = a;
            o[1] = b;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
norm_stats_finalize_kernel(const T* __restrict__ x, const double* __restrict__ part,
                           float* __restrict__ mean, float* __restrict__ invstd,
                           float* __restrict__ running_mean, float* __restrict__ running_var,
                           float momentum, float eps, int C, int ld, int64_t gvox, int nblk, int groups,
                           const float* __restrict__ shift = nullptr, int use_shift = 0) {
    // 256 threads = 4 (group,channel) slots x kFinQL partial lanes
    __shared__ double ra[256], rb[256];
    const int slot = threadIdx.x / kFinQL, ql = threadIdx.x % kFinQL;
    const int i = blockIdx.x * (256 / kFinQL) + slot;
    const bool ok = i < groups * C;
    const int group = ok ? i / C : 0, c = ok ? i - group * C : 0;
    double a = 0.0, b = 0.0;
    if (ok) {
        const double* p = part + ((size_t)group * nblk * C + c) * 2;
        double a1 = 0.0, b1 = 0.0;   // two independent chains: more partial loads in flight
        int q = ql;
        for (; q + kFinQL < nblk; q += 2 * kFinQL) {
            a += p[(size_t)q * C * 2];
            b += p[(size_t)q * C * 2 + 1];
            a1 += p[(size_t)(q + kFinQL) * C * 2];
            b1 += p[(size_t)(q + kFinQL) * C * 2 + 1];
        }
        if (q < nblk) {
            a += p[(size_t)q * C * 2];
            b += p[(size_t)q * C * 2 + 1];
        }
        a += a1;
        b += b1;
    }
    ra[threadIdx.x] = a;
    rb[threadIdx.x] = b;
    __syncthreads();
    if (!ok || ql != 0) return;
    a = 0.0;
    b = 0.0;
    for (int q = 0; q < kFinQL; ++q) {
        a += ra[slot * kFinQL + q];
        b += rb[slot * kFinQL + q];
    }
    // the partial sums are of (x - k): k = the first voxel's value (norm_stats_kernel), or the caller's per-channel shift (the
    // conv epilogue's sums are of the result without its bias: k = bias, or 0 without one)
    double k = use_shift ? (shift != nullptr ? (double)shift[c] : 0.0) : (double)x[(int64_t)group * gvox * ld + c];
    double cnt = (double)gvox;
    double dm = a / cnt;
    double var = b / cnt - dm * dm;
    if (var < 0.0) var = 0.0;
    double m = k + dm;
    mean[i] = (float)m;
    invstd[i] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean != nullptr && groups == 1) {
        double unb = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unb);
    }
}

// GroupNorm statistics: one thread per (n, group) pools the per-channel shifted moments of its group_c channels.
//   per channel: s = sum(x - k), ss = sum((x - k)^2) with k = first voxel  =>  sum x = s + cnt*k, sum x^2 = ss + 2k*s + cnt*k^2
template <typename T>
__global__ void norm_stats_group_finalize_kernel(const T* __restrict__ x, const double* __restrict__ part,
                                                 float* __restrict__ mean, float* __restrict__ invstd, float eps, int C,
                                                 int ld, int64_t gvox, int nblk, int groups, int group_c) {
    const int G = C / group_c;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= groups * G) return;
    const int n = i / G, g = i - n * G;
    double sx = 0.0, sxx = 0.0;
    const double cnt = (double)gvox;
    for (int c = g * group_c; c < (g + 1) * group_c; ++c) {
        double a = 0.0, b = 0.0;
        const double* p = part + ((size_t)n * nblk * C + c) * 2;
        for (int q = 0; q < nblk; ++q) {
            a += p[(size_t)q * C * 2];
            b += p[(size_t)q * C * 2 + 1];
        }
        const double k = (double)x[(int64_t)n * gvox * ld + c];
        sx += a + cnt * k;
        sxx += b + 2.0 * k * a + cnt * k * k;
    }
    const double m = (double)group_c * cnt;
    const double mu = sx / m;
    double var = sxx / m - mu * mu;
    if (var < 0.0) var = 0.0;
    const float fm = (float)mu, fi = (float)(1.0 / sqrt(var + (double)eps));
    for (int c = g * group_c; c < (g + 1) * group_c; ++c) {
        mean[n * C + c] = fm;
        invstd[n * C + c] = fi;
    }
}

// GroupNorm backward: replace the per-(n,c) sums by the gamma-weighted sums of the channel's group (after dgamma/dbeta
// have been taken from the per-channel sums).
__global__ void norm_act_bwd_group_combine_kernel(float* __restrict__ sums, const float* __restrict__ gamma, int C,
                                                  int groups, int group_c) {
    const int G = C / group_c;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= groups * G) return;
    const int n = i / G, g = i - n * G;
    double g0 = 0.0, g1 = 0.0;
    for (int c = g * group_c; c < (g + 1) * group_c; ++c) {
        const double gm = gamma ? (double)gamma[c] : 1.0;
        g0 += gm * (double)sums[((size_t)n * C + c) * 3];
        g1 += gm * (double)sums[((size_t)n * C + c) * 3 + 1];
    }
    for (int c = g * group_c; c < (g + 1) * group_c; ++c) {
        sums[((size_t)n * C + c) * 3] = (float)g0;
        sums[((size_t)n * C + c) * 3 + 1] = (float)g1;
    }
}

// ------------------------------------------------------------------ forward apply
template <typename T, int VEC>
__global__ void __launch_bounds__(256)
norm_act_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean,
                    const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                    const float* __restrict__ alpha, int alpha_n, int act, float slope, int C, int x_ld, int y_ld,
                    int64_t gvox, int CL, int VT) {
    const int tid = threadIdx.x;
    const int cl = tid % CL, vt = tid / CL;
    const int c0 = (blockIdx.y * CL + cl) * VEC;
    if (vt >= VT || c0 >= C) return;
    const int group = blockIdx.z;
    float sc[VEC], sh[VEC], al[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        int c = c0 + j;
        float gm = gamma ? gamma[c] : 1.f;
        float bt = beta ? beta[c] : 0.f;
        float mu = mean ? mean[group * C + c] : 0.f;
        float is = invstd ? invstd[group * C + c] : 1.f;
        sc[j] = gm * is;
        sh[j] = bt - mu * sc[j];
        al[j] = (act == MRI3D_ACT_PRELU) ? alpha[alpha_n == 1 ? 0 : c] : slope;
    }
    const T* xg = x + (int64_t)group * gvox * x_ld;
    T* yg = y + (int64_t)group * gvox * y_ld;
    for (int64_t v = (int64_t)blockIdx.x * VT + vt; v < gvox; v += (int64_t)gridDim.x * VT) {
        float xv[VEC], yv[VEC];
        Ld<VEC>::load(xg + v * x_ld + c0, xv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) yv[j] = apply_act(fmaf(xv[j], sc[j], sh[j]), act, al[j]);
        Ld<VEC>::store(yg + v * y_ld + c0, yv);
    }
}

// ------------------------------------------------------------------ backward: reductions
// part[group][blk][c][3] = (sum du, sum du*xhat, sum dy*u*[u<=0])
// DX: also write dx = gamma*invstd*du, the whole data gradient when the statistics do not depend on x (training == 0: eval-mode
// BatchNorm, activation-only layers, the frozen-statistics formula of the sync mode) — one pass over x and dy instead of two.
template <typename T, int VEC, bool DX>
__device__ __forceinline__ void
norm_act_bwd_reduce_body(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, double* __restrict__ part,
                         const float* __restrict__ mean, const float* __restrict__ invstd,
                         const float* __restrict__ gamma, const float* __restrict__ beta,
                         const float* __restrict__ alpha, int alpha_n, int act, float slope, int C, int x_ld,
                         int y_ld, int64_t gvox, int CL, int VT) {
    __shared__ double red[256 * 3 * VEC];
    const int tid = threadIdx.x;
    const int cl = tid % CL, vt = tid / CL;
    const int c0 = (blockIdx.y * CL + cl) * VEC;
    const bool active = vt < VT && c0 < C;
    const int group = blockIdx.z;
    double s0[VEC], s1[VEC], s2[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { s0[j] = 0.0; s1[j] = 0.0; s2[j] = 0.0; }
    if (active) {
        float mu[VEC], is[VEC], gm[VEC], bt[VEC], al[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            int c = c0 + j;
            gm[j] = gamma ? gamma[c] : 1.f;
            bt[j] = beta ? beta[c] : 0.f;
            mu[j] = mean ? mean[group * C + c] : 0.f;
            is[j] = invstd ? invstd[group * C + c] : 1.f;
            al[j] = (act == MRI3D_ACT_PRELU) ? alpha[alpha_n == 1 ? 0 : c]
                                              : (act == MRI3D_ACT_LEAKY ? slope : (act == MRI3D_ACT_RELU ? 0.f : 1.f));
        }
        const T* xg = x + (int64_t)group * gvox * x_ld;
        const T* dg = dy + (int64_t)group * gvox * y_ld;
        T* og = DX ? dx + (int64_t)group * gvox * x_ld : nullptr;
        auto accumulate = [&](const float (&xv)[VEC], const float (&gv)[VEC], int64_t v) {
            float ov[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float xh = (xv[j] - mu[j]) * is[j];
                float u = fmaf(gm[j], xh, bt[j]);
                bool pos = u > 0.f;
                float du = pos ? gv[j] : gv[j] * al[j];
                s0[j] += (double)du;
                s1[j] = fma((double)du, (double)xh, s1[j]);
                s2[j] += pos ? 0.0 : (double)gv[j] * (double)u;
                if constexpr (DX) ov[j] = (gm[j] * is[j]) * du;
            }
            if constexpr (DX) Ld<VEC>::store(og + v * x_ld + c0, ov);
        };
        // two voxel rows per trip: four independent 16-byte loads in flight per lane, sums still in voxel order
        const int64_t step = (int64_t)gridDim.x * VT;
        int64_t v = (int64_t)blockIdx.x * VT + vt;
        for (; v + step < gvox; v += 2 * step) {
            float xa[VEC], ga[VEC], xb[VEC], gb[VEC];
            Ld<VEC>::load(xg + v * x_ld + c0, xa);
            Ld<VEC>::load(dg + v * y_ld + c0, ga);
            Ld<VEC>::load(xg + (v + step) * x_ld + c0, xb);
            Ld<VEC>::load(dg + (v + step) * y_ld + c0, gb);
            accumulate(xa, ga, v);
            accumulate(xb, gb, v + step);
        }
        for (; v < gvox; v += step) {
            float xv[VEC], gv[VEC];
            Ld<VEC>::load(xg + v * x_ld + c0, xv);
            Ld<VEC>::load(dg + v * y_ld + c0, gv);
            accumulate(xv, gv, v);
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        red[(tid * VEC + j) * 3] = s0[j];
        red[(tid * VEC + j) * 3 + 1] = s1[j];
        red[(tid * VEC + j) * 3 + 2] = s2[j];
    }
    __syncthreads();
    if (vt == 0 && c0 < C) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            double a = 0.0, b = 0.0, d = 0.0;
            for (int q = 0; q < VT; ++q) {
                a += red[((q * CL + cl) * VEC + j) * 3];
                b += red[((q * CL + cl) * VEC + j) * 3 + 1];
                d += red[((q * CL + cl) * VEC + j) * 3 + 2];
            }
            double* o = part + (((size_t)group * gridDim.x + blockIdx.x) * C + c0 + j) * 3;
            o[0] = a;
            o[1] = b;
            o[2] = d;
        }
    }
}

template <typename T, int VEC>
__global__ void __launch_bounds__(256)
norm_act_bwd_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dy, double* __restrict__ part,
                           const float* __restrict__ mean, const float* __restrict__ invstd,
                           const float* __restrict__ gamma, const float* __restrict__ beta,
                           const float* __restrict__ alpha, int alpha_n, int act, float slope, int C, int x_ld,
                           int y_ld, int64_t gvox, int CL, int VT) {
    norm_act_bwd_reduce_body<T, VEC, false>(x, dy, nullptr, part, mean, invstd, gamma, beta, alpha, alpha_n, act, slope, C, x_ld,
                                            y_ld, gvox, CL, VT);
}

// training == 0 with a parameter gradient wanted: the sums AND dx in one pass (norm_act_bwd_apply_kernel's k1 = k2 = 0)
template <typename T, int VEC>
__global__ void __launch_bounds__(256)
norm_act_bwd_frozen_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, double* __restrict__ part,
                           const float* __restrict__ mean, const float* __restrict__ invstd,
                           const float* __restrict__ gamma, const float* __restrict__ beta,
                           const float* __restrict__ alpha, int alpha_n, int act, float slope, int C, int x_ld,
                           int y_ld, int64_t gvox, int CL, int VT) {
    norm_act_bwd_reduce_body<T, VEC, true>(x, dy, dx, part, mean, invstd, gamma, beta, alpha, alpha_n, act, slope, C, x_ld, y_ld,
                                           gvox, CL, VT);
}

// Stage A: sums[group][c][3] = fixed-order double sums of the per-block partials.
__global__ void __launch_bounds__(256)
norm_act_bwd_sums_kernel(const double* __restrict__ part, float* __restrict__ sums, int C, int nblk, int groups) {
    __shared__ double r0[256], r1[256], r2[256];
    const int slot = threadIdx.x / kFinQL, ql = threadIdx.x % kFinQL;
    const int i = blockIdx.x * (256 / kFinQL) + slot;
    const bool ok = i < groups * C;
    const int group = ok ? i / C : 0, c = ok ? i - group * C : 0;
    double a = 0.0, b = 0.0, d = 0.0;
    if (ok) {
        const double* p = part + ((size_t)group * nblk * C + c) * 3;
        double a1 = 0.0, b1 = 0.0, d1 = 0.0;
        int q = ql;
        for (; q + kFinQL < nblk; q += 2 * kFinQL) {
            a += p[(size_t)q * C * 3];
            b += p[(size_t)q * C * 3 + 1];
            d += p[(size_t)q * C * 3 + 2];
            a1 += p[(size_t)(q + kFinQL) * C * 3];
            b1 += p[(size_t)(q + kFinQL) * C * 3 + 1];
            d1 += p[(size_t)(q + kFinQL) * C * 3 + 2];
        }
        if (q < nblk) {
            a += p[(size_t)q * C * 3];
            b += p[(size_t)q * C * 3 + 1];
            d += p[(size_t)q * C * 3 + 2];
        }
        a += a1;
        b += b1;
        d += d1;
    }
    r0[threadIdx.x] = a;
    r1[threadIdx.x] = b;
    r2[threadIdx.x] = d;
    __syncthreads();
    if (!ok || ql != 0) return;
    a = b = d = 0.0;
    for (int q = 0; q < kFinQL; ++q) {
        a += r0[slot * kFinQL + q];
        b += r1[slot * kFinQL + q];
        d += r2[slot * kFinQL + q];
    }
    sums[(size_t)i * 3] = (float)a;
    sums[(size_t)i * 3 + 1] = (float)b;
    sums[(size_t)i * 3 + 2] = (float)d;
}

// Stage B (one block): dbeta/dgamma = sum over groups; dalpha per channel or grand total.  Run by the first workgroup of the apply
// kernel (batch / instance norm: one launch less per backward, 5 us each, ten per step of the U-Net) or, for GroupNorm — whose
// combine step rewrites `sums` before the apply kernel — as the kernel below.
__device__ __forceinline__ void norm_act_bwd_params_block(const float* __restrict__ sums, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta, float* __restrict__ dalpha, int alpha_n, int C,
                                                          int groups) {
    __shared__ double dal[256];
    double my_dal = 0.0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double tg = 0.0, tb = 0.0, ta = 0.0;
        for (int g = 0; g < groups; ++g) {
            tb += (double)sums[((size_t)g * C + c) * 3];
            tg += (double)sums[((size_t)g * C + c) * 3 + 1];
            ta += (double)sums[((size_t)g * C + c) * 3 + 2];
        }
        if (dgamma) dgamma[c] = (float)tg;
        if (dbeta) dbeta[c] = (float)tb;
        if (dalpha && alpha_n > 1) dalpha[c] = (float)ta;
        my_dal += ta;
    }
    if (dalpha && alpha_n == 1) {
        dal[threadIdx.x] = my_dal;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int i = 0; i < (int)blockDim.x; ++i) t += dal[i];
            dalpha[0] = (float)t;
        }
    }
}

__global__ void norm_act_bwd_params_kernel(const float* __restrict__ sums, float* __restrict__ dgamma,
                                           float* __restrict__ dbeta, float* __restrict__ dalpha, int alpha_n, int C,
                                           int groups) {
    norm_act_bwd_params_block(sums, dgamma, dbeta, dalpha, alpha_n, C, groups);
}

// ------------------------------------------------------------------ backward: dx
template <typename T, int VEC>
__global__ void __launch_bounds__(256)
norm_act_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
                          const float* __restrict__ sums, const float* __restrict__ mean,
                          const float* __restrict__ invstd, const float* __restrict__ gamma,
                          const float* __restrict__ beta, const float* __restrict__ alpha, int alpha_n, int act,
                          float slope, int training, int C, int x_ld, int y_ld, int64_t gvox, int CL, int VT, int group_c,
                          float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dalpha) {
    // the parameter gradients (stage B) ride on the first workgroup; every pointer null = already done / not wanted (uniform)
    if ((dgamma != nullptr || dbeta != nullptr || dalpha != nullptr) && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        norm_act_bwd_params_block(sums, dgamma, dbeta, dalpha, alpha_n, C, (int)gridDim.z);
    const int tid = threadIdx.x;
    const int cl = tid % CL, vt = tid / CL;
    const int c0 = (blockIdx.y * CL + cl) * VEC;
    if (vt >= VT || c0 >= C) return;
    const int group = blockIdx.z;
    float mu[VEC], is[VEC], gm[VEC], bt[VEC], al[VEC], k0[VEC], k1[VEC], k2[VEC];
    const float invM = 1.f / ((float)gvox * (float)(group_c > 0 ? group_c : 1));
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        int c = c0 + j;
        gm[j] = gamma ? gamma[c] : 1.f;
        bt[j] = beta ? beta[c] : 0.f;
        mu[j] = mean ? mean[group * C + c] : 0.f;
        is[j] = invstd ? invstd[group * C + c] : 1.f;
        al[j] = (act == MRI3D_ACT_PRELU) ? alpha[alpha_n == 1 ? 0 : c]
                                          : (act == MRI3D_ACT_LEAKY ? slope : (act == MRI3D_ACT_RELU ? 0.f : 1.f));
        // dx = k0*du - k1 - xhat*k2
        k0[j] = gm[j] * is[j];
        if (training) {
            // batch / instance norm: sums are per channel and scale with gamma*invstd; group norm: sums already hold the
            // gamma-weighted totals of the channel's group and scale with invstd only
            const float kk = group_c > 0 ? is[j] : k0[j];
            k1[j] = kk * sums[((size_t)group * C + c) * 3] * invM;
            k2[j] = kk * sums[((size_t)group * C + c) * 3 + 1] * invM;
        } else {
            k1[j] = 0.f;
            k2[j] = 0.f;
        }
    }
    const T* xg = x + (int64_t)group * gvox * x_ld;
    const T* dg = dy + (int64_t)group * gvox * y_ld;
    T* og = dx + (int64_t)group * gvox * x_ld;
    auto apply = [&](const float (&xv)[VEC], const float (&gv)[VEC], float (&ov)[VEC]) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float xh = (xv[j] - mu[j]) * is[j];
            float u = fmaf(gm[j], xh, bt[j]);
            float du = (u > 0.f) ? gv[j] : gv[j] * al[j];
            ov[j] = fmaf(k0[j], du, -k1[j]) - xh * k2[j];
        }
    };
    // two voxel rows per trip: four independent 16-byte loads in flight per lane
    const int64_t step = (int64_t)gridDim.x * VT;
    int64_t v = (int64_t)blockIdx.x * VT + vt;
    for (; v + step < gvox; v += 2 * step) {
        float xa[VEC], ga[VEC], xb[VEC], gb[VEC], ov[VEC];
        Ld<VEC>::load(xg + v * x_ld + c0, xa);
        Ld<VEC>::load(dg + v * y_ld + c0, ga);
        Ld<VEC>::load(xg + (v + step) * x_ld + c0, xb);
        Ld<VEC>::load(dg + (v + step) * y_ld + c0, gb);
        apply(xa, ga, ov);
        Ld<VEC>::store(og + v * x_ld + c0, ov);
        apply(xb, gb, ov);
        Ld<VEC>::store(og + (v + step) * x_ld + c0, ov);
    }
    for (; v < gvox; v += step) {
        float xv[VEC], gv[VEC], ov[VEC];
        Ld<VEC>::load(xg + v * x_ld + c0, xv);
        Ld<VEC>::load(dg + v * y_ld + c0, gv);
        apply(xv, gv, ov);
        Ld<VEC>::store(og + v * x_ld + c0, ov);
    }
}


// ------------------------------------------------------------------ norm + activation + pointwise head, fused
// out = W . act(norm(x)) + b for a narrow 1x1x1 head (unet.UNet's 16 -> 2 classifier after its last conv -> BatchNorm -> PReLU
// block): the activation a and its gradient da are never stored.  Lane = (voxel row, 4-channel quad), the QC = C/4 lanes of a
// voxel are neighbours (the mapping of norm_act_* with VEC = 4 and of pw_fwd_kernel / pw_dgrad_kernel), so the arithmetic below
// is theirs, expression for expression: the fp32 logits are bit-identical to norm_act_fwd_kernel + pw_fwd_kernel.  In bf16 the
// values the two-operator path stores (a, da) are rounded through bf16 here too.
struct NapArgs {
    const float *mean, *invstd, *gamma, *beta, *alpha;
    int alpha_n, act;
    float slope;
    int C, x_ld;
    int64_t nvox;
};

constexpr int kNapMaxCo = 4;

template <typename T>
__device__ __forceinline__ float through_storage(float v) {
    if constexpr (sizeof(T) == 2) return (float)(bf16_t)v;
    else return v;
}

// per-lane constants of the forward: y = act(x * sc + sh), as norm_act_fwd_kernel forms them
template <int VEC>
__device__ __forceinline__ void nap_fwd_consts(const NapArgs& p, int c0, float (&sc)[VEC], float (&sh)[VEC], float (&al)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        int c = c0 + j;
        float gm = p.gamma ? p.gamma[c] : 1.f;
        float bt = p.beta ? p.beta[c] : 0.f;
        float mu = p.mean ? p.mean[c] : 0.f;
        float is = p.invstd ? p.invstd[c] : 1.f;
        sc[j] = gm * is;
        sh[j] = bt - mu * sc[j];
        al[j] = (p.act == MRI3D_ACT_PRELU) ? p.alpha[p.alpha_n == 1 ? 0 : c] : p.slope;
    }
}

template <typename T, int CO>
__global__ void __launch_bounds__(256)
norm_act_pw_fwd_kernel(const T* __restrict__ x, T* __restrict__ out, const float* __restrict__ w,
                       const float* __restrict__ bias, int Co, int o_ld, NapArgs p) {
    const int QC = p.C >> 2, VT = 256 / QC;
    const int q = threadIdx.x % QC, vt = threadIdx.x / QC;
    float sc[4], sh[4], al[4];
    nap_fwd_consts(p, 4 * q, sc, sh, al);
    float4 wq[CO];
    float bq[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) {   // scalar loads: parameters may be views into a flat buffer (only 4-byte aligned)
        const float* wr = w + (size_t)(co < Co ? co : 0) * p.C + 4 * q;
        wq[co] = co < Co ? make_float4(wr[0], wr[1], wr[2], wr[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        bq[co] = (bias != nullptr && co < Co) ? bias[co] : 0.f;
    }
    constexpr int U = 4;   // read-mostly pass: four voxel rows in flight (as pw_fwd_kernel and norm_stats_kernel)
    const int64_t stride = (int64_t)gridDim.x * VT;
    for (int64_t v0 = (int64_t)blockIdx.x * VT + vt; v0 < p.nvox; v0 += stride * U) {
        float xv[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {   // out-of-range voxels re-read the last one (every lane takes part in the exchanges below)
            const int64_t v = v0 + u * stride;
            Ld<4>::load(x + (v < p.nvox ? v : p.nvox - 1) * p.x_ld + 4 * q, xv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t v = v0 + u * stride;
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = through_storage<T>(apply_act(fmaf(xv[u][j], sc[j], sh[j]), p.act, al[j]));
            float acc[CO];
#pragma unroll
            for (int co = 0; co < CO; ++co) {
                float t = a[0] * wq[co].x;
                t = fmaf(a[1], wq[co].y, t);
                t = fmaf(a[2], wq[co].z, t);
                t = fmaf(a[3], wq[co].w, t);
                for (int d = 1; d < QC; d <<= 1) t += __shfl_xor(t, d, 64);   // the voxel's quads are QC neighbouring lanes
                acc[co] = t + bq[co];
            }
            if (q == 0 && v < p.nvox) {
                T* op = out + v * o_ld;
#pragma unroll
                for (int co = 0; co < CO; ++co)
                    if (co < Co) stf(op + co, acc[co]);
            }
        }
    }
}

// Where the backward kernels below take the gradient of the activation from.  Here: da = W^T dout of the pointwise head, with
// the head's own parameter gradients (dw, dbias) as side sums.  Another source (a skip gradient plus a pool scatter) plugs in
// with the same five members.
template <typename T, int CO>
struct PwHeadGrad {
    struct Args {
        const T* dout;
        const float* w;
        int Co, ld;
    };
    struct Val {                           // what a lane loads per voxel row
        float g[CO];
    };
    static constexpr int kSide = 5 * CO;   // doubles per lane: dw[4][CO], dbias[CO]
    const T* dout;
    int Co, ld;
    float4 wq[CO];
    double dw[4][CO], db[CO];

    __device__ __forceinline__ void init(const Args& a, int C, int q) {
        dout = a.dout, Co = a.Co, ld = a.ld;
#pragma unroll
        for (int co = 0; co < CO; ++co) {
            const float* wr = a.w + (size_t)(co < Co ? co : 0) * C + 4 * q;
            wq[co] = co < Co ? make_float4(wr[0], wr[1], wr[2], wr[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            db[co] = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) dw[j][co] = 0.0;
        }
    }
    __device__ __forceinline__ void load(int64_t v, Val& val) const {
#pragma unroll
        for (int co = 0; co < CO; ++co) val.g[co] = co < Co ? ldf(dout + v * ld + co) : 0.f;
    }
    // pw_dgrad_kernel's order; the two-operator path stores da in the activation's storage type
    __device__ __forceinline__ void grad(const Val& val, float (&da)[4]) const {
        const float (&gv)[CO] = val.g;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int co = 0; co < CO; ++co) {
            acc.x = fmaf(gv[co], wq[co].x, acc.x);
            acc.y = fmaf(gv[co], wq[co].y, acc.y);
            acc.z = fmaf(gv[co], wq[co].z, acc.z);
            acc.w = fmaf(gv[co], wq[co].w, acc.w);
        }
        da[0] = through_storage<T>(acc.x), da[1] = through_storage<T>(acc.y);
        da[2] = through_storage<T>(acc.z), da[3] = through_storage<T>(acc.w);
    }
    // a = the forward's activation of this lane's quad (pw_wgrad_kernel: float product, double sum)
    __device__ __forceinline__ void side(const float (&a)[4], const Val& val, bool lead) {
        const float (&gv)[CO] = val.g;
#pragma unroll
        for (int co = 0; co < CO; ++co) {
#pragma unroll
            for (int j = 0; j < 4; ++j) dw[j][co] += (double)(a[j] * gv[co]);
            if (lead) db[co] += (double)gv[co];
        }
    }
    // block partial: spart[blk][Co*C + Co] = (dw[co][c], dbias[co]), summed over the block's VT voxel rows in row order
    __device__ __forceinline__ void flush(double* red, double* __restrict__ spart, int C, int QC, int VT) const {
        const int tid = threadIdx.x;
#pragma unroll
        for (int co = 0; co < CO; ++co) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[tid * kSide + j * CO + co] = dw[j][co];
            red[tid * kSide + 4 * CO + co] = db[co];
        }
        __syncthreads();
        double* o = spart + (size_t)blockIdx.x * (Co * C + Co);
        for (int e = tid; e < QC * 4 * CO; e += 256) {
            const int co = e % CO, j = (e / CO) % 4, qq = e / (4 * CO);
            double s = 0.0;
            for (int l = 0; l < VT; ++l) s += red[(l * QC + qq) * kSide + j * CO + co];
            if (co < Co) o[co * C + 4 * qq + j] = s;
        }
        if (tid < Co) {
            double s = 0.0;
            for (int l = 0; l < VT; ++l) s += red[(l * QC) * kSide + 4 * CO + tid];
            o[Co * C + tid] = s;
        }
    }
};

// SUMS: the per-block partials of (sum du, sum du*xhat, sum da*u*[u<=0]) as norm_act_bwd_reduce_kernel forms them, plus the
// source's side sums.  DX: dx = k0*du - k1 - xhat*k2 as norm_act_bwd_apply_kernel writes it.  Training statistics take two
// launches (<true, false>, then <false, true> once the sums are combined); with frozen statistics k1 = k2 = 0 and <true, true>
// does both in one pass.  The body is shared by one entry point per gradient source.
template <typename T, class SRC, bool SUMS, bool DX>
__device__ __forceinline__ void
norm_act_src_bwd_body(const T* __restrict__ x, T* __restrict__ dx, const typename SRC::Args& sa, const NapArgs& p,
                      const float* __restrict__ sums, int training, double* __restrict__ part, double* __restrict__ spart,
                      float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dalpha) {
    constexpr int kRed = SUMS ? (SRC::kSide > 12 ? SRC::kSide : 12) : 1;
    __shared__ double red[256 * kRed];
    // the parameter gradients ride on the first workgroup of the dx pass that follows the combined sums (uniform branch)
    if (!SUMS && (dgamma != nullptr || dbeta != nullptr || dalpha != nullptr) && blockIdx.x == 0)
        norm_act_bwd_params_block(sums, dgamma, dbeta, dalpha, p.alpha_n, p.C, 1);
    const int QC = p.C >> 2, VT = 256 / QC;
    const int tid = threadIdx.x;
    const int q = tid % QC, vt = tid / QC;
    const int c0 = 4 * q;
    float mu[4], is[4], gm[4], bt[4], al[4], k0[4], k1[4], k2[4];
    const float invM = 1.f / (float)p.nvox;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c = c0 + j;
        gm[j] = p.gamma ? p.gamma[c] : 1.f;
        bt[j] = p.beta ? p.beta[c] : 0.f;
        mu[j] = p.mean ? p.mean[c] : 0.f;
        is[j] = p.invstd ? p.invstd[c] : 1.f;
        al[j] = (p.act == MRI3D_ACT_PRELU) ? p.alpha[p.alpha_n == 1 ? 0 : c]
                                            : (p.act == MRI3D_ACT_LEAKY ? p.slope : (p.act == MRI3D_ACT_RELU ? 0.f : 1.f));
        k0[j] = gm[j] * is[j];
        if (DX && !SUMS && training) {
            k1[j] = k0[j] * sums[(size_t)c * 3] * invM;
            k2[j] = k0[j] * sums[(size_t)c * 3 + 1] * invM;
        } else {
            k1[j] = 0.f;
            k2[j] = 0.f;
        }
    }
    float sc[4], sh[4], af[4];   // the forward's constants: the side sums want the activation exactly as the forward formed it
    if constexpr (SUMS && SRC::kSide > 0) nap_fwd_consts(p, c0, sc, sh, af);
    SRC src;
    src.init(sa, p.C, q);
    double s0[4], s1[4], s2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { s0[j] = 0.0; s1[j] = 0.0; s2[j] = 0.0; }
    auto row = [&](const float (&xv)[4], const typename SRC::Val& gv, int64_t v) {
        float da[4], ov[4];
        src.grad(gv, da);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float xh = (xv[j] - mu[j]) * is[j];
            float u = fmaf(gm[j], xh, bt[j]);
            bool pos = u > 0.f;
            float du = pos ? da[j] : da[j] * al[j];
            if constexpr (SUMS) {
                s0[j] += (double)du;
                s1[j] = fma((double)du, (double)xh, s1[j]);
                s2[j] += pos ? 0.0 : (double)da[j] * (double)u;
            }
            if constexpr (DX) ov[j] = fmaf(k0[j], du, -k1[j]) - xh * k2[j];
        }
        if constexpr (SUMS && SRC::kSide > 0) {
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = through_storage<T>(apply_act(fmaf(xv[j], sc[j], sh[j]), p.act, af[j]));
            src.side(a, gv, q == 0);
        }
        if constexpr (DX) Ld<4>::store(dx + v * p.x_ld + c0, ov);
    };
    // two voxel rows per trip, sums in voxel order
    const int64_t step = (int64_t)gridDim.x * VT;
    int64_t v = (int64_t)blockIdx.x * VT + vt;
    for (; v + step < p.nvox; v += 2 * step) {
        float xa[4], xb[4];
        typename SRC::Val ga, gb;
        Ld<4>::load(x + v * p.x_ld + c0, xa);
        src.load(v, ga);
        Ld<4>::load(x + (v + step) * p.x_ld + c0, xb);
        src.load(v + step, gb);
        row(xa, ga, v);
        row(xb, gb, v + step);
    }
    for (; v < p.nvox; v += step) {
        float xv[4];
        typename SRC::Val gv;
        Ld<4>::load(x + v * p.x_ld + c0, xv);
        src.load(v, gv);
        row(xv, gv, v);
    }
    if constexpr (SUMS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            red[(tid * 4 + j) * 3] = s0[j];
            red[(tid * 4 + j) * 3 + 1] = s1[j];
            red[(tid * 4 + j) * 3 + 2] = s2[j];
        }
        __syncthreads();
        if (vt == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double a = 0.0, b = 0.0, d = 0.0;
                for (int l = 0; l < VT; ++l) {
                    a += red[((l * QC + q) * 4 + j) * 3];
                    b += red[((l * QC + q) * 4 + j) * 3 + 1];
                    d += red[((l * QC + q) * 4 + j) * 3 + 2];
                }
                double* o = part + ((size_t)blockIdx.x * p.C + c0 + j) * 3;
                o[0] = a;
                o[1] = b;
                o[2] = d;
            }
        }
        if constexpr (SRC::kSide > 0) {
            __syncthreads();
            src.flush(red, spart, p.C, QC, VT);
        }
    }
}

template <typename T, class SRC, bool SUMS, bool DX>
__global__ void __launch_bounds__(256)
norm_act_src_bwd_kernel(const T* __restrict__ x, T* __restrict__ dx, typename SRC::Args sa, NapArgs p,
                        const float* __restrict__ sums, int training, double* __restrict__ part, double* __restrict__ spart,
                        float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dalpha) {
    norm_act_src_bwd_body<T, SRC, SUMS, DX>(x, dx, sa, p, sums, training, part, spart, dgamma, dbeta, dalpha);
}

// dw[co][c], dbias[co] = fixed-order double sums of the per-block side partials: 256 threads = 8 elements x 32 partial lanes
__global__ void __launch_bounds__(256)
norm_act_pw_wsum_kernel(const double* __restrict__ spart, float* __restrict__ dw, float* __restrict__ dbias, int nb, int nw,
                        int Co) {
    __shared__ double red[256];
    const int el = threadIdx.x >> 5, ql = threadIdx.x & 31;
    const int ntot = nw + Co;
    const int i = blockIdx.x * 8 + el;
    double s = 0.0;
    if (i < ntot)
        for (int b = ql; b < nb; b += 32) s += spart[(size_t)b * ntot + i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (ql == 0 && i < ntot) {
        double t = 0.0;
        for (int k = 0; k < 32; ++k) t += red[el * 32 + k];
        if (i < nw) {
            if (dw != nullptr) dw[i] = (float)t;
        } else if (dbias != nullptr) {
            dbias[i - nw] = (float)t;
        }
    }
}

// ------------------------------------------------------------------ norm + activation + MaxPool3d(2), fused
// An encoder level of unet.UNet ends conv -> BatchNorm -> PReLU -> (skip, MaxPool3d(2)).  Forward: one pass reads the conv output
// and writes the activation (the skip tensor), the pooled tensor and the arg-max bytes — the pool does not read the activation
// back.  Lane mapping and selection rule are maxpool2_fwd_kernel's (resample.hip): a lane owns one input column x VEC channels,
// takes its four (kd, kh) taps and meets its kw partner, CV lanes away, in one shuffle; the first maximum in raster order wins,
// NaN propagates with the later NaN's index.  The activation is formed as norm_act_fwd_kernel forms it and, in bf16, rounded
// through storage before it is compared: skip, pooled and index bytes are those of the two operators.
template <typename T, int VEC>
__global__ void __launch_bounds__(256)
norm_act_pool_fwd_kernel(Mri3dPoolGeom g, const T* __restrict__ x, T* __restrict__ skip, T* __restrict__ y,
                         uint8_t* __restrict__ idx, int hch, NapArgs p) {
    const unsigned CV = g.c / VEC;            // lanes per voxel: a power of two <= 16 (host)
    const int hchunks = (g.ho + hch - 1) / hch;
    const int slabs = g.n * g.dout * hchunks;
    // element strides of x (pitch p.x_ld) and of skip (pitch g.x_ld): one sample of either is below 2^31 elements (host)
    const unsigned xrow = (unsigned)g.wi * p.x_ld, xplane = (unsigned)g.hi * xrow;
    const unsigned srow = (unsigned)g.wi * g.x_ld, splane = (unsigned)g.hi * srow;
    const unsigned cv = threadIdx.x % CV;     // 256 % CV == 0: a lane keeps its channels
    float sc[VEC], sh[VEC], al[VEC];
    nap_fwd_consts(p, (int)cv * VEC, sc, sh, al);
    for (int slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
        const int hc = slab % hchunks, nd = slab / hchunks;
        const int n = nd / g.dout, od = nd - n * g.dout;
        const int h0 = hc * hch, hn = min(hch, g.ho - h0);
        const unsigned inner = (unsigned)hn * g.wi * CV;   // lanes walk (oh, input column iw, channel vector)
        const int64_t sample = ((int64_t)n * g.di + 2 * od) * g.hi * g.wi;
        const T* xs = x + sample * p.x_ld;
        T* ss = skip + sample * g.x_ld;
        const int64_t obase = ((int64_t)nd * g.ho + h0) * g.wo;
        for (unsigned e0 = 0; e0 < inner; e0 += blockDim.x) {   // whole block iterates together: the shuffle needs both kw lanes
            const unsigned e = e0 + threadIdx.x;
            const bool live = e < inner;
            const unsigned col = (live ? e : 0) / CV;
            const unsigned iw = col % g.wi, ohl = col / g.wi;
            const unsigned kw = iw & 1, ow = iw >> 1, oh = h0 + ohl;
            const T* xp = xs + (2 * oh) * xrow + iw * (unsigned)p.x_ld + cv * VEC;
            T* sp = ss + (2 * oh) * srow + iw * (unsigned)g.x_ld + cv * VEC;
            float v[4][VEC];
#pragma unroll
            for (int t = 0; t < 4; ++t) Ld<VEC>::load(xp + (t >> 1) * xplane + (t & 1) * xrow, v[t]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[t][j] = through_storage<T>(apply_act(fmaf(v[t][j], sc[j], sh[j]), p.act, al[j]));
                if (live) Ld<VEC>::store(sp + (t >> 1) * splane + (t & 1) * srow, v[t]);
            }
            float best[VEC];
            int bi[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) { best[j] = v[0][j]; bi[j] = (int)kw; }
#pragma unroll
            for (int t = 1; t < 4; ++t)
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    if (v[t][j] > best[j] || v[t][j] != v[t][j]) { best[j] = v[t][j]; bi[j] = 2 * t + (int)kw; }
            // merge with the other kw lane (CV lanes away; wi is even and CV | 64, so both are in the same wave and both live)
            float o[VEC];
            int oi[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float pb = __shfl_xor(best[j], (int)CV, 64);
                const int pi = __shfl_xor(bi[j], (int)CV, 64);
                const bool mine_nan = best[j] != best[j], his_nan = pb != pb;
                bool take_his;
                if (mine_nan || his_nan) take_his = his_nan && (!mine_nan || pi > bi[j]);     // the LAST NaN in raster order
                else take_his = pb > best[j] || (pb == best[j] && pi < bi[j]);                  // the FIRST maximum
                o[j] = take_his ? pb : best[j];
                oi[j] = take_his ? pi : bi[j];
            }
            if (live && kw == 0) {
                const int64_t ov = obase + (int64_t)ohl * g.wo + ow;
                Ld<VEC>::store(y + ov * g.y_ld + cv * VEC, o);
                uint8_t* ip = idx + ov * g.c + cv * VEC;
                if constexpr (VEC == 8) {
                    uint2 pk;
                    pk.x = (uint32_t)oi[0] | ((uint32_t)oi[1] << 8) | ((uint32_t)oi[2] << 16) | ((uint32_t)oi[3] << 24);
                    pk.y = (uint32_t)oi[4] | ((uint32_t)oi[5] << 8) | ((uint32_t)oi[6] << 16) | ((uint32_t)oi[7] << 24);
                    *reinterpret_cast<uint2*>(ip) = pk;
                } else {
                    *reinterpret_cast<uint32_t*>(ip) = (uint32_t)oi[0] | ((uint32_t)oi[1] << 8) | ((uint32_t)oi[2] << 16) | ((uint32_t)oi[3] << 24);
                }
            }
        }
    }
}

// Gradient source of the encoder tail: da = dskip + scatter(dpool), the sum maxpool_bwd_kernel forms with the skip gradient as
// its addend (addend first, one add where the window's arg-max is this voxel; in bf16 rounded through storage as the stored da
// was).  Either gradient may be absent (NULL = zeros).  No side sums.  A lane finds its window from the flat voxel index with
// 32-bit arithmetic: v = (n*di + d)*hi*wi + h*wi + w below 2^31 (host), extents even, so the pooled row is (nd/2)*ho + h/2.
template <typename T>
struct PoolSkipGrad {
    struct Args {
        const T *dskip, *dpool;
        const uint8_t* idx;
        int s_ld, p_ld;          // voxel pitch of dskip and of dpool
        unsigned wi, hi;         // input extents (wo = wi/2, ho = hi/2)
    };
    struct Val {
        float ds[4], dp[4];
        uint32_t ib, tap;        // the window's four index bytes; this voxel's tap
    };
    static constexpr int kSide = 0;
    Args a;
    int C, c0;

    __device__ __forceinline__ void init(const Args& args, int C_, int q) { a = args, C = C_, c0 = 4 * q; }
    __device__ __forceinline__ void load(int64_t v, Val& val) const {
        if (a.dskip != nullptr) {
            Ld<4>::load(a.dskip + v * a.s_ld + c0, val.ds);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) val.ds[j] = 0.f;
        }
        val.ib = 0, val.tap = 0xff;   // no tap is 255: without dpool nothing is added
        if (a.dpool != nullptr) {
            const unsigned u = (unsigned)v;
            const unsigned r = u / a.wi, w = u - r * a.wi;   // r = (n*di + d)*hi + h
            const unsigned nd = r / a.hi, h = r - nd * a.hi;
            const int64_t pv = ((int64_t)(nd >> 1) * (a.hi >> 1) + (h >> 1)) * (a.wi >> 1) + (w >> 1);
            Ld<4>::load(a.dpool + pv * a.p_ld + c0, val.dp);
            val.ib = *reinterpret_cast<const uint32_t*>(a.idx + pv * C + c0);
            val.tap = ((nd & 1) * 2 + (h & 1)) * 2 + (w & 1);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) val.dp[j] = 0.f;
        }
    }
    __device__ __forceinline__ void grad(const Val& val, float (&da)[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = val.ds[j];
            if (((val.ib >> (8 * j)) & 0xff) == val.tap) acc += val.dp[j];
            da[j] = through_storage<T>(acc);
        }
    }
    __device__ __forceinline__ void side(const float (&)[4], const Val&, bool) {}
    __device__ __forceinline__ void flush(double*, double* __restrict__, int, int, int) const {}
};

template <typename T, bool SUMS, bool DX>
__global__ void __launch_bounds__(256)
norm_act_pool_bwd_kernel(const T* __restrict__ x, T* __restrict__ dx, typename PoolSkipGrad<T>::Args sa, NapArgs p,
                         const float* __restrict__ sums, int training, double* __restrict__ part,
                         float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dalpha) {
    norm_act_src_bwd_body<T, PoolSkipGrad<T>, SUMS, DX>(x, dx, sa, p, sums, training, part, nullptr, dgamma, dbeta, dalpha);
}

struct NapPlan {
    int QC, VT, nblk;
    size_t sums_off, side_off, bytes;   // byte offsets into the workspace (the norm partials start it)
    // the regions of a workspace of `bytes` bytes: per-block norm partials, combined sums, per-block side partials of the source
    double* part(void* ws) const { return static_cast<double*>(ws); }
    float* sums(void* ws) const { return reinterpret_cast<float*>(static_cast<char*>(ws) + sums_off); }
    double* spart(void* ws) const { return reinterpret_cast<double*>(static_cast<char*>(ws) + side_off); }
};

static bool nap_supported(const Mri3dNormGeom& g, int co) {
    if (g.dtype != MRI3D_F32 && g.dtype != MRI3D_BF16) return false;
    if (g.n <= 0 || g.vox <= 0 || g.instance || g.group_c != 0) return false;
    const int qc = g.c / 4;
    if (g.c <= 0 || g.c % 4 != 0 || qc > 16 || (qc & (qc - 1)) != 0) return false;
    if (co < 1 || co > kNapMaxCo) return false;
    if (g.x_ld < g.c || g.x_ld % 4 != 0 || g.y_ld < co) return false;
    if (g.act < MRI3D_ACT_NONE || g.act > MRI3D_ACT_PRELU) return false;
    if (g.act == MRI3D_ACT_PRELU && g.alpha_n != 1 && g.alpha_n != g.c) return false;
    return true;
}

static NapPlan nap_plan(const Mri3dNormGeom& g, int co) {
    NapPlan p;
    p.QC = g.c / 4;
    p.VT = 256 / p.QC;
    const int64_t nvox = (int64_t)g.n * g.vox;
    const int64_t want = cdiv64(nvox, (int64_t)p.VT * 8);   // >= 8 voxel rows per thread, as norm_plan
    p.nblk = (int)(want < kNormMaxBlocks ? want : kNormMaxBlocks);
    if (p.nblk < 1) p.nblk = 1;
    p.sums_off = (size_t)p.nblk * g.c * 3 * sizeof(double);
    p.side_off = p.sums_off + align_up((size_t)g.c * 3 * sizeof(float), sizeof(double));
    p.bytes = p.side_off + (size_t)p.nblk * (co * g.c + co) * sizeof(double);
    return p;
}

}  // namespace mri3d

using namespace mri3d;

extern "C" size_t mri3d_norm_workspace_bytes(const Mri3dNormGeom* g) {
    if (!g) return 0;
    return norm_workspace_floats(*g) * sizeof(float);
}

static int norm_check(const Mri3dNormGeom* g, const char* who) {
    MRI3D_REQUIRE(g != nullptr, MRI3D_EINVAL, "%s: null geometry", who);
    MRI3D_REQUIRE(g->dtype == MRI3D_F32 || g->dtype == MRI3D_BF16, MRI3D_ENOTSUP, "%s: unknown dtype %d", who, g->dtype);
    MRI3D_REQUIRE(g->n > 0 && g->vox > 0 && g->c > 0 && g->x_ld >= g->c && g->y_ld >= g->c, MRI3D_EINVAL,
                  "%s: bad geometry n=%d vox=%lld c=%d x_ld=%d y_ld=%d", who, g->n, (long long)g->vox, g->c, g->x_ld,
                  g->y_ld);
    MRI3D_REQUIRE(g->act != MRI3D_ACT_PRELU || g->alpha_n == 1 || g->alpha_n == g->c, MRI3D_EINVAL,
                  "%s: PReLU alpha_n=%d must be 1 or C=%d", who, g->alpha_n, g->c);
    MRI3D_REQUIRE(g->group_c == 0 || (g->group_c > 0 && g->instance && g->c % g->group_c == 0), MRI3D_EINVAL,
                  "%s: group_c=%d needs instance mode and must divide C=%d", who, g->group_c, g->c);
    return MRI3D_OK;
}

extern "C" int32_t mri3d_norm_plan_query(const Mri3dNormGeom* g, int32_t pass, int32_t align, Mri3dNormPlanInfo* out) {
    int rc = norm_check(g, "norm_plan_query");
    if (rc) return rc;
    MRI3D_REQUIRE(out != nullptr, MRI3D_EINVAL, "norm_plan_query: null result");
    MRI3D_REQUIRE(pass == MRI3D_NORM_PASS_STATS || pass == MRI3D_NORM_PASS_FWD || pass == MRI3D_NORM_PASS_BWD, MRI3D_EINVAL,
                  "norm_plan_query: unknown pass %d", pass);
    MRI3D_REQUIRE(align > 0 && (align & (align - 1)) == 0, MRI3D_EINVAL, "norm_plan_query: align %d is no power of two", align);
    const NormPlan p = norm_plan_for(*g, pass, align);
    out->vec = p.vec, out->CL = p.CL, out->VT = p.VT, out->cy = p.cy, out->nblk = p.nblk, out->groups = p.groups;
    out->gvox = p.gvox;
    return MRI3D_OK;
}

// what every norm_act entry point asks of its statistics and activation arguments (the forward ones pass training = 0)
static int norm_act_args_check(const Mri3dNormGeom* g, int training, const float* mean, const float* invstd, const float* alpha,
                               const char* who) {
    MRI3D_REQUIRE((mean == nullptr) == (invstd == nullptr), MRI3D_EINVAL, "%s: mean/invstd must both be set", who);
    MRI3D_REQUIRE(!(training && mean == nullptr), MRI3D_EINVAL, "%s: training mode needs statistics", who);
    MRI3D_REQUIRE(g->act != MRI3D_ACT_PRELU || alpha, MRI3D_EINVAL, "%s: PReLU needs alpha", who);
    return MRI3D_OK;
}

extern "C" int mri3d_norm_stats(const Mri3dNormGeom* g, const void* x, float* mean, float* invstd, float* running_mean,
                                float* running_var, float momentum, void* workspace, size_t ws_bytes,
                                mri3d_stream_t stream) {
    int rc = norm_check(g, "norm_stats");
    if (rc) return rc;
    MRI3D_REQUIRE(x && mean && invstd, MRI3D_EINVAL, "norm_stats: null pointer");
    MRI3D_REQUIRE(workspace && ws_bytes >= mri3d_norm_workspace_bytes(g), MRI3D_EWORKSPACE,
                  "norm_stats: workspace %zu < %zu", ws_bytes, mri3d_norm_workspace_bytes(g));
    hipStream_t s = static_cast<hipStream_t>(stream);
    NormPlan p = norm_plan_for(*g, MRI3D_NORM_PASS_STATS, ptr_align(x));
    double* part = static_cast<double*>(workspace);
    dim3 grid(p.nblk, p.cy, p.groups);
    const int tot = p.groups * g->c;
    MRI3D_DISPATCH_DTYPE(g->dtype, T, {
        const T* xf = static_cast<const T*>(x);
        MRI3D_DISPATCH_VEC(p.vec, false, VEC, {
            hipLaunchKernelGGL((norm_stats_kernel<T, VEC>), grid, dim3(256), 0, s, xf, part, g->c, g->x_ld, p.gvox, p.CL, p.VT);
        });
        hipLaunchKernelGGL(norm_stats_finalize_kernel<T>, dim3(cdiv(tot, 256 / kFinQL)), dim3(256), 0, s, xf, part, mean,
                           invstd, running_mean, running_var, momentum, g->eps, g->c, g->x_ld, p.gvox, p.nblk, p.groups);
        if (g->group_c > 0) {
            const int ng = p.groups * (g->c / g->group_c);
            hipLaunchKernelGGL(norm_stats_group_finalize_kernel<T>, dim3(cdiv(ng, 64)), dim3(64), 0, s, xf, part, mean,
                               invstd, g->eps, g->c, g->x_ld, p.gvox, p.nblk, p.groups, g->group_c);
        }
    });
    return check_launch("norm_stats");
}

extern "C" int mri3d_norm_stats_from_partials(const Mri3dNormGeom* g, const double* partials, int32_t nblk, const float* shift,
                                              float* mean, float* invstd, float* running_mean, float* running_var,
                                              float momentum, mri3d_stream_t stream) {
    int rc = norm_check(g, "norm_stats_from_partials");
    if (rc) return rc;
    MRI3D_REQUIRE(partials && mean && invstd && nblk > 0, MRI3D_EINVAL, "norm_stats_from_partials: null pointer / no partials");
    MRI3D_REQUIRE(!g->instance && g->group_c == 0, MRI3D_ENOTSUP,
                  "norm_stats_from_partials: batch statistics only (one group over N x voxels)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t gvox = (int64_t)g->n * g->vox;
    hipLaunchKernelGGL(norm_stats_finalize_kernel<float>, dim3(cdiv(g->c, 256 / kFinQL)), dim3(256), 0, s,
                       static_cast<const float*>(nullptr), partials, mean, invstd, running_mean, running_var, momentum, g->eps,
                       g->c, g->x_ld, gvox, nblk, 1, shift, 1);
    return check_launch("norm_stats_from_partials");
}

extern "C" int mri3d_norm_act_fwd(const Mri3dNormGeom* g, const void* x, const float* mean, const float* invstd,
                                  const float* gamma, const float* beta, const float* alpha, void* y,
                                  mri3d_stream_t stream) {
    int rc = norm_check(g, "norm_act_fwd");
    if (rc) return rc;
    MRI3D_REQUIRE(x && y, MRI3D_EINVAL, "norm_act_fwd: null pointer");
    if ((rc = norm_act_args_check(g, 0, mean, invstd, alpha, "norm_act_fwd"))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    NormPlan p = norm_plan_for(*g, MRI3D_NORM_PASS_FWD, ptr_align(x, y));
    dim3 grid(p.nblk, p.cy, p.groups);
    MRI3D_DISPATCH_DTYPE(g->dtype, T, {
        const T* xf = static_cast<const T*>(x);
        T* yf = static_cast<T*>(y);
        MRI3D_DISPATCH_VEC(p.vec, sizeof(T) == 2, VEC, {
            hipLaunchKernelGGL((norm_act_fwd_kernel<T, VEC>), grid, dim3(256), 0, s, xf, yf, mean, invstd, gamma, beta, alpha,
                               g->alpha_n, g->act, g->slope, g->c, g->x_ld, g->y_ld, p.gvox, p.CL, p.VT);
        });
    });
    return check_launch("norm_act_fwd");
}

extern "C" int mri3d_norm_act_bwd(const Mri3dNormGeom* g, int training, const void* x, const void* dy,
                                  const float* mean, const float* invstd, const float* gamma, const float* beta,
                                  const float* alpha, void* dx, float* dgamma, float* dbeta, float* dalpha,
                                  void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = norm_check(g, "norm_act_bwd");
    if (rc) return rc;
    MRI3D_REQUIRE(x && dy && dx, MRI3D_EINVAL, "norm_act_bwd: null pointer");
    if ((rc = norm_act_args_check(g, training, mean, invstd, alpha, "norm_act_bwd"))) return rc;
    MRI3D_REQUIRE(workspace && ws_bytes >= mri3d_norm_workspace_bytes(g), MRI3D_EWORKSPACE,
                  "norm_act_bwd: workspace %zu < %zu", ws_bytes, mri3d_norm_workspace_bytes(g));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // x/dx share pitch x_ld, dy has pitch y_ld
    NormPlan p = norm_plan_for(*g, MRI3D_NORM_PASS_BWD, ptr_align(x, dy, dx));   // 8 channels per lane: reduce 66 -> 101 us, apply 74 -> 83 us (bf16 bench): not used
    dim3 grid(p.nblk, p.cy, p.groups);
    double* part = static_cast<double*>(workspace);
    float* sums = reinterpret_cast<float*>(part + (size_t)p.groups * p.nblk * g->c * 3);
    const bool need_reduce = training || dgamma || dbeta || dalpha;
    bool params_done = false;
    MRI3D_DISPATCH_DTYPE(g->dtype, T, {
        const T* xf = static_cast<const T*>(x);
        const T* df = static_cast<const T*>(dy);
        T* of = static_cast<T*>(dx);
        if (need_reduce && !training) {
            // nothing in dx depends on the sums: one pass writes dx and the per-block partials, then the two small kernels
            MRI3D_DISPATCH_VEC(p.vec, false, VEC, {
                hipLaunchKernelGGL((norm_act_bwd_frozen_kernel<T, VEC>), grid, dim3(256), 0, s, xf, df, of, part, mean, invstd,
                                   gamma, beta, alpha, g->alpha_n, g->act, g->slope, g->c, g->x_ld, g->y_ld, p.gvox, p.CL,
                                   p.VT);
            });
            hipLaunchKernelGGL(norm_act_bwd_sums_kernel, dim3(cdiv(p.groups * g->c, 256 / kFinQL)), dim3(256), 0, s, part,
                               sums, g->c, p.nblk, p.groups);
            hipLaunchKernelGGL(norm_act_bwd_params_kernel, dim3(1), dim3(256), 0, s, sums, dgamma, dbeta, dalpha, g->alpha_n,
                               g->c, p.groups);
            return check_launch("norm_act_bwd");
        }
        if (need_reduce) {
            MRI3D_DISPATCH_VEC(p.vec, false, VEC, {
                hipLaunchKernelGGL((norm_act_bwd_reduce_kernel<T, VEC>), grid, dim3(256), 0, s, xf, df, part, mean, invstd,
                                   gamma, beta, alpha, g->alpha_n, g->act, g->slope, g->c, g->x_ld, g->y_ld, p.gvox, p.CL,
                                   p.VT);
            });
            hipLaunchKernelGGL(norm_act_bwd_sums_kernel, dim3(cdiv(p.groups * g->c, 256 / kFinQL)), dim3(256), 0, s, part,
                               sums, g->c, p.nblk, p.groups);
            if ((dgamma || dbeta || dalpha) && g->group_c > 0) {   // GroupNorm: before the combine step rewrites `sums`
                hipLaunchKernelGGL(norm_act_bwd_params_kernel, dim3(1), dim3(256), 0, s, sums, dgamma, dbeta, dalpha,
                                   g->alpha_n, g->c, p.groups);
                params_done = true;
            }
            if (g->group_c > 0 && training) {
                const int ng = p.groups * (g->c / g->group_c);
                hipLaunchKernelGGL(norm_act_bwd_group_combine_kernel, dim3(cdiv(ng, 64)), dim3(64), 0, s, sums, gamma,
                                   g->c, p.groups, g->group_c);
            }
        }
        float* pg = params_done ? nullptr : dgamma;
        float* pb = params_done ? nullptr : dbeta;
        float* pa = params_done ? nullptr : dalpha;
        MRI3D_DISPATCH_VEC(p.vec, false, VEC, {
            hipLaunchKernelGGL((norm_act_bwd_apply_kernel<T, VEC>), grid, dim3(256), 0, s, xf, df, of, sums, mean, invstd,
                               gamma, beta, alpha, g->alpha_n, g->act, g->slope, training, g->c, g->x_ld, g->y_ld, p.gvox,
                               p.CL, p.VT, g->group_c, pg, pb, pa);
        });
    });
    return check_launch("norm_act_bwd");
}

extern "C" int32_t mri3d_norm_act_pw_supported(const Mri3dNormGeom* g, int32_t co) {
    return (g != nullptr && nap_supported(*g, co)) ? 1 : 0;
}

extern "C" size_t mri3d_norm_act_pw_workspace_bytes(const Mri3dNormGeom* g, int32_t co) {
    if (g == nullptr || !nap_supported(*g, co)) return 0;
    return nap_plan(*g, co).bytes;
}

static NapArgs nap_args(const Mri3dNormGeom& g, const float* mean, const float* invstd, const float* gamma, const float* beta,
                        const float* alpha) {
    NapArgs a;
    a.mean = mean, a.invstd = invstd, a.gamma = gamma, a.beta = beta, a.alpha = alpha;
    a.alpha_n = g.alpha_n, a.act = g.act, a.slope = g.slope, a.C = g.c, a.x_ld = g.x_ld;
    a.nvox = (int64_t)g.n * g.vox;
    return a;
}

extern "C" int mri3d_norm_act_pw_fwd(const Mri3dNormGeom* g, int32_t co, const void* x, const float* mean, const float* invstd,
                                     const float* gamma, const float* beta, const float* alpha, const float* w,
                                     const float* bias, void* out, mri3d_stream_t stream) {
    MRI3D_REQUIRE(g != nullptr, MRI3D_EINVAL, "norm_act_pw_fwd: null geometry");
    MRI3D_REQUIRE(nap_supported(*g, co), MRI3D_ENOTSUP, "norm_act_pw_fwd: c=%d co=%d x_ld=%d y_ld=%d instance=%d not served",
                  g->c, co, g->x_ld, g->y_ld, g->instance);
    MRI3D_REQUIRE(x && w && out, MRI3D_EINVAL, "norm_act_pw_fwd: null pointer");
    if (int rc = norm_act_args_check(g, 0, mean, invstd, alpha, "norm_act_pw_fwd")) return rc;
    MRI3D_REQUIRE(aligned_vec4(g->dtype, x), MRI3D_EINVAL, "norm_act_pw_fwd: x must be aligned to 4 elements");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const NapArgs a = nap_args(*g, mean, invstd, gamma, beta, alpha);
    const int VT = 256 / (g->c / 4);
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(a.nvox, (int64_t)VT * 4), kMaxStreamBlocks));
    MRI3D_DISPATCH_DTYPE(g->dtype, T, {
        if (co <= 2)
            hipLaunchKernelGGL((norm_act_pw_fwd_kernel<T, 2>), dim3(grid), dim3(256), 0, s, (const T*)x, (T*)out, w, bias, co,
                               g->y_ld, a);
        else
            hipLaunchKernelGGL((norm_act_pw_fwd_kernel<T, 4>), dim3(grid), dim3(256), 0, s, (const T*)x, (T*)out, w, bias, co,
                               g->y_ld, a);
    });
    return check_launch("norm_act_pw_fwd");
}

// The launch sequence of a gradient-source backward (PwHeadGrad, PoolSkipGrad), decided by (training statistics, dx wanted,
// parameter gradients wanted, side sums wanted).  Training statistics: a sums pass, the combined sums, then the dx pass, whose
// first workgroup writes the parameter gradients.  Frozen statistics: one pass does both (or only one of them is wanted), and
// the parameter kernel follows the combined sums.  dw / dbias: the side sums of a source with kSide > 0 (co rows of c).
template <typename T, class SRC>
static void nap_bwd_launch(const Mri3dNormGeom& g, const NapPlan& p, void* ws, hipStream_t s, int training, const T* x, T* dx,
                           const typename SRC::Args& sa, const NapArgs& a, float* dgamma, float* dbeta, float* dalpha,
                           int co = 0, float* dw = nullptr, float* dbias = nullptr) {
    double* part = p.part(ws);
    float* sums = p.sums(ws);
    double* spart = p.spart(ws);
    const dim3 grid(p.nblk), blk(256);
    auto pass = [&](auto sums_pass, auto dx_pass) {
        constexpr bool SUMS = decltype(sums_pass)::value, DX = decltype(dx_pass)::value;
        if constexpr (std::is_same_v<SRC, PoolSkipGrad<T>>)   // its entry point has no side-partials parameter
            hipLaunchKernelGGL((norm_act_pool_bwd_kernel<T, SUMS, DX>), grid, blk, 0, s, x, dx, sa, a, sums, training, part,
                               dgamma, dbeta, dalpha);
        else
            hipLaunchKernelGGL((norm_act_src_bwd_kernel<T, SRC, SUMS, DX>), grid, blk, 0, s, x, dx, sa, a, sums, training, part,
                               spart, dgamma, dbeta, dalpha);
    };
    const bool params = dgamma || dbeta || dalpha;
    const bool side = SRC::kSide > 0 && (dw || dbias);
    const bool need_sums = training || params || side;
    if (need_sums) {
        if (training || dx == nullptr)
            pass(std::true_type{}, std::false_type{});
        else   // frozen statistics: dx does not wait for the sums
            pass(std::true_type{}, std::true_type{});
        hipLaunchKernelGGL(norm_act_bwd_sums_kernel, dim3(cdiv(g.c, 256 / kFinQL)), dim3(256), 0, s, part, sums, g.c, p.nblk, 1);
        if (side)
            hipLaunchKernelGGL(norm_act_pw_wsum_kernel, dim3(cdiv(co * g.c + co, 8)), dim3(256), 0, s, spart, dw, dbias, p.nblk,
                               co * g.c, co);
        if (params && !(training && dx != nullptr))
            hipLaunchKernelGGL(norm_act_bwd_params_kernel, dim3(1), dim3(256), 0, s, sums, dgamma, dbeta, dalpha, g.alpha_n, g.c,
                               1);
    }
    if (dx != nullptr && (training || !need_sums)) pass(std::false_type{}, std::true_type{});
}

extern "C" int mri3d_norm_act_pw_bwd(const Mri3dNormGeom* g, int32_t co, int training, const void* x, const void* dout,
                                     const float* mean, const float* invstd, const float* gamma, const float* beta,
                                     const float* alpha, const float* w, void* dx, float* dgamma, float* dbeta, float* dalpha,
                                     float* dw, float* dbias, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(g != nullptr, MRI3D_EINVAL, "norm_act_pw_bwd: null geometry");
    MRI3D_REQUIRE(nap_supported(*g, co), MRI3D_ENOTSUP, "norm_act_pw_bwd: c=%d co=%d x_ld=%d y_ld=%d instance=%d not served",
                  g->c, co, g->x_ld, g->y_ld, g->instance);
    MRI3D_REQUIRE(x && dout && w, MRI3D_EINVAL, "norm_act_pw_bwd: null pointer");
    if (int rc = norm_act_args_check(g, training, mean, invstd, alpha, "norm_act_pw_bwd")) return rc;
    MRI3D_REQUIRE(aligned_vec4(g->dtype, x, dx), MRI3D_EINVAL, "norm_act_pw_bwd: x and dx must be aligned to 4 elements");
    const NapPlan p = nap_plan(*g, co);
    MRI3D_REQUIRE(workspace && ws_bytes >= p.bytes && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MRI3D_EWORKSPACE,
                  "norm_act_pw_bwd: workspace %zu < %zu (or not 8-byte aligned)", ws_bytes, p.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const NapArgs a = nap_args(*g, mean, invstd, gamma, beta, alpha);
    MRI3D_DISPATCH_DTYPE(g->dtype, T, {
        if (co <= 2)
            nap_bwd_launch<T, PwHeadGrad<T, 2>>(*g, p, workspace, s, training, (const T*)x, (T*)dx, {(const T*)dout, w, co, g->y_ld},
                                                a, dgamma, dbeta, dalpha, co, dw, dbias);
        else
            nap_bwd_launch<T, PwHeadGrad<T, 4>>(*g, p, workspace, s, training, (const T*)x, (T*)dx, {(const T*)dout, w, co, g->y_ld},
                                                a, dgamma, dbeta, dalpha, co, dw, dbias);
    });
    return check_launch("norm_act_pw_bwd");
}

// ------------------------------------------------------------------ norm + activation + MaxPool3d(2): host side
// g: the norm_act part (x_ld = pitch of x / dx, y_ld = pitch of skip / dskip); pg: the pool (x_ld = its input = skip, y_ld = pooled).
static bool napool_supported(const Mri3dNormGeom& g, const Mri3dPoolGeom& pg) {
    if (!nap_supported(g, 1) || g.y_ld < g.c || g.y_ld % 4 != 0) return false;   // co = 1: the head's width plays no part here
    if (pg.dtype != g.dtype || pg.n != g.n || pg.c != g.c || pg.x_ld != g.y_ld || pg.y_ld < g.c || pg.y_ld % 4 != 0) return false;
    if (pg.di <= 0 || pg.hi <= 0 || pg.wi <= 0 || (int64_t)pg.di * pg.hi * pg.wi != g.vox) return false;
    if (!pool2_ok(pg, 4)) return false;
    const int64_t ld = g.x_ld > g.y_ld ? g.x_ld : g.y_ld;
    if (g.vox * ld >= ((int64_t)1 << 31)) return false;           // 32-bit element offsets inside one sample (forward)
    if ((int64_t)g.n * g.vox >= ((int64_t)1 << 31)) return false;  // 32-bit decode of the flat voxel index (backward)
    return true;
}

extern "C" int32_t mri3d_norm_act_pool_supported(const Mri3dNormGeom* g, const Mri3dPoolGeom* pg) {
    return (g != nullptr && pg != nullptr && napool_supported(*g, *pg)) ? 1 : 0;
}

extern "C" size_t mri3d_norm_act_pool_workspace_bytes(const Mri3dNormGeom* g, const Mri3dPoolGeom* pg) {
    if (g == nullptr || pg == nullptr || !napool_supported(*g, *pg)) return 0;
    return nap_plan(*g, 0).bytes;
}

extern "C" int mri3d_norm_act_pool_fwd(const Mri3dNormGeom* g, const Mri3dPoolGeom* pg, const void* x, const float* mean,
                                       const float* invstd, const float* gamma, const float* beta, const float* alpha,
                                       void* skip, void* pooled, uint8_t* idx, mri3d_stream_t stream) {
    MRI3D_REQUIRE(g != nullptr && pg != nullptr, MRI3D_EINVAL, "norm_act_pool_fwd: null geometry");
    MRI3D_REQUIRE(napool_supported(*g, *pg), MRI3D_ENOTSUP,
                  "norm_act_pool_fwd: c=%d x_ld=%d y_ld=%d instance=%d pool %dx%dx%d/%d -> %dx%dx%d not served", g->c, g->x_ld,
                  g->y_ld, g->instance, pg->di, pg->hi, pg->wi, pg->kd, pg->dout, pg->ho, pg->wo);
    MRI3D_REQUIRE(x && skip && pooled && idx, MRI3D_EINVAL, "norm_act_pool_fwd: null pointer");
    if (int rc = norm_act_args_check(g, 0, mean, invstd, alpha, "norm_act_pool_fwd")) return rc;
    MRI3D_REQUIRE(aligned_vec4(g->dtype, x, skip, pooled) && (reinterpret_cast<uintptr_t>(idx) & 3) == 0, MRI3D_EINVAL,
                  "norm_act_pool_fwd: x, skip, pooled and idx must be aligned to 4 elements");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const NapArgs a = nap_args(*g, mean, invstd, gamma, beta, alpha);
    // the lanes of the pool forward (bf16: 16-byte accesses where the layout allows them), with x as a third tensor
    const PoolFwdLanes p = pool_fwd_lanes(*pg, {g->x_ld, g->y_ld, pg->y_ld}, {ptr_align(x, skip, pooled)}, ptr_align(idx));
    MRI3D_DISPATCH_DTYPE(g->dtype, T, {
        if constexpr (sizeof(T) == 2) {
            if (p.vec == 8)
                hipLaunchKernelGGL((norm_act_pool_fwd_kernel<T, 8>), dim3(p.grid), dim3(256), 0, s, *pg, (const T*)x, (T*)skip,
                                   (T*)pooled, idx, p.hch, a);
        }
        if (p.vec != 8)
            hipLaunchKernelGGL((norm_act_pool_fwd_kernel<T, 4>), dim3(p.grid), dim3(256), 0, s, *pg, (const T*)x, (T*)skip, (T*)pooled,
                               idx, p.hch, a);
    });
    return check_launch("norm_act_pool_fwd");
}

extern "C" int mri3d_norm_act_pool_bwd(const Mri3dNormGeom* g, const Mri3dPoolGeom* pg, int training, const void* x,
                                       const void* dskip, const void* dpool, const uint8_t* idx, const float* mean,
                                       const float* invstd, const float* gamma, const float* beta, const float* alpha, void* dx,
                                       float* dgamma, float* dbeta, float* dalpha, void* workspace, size_t ws_bytes,
                                       mri3d_stream_t stream) {
    MRI3D_REQUIRE(g != nullptr && pg != nullptr, MRI3D_EINVAL, "norm_act_pool_bwd: null geometry");
    MRI3D_REQUIRE(napool_supported(*g, *pg), MRI3D_ENOTSUP,
                  "norm_act_pool_bwd: c=%d x_ld=%d y_ld=%d instance=%d pool %dx%dx%d/%d -> %dx%dx%d not served", g->c, g->x_ld,
                  g->y_ld, g->instance, pg->di, pg->hi, pg->wi, pg->kd, pg->dout, pg->ho, pg->wo);
    MRI3D_REQUIRE(x != nullptr, MRI3D_EINVAL, "norm_act_pool_bwd: null pointer");
    MRI3D_REQUIRE(dpool == nullptr || idx != nullptr, MRI3D_EINVAL, "norm_act_pool_bwd: dpool needs the index bytes");
    if (int rc = norm_act_args_check(g, training, mean, invstd, alpha, "norm_act_pool_bwd")) return rc;
    MRI3D_REQUIRE(aligned_vec4(g->dtype, x, dx) && aligned_vec4(g->dtype, dskip, dpool) &&
                      (reinterpret_cast<uintptr_t>(idx) & 3) == 0,
                  MRI3D_EINVAL, "norm_act_pool_bwd: x, dx, dskip, dpool and idx must be aligned to 4 elements");
    const NapPlan p = nap_plan(*g, 0);
    MRI3D_REQUIRE(workspace && ws_bytes >= p.bytes && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MRI3D_EWORKSPACE,
                  "norm_act_pool_bwd: workspace %zu < %zu (or not 8-byte aligned)", ws_bytes, p.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const NapArgs a = nap_args(*g, mean, invstd, gamma, beta, alpha);
    MRI3D_DISPATCH_DTYPE(g->dtype, T, {
        const typename PoolSkipGrad<T>::Args sa = {(const T*)dskip, (const T*)dpool, idx, g->y_ld, pg->y_ld, (unsigned)pg->wi,
                                                   (unsigned)pg->hi};
        nap_bwd_launch<T, PoolSkipGrad<T>>(*g, p, workspace, s, training, (const T*)x, (T*)dx, sa, a, dgamma, dbeta, dalpha);
    });
    return check_launch("norm_act_pool_bwd");
}
