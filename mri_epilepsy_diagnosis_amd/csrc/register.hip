// register.hip — the device pieces of an intensity-based affine registration of a subject's volume ("moving") to a template
// ("fixed"): intensity quantisation, the joint histogram of the fixed bins and the moving volume sampled under up to 64 candidate
// affines per launch, the similarity costs of those histograms, a resampler between two different grids and the 2x mean pyramid.
// Reference: get_registered_img_and_mask / get_registered_img (detection/preprocessing_utils.py:11-73) call FSL FLIRT for this;
// the host optimiser that drives these kernels is mri_epilepsy_diagnosis_amd/registration/.
//
// The file is compiled with -ffp-contract=off and writes no fmaf: every * and + is one fp32 rounding in the order written, which
// tests/register_ref.py restates.  An affine A is a row-major (3, 4) matrix from a fixed voxel index (d, h, w) to a moving one:
//     r_a = (A[a][0]*d + A[a][1]*h) + A[a][3]            once per fixed row
//     s_a = A[a][2]*w + r_a                               per voxel
//     inside = -0.5 <= s_a <= N_a - 0.5 on all axes      (warp3d's rule; NaN is outside)
//     q_a = min(max(s_a, -1), N_a), e_a = floor(q_a), f_a = q_a - e_a, indices e_a and e_a + 1 clamped to [0, N_a - 1]
//     x_dh = v_dh0 + f_2*(v_dh1 - v_dh0)   y_d = x_d0 + f_1*(x_d1 - x_d0)   v = y_0 + f_0*(y_1 - y_0)
//     nearest index = clamp(floor(q_a + 0.5), 0, N_a - 1)
//
// Plan of the joint histogram (mri3d_joint_hist_plan reports it).  Lanes run along w of the fixed grid: one wave owns one fixed
// row (d, h) and walks it 64 voxels at a time, so the fixed bytes are one contiguous load and consecutive lanes step the source
// by the affine's third column.  A block is 4 waves = 4 rows per trip; block b of a candidate group takes row quads b, b + blocks,
// ..., blocks = min(quads, 512).  A block scores a GROUP of up to 4 candidates against one load of its fixed bytes: grid.y is the
// group.  Each candidate of the group has its own bins x bins uint32 histogram in LDS (4 x 16 KB at 64 bins), added to with LDS
// integer atomics; a wave step whose 64 fixed bytes are all "skip" costs one load and one ballot.  Reduction, two stages: after
// its rows a block adds its non-zero LDS cells to uint32 accumulators in the workspace with global integer atomics (a kernel
// zeroed them first), and a last kernel widens the accumulators to the int64 result.  Integer sums do not depend on their order.
// Not done: per-wave sub-histograms or a merge of equal bins inside a wave.  Measured instead: a moving volume that
// puts every sample of a fixed bin on ONE LDS address takes the same time as one that spreads them over all bins.
#include "common.h"
#include <math.h>

namespace mri3d {

constexpr int kRegWaves = 4;          // fixed rows per block and trip
constexpr int kHistGroup = 4;         // candidates that share a block's fixed loads
constexpr int kHistMaxBlocks = 512;   // per candidate group
constexpr int kHistMaxK = 64;
constexpr int kHistMaxBins = 64;
constexpr int kSkipBin = 255;

// the row's share of the map and the step along w, per axis
struct RowMap { float r0, r1, r2, a0, a1, a2; };

__device__ __forceinline__ RowMap row_map(const float* __restrict__ A, int d, int h) {
    const float fd = (float)d, fh = (float)h;
    RowMap m;
    m.r0 = (A[0] * fd + A[1] * fh) + A[3], m.a0 = A[2];
    m.r1 = (A[4] * fd + A[5] * fh) + A[7], m.a1 = A[6];
    m.r2 = (A[8] * fd + A[9] * fh) + A[11], m.a2 = A[10];
    return m;
}

struct Src { float q0, q1, q2; bool inside; };

__device__ __forceinline__ Src src_at(const RowMap& m, int w, int D, int H, int W) {
    const float fw = (float)w;
    const float s0 = m.a0 * fw + m.r0, s1 = m.a1 * fw + m.r1, s2 = m.a2 * fw + m.r2;
    Src s;
    s.inside = s0 >= -0.5f && s0 <= (float)D - 0.5f && s1 >= -0.5f && s1 <= (float)H - 0.5f && s2 >= -0.5f && s2 <= (float)W - 0.5f;
    // clamp before the float -> int conversion: any value (NaN included) yields an in-range address
    s.q0 = fminf(fmaxf(s0, -1.f), (float)D), s.q1 = fminf(fmaxf(s1, -1.f), (float)H), s.q2 = fminf(fmaxf(s2, -1.f), (float)W);
    return s;
}

// the eight loads are issued together from clamped addresses; the caller applies `inside` to the result
__device__ __forceinline__ float trilinear(const float* __restrict__ v, const Src& s, int D, int H, int W) {
    const float e0 = floorf(s.q0), e1 = floorf(s.q1), e2 = floorf(s.q2);
    const float f0 = s.q0 - e0, f1 = s.q1 - e1, f2 = s.q2 - e2;
    const int i0 = (int)e0, i1 = (int)e1, i2 = (int)e2;
    const size_t d_lo = (size_t)min(max(i0, 0), D - 1) * H, d_hi = (size_t)min(max(i0 + 1, 0), D - 1) * H;
    const size_t h_lo = (size_t)min(max(i1, 0), H - 1), h_hi = (size_t)min(max(i1 + 1, 0), H - 1);
    const int w_lo = min(max(i2, 0), W - 1), w_hi = min(max(i2 + 1, 0), W - 1);
    const float* p00 = v + (d_lo + h_lo) * W;
    const float* p01 = v + (d_lo + h_hi) * W;
    const float* p10 = v + (d_hi + h_lo) * W;
    const float* p11 = v + (d_hi + h_hi) * W;
    const float v000 = p00[w_lo], v001 = p00[w_hi], v010 = p01[w_lo], v011 = p01[w_hi];
    const float v100 = p10[w_lo], v101 = p10[w_hi], v110 = p11[w_lo], v111 = p11[w_hi];
    const float x00 = v000 + f2 * (v001 - v000), x01 = v010 + f2 * (v011 - v010);
    const float x10 = v100 + f2 * (v101 - v100), x11 = v110 + f2 * (v111 - v110);
    const float y0 = x00 + f1 * (x01 - x00), y1 = x10 + f1 * (x11 - x10);
    return y0 + f0 * (y1 - y0);
}

// clamp(floor((v - lo) * scale), 0, bins - 1); NaN goes to bin 0 (fmaxf returns its other operand)
__device__ __forceinline__ int bin_of(float v, float lo, float scale, int bins) {
    return (int)fminf(fmaxf(floorf((v - lo) * scale), 0.f), (float)(bins - 1));
}

// ------------------------------------------------------------------ quantisation
__global__ void __launch_bounds__(256)
quantize_u8_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, int64_t n, float lo, float scale, int bins,
                   uint8_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = x[i];
        const bool counted = (mask ? mask[i] != 0 : true) && isfinite(v);
        out[i] = counted ? (uint8_t)bin_of(v, lo, scale, bins) : (uint8_t)kSkipBin;
    }
}

// ------------------------------------------------------------------ joint histogram
__global__ void __launch_bounds__(256)
fill_u32_kernel(uint32_t* __restrict__ p, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = 0u;
}

__global__ void __launch_bounds__(256)
widen_u32_kernel(const uint32_t* __restrict__ acc, int n, int64_t* __restrict__ hist) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) hist[i] = (int64_t)acc[i];
}

__global__ void __launch_bounds__(64 * kRegWaves)
joint_hist_kernel(const uint8_t* __restrict__ fixed_bins, int Df, int Hf, int Wf, const float* __restrict__ moving, int Dm, int Hm,
                  int Wm, const float* __restrict__ affines, int k, float m_lo, float m_scale, int bins, uint32_t* __restrict__ acc) {
    extern __shared__ uint32_t lh[];   // [candidates of the group][bins][bins]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c0 = blockIdx.y * kHistGroup;
    const int cg = min(kHistGroup, k - c0);
    const int cells = bins * bins;
    for (int i = threadIdx.x; i < cg * cells; i += 64 * kRegWaves) lh[i] = 0u;
    __syncthreads();
    const int rows = Df * Hf;   // < 2^31, checked by the host
    // no barrier inside the loop: a wave without a row in the last trip just leaves it
    for (int row = blockIdx.x * kRegWaves + wave; row < rows; row += gridDim.x * kRegWaves) {
        const int d = row / Hf, h = row - d * Hf;
        RowMap m[kHistGroup];
#pragma unroll
        for (int c = 0; c < kHistGroup; ++c) m[c] = row_map(affines + (size_t)(c0 + min(c, cg - 1)) * 12, d, h);
        const uint8_t* fr = fixed_bins + (size_t)row * Wf;
        for (int w0 = 0; w0 < Wf; w0 += 64) {
            const int w = w0 + lane;
            const int bf = w < Wf ? (int)fr[w] : kSkipBin;
            const bool counted = bf < bins;
            if (__ballot(counted) == 0ull) continue;   // wave-uniform: background of the fixed image
#pragma unroll
            for (int c = 0; c < kHistGroup; ++c) {
                if (c < cg) {
                    const Src s = src_at(m[c], w, Dm, Hm, Wm);
                    const float v = trilinear(moving, s, Dm, Hm, Wm);
                    const int bm = bin_of(v, m_lo, m_scale, bins);
                    if (counted && s.inside) atomicAdd(&lh[c * cells + bf * bins + bm], 1u);
                }
            }
        }
    }
    __syncthreads();
    uint32_t* dst = acc + (size_t)c0 * cells;
    for (int i = threadIdx.x; i < cg * cells; i += 64 * kRegWaves) {
        const uint32_t v = lh[i];
        if (v) atomicAdd(&dst[i], v);
    }
}

// ------------------------------------------------------------------ costs
// One block of 64 lanes per candidate; lane t owns row t and column t of the histogram.  Counts and their first moments are
// integers (times 1/2) below 2^53: exact in float64.  Every sum over lanes is taken by index in ascending order.
__device__ __forceinline__ double plogp(double cnt, double n) {
    if (!(cnt > 0.0)) return 0.0;
    const double p = cnt / n;
    return p * log(p);
}

__global__ void __launch_bounds__(64)
hist_costs_kernel(const int64_t* __restrict__ hist, int bins, int kind, double min_count, double* __restrict__ out) {
    __shared__ double sa[64], sb[64], sc[64];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t* H = hist + (size_t)c * bins * bins;
    double rn = 0.0, cn = 0.0, s1 = 0.0;
    if (t < bins) {
        for (int j = 0; j < bins; ++j) {
            const double hv = (double)H[t * bins + j];
            rn += hv;
            s1 += hv * ((double)j + 0.5);
            cn += (double)H[j * bins + t];
        }
    }
    sa[t] = rn, sb[t] = s1;
    __syncthreads();
    double n = 0.0, S1 = 0.0;
    for (int i = 0; i < bins; ++i) n += sa[i], S1 += sb[i];
    __syncthreads();
    double cost = (double)INFINITY;
    const bool enough = n >= min_count && n > 0.0;   // block-uniform
    if (enough && kind == 0) {
        const double mean = S1 / n;
        double within = 0.0, total = 0.0;
        if (t < bins) {
            if (rn > 0.0) {
                const double mi = s1 / rn;
                for (int j = 0; j < bins; ++j) {
                    const double dy = ((double)j + 0.5) - mi;
                    within += (double)H[t * bins + j] * (dy * dy);
                }
            }
            const double dy = ((double)t + 0.5) - mean;
            total = cn * (dy * dy);
        }
        sa[t] = within, sb[t] = total;
        __syncthreads();
        if (t == 0) {
            double Wn = 0.0, Tn = 0.0;
            for (int i = 0; i < bins; ++i) Wn += sa[i], Tn += sb[i];
            if (Tn > 0.0) cost = Wn / Tn;
        }
    } else if (enough) {
        double ej = 0.0;
        if (t < bins)
            for (int j = 0; j < bins; ++j) ej += plogp((double)H[t * bins + j], n);
        sa[t] = ej, sb[t] = plogp(rn, n), sc[t] = plogp(cn, n);
        __syncthreads();
        if (t == 0) {
            double Ej = 0.0, Ef = 0.0, Em = 0.0;
            for (int i = 0; i < bins; ++i) Ej += sa[i], Ef += sb[i], Em += sc[i];
            const double Hfm = -Ej, Hf = -Ef, Hm = -Em;
            if (kind == 1) cost = -((Hf + Hm) - Hfm);
            else if (Hfm > 0.0) cost = -(Hf + Hm) / Hfm;
        }
    }
    if (t == 0) out[2 * c] = cost, out[2 * c + 1] = n;
}

// ------------------------------------------------------------------ resampling between two grids
template <int LB> struct RegLabel { typedef uint8_t type; };
template <> struct RegLabel<2> { typedef uint16_t type; };
template <> struct RegLabel<4> { typedef uint32_t type; };

// LB = label element bytes (0: no label).  One wave per destination row, 64 voxels of w per step: stores are contiguous.
template <int LB>
__global__ void __launch_bounds__(64 * kRegWaves)
resample_affine_kernel(const float* __restrict__ img, float* __restrict__ img_out, const void* __restrict__ lab_v,
                       void* __restrict__ lab_out_v, int Dm, int Hm, int Wm, int Df, int Hf, int Wf,
                       const float* __restrict__ affine, float pad) {
    typedef typename RegLabel<LB>::type L;
    const L* __restrict__ lab = static_cast<const L*>(lab_v);
    L* __restrict__ lab_out = static_cast<L*>(lab_out_v);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rows = Df * Hf;
    for (int row = blockIdx.x * kRegWaves + wave; row < rows; row += gridDim.x * kRegWaves) {
        const int d = row / Hf, h = row - d * Hf;
        const RowMap m = row_map(affine, d, h);
        const size_t out_row = (size_t)row * Wf;
        for (int w = lane; w < Wf; w += 64) {
            const Src s = src_at(m, w, Dm, Hm, Wm);
            if (img) {
                const float r = trilinear(img, s, Dm, Hm, Wm);
                img_out[out_row + w] = s.inside ? r : pad;
            }
            if (LB) {
                const int n0 = min(max((int)floorf(s.q0 + 0.5f), 0), Dm - 1), n1 = min(max((int)floorf(s.q1 + 0.5f), 0), Hm - 1),
                          n2 = min(max((int)floorf(s.q2 + 0.5f), 0), Wm - 1);
                const L v = lab[((size_t)n0 * Hm + n1) * Wm + n2];
                lab_out[out_row + w] = s.inside ? v : (L)0;
            }
        }
    }
}

// ------------------------------------------------------------------ pyramid
__global__ void __launch_bounds__(256)
downsample2_mean_kernel(const float* __restrict__ x, int D, int H, int W, float* __restrict__ y, int Do, int Ho, int Wo) {
    const int64_t total = (int64_t)Do * Ho * Wo;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int wo = (int)(i % Wo);
        const int64_t r = i / Wo;
        const int ho = (int)(r % Ho), dd = (int)(r / Ho);
        const int nd = min(2, D - 2 * dd), nh = min(2, H - 2 * ho), nw = min(2, W - 2 * wo);
        float sum = 0.f;
        bool first = true;
        for (int a = 0; a < nd; ++a)
            for (int b = 0; b < nh; ++b)
                for (int c = 0; c < nw; ++c) {
                    const float v = x[((size_t)(2 * dd + a) * H + (2 * ho + b)) * W + (2 * wo + c)];
                    sum = first ? v : sum + v;
                    first = false;
                }
        y[i] = sum * (1.f / (float)(nd * nh * nw));
    }
}

static bool vol_ok(int32_t d, int32_t h, int32_t w) { return d > 0 && h > 0 && w > 0; }
static bool vol_small(int32_t d, int32_t h, int32_t w) { return (int64_t)d * h * w < 0x7fffffffLL; }
static bool hist_args_ok(int32_t df, int32_t hf, int32_t wf, int32_t k, int32_t bins) {
    return vol_ok(df, hf, wf) && vol_small(df, hf, wf) && k >= 1 && k <= kHistMaxK && bins >= 2 && bins <= kHistMaxBins;
}
static int hist_blocks(int32_t df, int32_t hf) { return (int)std::min<int64_t>(cdiv64((int64_t)df * hf, kRegWaves), kHistMaxBlocks); }

}  // namespace mri3d

using namespace mri3d;

extern "C" int mri3d_quantize_u8(const float* x, const uint8_t* mask, int64_t n, float lo, float scale, int32_t bins, uint8_t* out,
                                 mri3d_stream_t stream) {
    MRI3D_REQUIRE(x && out && n > 0, MRI3D_EINVAL, "quantize_u8: bad arguments (x %p, out %p, n %lld)", (const void*)x, (void*)out, (long long)n);
    MRI3D_REQUIRE(bins >= 2 && bins <= kHistMaxBins, MRI3D_EINVAL, "quantize_u8: bins = %d outside 2..%d", bins, kHistMaxBins);
    MRI3D_REQUIRE(isfinite(lo) && isfinite(scale), MRI3D_EINVAL, "quantize_u8: lo = %g, scale = %g must be finite", (double)lo, (double)scale);
    MRI3D_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, MRI3D_EINVAL, "quantize_u8: x is not 4-byte aligned");
    MRI3D_REQUIRE(!overlaps(x, (size_t)n * 4, out, (size_t)n) && !overlaps(mask, (size_t)n, out, (size_t)n), MRI3D_EINVAL,
                  "quantize_u8: the output overlaps an input");
    hipLaunchKernelGGL(quantize_u8_kernel, dim3(stream_grid(n, 1024)), dim3(256), 0, static_cast<hipStream_t>(stream), x, mask, n, lo,
                       scale, bins, out);
    return check_launch("quantize_u8");
}

extern "C" size_t mri3d_joint_hist_workspace_bytes(int32_t df, int32_t hf, int32_t wf, int32_t k, int32_t bins) {
    if (!hist_args_ok(df, hf, wf, k, bins)) return 0;
    return (size_t)k * bins * bins * sizeof(uint32_t);
}

extern "C" int mri3d_joint_hist_plan(int32_t df, int32_t hf, int32_t wf, int32_t k, int32_t bins, int32_t out[8]) {
    MRI3D_REQUIRE(out != nullptr, MRI3D_EINVAL, "joint_hist_plan: null output");
    MRI3D_REQUIRE(vol_ok(df, hf, wf), MRI3D_EINVAL, "joint_hist_plan: fixed extents %d,%d,%d", df, hf, wf);
    MRI3D_REQUIRE(vol_small(df, hf, wf), MRI3D_ENOTSUP, "joint_hist_plan: fixed volume too large");
    MRI3D_REQUIRE(k >= 1 && k <= kHistMaxK, MRI3D_EINVAL, "joint_hist_plan: k = %d outside 1..%d", k, kHistMaxK);
    MRI3D_REQUIRE(bins >= 2 && bins <= kHistMaxBins, MRI3D_EINVAL, "joint_hist_plan: bins = %d outside 2..%d", bins, kHistMaxBins);
    const int blocks = hist_blocks(df, hf), cg = std::min<int>(k, kHistGroup);
    out[0] = blocks;
    out[1] = cdiv(k, kHistGroup);
    out[2] = cg;
    out[3] = kRegWaves;
    out[4] = (int32_t)cdiv64(cdiv64((int64_t)df * hf, kRegWaves), blocks);
    out[5] = cg * bins * bins * (int)sizeof(uint32_t);
    out[6] = 2;
    out[7] = 64;
    return MRI3D_OK;
}

extern "C" int mri3d_joint_hist(const uint8_t* fixed_bins, int32_t df, int32_t hf, int32_t wf, const float* moving, int32_t dm,
                                int32_t hm, int32_t wm, const float* affines, int32_t k, float m_lo, float m_scale, int32_t bins,
                                int64_t* hist, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(vol_ok(df, hf, wf) && vol_ok(dm, hm, wm), MRI3D_EINVAL, "joint_hist: extents fixed %d,%d,%d moving %d,%d,%d", df, hf, wf,
                  dm, hm, wm);
    MRI3D_REQUIRE(vol_small(df, hf, wf) && vol_small(dm, hm, wm), MRI3D_ENOTSUP, "joint_hist: volume too large");
    MRI3D_REQUIRE(k >= 1 && k <= kHistMaxK, MRI3D_EINVAL, "joint_hist: k = %d outside 1..%d", k, kHistMaxK);
    MRI3D_REQUIRE(bins >= 2 && bins <= kHistMaxBins, MRI3D_EINVAL, "joint_hist: bins = %d outside 2..%d", bins, kHistMaxBins);
    MRI3D_REQUIRE(isfinite(m_lo) && isfinite(m_scale), MRI3D_EINVAL, "joint_hist: m_lo = %g, m_scale = %g must be finite", (double)m_lo,
                  (double)m_scale);
    MRI3D_REQUIRE(fixed_bins && moving && affines && hist, MRI3D_EINVAL, "joint_hist: null pointer");
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(moving) | reinterpret_cast<uintptr_t>(affines)) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(hist) & 7) == 0,
                  MRI3D_EINVAL, "joint_hist: a pointer is not aligned to its element");
    const size_t need = mri3d_joint_hist_workspace_bytes(df, hf, wf, k, bins), hist_bytes = (size_t)k * bins * bins * sizeof(int64_t);
    MRI3D_REQUIRE(workspace && ws_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0, MRI3D_EWORKSPACE,
                  "joint_hist: workspace %zu < %zu, or not 4-byte aligned", ws_bytes, need);
    const size_t fb = (size_t)df * hf * wf, mb = (size_t)dm * hm * wm * 4, ab = (size_t)k * 12 * 4;
    MRI3D_REQUIRE(!overlaps(hist, hist_bytes, workspace, need) && !overlaps(hist, hist_bytes, fixed_bins, fb) &&
                      !overlaps(hist, hist_bytes, moving, mb) && !overlaps(hist, hist_bytes, affines, ab) &&
                      !overlaps(workspace, need, fixed_bins, fb) && !overlaps(workspace, need, moving, mb) &&
                      !overlaps(workspace, need, affines, ab),
                  MRI3D_EINVAL, "joint_hist: the histogram or the workspace overlaps another buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* acc = static_cast<uint32_t*>(workspace);
    const int cells = k * bins * bins, cg = std::min<int>(k, kHistGroup);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(cdiv(cells, 1024)), dim3(256), 0, s, acc, cells);
    hipLaunchKernelGGL(joint_hist_kernel, dim3(hist_blocks(df, hf), cdiv(k, kHistGroup)), dim3(64 * kRegWaves),
                       (size_t)cg * bins * bins * sizeof(uint32_t), s, fixed_bins, df, hf, wf, moving, dm, hm, wm, affines, k, m_lo, m_scale,
                       bins, acc);
    hipLaunchKernelGGL(widen_u32_kernel, dim3(cdiv(cells, 1024)), dim3(256), 0, s, acc, cells, hist);
    return check_launch("joint_hist");
}

extern "C" int mri3d_hist_costs(const int64_t* hist, int32_t k, int32_t bins, int32_t kind, double min_count, double* out,
                                mri3d_stream_t stream) {
    MRI3D_REQUIRE(k >= 1 && k <= kHistMaxK, MRI3D_EINVAL, "hist_costs: k = %d outside 1..%d", k, kHistMaxK);
    MRI3D_REQUIRE(bins >= 2 && bins <= kHistMaxBins, MRI3D_EINVAL, "hist_costs: bins = %d outside 2..%d", bins, kHistMaxBins);
    MRI3D_REQUIRE(kind >= 0 && kind <= 2, MRI3D_EINVAL, "hist_costs: kind %d outside 0..2", kind);
    MRI3D_REQUIRE(min_count >= 0.0, MRI3D_EINVAL, "hist_costs: min_count = %g must be >= 0", min_count);
    MRI3D_REQUIRE(hist && out, MRI3D_EINVAL, "hist_costs: null pointer");
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(out)) & 7) == 0, MRI3D_EINVAL,
                  "hist_costs: a pointer is not 8-byte aligned");
    MRI3D_REQUIRE(!overlaps(hist, (size_t)k * bins * bins * 8, out, (size_t)k * 16), MRI3D_EINVAL, "hist_costs: the output overlaps the histograms");
    hipLaunchKernelGGL(hist_costs_kernel, dim3(k), dim3(64), 0, static_cast<hipStream_t>(stream), hist, bins, kind, min_count, out);
    return check_launch("hist_costs");
}

extern "C" int mri3d_resample_affine(const float* image, float* image_out, const void* label, void* label_out, int32_t label_bytes,
                                     int32_t dm, int32_t hm, int32_t wm, int32_t df, int32_t hf, int32_t wf, const float* affine,
                                     float pad_value, mri3d_stream_t stream) {
    MRI3D_REQUIRE(affine && vol_ok(dm, hm, wm) && vol_ok(df, hf, wf), MRI3D_EINVAL,
                  "resample_affine: bad arguments (affine %p, source %d,%d,%d, destination %d,%d,%d)", (const void*)affine, dm, hm, wm, df, hf, wf);
    MRI3D_REQUIRE(vol_small(dm, hm, wm) && vol_small(df, hf, wf), MRI3D_ENOTSUP, "resample_affine: volume too large");
    MRI3D_REQUIRE((image != nullptr) == (image_out != nullptr) && (label != nullptr) == (label_out != nullptr), MRI3D_EINVAL,
                  "resample_affine: a source without its destination (or the reverse)");
    MRI3D_REQUIRE(image || label, MRI3D_EINVAL, "resample_affine: neither an image nor a label map given");
    if (label)
        MRI3D_REQUIRE(label_bytes == 1 || label_bytes == 2 || label_bytes == 4, MRI3D_EINVAL,
                      "resample_affine: label element size %d (1, 2 or 4 bytes)", label_bytes);
    const int lb = label ? label_bytes : 0;
    const size_t src = (size_t)dm * hm * wm, dst = (size_t)df * hf * wf;
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(image_out) | reinterpret_cast<uintptr_t>(affine)) & 3) == 0 &&
                      (lb == 0 || ((reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(label_out)) & (uintptr_t)(lb - 1)) == 0),
                  MRI3D_EINVAL, "resample_affine: pointers not aligned to their element size");
    MRI3D_REQUIRE(!overlaps(image_out, dst * 4, image, src * 4) && !overlaps(image_out, dst * 4, label, src * lb) &&
                      !overlaps(label_out, dst * lb, image, src * 4) && !overlaps(label_out, dst * lb, label, src * lb) &&
                      !overlaps(image_out, dst * 4, label_out, dst * lb) && !overlaps(image_out, dst * 4, affine, 48) &&
                      !overlaps(label_out, dst * lb, affine, 48),
                  MRI3D_EINVAL, "resample_affine: a destination overlaps a source, the affine or the other destination");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(stream_grid((int64_t)df * hf, kRegWaves)), block(64 * kRegWaves);
#define RESAMPLE_LAUNCH(LB) \
    hipLaunchKernelGGL((resample_affine_kernel<LB>), grid, block, 0, st, image, image_out, label, label_out, dm, hm, wm, df, hf, wf, affine, pad_value)
    switch (lb) {
        case 0: RESAMPLE_LAUNCH(0); break;
        case 1: RESAMPLE_LAUNCH(1); break;
        case 2: RESAMPLE_LAUNCH(2); break;
        default: RESAMPLE_LAUNCH(4); break;
    }
#undef RESAMPLE_LAUNCH
    return check_launch("resample_affine");
}

extern "C" int mri3d_downsample2_mean_f32(const float* x, int32_t d, int32_t h, int32_t w, float* y, mri3d_stream_t stream) {
    MRI3D_REQUIRE(x && y && vol_ok(d, h, w), MRI3D_EINVAL, "downsample2_mean: bad arguments (x %p, y %p, extents %d,%d,%d)", (const void*)x,
                  (void*)y, d, h, w);
    MRI3D_REQUIRE(vol_small(d, h, w), MRI3D_ENOTSUP, "downsample2_mean: volume too large");
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 3) == 0, MRI3D_EINVAL,
                  "downsample2_mean: pointers not 4-byte aligned");
    const int dd = (d + 1) / 2, ho = (h + 1) / 2, wo = (w + 1) / 2;
    MRI3D_REQUIRE(!overlaps(x, (size_t)d * h * w * 4, y, (size_t)dd * ho * wo * 4), MRI3D_EINVAL, "downsample2_mean: y overlaps x");
    hipLaunchKernelGGL(downsample2_mean_kernel, dim3(stream_grid((int64_t)dd * ho * wo, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       d, h, w, y, dd, ho, wo);
    return check_launch("downsample2_mean");
}
