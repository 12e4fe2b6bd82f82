// kspace.hip — the k-space half of TorchIO's RandomMotion on HBM-resident volumes, without a Fourier transform.
// Reference call sites: the `training_transform` cells of segmentation/results_validation.ipynb and pretraining_3d_unet.ipynb
// open with `RescaleIntensity((0, 1)), RandomMotion()` (commented out); segmentation/routine.py imports both names.  TorchIO is
// absent from the reference tree ("parity unpinned"): the arithmetic is this project's definition (include/mri3d.h,
// "Augmentation"), restated in float64 numpy by tests/motion_ref.py.
//
// The motion artefact Fourier-transforms n = K + 1 volumes (the unmoved one and K rigidly moved copies), fills slabs of the
// shifted spectrum ALONG THE LAST AXIS ONLY, each slab from one spectrum, transforms back and keeps the real part.  The slab
// masks depend on the w frequency alone, so the transforms along d and h cancel against their inverses and what is left is a
// sum of 1-D circular filters along w:
//     out[i,d,h,z] = sum_{m<n} sum_{z'<w} coef[i,m,(z - z') mod w] * images[i,m,d,h,z']
//     coef[i,m,r]  = (1/w) sum_{k in S_m} cos(2 pi k r / w)        (S_m: the frequencies filled from image m; host, float64)
//
// kspace_mix_kernel: a block of 4 waves works on rows (d,h) of ONE subject (blockIdx.y), so that subject's n w coefficients are
// brought to LDS once per block, written twice over (c2[m][j] = coef[m][j mod w], j < 2w): the tap for output z and input z' is
// c2[m][z - z' + w], no modulo.  Per row a wave stages its n input rows in LDS with coalesced loads; a lane owns the outputs
// z = lane, lane + 64, ... (NT <= 4 of them, in registers).  In the inner loop the input samples are one LDS broadcast of four
// (ds_read_b128, every lane the same address) and the coefficient reads are consecutive dwords across lanes (conflict-free);
// stores are 256 contiguous bytes per wave.  Each output is ONE fmaf chain, m ascending then z' ascending: the same bits on every
// run, no atomics, no workspace.  By instruction count the loop is bound by LDS issue (about NT + 1/4 reads per NT FMAs), not
// by HBM (DESIGN §4 has the measurement).
#include "common.h"
#include <algorithm>

namespace mri3d {

constexpr int kMixWaves = 4;        // rows per block and step
constexpr int kMixMaxW = 256;       // w limit: a lane holds kMixMaxW / 64 outputs; LDS = (2 + kMixWaves) n w floats <= 48 KiB
constexpr int kMixMaxN = 8;
constexpr int kMixMaxBlocksX = 1024;

// LDS floats: c2 [n][2w] then rows [kMixWaves][n][wp], wp = w rounded up to 4 (16-byte aligned rows for the b128 broadcast)
template <int NT>
__global__ void __launch_bounds__(64 * kMixWaves)
kspace_mix_kernel(const float* __restrict__ images, float* __restrict__ out, int n, int rows, int W,
                  const float* __restrict__ coef) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wp = (W + 3) & ~3;
    float* c2 = lds;                          // 2 W n floats, rounded up to 4 below: the rows start 16-byte aligned
    float* xrows = lds + (((2 * W * n) + 3) & ~3);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int subject = blockIdx.y;
    const float* cs = coef + (size_t)subject * n * W;
    for (int j = threadIdx.x; j < 2 * W * n; j += 64 * kMixWaves) {
        const int m = j / (2 * W), r = j - m * 2 * W;
        c2[j] = cs[m * W + (r >= W ? r - W : r)];
    }
    float* xr = xrows + (size_t)wave * n * wp;
    const size_t vol = (size_t)rows * W;                                   // one (d,h,w) volume
    const float* img = images + (size_t)subject * n * vol;
    float* dst = out + (size_t)subject * vol;
    // the tap index of this lane's k-th output at z' = 0; lanes past the row read a valid tap and store nothing
    int tap[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) tap[k] = min(lane + 64 * k, W - 1) + W;
    // every wave of the block runs the same number of iterations: the barriers below are block-wide
    for (int base = blockIdx.x * kMixWaves; base < rows; base += gridDim.x * kMixWaves) {
        const int row = base + wave;
        const bool live = row < rows;   // wave-uniform
        __syncthreads();                // the previous row has been read (first pass: nothing to wait for)
        if (live)
            for (int m = 0; m < n; ++m)
                for (int z = lane; z < W; z += 64) xr[m * wp + z] = img[(size_t)m * vol + (size_t)row * W + z];
        __syncthreads();                // rows staged (first pass: c2 too)
        if (!live) continue;
        float acc[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) acc[k] = 0.f;
        for (int m = 0; m < n; ++m) {
            const float* x = xr + m * wp;
            const float* c = c2 + m * 2 * W;
            int zp = 0;
            for (; zp + 4 <= W; zp += 4) {
                const float4 v = *reinterpret_cast<const float4*>(x + zp);
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const float* ck = c + tap[k] - zp;
                    acc[k] = fmaf(ck[0], v.x, acc[k]);
                    acc[k] = fmaf(ck[-1], v.y, acc[k]);
                    acc[k] = fmaf(ck[-2], v.z, acc[k]);
                    acc[k] = fmaf(ck[-3], v.w, acc[k]);
                }
            }
            for (; zp < W; ++zp) {
                const float v = x[zp];
#pragma unroll
                for (int k = 0; k < NT; ++k) acc[k] = fmaf(c[tap[k] - zp], v, acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int z = lane + 64 * k;
            if (z < W) dst[(size_t)row * W + z] = acc[k];
        }
    }
}

}  // namespace mri3d

using namespace mri3d;

extern "C" int mri3d_kspace_mix_f32(const float* images, float* out, int32_t s, int32_t n, int32_t d, int32_t h, int32_t w,
                                    const float* coef, mri3d_stream_t stream) {
    MRI3D_REQUIRE(images && out && coef, MRI3D_EINVAL, "kspace_mix: null pointer (images %p, out %p, coef %p)",
                  (const void*)images, (const void*)out, (const void*)coef);
    MRI3D_REQUIRE(s > 0 && d > 0 && h > 0 && w > 0, MRI3D_EINVAL, "kspace_mix: extents must be positive (%d x %d,%d,%d)", s, d, h, w);
    MRI3D_REQUIRE(n >= 1 && n <= kMixMaxN, MRI3D_EINVAL, "kspace_mix: %d images per subject (1..%d)", n, kMixMaxN);
    MRI3D_REQUIRE(w <= kMixMaxW, MRI3D_EINVAL, "kspace_mix: w = %d (at most %d: a lane holds w / 64 outputs and a block the rows of 4 waves in LDS)",
                  w, kMixMaxW);
    MRI3D_REQUIRE(s <= 65535 && (int64_t)d * h < 0x7fffffffLL, MRI3D_ENOTSUP, "kspace_mix: batch or volume too large");
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(coef)) & 3) == 0,
                  MRI3D_EINVAL, "kspace_mix: pointers not aligned to float");
    const size_t vol = (size_t)d * h * w * 4;
    MRI3D_REQUIRE(!overlaps(images, (size_t)s * n * vol, out, (size_t)s * vol) &&
                      !overlaps(coef, (size_t)s * n * w * 4, out, (size_t)s * vol),
                  MRI3D_EINVAL, "kspace_mix: out must not overlap images or coef");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rows = d * h;
    const int wp = (w + 3) & ~3;
    const size_t lds_bytes = ((size_t)((2 * w * n + 3) & ~3) + (size_t)kMixWaves * n * wp) * sizeof(float);   // <= 48 KiB
    const dim3 grid((unsigned)std::min(cdiv(rows, kMixWaves), kMixMaxBlocksX), (unsigned)s), block(64 * kMixWaves);
#define MRI3D_MIX_LAUNCH(NT) \
    hipLaunchKernelGGL(kspace_mix_kernel<NT>, grid, block, lds_bytes, st, images, out, n, rows, w, coef)
    switch (cdiv(w, 64)) {
        case 1: MRI3D_MIX_LAUNCH(1); break;
        case 2: MRI3D_MIX_LAUNCH(2); break;
        case 3: MRI3D_MIX_LAUNCH(3); break;
        default: MRI3D_MIX_LAUNCH(4); break;
    }
#undef MRI3D_MIX_LAUNCH
    return check_launch("kspace_mix");
}
