// augment.hip — the random stages of the reference's TorchIO training transform on HBM-resident volumes.
// Reference call sites: `training_transform = Compose([... RandomBiasField(), ... RandomFlip(axes=(0,)),
// OneOf({RandomAffine(): 0.8, RandomElasticDeformation(): 0.2})])`, segmentation/results_validation.ipynb (the cell that
// builds `training_transform`) and segmentation/pretraining_3d_unet.ipynb cell 24; handed to
// `torchio.ImagesDataset(subjects, transform=transform)` at segmentation/routine.py:91.  TorchIO is a third-party dependency
// that is absent from the reference tree ("parity unpinned"): the arithmetic below is this project's own definition, restated
// in float64 numpy by tests/augment_ref.py.  Random numbers are drawn on the host; the kernels are deterministic maps.
//
//   mri3d_warp3d         for every output voxel o = (d, h, w) of subject s:   src = A[s][:, :3] o + A[s][:, 3] + u_s(o)
//                        u = tensor-product uniform cubic B-spline over a (g_d, g_h, g_w) control grid, per axis
//                        p = (o + 0.5) m / N, m = g - 3, i = clamp(floor p, 0, m - 1), f = p - i, control points i .. i + 3.
//                        inside = -0.5 <= src_a <= N_a - 0.5 on all axes.  Image: trilinear over floor(src), floor(src) + 1
//                        (indices clamped), pad value outside.  Label: raw bits of the element at clamp(floor(src + 0.5)),
//                        zero bits outside.  One pass: the source coordinate is computed once for both.
//   mri3d_bias_field_f32 y = x exp(P(xh, yh, zh)), (xh, yh, zh) = np.linspace(-1, 1, N) per axis (0 when N == 1),
//                        P = sum c_ijk xh^i yh^j zh^k, i in 0..order, j in 0..order-i, k in 0..order-i-j (that nesting order).
//
// warp3d: one wave owns one (subject, d, h) row and walks it 64 voxels of w at a time, so stores are 256 contiguous bytes.
// What does not depend on w is formed once per row: the d, h terms of the affine map, and the control grid contracted over its
// d and h weights, which leaves 3 g_w numbers in LDS; a voxel then costs 4 taps x 3 FMAs for u.  That row prologue is NOT
// latency-hidden as written: only 3 g_w lanes work (21 for g = 7), hipcc issues their 16 loads in groups of two to four with a
// full wait after each, and the prologue sits between two block-wide barriers although ctr[wave] is private to a wave — about
// ten dependent round trips per row, the first thing to look at on the elastic path.
// In the voxel loop the eight neighbour loads are issued together from clamped addresses and the inside mask is applied to the
// result (a load behind `valid ? load : 0` gets a wait of its own).  The gather is served by L2: the four rows of a
// block are neighbours in h, and for +-10 degrees a wave's 64 sources span a few source rows.  No atomics.
#include "common.h"
#include <algorithm>

namespace mri3d {

constexpr int kWarpWaves = 4;       // rows per block
constexpr int kMaxGridW = 64;       // control points along w held in LDS per wave
constexpr int kBiasChunk = 32;      // subjects per bias-field launch (coefficients travel by value)
constexpr int kBiasCoef = 20;       // order 3

struct SplineTap { int i; float b0, b1, b2, b3; };

// p = (o + 0.5) m / N;  uniform cubic B-spline weights on control points i .. i + 3
__device__ __forceinline__ SplineTap spline_tap(int o, int m, float m_over_n) {
    const float p = ((float)o + 0.5f) * m_over_n;
    SplineTap t;
    t.i = min(max((int)floorf(p), 0), m - 1);
    const float f = p - (float)t.i, g = 1.f - f, f2 = f * f, f3 = f2 * f;
    t.b0 = g * g * g * (1.f / 6.f);
    t.b1 = (3.f * f3 - 6.f * f2 + 4.f) * (1.f / 6.f);
    t.b2 = (-3.f * f3 + 3.f * f2 + 3.f * f + 1.f) * (1.f / 6.f);
    t.b3 = f3 * (1.f / 6.f);
    return t;
}

template <int LB> struct LabelElem { typedef uint8_t type; };
template <> struct LabelElem<2> { typedef uint16_t type; };
template <> struct LabelElem<4> { typedef uint32_t type; };

// LB = label element bytes (0: no label);  GRID = a control grid is given
template <int LB, bool GRID>
__global__ void __launch_bounds__(64 * kWarpWaves)
warp3d_kernel(const float* __restrict__ img, float* __restrict__ img_out, const void* __restrict__ lab_v,
              void* __restrict__ lab_out_v, int S, int D, int H, int W, const float* __restrict__ affine,
              const float* __restrict__ cgrid, int gd, int gh, int gw, float pad, const float* __restrict__ pad_dev) {
    typedef typename LabelElem<LB>::type L;
    const L* __restrict__ lab = static_cast<const L*>(lab_v);
    L* __restrict__ lab_out = static_cast<L*>(lab_out_v);
    __shared__ float ctr[kWarpWaves][3][kMaxGridW];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rows = S * D * H;   // < 2^31, checked by the host
    const float w_scale = GRID ? (float)(gw - 3) / (float)W : 0.f;
    // every wave of the block runs the same number of iterations: the barriers below are block-wide
    for (int base = blockIdx.x * kWarpWaves; base < rows; base += gridDim.x * kWarpWaves) {
        const int row = base + wave;
        const bool live = row < rows;   // wave-uniform
        const int rr = live ? row : rows - 1;
        const int h = rr % H, sd = rr / H;
        const int d = sd % D, s = sd / D;
        if (GRID) {
            __syncthreads();   // the previous row's taps have been read
            const SplineTap td = spline_tap(d, gd - 3, (float)(gd - 3) / (float)D), th = spline_tap(h, gh - 3, (float)(gh - 3) / (float)H);
            const float bd[4] = {td.b0, td.b1, td.b2, td.b3}, bh[4] = {th.b0, th.b1, th.b2, th.b3};
            for (int j = lane; j < 3 * gw; j += 64) {
                const int comp = j / gw, k = j - comp * gw;
                const float* g = cgrid + (((size_t)(s * 3 + comp) * gd + td.i) * gh + th.i) * gw + k;
                float acc = 0.f;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc = fmaf(bd[a] * bh[b], g[((size_t)a * gh + b) * gw], acc);
                ctr[wave][comp][k] = acc;
            }
            __syncthreads();
        }
        if (!live) continue;
        const float* A = affine + (size_t)s * 12;
        const float fd = (float)d, fh = (float)h;
        // the row's share of the map: A[:, 0] d + A[:, 1] h + A[:, 3]
        const float r0 = fmaf(A[0], fd, fmaf(A[1], fh, A[3])), a0 = A[2];
        const float r1 = fmaf(A[4], fd, fmaf(A[5], fh, A[7])), a1 = A[6];
        const float r2 = fmaf(A[8], fd, fmaf(A[9], fh, A[11])), a2 = A[10];
        const float padv = pad_dev ? pad_dev[s] : pad;
        const size_t vol = (size_t)s * D * H * W, out_row = (size_t)rr * W;
        for (int w = lane; w < W; w += 64) {
            const float fw = (float)w;
            float s0 = fmaf(a0, fw, r0), s1 = fmaf(a1, fw, r1), s2 = fmaf(a2, fw, r2);
            if (GRID) {
                const SplineTap tw = spline_tap(w, gw - 3, w_scale);
                const float* c0 = &ctr[wave][0][tw.i];
                const float* c1 = &ctr[wave][1][tw.i];
                const float* c2 = &ctr[wave][2][tw.i];
                s0 += fmaf(tw.b3, c0[3], fmaf(tw.b2, c0[2], fmaf(tw.b1, c0[1], tw.b0 * c0[0])));
                s1 += fmaf(tw.b3, c1[3], fmaf(tw.b2, c1[2], fmaf(tw.b1, c1[1], tw.b0 * c1[0])));
                s2 += fmaf(tw.b3, c2[3], fmaf(tw.b2, c2[2], fmaf(tw.b1, c2[1], tw.b0 * c2[0])));
            }
            const bool inside = s0 >= -0.5f && s0 <= (float)D - 0.5f && s1 >= -0.5f && s1 <= (float)H - 0.5f &&
                                s2 >= -0.5f && s2 <= (float)W - 0.5f;
            // clamp before the float -> int conversion: any value (NaN included) yields an in-range address
            const float q0 = fminf(fmaxf(s0, -1.f), (float)D), q1 = fminf(fmaxf(s1, -1.f), (float)H),
                        q2 = fminf(fmaxf(s2, -1.f), (float)W);
            if (img) {
                const float e0 = floorf(q0), e1 = floorf(q1), e2 = floorf(q2);
                const float f0 = q0 - e0, f1 = q1 - e1, f2 = q2 - e2;
                const int i0 = (int)e0, i1 = (int)e1, i2 = (int)e2;
                const size_t d_lo = (size_t)min(max(i0, 0), D - 1) * H, d_hi = (size_t)min(max(i0 + 1, 0), D - 1) * H;
                const size_t h_lo = (size_t)min(max(i1, 0), H - 1), h_hi = (size_t)min(max(i1 + 1, 0), H - 1);
                const int w_lo = min(max(i2, 0), W - 1), w_hi = min(max(i2 + 1, 0), W - 1);
                const float* v = img + vol;
                const float* p00 = v + (d_lo + h_lo) * W;
                const float* p01 = v + (d_lo + h_hi) * W;
                const float* p10 = v + (d_hi + h_lo) * W;
                const float* p11 = v + (d_hi + h_hi) * W;
                const float v000 = p00[w_lo], v001 = p00[w_hi], v010 = p01[w_lo], v011 = p01[w_hi];
                const float v100 = p10[w_lo], v101 = p10[w_hi], v110 = p11[w_lo], v111 = p11[w_hi];
                const float x00 = fmaf(f2, v001 - v000, v000), x01 = fmaf(f2, v011 - v010, v010);
                const float x10 = fmaf(f2, v101 - v100, v100), x11 = fmaf(f2, v111 - v110, v110);
                const float y0 = fmaf(f1, x01 - x00, x00), y1 = fmaf(f1, x11 - x10, x10);
                const float r = fmaf(f0, y1 - y0, y0);
                img_out[out_row + w] = inside ? r : padv;
            }
            if (LB) {
                const int n0 = min(max((int)floorf(q0 + 0.5f), 0), D - 1), n1 = min(max((int)floorf(q1 + 0.5f), 0), H - 1),
                          n2 = min(max((int)floorf(q2 + 0.5f), 0), W - 1);
                const L v = lab[vol + ((size_t)n0 * H + n1) * W + n2];
                lab_out[out_row + w] = inside ? v : (L)0;
            }
        }
    }
}

struct BiasCoef { float c[kBiasChunk][kBiasCoef]; };   // order-3 layout; terms above the caller's order are zero

// P at (xh, yh) as a cubic in zh: q[k] = sum_{i + j <= 3 - k} c_ijk xh^i yh^j  (fully unrolled: q stays in registers)
__device__ __forceinline__ void bias_row(const float* c, float xh, float yh, float q[4]) {
    q[0] = q[1] = q[2] = q[3] = 0.f;
    int n = 0;
    float xi = 1.f;
#pragma unroll
    for (int i = 0; i <= 3; ++i) {
        float yj = xi;
#pragma unroll
        for (int j = 0; j <= 3 - i; ++j) {
#pragma unroll
            for (int k = 0; k <= 3 - i - j; ++k) q[k] = fmaf(c[n++], yj, q[k]);
            yj *= yh;
        }
        xi *= xh;
    }
}

__device__ __forceinline__ float bias_apply(float x, const float q[4], float zh) {
    return x * expf(fmaf(fmaf(fmaf(q[3], zh, q[2]), zh, q[1]), zh, q[0]));
}

// blockIdx.y = subject of this launch (its coefficients are scalar loads of the kernel arguments).
// VEC = 4: W % 4 == 0 and 16-byte aligned pointers, a lane takes 4 consecutive w (16 B);  VEC = 1: any W
template <int VEC>
__global__ void __launch_bounds__(256)
bias_field_kernel(const float* __restrict__ x, float* __restrict__ y, int D, int H, int W, BiasCoef coef, float step_d,
                  float step_h, float step_w) {
    const int wv = W / VEC;
    const long long per = (long long)D * H * wv;
    const float* c = coef.c[blockIdx.y];
    x += (long long)blockIdx.y * per * VEC;
    y += (long long)blockIdx.y * per * VEC;
    const float z0 = W > 1 ? -1.f : 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(i / wv), w = (int)(i - (long long)row * wv) * VEC;
        const int h = row % H, d = row / H;
        float q[4];
        bias_row(c, fmaf((float)d, step_d, D > 1 ? -1.f : 0.f), fmaf((float)h, step_h, H > 1 ? -1.f : 0.f), q);
        if (VEC == 4) {
            float4 v = ldf4(x + i * 4);
            v.x = bias_apply(v.x, q, fmaf((float)w, step_w, z0));
            v.y = bias_apply(v.y, q, fmaf((float)(w + 1), step_w, z0));
            v.z = bias_apply(v.z, q, fmaf((float)(w + 2), step_w, z0));
            v.w = bias_apply(v.w, q, fmaf((float)(w + 3), step_w, z0));
            stf4(y + i * 4, v);
        } else {
            y[i] = bias_apply(x[i], q, fmaf((float)w, step_w, z0));
        }
    }
}

}  // namespace mri3d

using namespace mri3d;

extern "C" int mri3d_warp3d(const float* image, float* image_out, const void* label, void* label_out, int32_t label_bytes,
                            int32_t s, int32_t d, int32_t h, int32_t w, const float* affine, const float* grid, int32_t gd,
                            int32_t gh, int32_t gw, float pad_value, const float* pad_values, mri3d_stream_t stream) {
    MRI3D_REQUIRE(affine && s > 0 && d > 0 && h > 0 && w > 0, MRI3D_EINVAL, "warp3d: bad arguments (affine %p, extents %d x %d,%d,%d)",
                  (const void*)affine, s, d, h, w);
    MRI3D_REQUIRE((image != nullptr) == (image_out != nullptr) && (label != nullptr) == (label_out != nullptr), MRI3D_EINVAL,
                  "warp3d: a source without its destination (or the reverse)");
    MRI3D_REQUIRE(image || label, MRI3D_EINVAL, "warp3d: neither an image nor a label map given");
    if (label)
        MRI3D_REQUIRE(label_bytes == 1 || label_bytes == 2 || label_bytes == 4, MRI3D_ENOTSUP,
                      "warp3d: label element size %d (1, 2 or 4 bytes)", label_bytes);
    MRI3D_REQUIRE((int64_t)s * d * h < 0x7fffffffLL && (int64_t)d * h * w < 0x7fffffffLL, MRI3D_ENOTSUP, "warp3d: volume too large");
    if (grid) {
        MRI3D_REQUIRE(gd >= 4 && gh >= 4 && gw >= 4, MRI3D_EINVAL, "warp3d: control grid (%d,%d,%d) needs at least 4 points per axis",
                      gd, gh, gw);
        MRI3D_REQUIRE(gw <= kMaxGridW, MRI3D_ENOTSUP, "warp3d: %d control points along w (at most %d: a row's contracted grid is held in LDS)",
                      gw, kMaxGridW);
        MRI3D_REQUIRE((int64_t)s * 3 * gd * gh * gw < 0x7fffffffLL, MRI3D_ENOTSUP, "warp3d: control grid too large");
    }
    const size_t nvox = (size_t)s * d * h * w, lb = label ? (size_t)label_bytes : 0;
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(image_out) | reinterpret_cast<uintptr_t>(affine) |
                    reinterpret_cast<uintptr_t>(grid) | reinterpret_cast<uintptr_t>(pad_values)) & 3) == 0 &&
                      (!label || ((reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(label_out)) & (lb - 1)) == 0),
                  MRI3D_EINVAL, "warp3d: pointers not aligned to their element size");
    MRI3D_REQUIRE(!overlaps(image, nvox * 4, image_out, nvox * 4) && !overlaps(label, nvox * lb, label_out, nvox * lb) &&
                      !overlaps(image, nvox * 4, label_out, nvox * lb) && !overlaps(label, nvox * lb, image_out, nvox * 4) &&
                      !overlaps(image_out, nvox * 4, label_out, nvox * lb),
                  MRI3D_EINVAL, "warp3d: source and destination must not alias");
    const size_t abytes = (size_t)s * 12 * 4, gbytes = grid ? (size_t)s * 3 * gd * gh * gw * 4 : 0, pbytes = (size_t)s * 4;
    for (const void* dst : {(const void*)image_out, (const void*)label_out}) {
        const size_t dbytes = dst == image_out ? nvox * 4 : nvox * lb;
        MRI3D_REQUIRE(!overlaps(affine, abytes, dst, dbytes) && !overlaps(grid, gbytes, dst, dbytes) &&
                          !overlaps(pad_values, pbytes, dst, dbytes),
                      MRI3D_EINVAL, "warp3d: a destination must not alias the affine, grid or pad buffers");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rows = s * d * h;
    const dim3 grid_dim((unsigned)std::min<int64_t>(cdiv64(rows, kWarpWaves), 8 * kMaxStreamBlocks)), block(64 * kWarpWaves);
#define MRI3D_WARP_LAUNCH(LB, G)                                                                                              \
    hipLaunchKernelGGL((warp3d_kernel<LB, G>), grid_dim, block, 0, st, image, image_out, label, label_out, s, d, h, w, affine, \
                       grid, gd, gh, gw, pad_value, pad_values)
    switch ((int)lb) {
        case 0: if (grid) MRI3D_WARP_LAUNCH(0, true); else MRI3D_WARP_LAUNCH(0, false); break;
        case 1: if (grid) MRI3D_WARP_LAUNCH(1, true); else MRI3D_WARP_LAUNCH(1, false); break;
        case 2: if (grid) MRI3D_WARP_LAUNCH(2, true); else MRI3D_WARP_LAUNCH(2, false); break;
        default: if (grid) MRI3D_WARP_LAUNCH(4, true); else MRI3D_WARP_LAUNCH(4, false); break;
    }
#undef MRI3D_WARP_LAUNCH
    return check_launch("warp3d");
}

extern "C" int mri3d_bias_field_f32(const float* x, float* y, int32_t s, int32_t d, int32_t h, int32_t w,
                                    const float* coef_host, int32_t order, mri3d_stream_t stream) {
    MRI3D_REQUIRE(x && y && coef_host && s > 0 && d > 0 && h > 0 && w > 0, MRI3D_EINVAL, "bias_field: bad arguments");
    MRI3D_REQUIRE(order >= 0, MRI3D_EINVAL, "bias_field: negative order %d", order);
    MRI3D_REQUIRE(order <= 3, MRI3D_ENOTSUP, "bias_field: order %d (at most 3)", order);
    MRI3D_REQUIRE((int64_t)d * h < 0x7fffffffLL, MRI3D_ENOTSUP, "bias_field: volume too large");
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 3) == 0, MRI3D_EINVAL,
                  "bias_field: pointers not aligned to float");
    const size_t per = (size_t)d * h * w;
    // in place (y == x) is allowed; a partial overlap is not: a voxel would be read after a neighbour's write
    MRI3D_REQUIRE(x == y || !overlaps(x, (size_t)s * per * 4, y, (size_t)s * per * 4), MRI3D_EINVAL,
                  "bias_field: x and y overlap without being equal");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ncoef = (order + 1) * (order + 2) * (order + 3) / 6;
    // where term n of the caller's nesting (i, j, k up to `order`) sits in the kernel's order-3 nesting
    int slot[kBiasCoef], n = 0, n3 = 0;
    for (int i = 0; i <= 3; ++i)
        for (int j = 0; j <= 3 - i; ++j)
            for (int k = 0; k <= 3 - i - j; ++k, ++n3)
                if (i + j + k <= order) slot[n++] = n3;
    auto step = [](int len) { return len > 1 ? (float)(2.0 / (double)(len - 1)) : 0.f; };
    const bool vec = (w % 4) == 0 && aligned16(x, y);
    const int64_t items = (int64_t)per / (vec ? 4 : 1);
    BiasCoef coef;
    for (int first = 0; first < s; first += kBiasChunk) {
        const int count = std::min(kBiasChunk, s - first);
        for (int i = 0; i < kBiasChunk; ++i) {
            for (int k = 0; k < kBiasCoef; ++k) coef.c[i][k] = 0.f;
            for (int k = 0; i < count && k < ncoef; ++k) coef.c[i][slot[k]] = coef_host[(size_t)(first + i) * ncoef + k];
        }
        const float* xs = x + (size_t)first * per;
        float* ys = y + (size_t)first * per;
        if (vec)
            hipLaunchKernelGGL(bias_field_kernel<4>, dim3(stream_grid(items, 256 * 2), count), dim3(256), 0, st, xs, ys, d, h, w,
                               coef, step(d), step(h), step(w));
        else
            hipLaunchKernelGGL(bias_field_kernel<1>, dim3(stream_grid(items, 256 * 4), count), dim3(256), 0, st, xs, ys, d, h, w,
                               coef, step(d), step(h), step(w));
    }
    return check_launch("bias_field");
}
