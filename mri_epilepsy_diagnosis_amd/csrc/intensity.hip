// intensity.hip — intensity statistics of a stack of volumes on the device: the moments of each volume (count, range, mean,
// unbiased variance) and its Gaussian kernel density estimate at m positions, scipy.stats.gaussian_kde's closed form
//     density[j] = sum_i exp(-(p_j - x_i)^2 / 2h^2) / (count * sqrt(2 pi h^2)),    h^2 = variance * factor^2.
// Reference: plot_histogram (classification/transfer/full_sample_classification.ipynb cell 9), gaussian_kde over all voxels of a
// volume at np.linspace(min, max, 100).
//
// The file is compiled with -ffp-contract=off: np.linspace rounds its multiply and its add separately, and so do the positions
// here; the restatement in tests/intensity_ref.py rounds where this file rounds.
//
// Moments: an HBM-bound pass, 4 bytes (+ 1 with a mask) per voxel.  KDE: count * m exponentials, bound by the issue rate of
// v_exp_f32; the volume is read once.  Both assign voxels to lanes by their index in the row alone, so a row's bits do not depend
// on its alignment, on the other rows of the batch or on what the workspace held.
//
// Plan of the KDE (mri3d_kde_plan reports it): a block of 4 waves walks tiles of kKdeTile = 1024 voxels, tile t of a row going to
// block t mod blocks, blocks = min(tiles, 1024) per row.  A tile is staged in LDS as (x - mean) * sqrt(log2 e / 2h^2) in fp32, a
// voxel that does not count as +inf (it then adds exp2(-inf) = 0 exactly).  Wave w takes voxels [256 w, 256 w + 256) of the tile.
// Lanes are positions: lane l owns positions l, l + 64, ... in `slots` registers (slots = the power of two >= ceil(m / 64)), every
// lane reads the same LDS words (a broadcast), and no cross-lane reduction exists.  Per pair: one subtract, one multiply, one
// exp2, one add into an fp32 sum that runs over the wave's 256 voxels of a tile and is then added to a float64 of the lane.  The
// four waves' float64 sums are added in wave order and written as one partial per (block, position); a second kernel adds the
// partials of a row in a fixed order and scales.
#include "common.h"
#include <math.h>

namespace mri3d {

constexpr int kIntMaxBlocks = 1024;   // per row, both passes: 256 CUs x 4 blocks
constexpr int kMomTile = 4096;        // voxels a block takes per trip of the moments pass: 16 per lane
constexpr int kKdeTile = 1024;        // voxels per LDS tile of the KDE: 4 per lane to stage, 256 per wave to evaluate
constexpr int kKdeRun = kKdeTile / 4; // voxels whose terms are summed in fp32 before the sum goes into a float64
constexpr int kKdeMaxM = 1024;
constexpr int kMomFields = 6;         // count, non-finite count, min, max, sum, sum of squares

// Four consecutive voxels of a row from element e (a multiple of 4), and for each whether it counts (one byte of `counted` per
// voxel: in the row and, with a mask, mask byte non-zero).  vec: the row's x is 16-byte aligned and its mask 4-byte aligned.
struct Quad {
    float v[4];
    uint32_t counted;
};

__device__ __forceinline__ Quad load_quad(const float* __restrict__ xr, const uint8_t* __restrict__ mr, int64_t e, int64_t n, bool vec) {
    Quad q;
    q.v[0] = q.v[1] = q.v[2] = q.v[3] = 0.f;
    q.counted = 0u;
    if (vec && e + 4 <= n) {
        const float4 t = *reinterpret_cast<const float4*>(xr + e);
        q.v[0] = t.x, q.v[1] = t.y, q.v[2] = t.z, q.v[3] = t.w;
        q.counted = mr ? *reinterpret_cast<const uint32_t*>(mr + e) : 0x01010101u;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (e + c < n) {
                q.v[c] = xr[e + c];
                const uint32_t mk = mr ? (uint32_t)mr[e + c] : 1u;
                q.counted |= mk << (8 * c);
            }
        }
    }
    return q;
}

__device__ __forceinline__ bool quad_counts(const Quad& q, int c) { return ((q.counted >> (8 * c)) & 0xffu) != 0u; }

__device__ __forceinline__ bool row_vec(const float* xr, const uint8_t* mr) {
    return (reinterpret_cast<uintptr_t>(xr) & 15) == 0 && (reinterpret_cast<uintptr_t>(mr) & 3) == 0;
}

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ------------------------------------------------------------------ moments
// part[row][block][6] doubles.  A lane adds the 16 voxels of its trip in index order into a float64 that starts at 0, then that
// into its running sum; squares of fp32 values are exact in float64.  Non-finite voxels are counted and left out of every sum.
__global__ void __launch_bounds__(256)
moments_partial_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, int64_t n, double* __restrict__ part) {
    __shared__ double red[4][kMomFields];
    const int row = blockIdx.y;
    const float* xr = x + (int64_t)row * n;
    const uint8_t* mr = mask ? mask + (int64_t)row * n : nullptr;
    const bool vec = row_vec(xr, mr);
    unsigned cnt = 0u, bad = 0u;
    float lo = INFINITY, hi = -INFINITY;
    double S = 0.0, Q = 0.0;
    const int64_t tiles = (n + kMomTile - 1) / kMomTile;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        Quad q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = load_quad(xr, mr, t * kMomTile + 4 * ((int64_t)threadIdx.x + 256 * k), n, vec);
        double s = 0.0, qq = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (quad_counts(q[k], c)) {
                    const float v = q[k].v[c];
                    ++cnt;
                    if (isfinite(v)) {
                        lo = fminf(lo, v), hi = fmaxf(hi, v);
                        const double d = (double)v;
                        s += d;
                        qq += d * d;
                    } else {
                        ++bad;
                    }
                }
            }
        }
        S += s;
        Q += qq;
    }
    const unsigned wc = wave_sum_u(cnt), wb = wave_sum_u(bad);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    S = wave_sum_d(S);
    Q = wave_sum_d(Q);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red[wave][0] = (double)wc, red[wave][1] = (double)wb, red[wave][2] = (double)lo, red[wave][3] = (double)hi;
        red[wave][4] = S, red[wave][5] = Q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)row * gridDim.x + blockIdx.x) * kMomFields;
        p[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        p[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        p[2] = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
        p[3] = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
        p[4] = ((red[0][4] + red[1][4]) + red[2][4]) + red[3][4];
        p[5] = ((red[0][5] + red[1][5]) + red[2][5]) + red[3][5];
    }
}

// one block per row: lane t adds partials t, t + 256, ... in that order, then a tree over the 256 lanes
__global__ void __launch_bounds__(256)
moments_finalize_kernel(const double* __restrict__ part, int nblk, double* __restrict__ moments) {
    __shared__ double red[kMomFields][256];
    const int row = blockIdx.x;
    const double* p = part + (size_t)row * nblk * kMomFields;
    double a[kMomFields] = {0.0, 0.0, (double)INFINITY, -(double)INFINITY, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblk; b += 256) {
        const double* q = p + (size_t)b * kMomFields;
        a[0] += q[0], a[1] += q[1], a[2] = fmin(a[2], q[2]), a[3] = fmax(a[3], q[3]), a[4] += q[4], a[5] += q[5];
    }
#pragma unroll
    for (int f = 0; f < kMomFields; ++f) red[f][threadIdx.x] = a[f];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const int o = threadIdx.x + w;
            red[0][threadIdx.x] += red[0][o];
            red[1][threadIdx.x] += red[1][o];
            red[2][threadIdx.x] = fmin(red[2][threadIdx.x], red[2][o]);
            red[3][threadIdx.x] = fmax(red[3][threadIdx.x], red[3][o]);
            red[4][threadIdx.x] += red[4][o];
            red[5][threadIdx.x] += red[5][o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double cnt = red[0][0], bad = red[1][0], lo = red[2][0], hi = red[3][0], S = red[4][0], Q = red[5][0];
        const double nf = cnt - bad;                       // the finite voxels: what min, max, mean and variance describe
        const double mean = S / nf;                        // 0 / 0 = NaN for an empty row
        double var = NAN;
        if (nf >= 2.0) {
            var = (Q - S * mean) / (nf - 1.0);
            if (lo == hi || !(var > 0.0)) var = 0.0;       // a constant row has no variance, whatever the rounding of Q and S left
        }
        double* m = moments + (size_t)row * 8;
        m[0] = cnt, m[1] = bad, m[2] = lo, m[3] = hi, m[4] = mean, m[5] = var, m[6] = 0.0, m[7] = 0.0;
    }
}

// ------------------------------------------------------------------ KDE
// What both KDE kernels derive from a moments row, by the same operations: whether the row has a density at all, the centre and
// scale of the staged values, and the normalisation.
struct KdeRow {
    bool ok;
    double lo, hi, mean, scale, norm;
};

__device__ __forceinline__ KdeRow kde_row(const double* __restrict__ mom, int bw_rule, double bw_scalar) {
    KdeRow r;
    const double cnt = mom[0], bad = mom[1], var = mom[5];
    r.lo = mom[2], r.hi = mom[3], r.mean = mom[4];
    r.ok = cnt >= 2.0 && bad == 0.0 && var > 0.0 && var < (double)INFINITY;
    r.scale = 0.0, r.norm = NAN;
    if (r.ok) {
        const double factor = bw_rule == 0 ? pow(cnt, -0.2) : bw_rule == 1 ? pow(cnt * 3.0 / 4.0, -0.2) : bw_scalar;
        const double h2 = var * (factor * factor);
        r.scale = sqrt(1.4426950408889634 / (2.0 * h2));        // exp(-d^2 / 2h^2) = exp2(-(d scale)^2)
        r.norm = cnt * sqrt(6.283185307179586 * h2);
        r.ok = r.scale > 0.0 && r.scale < (double)INFINITY && r.norm > 0.0 && r.norm < (double)INFINITY;
    }
    return r;
}

// np.linspace(lo, hi, num=m)[j] to the bit: j * step and + lo rounded separately, the last element hi itself
__device__ __forceinline__ double kde_position(const double* __restrict__ positions, const KdeRow& r, int j, int m) {
    if (positions) return positions[j];
    if (m == 1) return r.lo;
    if (j == m - 1) return r.hi;
    const double step = (r.hi - r.lo) / (double)(m - 1);
    const double t = (double)j * step;
    return t + r.lo;
}

template <int SLOTS>
__global__ void __launch_bounds__(256)
kde_partial_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, int64_t n, const double* __restrict__ moments,
                   const double* __restrict__ positions, int m, int bw_rule, double bw_scalar, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float tile[kKdeTile];
    __shared__ double red[SLOTS * 64];
    const int row = blockIdx.y;
    const KdeRow r = kde_row(moments + (size_t)row * 8, bw_rule, bw_scalar);
    if (!r.ok) return;                                   // the whole block: the finalize kernel writes NaN for this row
    const float* xr = x + (int64_t)row * n;
    const uint8_t* mr = mask ? mask + (int64_t)row * n : nullptr;
    const bool vec = row_vec(xr, mr);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

    float ps[SLOTS], acc[SLOTS];
    double sum[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int j = lane + 64 * s;
        ps[s] = j < m ? (float)((kde_position(positions, r, j, m) - r.mean) * r.scale) : 0.f;
        sum[s] = 0.0;
    }

    const int64_t tiles = (n + kKdeTile - 1) / kKdeTile;
    int64_t t = blockIdx.x;
    Quad q = load_quad(xr, mr, t * kKdeTile + 4 * (int64_t)threadIdx.x, n, vec);
    for (; t < tiles; t += gridDim.x) {
        float4 st;
        float* sv = reinterpret_cast<float*>(&st);
#pragma unroll
        for (int c = 0; c < 4; ++c) sv[c] = quad_counts(q, c) ? (float)(((double)q.v[c] - r.mean) * r.scale) : INFINITY;
        *reinterpret_cast<float4*>(&tile[4 * threadIdx.x]) = st;
        __syncthreads();
        if (t + gridDim.x < tiles) q = load_quad(xr, mr, (t + gridDim.x) * kKdeTile + 4 * (int64_t)threadIdx.x, n, vec);
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) acc[s] = 0.f;
        const float* mine = tile + wave * kKdeRun;
#pragma unroll 2
        for (int v = 0; v < kKdeRun; v += 4) {
            const float4 xv = *reinterpret_cast<const float4*>(mine + v);
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    const float d = ps[s] - xs[c];
                    acc[s] += __builtin_amdgcn_exp2f(-(d * d));
                }
            }
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) sum[s] += (double)acc[s];
        __syncthreads();
    }
    // ((wave 0 + wave 1) + wave 2) + wave 3, per position
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const int j = lane + 64 * s;
                const double tot = w == 0 ? sum[s] : red[j] + sum[s];
                if (w < 3) red[j] = tot;
                else if (j < m) part[((size_t)row * gridDim.x + blockIdx.x) * m + j] = tot;
            }
        }
        if (w < 3) __syncthreads();
    }
}

// 4 positions x 64 chains per block: chain c adds partials c, c + 64, ... of its position in that order (at most 16, their loads all
// in flight at once), then the 64 chains are added in chain order.  Writes the positions as well.
constexpr int kFinPos = 4, kFinChains = 64;

__global__ void __launch_bounds__(256)
kde_finalize_kernel(const double* __restrict__ part, int nblk, const double* __restrict__ moments, const double* __restrict__ positions,
                    int m, int bw_rule, double bw_scalar, double* __restrict__ positions_out, double* __restrict__ density) {
    __shared__ double red[kFinChains][kFinPos];
    const int row = blockIdx.y;
    const KdeRow r = kde_row(moments + (size_t)row * 8, bw_rule, bw_scalar);
    const int pj = threadIdx.x % kFinPos, chain = threadIdx.x / kFinPos;
    const int j = blockIdx.x * kFinPos + pj;
    double a = 0.0;
    if (r.ok && j < m) {
        const double* p = part + (size_t)row * nblk * m + j;
#pragma unroll 16
        for (int b = chain; b < nblk; b += kFinChains) a += p[(size_t)b * m];
    }
    red[chain][pj] = a;
    __syncthreads();
    if (chain == 0 && j < m) {
        double tot = red[0][pj];
        for (int c = 1; c < kFinChains; ++c) tot += red[c][pj];
        const size_t o = (size_t)row * m + j;
        positions_out[o] = kde_position(positions, r, j, m);
        density[o] = r.ok ? tot / r.norm : NAN;
    }
}

static int int_blocks(int64_t n, int tile) { return (int)std::min<int64_t>(cdiv64(n, tile), kIntMaxBlocks); }
static int kde_slots(int m) {
    int s = 1;
    while (s * 64 < m) s *= 2;
    return s;
}
static bool int_shape_ok(int64_t n, int32_t batch) { return n > 0 && batch > 0 && batch <= 65535 && n <= (INT64_MAX >> 8) / batch; }

}  // namespace mri3d

using namespace mri3d;

extern "C" size_t mri3d_intensity_workspace_bytes(int64_t n, int32_t batch, int32_t m) {
    if (!int_shape_ok(n, batch) || m < 0 || m > kKdeMaxM) return 0;
    const size_t mom = (size_t)int_blocks(n, kMomTile) * kMomFields, kde = (size_t)int_blocks(n, kKdeTile) * (size_t)m;
    return (size_t)batch * std::max(mom, kde) * sizeof(double);
}

extern "C" int mri3d_kde_plan(int64_t n, int32_t batch, int32_t m, int32_t out[4]) {
    MRI3D_REQUIRE(out != nullptr, MRI3D_EINVAL, "kde_plan: null output");
    MRI3D_REQUIRE(int_shape_ok(n, batch), MRI3D_EINVAL, "kde_plan: n = %lld, batch = %d", (long long)n, batch);
    MRI3D_REQUIRE(m >= 1 && m <= kKdeMaxM, MRI3D_EINVAL, "kde_plan: m = %d outside 1..%d", m, kKdeMaxM);
    const int nblk = int_blocks(n, kKdeTile);
    out[0] = nblk;
    out[1] = kKdeTile;
    out[2] = kde_slots(m);
    out[3] = (int32_t)std::min<int64_t>(cdiv64(cdiv64(n, kKdeTile), nblk), INT32_MAX);
    return MRI3D_OK;
}

extern "C" int mri3d_intensity_moments_f32(const float* x, const uint8_t* mask, int64_t n, int32_t batch, double* moments,
                                           void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(int_shape_ok(n, batch), MRI3D_EINVAL, "intensity_moments: n = %lld, batch = %d", (long long)n, batch);
    MRI3D_REQUIRE(x && moments, MRI3D_EINVAL, "intensity_moments: null pointer");
    MRI3D_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(moments) & 7) == 0, MRI3D_EINVAL,
                  "intensity_moments: a pointer is not aligned to its element");
    const size_t need = mri3d_intensity_workspace_bytes(n, batch, 0);
    MRI3D_REQUIRE(workspace && ws_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MRI3D_EWORKSPACE,
                  "intensity_moments: workspace %zu < %zu, or not 8-byte aligned", ws_bytes, need);
    MRI3D_REQUIRE(!overlaps(moments, (size_t)batch * 8 * sizeof(double), workspace, need), MRI3D_EINVAL,
                  "intensity_moments: moments overlap the workspace");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = int_blocks(n, kMomTile);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(moments_partial_kernel, dim3(nblk, batch), dim3(256), 0, s, x, mask, n, part);
    hipLaunchKernelGGL(moments_finalize_kernel, dim3(batch), dim3(256), 0, s, part, nblk, moments);
    return check_launch("intensity_moments");
}

extern "C" int mri3d_kde_f32(const float* x, const uint8_t* mask, int64_t n, int32_t batch, const double* moments,
                             const double* positions, int32_t m, int32_t bw_rule, double bw_scalar, double* positions_out,
                             double* density, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(int_shape_ok(n, batch), MRI3D_EINVAL, "kde: n = %lld, batch = %d", (long long)n, batch);
    MRI3D_REQUIRE(m >= 1 && m <= kKdeMaxM, MRI3D_EINVAL, "kde: m = %d outside 1..%d", m, kKdeMaxM);
    MRI3D_REQUIRE(bw_rule >= 0 && bw_rule <= 2, MRI3D_EINVAL, "kde: bandwidth rule %d outside 0..2", bw_rule);
    MRI3D_REQUIRE(bw_rule != 2 || (bw_scalar > 0.0 && bw_scalar < (double)INFINITY), MRI3D_EINVAL,
                  "kde: the bandwidth factor must be positive and finite, got %g", bw_scalar);
    MRI3D_REQUIRE(x && moments && positions_out && density, MRI3D_EINVAL, "kde: null pointer");
    MRI3D_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 &&
                      ((reinterpret_cast<uintptr_t>(moments) | reinterpret_cast<uintptr_t>(positions) |
                        reinterpret_cast<uintptr_t>(positions_out) | reinterpret_cast<uintptr_t>(density)) & 7) == 0,
                  MRI3D_EINVAL, "kde: a pointer is not aligned to its element");
    const size_t need = mri3d_intensity_workspace_bytes(n, batch, m), out_bytes = (size_t)batch * m * sizeof(double);
    MRI3D_REQUIRE(workspace && ws_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MRI3D_EWORKSPACE,
                  "kde: workspace %zu < %zu, or not 8-byte aligned", ws_bytes, need);
    MRI3D_REQUIRE(!overlaps(positions_out, out_bytes, density, out_bytes) && !overlaps(positions_out, out_bytes, workspace, need) &&
                      !overlaps(density, out_bytes, workspace, need) &&
                      !overlaps(moments, (size_t)batch * 8 * sizeof(double), workspace, need) &&
                      !overlaps(positions, (size_t)m * sizeof(double), positions_out, out_bytes) &&
                      !overlaps(positions, (size_t)m * sizeof(double), density, out_bytes),
                  MRI3D_EINVAL, "kde: outputs, workspace and inputs overlap");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = int_blocks(n, kKdeTile);
    double* part = static_cast<double*>(workspace);
#define KDE_LAUNCH(S)                                                                                                    \
    hipLaunchKernelGGL((kde_partial_kernel<S>), dim3(nblk, batch), dim3(256), 0, s, x, mask, n, moments, positions, m, \
                       bw_rule, bw_scalar, part)
    switch (kde_slots(m)) {
        case 1: KDE_LAUNCH(1); break;
        case 2: KDE_LAUNCH(2); break;
        case 4: KDE_LAUNCH(4); break;
        case 8: KDE_LAUNCH(8); break;
        default: KDE_LAUNCH(16); break;
    }
#undef KDE_LAUNCH
    hipLaunchKernelGGL(kde_finalize_kernel, dim3(cdiv(m, kFinPos), batch), dim3(256), 0, s, part, nblk, moments, positions, m, bw_rule,
                       bw_scalar, positions_out, density);
    return check_launch("kde");
}
