// tissue.hip — the device passes of a bias-field estimator over tissue classes: a K-class Gaussian mixture on log-intensity with
// a smooth multiplicative field, exp(b), b a polynomial of order <= 3 in the voxel's normalised coordinates (the field family
// of mri3d_bias_field_f32, same coordinates, same nesting of the coefficients).  Reference: get_registered_img_and_mask
// (detection/preprocessing_utils.py:11-53) calls FSL FAST for its bias-corrected `_restore` image; this is the model FAST's
// correction rests on (Wells / Van Leemput), not a clone of it.  The host loop that drives these passes is
// mri_epilepsy_diagnosis_amd/tissue/.
//
// All arithmetic is float64, log and exp included; the input is fp32 and the outputs of the final pass are rounded once.  The
// file is compiled with -ffp-contract=off.
//
// mri3d_tissue_em_pass, two stages, no float atomics:
//   rows   one wave per (d, h) row, 4 rows per block and trip; lanes stride along w, 64 voxels per wave step (a wave step whose
//          voxels are all unselected costs its loads and one ballot).  The (xh, yh) part of the polynomial is hoisted out of the
//          w loop: b = ((q3 zh + q2) zh + q1) zh + q0.  A lane keeps R = 2 + 3K + (2 order + 1) + (order + 1) sums: n, LL,
//          S0/S1/S2 per class, sum w zh^q, sum t zh^q; they are reduced over the wave in a fixed tree (tis_wave_sum) and lane 0 stores the
//          row's R numbers at part[slot][row] of the workspace.  Every row writes every slot: what the workspace held before
//          never reaches a result.
//   fold   one block of 1024 threads per entry of the table: thread t adds the rows t, t + 1024, ... of the entry's slot times
//          xh^a yh^b in ascending order, and the 1024 sums meet in a fixed tree in LDS.  Same inputs, same bits.
// mri3d_tissue_mrf_pass is the same two stages with a Potts prior on a label volume (hidden-MRF EM, red-black ICM): its row kernel
// adds beta n_k to a voxel's log-terms from the six face neighbours' labels and writes the voxel's new label; the fold is shared.
// The two row kernels and the final pass are one row walk (tis_walk) around each kernel's per-voxel body; tests/test_tissue_codegen.py
// holds what the compiler makes of that to the registers of the kernels written out one by one.
// 4-byte loads per lane on purpose: the pass is bound by its float64 arithmetic, and at the template's W = 182 a wave step of
// 64 voxels keeps 182 / 192 of the lanes busy where a 16-byte step of 256 voxels would keep 182 / 256.
#include "common.h"
#include <math.h>

namespace mri3d {

constexpr int kTisWaves = 4;            // rows per block and trip
constexpr int kTisMaxBlocks = 8192;     // stage-1 grid cap: blocks beyond the resident ones back-fill as others finish
constexpr int kTisFoldThreads = 1024;
constexpr int kTisMaxK = 4;
constexpr int kTisCoef = 20;            // order-3 nesting
constexpr int kTisMaxEntries = 128;     // >= 2 + 3*4 + 84 + 20
constexpr double kTisMaxBeta = 8.0;     // of the label prior: exp(6 beta) stays far inside float64

struct TisParams {
    double a[kTisMaxK];      // log pi - 0.5 log v (- 0.5 log 2 pi in the EM pass)
    double mu[kTisMaxK];
    double inv_v[kTisMaxK];  // 1 / v
    double hiv[kTisMaxK];    // 1 / (2 v)
    double c[kTisCoef];      // order-3 layout; terms above the caller's order are zero
    double d0, h0, w0, step_d, step_h, step_w;   // coordinate of index i along an axis: x0 + i * step
};

struct TisFold { uint8_t slot[kTisMaxEntries], a[kTisMaxEntries], b[kTisMaxEntries]; };

// b at (xh, yh) as a cubic in zh: q[k] = sum_{i + j <= 3 - k} c_ijk xh^i yh^j
__device__ __forceinline__ void tis_row(const double* c, double xh, double yh, double q[4]) {
    q[0] = q[1] = q[2] = q[3] = 0.0;
    int n = 0;
    double xi = 1.0;
#pragma unroll
    for (int i = 0; i <= 3; ++i) {
        double yj = xi;
#pragma unroll
        for (int j = 0; j <= 3 - i; ++j) {
#pragma unroll
            for (int k = 0; k <= 3 - i - j; ++k) q[k] = q[k] + c[n++] * yj;
            yj = yj * yh;
        }
        xi = xi * xh;
    }
}

// The sum of v over the wave, the same bits in every lane.  The four levels inside a row of 16 lanes are DPP moves (VALU, no LDS):
// lanes 1 apart, 2 apart (quad permutes), then the other quad of an 8 (half mirror) and the other 8 of the row (mirror); a level's
// partners hold equal sums, so a mirror pairs as well as an xor.  The two levels across rows are shuffles.  22 sums a row through six
// shuffle levels each kept the CU's one LDS pipe busier than its four SIMDs.
template <int CTRL>
__device__ __forceinline__ double tis_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double tis_wave_sum(double v) {
    v = v + tis_dpp<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    v = v + tis_dpp<0x4E>(v);    // quad_perm [2, 3, 0, 1]
    v = v + tis_dpp<0x141>(v);   // row_half_mirror
    v = v + tis_dpp<0x140>(v);   // row_mirror
    v = v + __shfl_xor(v, 16, 64);
    v = v + __shfl_xor(v, 32, 64);
    return v;
}

__device__ __forceinline__ bool tis_selected(const uint8_t* mr, int w, float xv) {
    return (mr ? mr[w] != 0 : true) && isfinite(xv) && xv > 0.f;
}

// One selected voxel's terms of the row sums, from its K log-terms l (consumed): the posteriors p_k = softmax_k l_k into S0/S1/S2 and
// the moments of w and t; acc[1] is the caller's.  Returns logsumexp_k l_k.  Both row kernels go through here, operation for operation.
template <int K, int ORDER>
__device__ __forceinline__ double tis_voxel_sums(const TisParams& p, double l[K], double y, double r, double zh, double* acc) {
    constexpr int NW = 2 * ORDER + 1, NT = ORDER + 1;
    double lmax = -(double)INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) lmax = fmax(lmax, l[k]);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        l[k] = exp(l[k] - lmax);
        s = s + l[k];
    }
    const double inv_s = 1.0 / s;
    acc[0] = acc[0] + 1.0;
    double wv = 0.0, tv = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double pk = l[k] * inv_s;
        acc[2 + k] = acc[2 + k] + pk;
        acc[2 + K + k] = acc[2 + K + k] + pk * r;
        acc[2 + 2 * K + k] = acc[2 + 2 * K + k] + pk * (r * r);
        wv = wv + pk * p.inv_v[k];
        tv = tv + pk * ((y - p.mu[k]) * p.inv_v[k]);
    }
    double zq = 1.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        acc[2 + 3 * K + i] = acc[2 + 3 * K + i] + wv * zq;
        if (i < NT) acc[2 + 3 * K + NW + i] = acc[2 + 3 * K + NW + i] + tv * zq;
        zq = zq * zh;
    }
    return lmax + log(s);
}

// zh of voxel w of a row and b there, from the row's cubic
__device__ __forceinline__ double tis_field(const TisParams& p, const double q[4], int w, double& zh) {
    zh = p.w0 + (double)w * p.step_w;
    return ((q[3] * zh + q[2]) * zh + q[1]) * zh + q[0];
}

// the Gaussian log-term of class k at the residual r = y - b
__device__ __forceinline__ double tis_log_term(const TisParams& p, int k, double r) {
    const double dk = r - p.mu[k];
    return p.a[k] - (dk * dk) * p.hiv[k];
}

// the running argmax over k = 0, 1, ...: the first of equal maxima, as label k + 1
__device__ __forceinline__ void tis_argmax(int k, double lk, double& best, int& lab) {
    if (k == 0 || lk > best) best = lk, lab = k + 1;
}

// ------------------------------------------------------------------ the row walk of the three kernels
// Block and wave -> rows, a row -> (d, h) and its cubic q, then wave steps of 64 voxels along w: voxel(acc, q, at, xv, sel) runs in
// every lane that has a voxel, selected or not, and a sums kernel (R > 0) ends a row with its R sums at part[slot][row].  What a
// wave step without a selected voxel does is the kernel's choice:
enum class TisIdle {
    unknown,      // no ballot is taken: the step is like any other
    skipped,      // the step ends at its ballot (for a body that does nothing for an unselected voxel)
    unselected,   // the body runs with sel = false, a constant
};

struct TisAt { int d, h, w; size_t row0; };   // row0: the index in the volume of the row's first voxel (wave-uniform)

template <int R, TisIdle IDLE, class Voxel>
__device__ __forceinline__ void tis_walk(const float* x, const uint8_t* mask, int D, int H, int W, const TisParams& p, double* part,
                                         Voxel&& voxel) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rows = D * H;   // < 2^31, checked by the host
    double acc[R > 0 ? R : 1] = {};
    for (int row = blockIdx.x * kTisWaves + wave; row < rows; row += gridDim.x * kTisWaves) {
        const int d = row / H, h = row - d * H;
        double q[4];
        tis_row(p.c, p.d0 + (double)d * p.step_d, p.h0 + (double)h * p.step_h, q);
        const size_t base = (size_t)row * W;
        const float* xr = x + base;
        const uint8_t* mr = mask ? mask + base : nullptr;
        for (int w = lane; w < W; w += 64) {   // lanes past the row's end leave: a ballot is over the ones that have a voxel
            const TisAt at = {d, h, w, base};
            const float xv = xr[w];
            const bool sel = tis_selected(mr, w, xv);
            if (IDLE != TisIdle::unknown && __ballot(sel) == 0ull) {   // wave-uniform: background
                if (IDLE == TisIdle::unselected) voxel(acc, q, at, xv, false);
                continue;
            }
            voxel(acc, q, at, xv, sel);
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {   // the end of a row: the sums meet over the wave, lane 0 stores them, the next row starts from zero
            const double v = tis_wave_sum(acc[i]);
            if (lane == 0) part[(size_t)i * rows + row] = v;
            acc[i] = 0.0;
        }
    }
}

// ------------------------------------------------------------------ EM pass, stage 1: per-row sums
template <int K, int ORDER>
__global__ void __launch_bounds__(64 * kTisWaves)
tissue_em_rows_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, int D, int H, int W, TisParams p,
                      double* __restrict__ part) {
    tis_walk<2 + 3 * K + (2 * ORDER + 1) + (ORDER + 1), TisIdle::skipped>(
        x, mask, D, H, W, p, part, [&](double* acc, const double* q, const TisAt& at, float xv, bool sel) {
            if (!sel) return;
            const double y = log((double)xv);
            double zh, l[K];
            const double r = y - tis_field(p, q, at.w, zh);
#pragma unroll
            for (int k = 0; k < K; ++k) l[k] = tis_log_term(p, k, r);
            acc[1] = acc[1] + tis_voxel_sums<K, ORDER>(p, l, y, r, zh, acc);
        });
}

// ------------------------------------------------------------------ MRF pass, stage 1: per-row sums and the labels
// The EM row kernel with a Potts prior on a label volume: l_k gains beta n_k, n_k the face neighbours inside the volume whose
// byte of `lin` is k + 1, and LL becomes the pseudo-log-likelihood (logsumexp_k l_k - log sum_k pi_k e^{beta n_k}); e^{beta n} for
// n = 0..6 comes from the host.  Every voxel reads `lin` only and writes its own byte of `lout`, a 0 where it is not selected (a
// wave step of background included): two buffers, no atomics, the same bits whatever the launch order.
struct TisMrf {
    double pi[kTisMaxK];
    double beta;
    double e[7];     // exp(beta n)
    int mode;        // 0, 1: that colour of (d + h + w) & 1 takes its new label, the other keeps lin's; 2: no neighbours, lin unread
};

template <int K, int ORDER>
__global__ void __launch_bounds__(64 * kTisWaves)
tissue_mrf_rows_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, int D, int H, int W, TisParams p, TisMrf m,
                       const uint8_t* __restrict__ lin, uint8_t* __restrict__ lout, double* __restrict__ part) {
    const bool prior = m.mode != 2;
    const size_t plane = (size_t)H * W;
    tis_walk<2 + 3 * K + (2 * ORDER + 1) + (ORDER + 1), TisIdle::unselected>(
        x, mask, D, H, W, p, part, [&](double* acc, const double* q, const TisAt& at, float xv, bool sel) {
            int lab = 0;
            if (sel) {
                const double y = log((double)xv);
                double zh;
                const double r = y - tis_field(p, q, at.w, zh);
                int own = 0, nb[6] = {0, 0, 0, 0, 0, 0};
                if (prior) {
                    const uint8_t* l0 = lin + at.row0;   // the row itself; the four rows around it where there is one
                    own = l0[at.w];
                    if (at.d > 0) nb[0] = (l0 - plane)[at.w];
                    if (at.d < D - 1) nb[1] = (l0 + plane)[at.w];
                    if (at.h > 0) nb[2] = (l0 - W)[at.w];
                    if (at.h < H - 1) nb[3] = (l0 + W)[at.w];
                    if (at.w > 0) nb[4] = l0[at.w - 1];
                    if (at.w < W - 1) nb[5] = l0[at.w + 1];
                }
                double l[K], z = 0.0, best = -(double)INFINITY;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    int n = 0;
#pragma unroll
                    for (int j = 0; j < 6; ++j) n += nb[j] == k + 1;
                    double en = m.e[0];
#pragma unroll
                    for (int j = 1; j <= 6; ++j) en = n == j ? m.e[j] : en;
                    l[k] = tis_log_term(p, k, r) + m.beta * (double)n;
                    z = z + m.pi[k] * en;
                    tis_argmax(k, l[k], best, lab);
                }
                if (prior && ((at.d + at.h + at.w) & 1) != m.mode) lab = own;
                acc[1] = acc[1] + (tis_voxel_sums<K, ORDER>(p, l, y, r, zh, acc) - log(z));
            }
            (lout + at.row0)[at.w] = (uint8_t)lab;
        });
}

// ------------------------------------------------------------------ EM pass, stage 2: rows -> table
__global__ void __launch_bounds__(kTisFoldThreads)
tissue_em_fold_kernel(const double* __restrict__ part, int D, int H, TisFold f, double d0, double step_d, double h0, double step_h,
                      double* __restrict__ sums) {
    __shared__ double sh[kTisFoldThreads];
    const int e = blockIdx.x, t = threadIdx.x;
    const int rows = D * H;
    const int a = f.a[e], b = f.b[e];
    const double* src = part + (size_t)f.slot[e] * rows;
    double acc = 0.0;
    for (int row = t; row < rows; row += kTisFoldThreads) {
        const int d = row / H, h = row - d * H;
        const double xh = d0 + (double)d * step_d, yh = h0 + (double)h * step_h;
        double wgt = 1.0;
        for (int i = 0; i < a; ++i) wgt = wgt * xh;
        for (int j = 0; j < b; ++j) wgt = wgt * yh;
        acc = acc + src[row] * wgt;
    }
    sh[t] = acc;
    __syncthreads();
    for (int s = kTisFoldThreads / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    if (t == 0) sums[e] = sh[0];
}

// ------------------------------------------------------------------ final pass
// x and restored may be the same buffer (a voxel is read and written by one lane): no __restrict__ on the two
template <int K>
__global__ void __launch_bounds__(64 * kTisWaves)
tissue_apply_kernel(const float* x, const uint8_t* __restrict__ mask, int D, int H, int W, TisParams p, float* restored,
                    uint8_t* __restrict__ labels, float* __restrict__ field) {
    tis_walk<0, TisIdle::unknown>(x, mask, D, H, W, p, nullptr, [&](double*, const double* q, const TisAt& at, float xv, bool sel) {
        double zh;
        const double b = tis_field(p, q, at.w, zh);
        int lab = 0;
        if (sel) {
            const double r = log((double)xv) - b;
            double best = -(double)INFINITY;
#pragma unroll
            for (int k = 0; k < K; ++k) tis_argmax(k, tis_log_term(p, k, r), best, lab);
        }
        (restored + at.row0)[at.w] = (float)((double)xv * exp(-b));
        (labels + at.row0)[at.w] = (uint8_t)lab;
        if (field) (field + at.row0)[at.w] = (float)exp(b);
    });
}

static int tis_ncoef(int order) { return (order + 1) * (order + 2) * (order + 3) / 6; }
static int tis_row_sums(int classes, int order) { return 2 + 3 * classes + (2 * order + 1) + (order + 1); }
static int tis_entries(int classes, int order) { return 2 + 3 * classes + tis_ncoef(2 * order) + tis_ncoef(order); }
static int tis_blocks(int64_t rows) { return (int)std::min<int64_t>(cdiv64(rows, kTisWaves), kTisMaxBlocks); }

// the checks every entry shares; `who` starts the error string
static int tis_check_dims(const char* who, int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order) {
    MRI3D_REQUIRE(d > 0 && h > 0 && w > 0, MRI3D_EINVAL, "%s: extents %d,%d,%d", who, d, h, w);
    MRI3D_REQUIRE((int64_t)d * h * w < 0x7fffffffLL, MRI3D_ENOTSUP, "%s: volume too large", who);
    MRI3D_REQUIRE(classes >= 2 && classes <= kTisMaxK, MRI3D_EINVAL, "%s: classes = %d outside 2..%d", who, classes, kTisMaxK);
    MRI3D_REQUIRE(order >= 0, MRI3D_EINVAL, "%s: negative order %d", who, order);
    MRI3D_REQUIRE(order <= 3, MRI3D_ENOTSUP, "%s: order %d (at most 3)", who, order);
    return MRI3D_OK;
}

// params_host = (pi[K], mu[K], v[K], c[M]) -> the kernels' constants.  Classes go to the kernel in ascending order of mu when
// `sort` is set (a stable order: equal means keep the caller's).
static int tis_params(const char* who, const double* ph, int K, int order, int d, int h, int w, bool with_2pi, bool sort, TisParams& p) {
    const int M = tis_ncoef(order);
    bool any_pi = false;
    for (int k = 0; k < K; ++k) {
        const double pi = ph[k], mu = ph[K + k], v = ph[2 * K + k];
        MRI3D_REQUIRE(isfinite(pi) && pi >= 0.0, MRI3D_EINVAL, "%s: pi[%d] = %g must be finite and >= 0", who, k, pi);
        MRI3D_REQUIRE(isfinite(mu), MRI3D_EINVAL, "%s: mu[%d] = %g must be finite", who, k, mu);
        MRI3D_REQUIRE(isfinite(v) && v > 0.0, MRI3D_EINVAL, "%s: v[%d] = %g must be finite and > 0", who, k, v);
        any_pi = any_pi || pi > 0.0;
    }
    MRI3D_REQUIRE(any_pi, MRI3D_EINVAL, "%s: every pi is 0", who);
    for (int n = 0; n < M; ++n) MRI3D_REQUIRE(isfinite(ph[3 * K + n]), MRI3D_EINVAL, "%s: c[%d] = %g must be finite", who, n, ph[3 * K + n]);
    int idx[kTisMaxK];
    for (int k = 0; k < K; ++k) idx[k] = k;
    if (sort) std::stable_sort(idx, idx + K, [&](int i, int j) { return ph[K + i] < ph[K + j]; });
    for (int k = 0; k < kTisMaxK; ++k) {
        const int s = idx[std::min(k, K - 1)];
        const double pi = ph[s], mu = ph[K + s], v = ph[2 * K + s];
        p.a[k] = (log(pi) - 0.5 * log(v)) - (with_2pi ? 0.5 * log(2.0 * M_PI) : 0.0);
        p.mu[k] = mu, p.inv_v[k] = 1.0 / v, p.hiv[k] = 1.0 / (2.0 * v);
    }
    // where term n of the caller's nesting (i, j, k up to `order`) sits in the kernel's order-3 nesting
    for (int n = 0; n < kTisCoef; ++n) p.c[n] = 0.0;
    int n = 0, n3 = 0;
    for (int i = 0; i <= 3; ++i)
        for (int j = 0; j <= 3 - i; ++j)
            for (int k = 0; k <= 3 - i - j; ++k, ++n3)
                if (i + j + k <= order) p.c[n3] = ph[3 * K + n++];
    auto step = [](int len) { return len > 1 ? 2.0 / (double)(len - 1) : 0.0; };
    auto start = [](int len) { return len > 1 ? -1.0 : 0.0; };
    p.d0 = start(d), p.h0 = start(h), p.w0 = start(w), p.step_d = step(d), p.step_h = step(h), p.step_w = step(w);
    return MRI3D_OK;
}

// the table: n, LL, S0[K], S1[K], S2[K], Mw[a][b][c] (a + b + c <= 2 order, c fastest), Mt[a][b][c] (a + b + c <= order)
static void tis_fold_table(int K, int order, TisFold& f) {
    const int nw = 2 * order + 1;
    int e = 0;
    for (; e < 2 + 3 * K; ++e) f.slot[e] = (uint8_t)e, f.a[e] = 0, f.b[e] = 0;
    for (int a = 0; a <= 2 * order; ++a)
        for (int b = 0; b <= 2 * order - a; ++b)
            for (int c = 0; c <= 2 * order - a - b; ++c, ++e) f.slot[e] = (uint8_t)(2 + 3 * K + c), f.a[e] = (uint8_t)a, f.b[e] = (uint8_t)b;
    for (int a = 0; a <= order; ++a)
        for (int b = 0; b <= order - a; ++b)
            for (int c = 0; c <= order - a - b; ++c, ++e) f.slot[e] = (uint8_t)(2 + 3 * K + nw + c), f.a[e] = (uint8_t)a, f.b[e] = (uint8_t)b;
    for (int i = e; i < kTisMaxEntries; ++i) f.slot[i] = 0, f.a[i] = 0, f.b[i] = 0;
}

// f(K) and f(K, ORDER) with (classes, order), both already checked, as compile-time constants: the kernels' instances
template <int N> using TisInt = std::integral_constant<int, N>;

template <class F>
static void tis_for_classes(int classes, F&& f) {
    switch (classes) {
        case 2: f(TisInt<2>{}); break;
        case 3: f(TisInt<3>{}); break;
        default: f(TisInt<4>{}); break;
    }
}

template <class F>
static void tis_for_instance(int classes, int order, F&& f) {
    tis_for_classes(classes, [&](auto k) {
        switch (order) {
            case 0: f(k, TisInt<0>{}); break;
            case 1: f(k, TisInt<1>{}); break;
            case 2: f(k, TisInt<2>{}); break;
            default: f(k, TisInt<3>{}); break;
        }
    });
}

// Whether a buffer that a call writes shares a byte with another buffer of the list; two that are only read may overlap, and a
// null pointer overlaps nothing.
struct TisBuf { const void* p; size_t bytes; bool written; };

static bool tis_clash(std::initializer_list<TisBuf> bufs) {
    for (const TisBuf* a = bufs.begin(); a != bufs.end(); ++a)
        for (const TisBuf* b = a + 1; b != bufs.end(); ++b)
            if ((a->written || b->written) && overlaps(a->p, a->bytes, b->p, b->bytes)) return true;
    return false;
}

}  // namespace mri3d

using namespace mri3d;

extern "C" size_t mri3d_tissue_em_workspace_bytes(int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order) {
    if (tis_check_dims("tissue_em_workspace_bytes", d, h, w, classes, order)) return 0;   // the query's 0 comes with the reason as the error string
    return (size_t)tis_row_sums(classes, order) * (size_t)d * (size_t)h * sizeof(double);
}

extern "C" int mri3d_tissue_em_plan(int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order, int32_t out[8]) {
    MRI3D_REQUIRE(out != nullptr, MRI3D_EINVAL, "tissue_em_plan: null output");
    if (int rc = tis_check_dims("tissue_em_plan", d, h, w, classes, order)) return rc;
    const int64_t rows = (int64_t)d * h;
    const int blocks = tis_blocks(rows);
    out[0] = blocks;
    out[1] = kTisWaves;
    out[2] = (int32_t)cdiv64(cdiv64(rows, kTisWaves), blocks);
    out[3] = cdiv(w, 64);
    out[4] = tis_row_sums(classes, order);
    out[5] = tis_entries(classes, order);
    out[6] = kTisFoldThreads;
    out[7] = (int32_t)rows;
    return MRI3D_OK;
}

// What the two passes share, in the order the checks are made: pointers, extents, parameters -> the kernels' constants, alignment,
// the workspace, the buffers the pass writes against the ones it reads, and the fold table.  `who` starts the error string.
struct TisPass {
    TisParams p;
    TisFold f;
    size_t need, sums_bytes, nvox;
    int entries;
};

static int tis_pass_setup(const char* who, const float* x, const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order,
                          const double* params_host, double* sums, void* workspace, size_t ws_bytes, TisPass& t) {
    MRI3D_REQUIRE(x && params_host && sums, MRI3D_EINVAL, "%s: null pointer (x %p, params %p, sums %p)", who, (const void*)x,
                  (const void*)params_host, (void*)sums);
    if (int rc = tis_check_dims(who, d, h, w, classes, order)) return rc;
    if (int rc = tis_params(who, params_host, classes, order, d, h, w, true, false, t.p)) return rc;
    MRI3D_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0, MRI3D_EINVAL,
                  "%s: a pointer is not aligned to its element", who);
    t.need = mri3d_tissue_em_workspace_bytes(d, h, w, classes, order);
    if (int rc = ws_check8(who, workspace, ws_bytes, t.need)) return rc;
    t.nvox = (size_t)d * h * w;
    t.entries = tis_entries(classes, order);
    t.sums_bytes = (size_t)t.entries * sizeof(double);
    MRI3D_REQUIRE(!tis_clash({{sums, t.sums_bytes, true}, {workspace, t.need, true}, {x, t.nvox * 4, false}, {mask, t.nvox, false}}), MRI3D_EINVAL,
                  "%s: the sums or the workspace overlap another buffer", who);
    tis_fold_table(classes, order, t.f);
    return MRI3D_OK;
}

// The launches of a pass that tis_pass_setup accepted: the row kernel instance that pick(K, ORDER) returns, on the arguments every
// row kernel starts with, then `extra`, then the workspace; and the fold.
template <class Pick, class... Extra>
static int tis_pass_launch(const char* who, const TisPass& t, const float* x, const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t classes,
                           int32_t order, double* sums, void* workspace, mri3d_stream_t stream, Pick&& pick, Extra... extra) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    const dim3 grid(tis_blocks((int64_t)d * h)), block(64 * kTisWaves);
    tis_for_instance(classes, order, [&](auto k, auto o) { hipLaunchKernelGGL(pick(k, o), grid, block, 0, st, x, mask, d, h, w, t.p, extra..., part); });
    hipLaunchKernelGGL(tissue_em_fold_kernel, dim3(t.entries), dim3(kTisFoldThreads), 0, st, part, d, h, t.f, t.p.d0, t.p.step_d, t.p.h0, t.p.step_h,
                       sums);
    return check_launch(who);
}

extern "C" int mri3d_tissue_em_pass(const float* x, const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order,
                                    const double* params_host, double* sums, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    TisPass t;
    if (int rc = tis_pass_setup("tissue_em_pass", x, mask, d, h, w, classes, order, params_host, sums, workspace, ws_bytes, t)) return rc;
    return tis_pass_launch("tissue_em_pass", t, x, mask, d, h, w, classes, order, sums, workspace, stream,
                           [](auto k, auto o) { return tissue_em_rows_kernel<decltype(k)::value, decltype(o)::value>; });
}

extern "C" int mri3d_tissue_mrf_pass(const float* x, const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order,
                                     const double* params_host, double beta, int32_t mode, const uint8_t* labels_in, uint8_t* labels_out,
                                     double* sums, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(labels_out, MRI3D_EINVAL, "tissue_mrf_pass: null pointer (labels_out)");
    TisPass t;
    if (int rc = tis_pass_setup("tissue_mrf_pass", x, mask, d, h, w, classes, order, params_host, sums, workspace, ws_bytes, t)) return rc;
    MRI3D_REQUIRE(isfinite(beta) && beta >= 0.0 && beta <= kTisMaxBeta, MRI3D_EINVAL, "tissue_mrf_pass: beta = %g must be finite and in 0..%g", beta,
                  kTisMaxBeta);
    MRI3D_REQUIRE(mode >= 0 && mode <= 2, MRI3D_EINVAL, "tissue_mrf_pass: mode = %d outside 0..2", mode);
    MRI3D_REQUIRE(labels_in || mode == 2, MRI3D_EINVAL, "tissue_mrf_pass: labels_in is null in mode %d (only the start pass, mode 2, reads none)", mode);
    // two label buffers: a pass in place would let the table depend on the launch order
    MRI3D_REQUIRE(!overlaps(labels_out, t.nvox, labels_in, t.nvox), MRI3D_EINVAL,
                  "tissue_mrf_pass: labels_in and labels_out overlap (a pass reads one buffer and writes another)");
    // the sums and the workspace count as written here too: labels_in may lie on x or the mask, not on them
    MRI3D_REQUIRE(!tis_clash({{labels_out, t.nvox, true}, {labels_in, t.nvox, false}, {x, t.nvox * 4, false}, {mask, t.nvox, false},
                              {sums, t.sums_bytes, true}, {workspace, t.need, true}}),
                  MRI3D_EINVAL, "tissue_mrf_pass: a label buffer overlaps x, the mask, the sums or the workspace");
    TisMrf m;
    for (int k = 0; k < kTisMaxK; ++k) m.pi[k] = params_host[std::min(k, classes - 1)];
    m.beta = beta, m.mode = mode;
    for (int n = 0; n <= 6; ++n) m.e[n] = exp(beta * (double)n);
    return tis_pass_launch("tissue_mrf_pass", t, x, mask, d, h, w, classes, order, sums, workspace, stream,
                           [](auto k, auto o) { return tissue_mrf_rows_kernel<decltype(k)::value, decltype(o)::value>; }, m, labels_in, labels_out);
}

extern "C" int mri3d_tissue_apply(const float* x, const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order,
                                  const double* params_host, float* restored, uint8_t* labels, float* field, mri3d_stream_t stream) {
    MRI3D_REQUIRE(x && params_host && restored && labels, MRI3D_EINVAL, "tissue_apply: null pointer (x %p, params %p, restored %p, labels %p)",
                  (const void*)x, (const void*)params_host, (void*)restored, (void*)labels);
    if (int rc = tis_check_dims("tissue_apply", d, h, w, classes, order)) return rc;
    TisParams p;
    if (int rc = tis_params("tissue_apply", params_host, classes, order, d, h, w, false, true, p)) return rc;
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(restored) | reinterpret_cast<uintptr_t>(field)) & 3) == 0,
                  MRI3D_EINVAL, "tissue_apply: pointers not aligned to float");
    const size_t nvox = (size_t)d * h * w;
    // in place (restored == x) is allowed, and x then is restored's entry of the list; any other overlap is not
    MRI3D_REQUIRE(!tis_clash({{x == restored ? nullptr : x, nvox * 4, false}, {mask, nvox, false}, {restored, nvox * 4, true}, {labels, nvox, true},
                              {field, nvox * 4, true}}),
                  MRI3D_EINVAL, "tissue_apply: an output overlaps another buffer (only restored == x is allowed)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(tis_blocks((int64_t)d * h)), block(64 * kTisWaves);
    tis_for_classes(classes, [&](auto k) {
        hipLaunchKernelGGL((tissue_apply_kernel<decltype(k)::value>), grid, block, 0, st, x, mask, d, h, w, p, restored, labels, field);
    });
    return check_launch("tissue_apply");
}
