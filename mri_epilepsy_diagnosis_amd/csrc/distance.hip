// distance.hip — the exact squared Euclidean distance transform of a batch of uint8 volumes, what is thresholded or signed from
// it in the same pass, and the boundary loss (Kervadec et al., MIDL 2019) that reads the signed map.
//
//   sq[v] = min over the zero voxels z of the same volume of |v - z|^2        (int32, voxels; MRI3D_EDT_INF when there is none)
// "inside" (not zero) is in != 0, or in == value for a class map; with outside_zero the volume stands in a sea of zeros.
//
// Three separable min-plus passes over squared integer distances, along w, h and d:  out[x] = min_q in[q] + (x - q)^2.  Each is
// exact in integers (every partial value stays below 2^31: d^2 + h^2 + w^2 < MRI3D_EDT_INF is required), so the result is scipy's
// distance_transform_edt squared, bit for bit.  What differs from the brute-force passes of surface.hip:
//   * a voxel searches outwards from its own position, r = 1, 2, ..., and stops once r^2 >= best: no candidate further out can
//     win.  Near a zero that is a handful of steps.
//   * a line that holds no finite value, or holds them in a short stretch [lo, hi] (a small lesion in a large volume), is not
//     walked: one lane per line finds [lo, hi] from both ends, and a search only visits positions inside it.  A saturated volume
//     costs one look per line, not a scan per voxel.
//   * a workgroup stages its lines in LDS first: `rows` whole rows of the w pass (a contiguous stretch of memory), or a tile of
//     len x tx values of the h and d passes, tx neighbouring lines wide, read as rows of tx consecutive ints: every global
//     access of the strided passes is a 4 * tx byte run.  A line longer than the tile (kEdtTile ints) is not staged: its lanes
//     do the same work on global memory directly — slow and correct, for shapes nobody scans.
// The last pass writes the int32 map, or a uint8 threshold of it (ball morphology: the int32 volume never reaches HBM), or the
// signed map of a class.  No atomics, integers only: the same bits every run.
//
// Boundary loss: L = (1 / cnt) sum over (n, k, v) with s != INT32_MIN of softmax(z)[n, c_k, v] * phi(s[n, k, v]),
//   phi(s) = sqrt(s) for s > 0, -(sqrt(-s) - 1) for s < 0, 0 for s = 0;  dL/dz_j = g / cnt * p_j (phi_j [j in ids] - sum_k p_ck phi_k).
// One streaming pass each way over loss_index.h's row reads and row store (class buckets, scalar or 4-element accesses), launched
// by its idx_plan with no label bytes, so without a 4-voxel path.  The two row loops stand here: they index a map by voxel where
// the class-map walk hands its body a label.  Float products, double sums per lane, block partials folded in a fixed order by the
// pair-sum helpers that the cross-entropy uses too.
#include "loss_index.h"
#include <limits.h>

namespace mri3d {

constexpr int kEdtInf = MRI3D_EDT_INF;
constexpr int kEdtTile = 8192;        // ints of LDS a workgroup stages its lines in (32 KiB)
constexpr int kEdtMaxRows = 256;      // rows of a w-pass tile: one lane finds the bounds of one row
constexpr int kEdtMaxTx = 32;         // lines of an h / d tile: 128-byte runs
constexpr int kEdtUnstagedTx = 64;    // lines a workgroup takes when the line is too long to stage
constexpr int kEdtMaskBlocks = 64;    // partial class masks per volume (signed map)

enum { kEdtTailSq = 0, kEdtTailLe = 1, kEdtTailGt = 2, kEdtTailSigned = 3 };

// what the last pass does with a finished squared distance
struct EdtTail {
    int mode, r2, cls, classes, nparts;
    int64_t nstride;                  // elements between the outputs of two consecutive `outer` slices
    int64_t vol;                      // voxels of a volume (signed map: where the labels of slice o start)
    const uint8_t* labels;            // signed map: the class map
    const unsigned* masks;            // signed map: [n][nparts] bit c set = class c occurs among the counted voxels
};

__device__ __forceinline__ int edt_f0(unsigned b, int val, int ne) { return (ne ? (int)b != val : (int)b == val) ? kEdtInf : 0; }

struct LdsLine {
    const int* p; int st;
    __device__ __forceinline__ int operator()(int q) const { return p[q * st]; }
};
struct GlobalLine {
    const int* p; int64_t st;
    __device__ __forceinline__ int operator()(int q) const { return p[(int64_t)q * st]; }
};
struct ByteLine {
    const uint8_t* p; int val, ne;
    __device__ __forceinline__ int operator()(int q) const { return edt_f0(p[q], val, ne); }
};

// [lo, hi]: the stretch outside which every value of the line is kEdtInf (lo > hi: the whole line)
template <typename F> __device__ __forceinline__ void edt_bounds(const F& f, int len, int& lo, int& hi) {
    int a = 0;
    while (a < len && f(a) >= kEdtInf) ++a;
    int b = -1;
    if (a < len) {
        b = len - 1;
        while (f(b) >= kEdtInf) --b;
    }
    lo = a, hi = b;
}

// min_q f(q) + (x - q)^2 over the line, the zeros outside it included when oz.  len < 32768 and f <= kEdtInf: no overflow.
template <typename F> __device__ __forceinline__ int edt_point(const F& f, int x, int len, int lo, int hi, int oz) {
    int best = f(x);
    if (oz) {
        const int a = x + 1, b = len - x;
        best = min(best, min(a * a, b * b));
    }
    if (lo <= hi) {
        for (int r = x < lo ? lo - x : x > hi ? x - hi : 1; r * r < best; ++r) {
            const int a = x - r, b = x + r;
            if (a < lo && b > hi) break;
            if (a >= lo) best = min(best, f(a) + r * r);
            if (b <= hi) best = min(best, f(b) + r * r);
        }
    }
    return best;
}

// pass along w: `rows` rows of `len` bytes in all; a workgroup takes R consecutive rows
__global__ void __launch_bounds__(256)
edt_w_kernel(const uint8_t* __restrict__ in, int* __restrict__ out, int64_t rows, int len, int R, int staged, int val, int ne,
             int oz) {
    __shared__ int tile[kEdtTile];
    __shared__ int slo[kEdtMaxRows], shi[kEdtMaxRows];
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int nr = rows - row0 < R ? (int)(rows - row0) : R;
    const uint8_t* src = in + row0 * len;
    int* dst = out + row0 * len;
    if (staged) {
        const int ls = len | 1;                       // odd row pitch: the lanes that walk one row each hit different banks
        const int items = nr * len;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int l = i / len, q = i - l * len;
            tile[l * ls + q] = edt_f0(src[i], val, ne);
        }
        __syncthreads();
        if ((int)threadIdx.x < nr) edt_bounds(LdsLine{tile + threadIdx.x * ls, 1}, len, slo[threadIdx.x], shi[threadIdx.x]);
        __syncthreads();
        for (int i = threadIdx.x; i < items; i += 256) {
            const int l = i / len, q = i - l * len;
            dst[i] = edt_point(LdsLine{tile + l * ls, 1}, q, len, slo[l], shi[l], oz);
        }
    } else {                                          // R == 1: the row is read where it lies
        if (threadIdx.x == 0) edt_bounds(ByteLine{src, val, ne}, len, slo[0], shi[0]);
        __syncthreads();
        for (int q = threadIdx.x; q < len; q += 256) dst[q] = edt_point(ByteLine{src, val, ne}, q, len, slo[0], shi[0], oz);
    }
}

__device__ __forceinline__ void edt_store(void* __restrict__ out, const EdtTail& t, int64_t o, int64_t v, int best, bool flat) {
    const int64_t idx = o * t.nstride + v;
    if (t.mode == kEdtTailSq) {
        static_cast<int*>(out)[idx] = best;
    } else if (t.mode == kEdtTailLe) {
        static_cast<uint8_t*>(out)[idx] = best <= t.r2 ? 1 : 0;
    } else if (t.mode == kEdtTailGt) {
        static_cast<uint8_t*>(out)[idx] = best > t.r2 ? 1 : 0;
    } else {
        // out holds the distance to the class already; `best` is the distance to what is not the class
        const int lab = t.labels[o * t.vol + v];
        int* p = static_cast<int*>(out) + idx;
        const int to_class = *p;
        int s = lab == t.cls ? -best : to_class;
        if (flat) s = 0;
        if (lab >= t.classes) s = INT_MIN;           // a label that is no class: the voxel is ignored
        *p = s;
    }
}

// pass along an axis of the (outer, len, inner) view: a workgroup takes all `len` values of `tx` neighbouring lines
__global__ void __launch_bounds__(256)
edt_axis_kernel(const int* __restrict__ in, void* __restrict__ out, int len, int64_t inner, int tx, int tiles, int staged, int oz,
                EdtTail tail) {
    __shared__ int tile[kEdtTile];
    __shared__ int slo[kEdtUnstagedTx], shi[kEdtUnstagedTx];
    __shared__ unsigned smask;
    const int64_t o = blockIdx.x / tiles;
    const int64_t col0 = (int64_t)(blockIdx.x % tiles) * tx;
    const int nc = inner - col0 < tx ? (int)(inner - col0) : tx;
    const int* src = in + o * len * inner + col0;     // value q of line l: src[q * inner + l]
    if (tail.mode == kEdtTailSigned && threadIdx.x == 0) {
        unsigned m = 0;
        for (int j = 0; j < tail.nparts; ++j) m |= tail.masks[o * tail.nparts + j];
        smask = m;
    }
    const int tw = staged ? tx : nc;                  // lanes walk (q, l) with l < tw; staged: the tile's own layout
    const int items = len * tw;
    if (staged) {
        for (int i = threadIdx.x; i < items; i += 256) {
            const int q = i / tx, l = i - q * tx;
            if (l < nc) tile[i] = src[(int64_t)q * inner + l];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nc) {
        if (staged) edt_bounds(LdsLine{tile + threadIdx.x, tx}, len, slo[threadIdx.x], shi[threadIdx.x]);
        else edt_bounds(GlobalLine{src + threadIdx.x, inner}, len, slo[threadIdx.x], shi[threadIdx.x]);
    }
    __syncthreads();
    bool flat = false;
    if (tail.mode == kEdtTailSigned) {
        const unsigned m = smask, bit = 1u << tail.cls;
        flat = (m & bit) == 0 || (m & ~bit) == 0;     // the class is absent, or nothing else is counted: no boundary
    }
    for (int i = threadIdx.x; i < items; i += 256) {
        const int q = i / tw, l = i - q * tw;
        if (l >= nc) continue;
        const int best = staged ? edt_point(LdsLine{tile + l, tx}, q, len, slo[l], shi[l], oz)
                                : edt_point(GlobalLine{src + l, inner}, q, len, slo[l], shi[l], oz);
        edt_store(out, tail, o, (int64_t)q * inner + col0 + l, best, flat);
    }
}

// masks[n][blockIdx.x]: bit c set when label c < classes occurs in the block's share of volume n
__global__ void __launch_bounds__(256)
edt_class_mask_kernel(const uint8_t* __restrict__ labels, unsigned* __restrict__ masks, int64_t vol, int classes) {
    __shared__ unsigned red[4];
    const uint8_t* ln = labels + (int64_t)blockIdx.y * vol;
    unsigned m = 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < vol; v += (int64_t)gridDim.x * 256) {
        const unsigned lab = ln[v];
        m |= lab < (unsigned)classes ? 1u << lab : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m |= __shfl_xor(m, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) masks[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0] | red[1] | red[2] | red[3];
}

// ------------------------------------------------------------------ boundary loss
__device__ __forceinline__ float bd_phi(int s) {
    if (s > 0) return sqrtf((float)s);
    if (s < 0) return -(sqrtf(-(float)s) - 1.f);
    return 0.f;
}

// slot[j]: which plane of the map belongs to class j, or -1
struct BdSlots { int8_t slot[kIdxMaxC]; };

// e = exp(z - max) in place, their sum in s; phi[j] of the planes (0 where the class has none or the term is left out); returns
// the number of terms that count
template <int CB>
__device__ __forceinline__ int bd_voxel(float (&z)[CB], float (&phi)[CB], float& s, const int* __restrict__ mapv, int64_t vox,
                                        const int8_t* slot) {
    float m = z[0];
#pragma unroll
    for (int j = 1; j < CB; ++j) m = fmaxf(m, z[j]);
    s = 0.f;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < CB; ++j) {
        z[j] = expf(z[j] - m);
        s += z[j];
        phi[j] = 0.f;
        const int k = slot[j];
        if (k >= 0) {
            const int sv = mapv[(int64_t)k * vox];
            if (sv != INT_MIN) { phi[j] = bd_phi(sv); ++cnt; }
        }
    }
    return cnt;
}

// part[(n * gridDim.x + blockIdx.x) * 2] = the block's (sum p phi, number of terms)
template <typename T, int CB>
__global__ void __launch_bounds__(256)
boundary_fwd_kernel(const T* __restrict__ logits, const int* __restrict__ map, double* __restrict__ part, int64_t vox, int C, int K,
                    int x_ld, int mode, BdSlots slots) {
    __shared__ int8_t sslot[kIdxMaxC];
    if (threadIdx.x < kIdxMaxC) sslot[threadIdx.x] = (int)threadIdx.x < CB ? slots.slot[threadIdx.x] : (int8_t)-1;
    __syncthreads();
    const int n = blockIdx.y;
    const int* mn = map + (int64_t)n * K * vox;
    double sum = 0.0;
    unsigned cnt = 0;
    const T* zn = logits + (int64_t)n * vox * x_ld;
#pragma unroll 1
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < vox; v += (int64_t)gridDim.x * 256) {
        float z[CB], phi[CB], s;
        idx_load_row<T, CB>(zn + v * x_ld, C, mode, z);
        cnt += (unsigned)bd_voxel<CB>(z, phi, s, mn + v, vox, sslot);
        float num = 0.f;
#pragma unroll
        for (int j = 0; j < CB; ++j) num = fmaf(z[j], phi[j], num);
        sum += (double)(num / s);
    }
    sum = wave_sum_d(sum);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    pair_block_row(sum, (double)cnt, n, part);
}

// stats = {loss, 1 / cnt (0 when nothing counts), cnt, sum}
__global__ void __launch_bounds__(256)
boundary_finalize_kernel(const double* __restrict__ part, int rows, float* __restrict__ stats, float* __restrict__ loss) {
    double num, den;
    pair_finalize_sum(part, rows, num, den);
    if (threadIdx.x == 0) {
        const float l = den > 0.0 ? (float)(num / den) : 0.f;
        stats[0] = l;
        stats[1] = den > 0.0 ? (float)(1.0 / den) : 0.f;
        stats[2] = (float)den;
        stats[3] = (float)num;
        loss[0] = l;
    }
}

template <typename T, int CB>
__global__ void __launch_bounds__(256)
boundary_bwd_kernel(const T* __restrict__ logits, const int* __restrict__ map, const float* __restrict__ stats,
                    const float* __restrict__ dloss, T* __restrict__ dlogits, int64_t vox, int C, int K, int x_ld, int dx_ld, int mode,
                    BdSlots slots) {
    __shared__ int8_t sslot[kIdxMaxC];
    if (threadIdx.x < kIdxMaxC) sslot[threadIdx.x] = (int)threadIdx.x < CB ? slots.slot[threadIdx.x] : (int8_t)-1;
    __syncthreads();
    const int n = blockIdx.y;
    const int* mn = map + (int64_t)n * K * vox;
    const float kc = dloss[0] * stats[1];
    const T* zn = logits + (int64_t)n * vox * x_ld;
    T* dn = dlogits + (int64_t)n * vox * dx_ld;
#pragma unroll 1
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < vox; v += (int64_t)gridDim.x * 256) {
        float z[CB], phi[CB], s;
        idx_load_row<T, CB>(zn + v * x_ld, C, mode, z);
        bd_voxel<CB>(z, phi, s, mn + v, vox, sslot);
        const float inv = 1.f / s;
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            z[j] *= inv;
            dot = fmaf(z[j], phi[j], dot);
        }
#pragma unroll
        for (int j = 0; j < CB; ++j) z[j] = kc * z[j] * (phi[j] - dot);
        idx_store_row<T, CB>(dn + v * dx_ld, C, mode, z);       // the gradient has its own pitch
    }
}

// ------------------------------------------------------------------ host
// One decision per transform: the query reports it, the launches go by it.
struct EdtPlan {
    int rows_w, staged_w, partial_w, tx_h, staged_h, partial_h, tx_d, staged_d, partial_d;
    int64_t grid_w, grid_h, grid_d;
};

static int edt_check(const char* who, int n, int d, int h, int w) {
    MRI3D_REQUIRE(n > 0 && d > 0 && h > 0 && w > 0, MRI3D_EINVAL, "%s: empty batch or volume (%d x %d x %d x %d)", who, n, d, h, w);
    MRI3D_REQUIRE((int64_t)d * d + (int64_t)h * h + (int64_t)w * w < (int64_t)kEdtInf, MRI3D_ENOTSUP,
                  "%s: d^2 + h^2 + w^2 must stay below %d", who, kEdtInf);
    MRI3D_REQUIRE((int64_t)d * h * w < ((int64_t)1 << 31), MRI3D_ENOTSUP, "%s: volume of 2^31 voxels or more", who);
    return MRI3D_OK;
}

// lines of an h / d tile: the largest power of two <= kEdtMaxTx whose tile fits, and no wider than there are lines
static void edt_axis_plan(int len, int64_t inner, int64_t outer, int& tx, int& staged, int& partial, int64_t& grid) {
    staged = len <= kEdtTile;
    if (staged) {
        tx = kEdtMaxTx;
        while (tx > 1 && ((int64_t)tx * len > kEdtTile || tx / 2 >= inner)) tx /= 2;
    } else {
        tx = kEdtUnstagedTx;
    }
    partial = (int)(inner % tx);
    grid = outer * cdiv64(inner, tx);
}

static EdtPlan edt_plan(int n, int d, int h, int w) {
    EdtPlan p;
    const int64_t rows = (int64_t)n * d * h;
    p.staged_w = (w | 1) <= kEdtTile;
    p.rows_w = p.staged_w ? (int)std::min<int64_t>(std::min<int64_t>(rows, kEdtMaxRows), kEdtTile / (w | 1)) : 1;
    p.partial_w = (int)(rows % p.rows_w);
    p.grid_w = cdiv64(rows, p.rows_w);
    edt_axis_plan(h, w, (int64_t)n * d, p.tx_h, p.staged_h, p.partial_h, p.grid_h);
    edt_axis_plan(d, (int64_t)h * w, n, p.tx_d, p.staged_d, p.partial_d, p.grid_d);
    return p;
}

static size_t edt_ws_bytes(int n, int d, int h, int w) {
    const size_t vol = (size_t)n * d * h * w;
    return align_up((size_t)n * kEdtMaskBlocks * sizeof(unsigned), 256) + 2 * align_up(vol * sizeof(int), 256);
}

struct EdtBuffers { unsigned* masks; int *fa, *fb; };
static EdtBuffers edt_buffers(void* workspace, int n, int d, int h, int w) {
    EdtBuffers b;
    char* base = static_cast<char*>(workspace);
    b.masks = reinterpret_cast<unsigned*>(base);
    base += align_up((size_t)n * kEdtMaskBlocks * sizeof(unsigned), 256);
    b.fa = reinterpret_cast<int*>(base);
    b.fb = reinterpret_cast<int*>(base + align_up((size_t)n * d * h * w * sizeof(int), 256));
    return b;
}

// the three passes of one transform; inside = ne ? in != val : in == val
static int edt_run(const char* who, const uint8_t* in, int n, int d, int h, int w, int val, int ne, int oz, void* out, EdtTail tail,
                   const EdtBuffers& b, hipStream_t s) {
    const EdtPlan p = edt_plan(n, d, h, w);
    MRI3D_REQUIRE(p.grid_w < 0x7fffffffLL && p.grid_h < 0x7fffffffLL && p.grid_d < 0x7fffffffLL, MRI3D_ENOTSUP, "%s: grid too large", who);
    hipLaunchKernelGGL(edt_w_kernel, dim3((unsigned)p.grid_w), dim3(256), 0, s, in, b.fa, (int64_t)n * d * h, w, p.rows_w, p.staged_w, val,
                       ne, oz);
    EdtTail mid;
    mid.mode = kEdtTailSq, mid.r2 = 0, mid.cls = 0, mid.classes = 0, mid.nparts = 0, mid.nstride = (int64_t)h * w, mid.vol = 0, mid.labels = nullptr,
    mid.masks = nullptr;
    hipLaunchKernelGGL(edt_axis_kernel, dim3((unsigned)p.grid_h), dim3(256), 0, s, (const int*)b.fa, (void*)b.fb, h, (int64_t)w, p.tx_h,
                       (int)cdiv64(w, p.tx_h), p.staged_h, oz, mid);
    hipLaunchKernelGGL(edt_axis_kernel, dim3((unsigned)p.grid_d), dim3(256), 0, s, (const int*)b.fb, out, d, (int64_t)h * w, p.tx_d,
                       (int)cdiv64((int64_t)h * w, p.tx_d), p.staged_d, oz, tail);
    return check_launch(who);
}

static int edt_common(const char* who, const void* in, int n, int d, int h, int w, int value, const void* out, void* workspace,
                      size_t ws_bytes) {
    int rc = edt_check(who, n, d, h, w);
    if (rc) return rc;
    MRI3D_REQUIRE(value >= -1 && value <= 255, MRI3D_EINVAL, "%s: value must be -1 (non-zero) or a byte, got %d", who, value);
    MRI3D_REQUIRE(in && out, MRI3D_EINVAL, "%s: null pointer", who);
    return ws_check8(who, workspace, ws_bytes, edt_ws_bytes(n, d, h, w));
}

static int bd_check(const Mri3dBoundaryGeom* g, const char* who, BdSlots* slots) {
    int rc = idx_check(g, who, kIdxMaxC, kIdxMaxBlocks);
    if (rc) return rc;
    MRI3D_REQUIRE(g->k >= 1 && g->k <= kIdxMaxC, MRI3D_EINVAL, "%s: 1 to %d class ids, got %d", who, kIdxMaxC, g->k);
    BdSlots sl;
    for (int j = 0; j < kIdxMaxC; ++j) sl.slot[j] = -1;
    for (int k = 0; k < g->k; ++k) {
        const int id = g->ids[k];
        MRI3D_REQUIRE(id >= 0 && id < g->c, MRI3D_EINVAL, "%s: class id %d outside [0, %d)", who, id, g->c);
        MRI3D_REQUIRE(sl.slot[id] < 0, MRI3D_EINVAL, "%s: class id %d given twice", who, id);
        sl.slot[id] = (int8_t)k;
    }
    if (slots) *slots = sl;
    return MRI3D_OK;
}

}  // namespace mri3d

using namespace mri3d;

extern "C" size_t mri3d_edt_workspace_bytes(int32_t n, int32_t d, int32_t h, int32_t w) {
    if (n <= 0 || d <= 0 || h <= 0 || w <= 0 || (int64_t)d * h * w >= ((int64_t)1 << 31)) return 0;
    return edt_ws_bytes(n, d, h, w);
}

extern "C" int mri3d_edt_plan(int32_t n, int32_t d, int32_t h, int32_t w, Mri3dEdtPlanInfo* out) {
    MRI3D_REQUIRE(out != nullptr, MRI3D_EINVAL, "edt_plan: null output");
    int rc = edt_check("edt_plan", n, d, h, w);
    if (rc) return rc;
    const EdtPlan p = edt_plan(n, d, h, w);
    out->rows_w = p.rows_w, out->staged_w = p.staged_w, out->partial_w = p.partial_w;
    out->tx_h = p.tx_h, out->staged_h = p.staged_h, out->partial_h = p.partial_h;
    out->tx_d = p.tx_d, out->staged_d = p.staged_d, out->partial_d = p.partial_d;
    out->batch = n;
    out->grid_w = p.grid_w, out->grid_h = p.grid_h, out->grid_d = p.grid_d;
    out->lds_bytes = (int64_t)(kEdtTile + 2 * kEdtMaxRows) * sizeof(int);
    out->ws_bytes = (int64_t)edt_ws_bytes(n, d, h, w);
    return MRI3D_OK;
}

extern "C" int mri3d_edt_sq_u8(const uint8_t* in, int32_t n, int32_t d, int32_t h, int32_t w, int32_t value, int32_t outside_zero,
                               int32_t* out, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = edt_common("edt_sq_u8", in, n, d, h, w, value, out, workspace, ws_bytes);
    if (rc) return rc;
    EdtTail tail;
    tail.mode = kEdtTailSq, tail.r2 = 0, tail.cls = 0, tail.classes = 0, tail.nparts = 0, tail.nstride = (int64_t)d * h * w, tail.vol = tail.nstride,
    tail.labels = nullptr, tail.masks = nullptr;
    return edt_run("edt_sq_u8", in, n, d, h, w, value < 0 ? 0 : value, value < 0, outside_zero != 0, out, tail,
                   edt_buffers(workspace, n, d, h, w), static_cast<hipStream_t>(stream));
}

extern "C" int mri3d_edt_threshold_u8(const uint8_t* in, int32_t n, int32_t d, int32_t h, int32_t w, int32_t value, int32_t outside_zero,
                                      int32_t r2, int32_t greater, uint8_t* out, void* workspace, size_t ws_bytes,
                                      mri3d_stream_t stream) {
    int rc = edt_common("edt_threshold_u8", in, n, d, h, w, value, out, workspace, ws_bytes);
    if (rc) return rc;
    MRI3D_REQUIRE(r2 >= 0 && r2 < kEdtInf, MRI3D_EINVAL, "edt_threshold_u8: r2 must be in [0, %d), got %d", kEdtInf, r2);
    EdtTail tail;
    tail.mode = greater ? kEdtTailGt : kEdtTailLe, tail.r2 = r2, tail.cls = 0, tail.classes = 0, tail.nparts = 0, tail.nstride = (int64_t)d * h * w,
    tail.vol = tail.nstride, tail.labels = nullptr, tail.masks = nullptr;
    return edt_run("edt_threshold_u8", in, n, d, h, w, value < 0 ? 0 : value, value < 0, outside_zero != 0, out, tail,
                   edt_buffers(workspace, n, d, h, w), static_cast<hipStream_t>(stream));
}

extern "C" int mri3d_signed_sqdist_u8(const uint8_t* labels, int32_t n, int32_t d, int32_t h, int32_t w, int32_t classes,
                                      const int32_t* ids, int32_t k, int32_t* out, void* workspace, size_t ws_bytes,
                                      mri3d_stream_t stream) {
    int rc = edt_check("signed_sqdist_u8", n, d, h, w);
    if (rc) return rc;
    MRI3D_REQUIRE(classes >= kIdxMinC && classes <= kIdxMaxC, MRI3D_ENOTSUP, "signed_sqdist_u8: classes must be in [%d,%d], got %d",
                  kIdxMinC, kIdxMaxC, classes);
    MRI3D_REQUIRE(k >= 1 && k <= kIdxMaxC, MRI3D_EINVAL, "signed_sqdist_u8: 1 to %d class ids, got %d", kIdxMaxC, k);
    MRI3D_REQUIRE(ids != nullptr, MRI3D_EINVAL, "signed_sqdist_u8: null ids");
    for (int i = 0; i < k; ++i)
        MRI3D_REQUIRE(ids[i] >= 0 && ids[i] < classes, MRI3D_EINVAL, "signed_sqdist_u8: class id %d outside [0, %d)", ids[i], classes);
    MRI3D_REQUIRE(labels && out, MRI3D_EINVAL, "signed_sqdist_u8: null pointer");
    rc = ws_check8("signed_sqdist_u8", workspace, ws_bytes, edt_ws_bytes(n, d, h, w));
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EdtBuffers b = edt_buffers(workspace, n, d, h, w);
    const int64_t vol = (int64_t)d * h * w;
    const int nparts = (int)std::max<int64_t>(1, std::min<int64_t>(kEdtMaskBlocks, cdiv64(vol, 256 * 16)));
    hipLaunchKernelGGL(edt_class_mask_kernel, dim3(nparts, n), dim3(256), 0, s, labels, b.masks, vol, classes);
    for (int i = 0; i < k; ++i) {
        EdtTail tail;
        tail.mode = kEdtTailSq, tail.r2 = 0, tail.cls = ids[i], tail.classes = classes, tail.nparts = nparts, tail.nstride = (int64_t)k * vol, tail.vol = vol,
        tail.labels = labels, tail.masks = b.masks;
        int32_t* plane = out + (int64_t)i * vol;
        // squared distance to the nearest voxel of the class (inside: every other voxel), straight into the output plane ...
        rc = edt_run("signed_sqdist_u8", labels, n, d, h, w, ids[i], 1, 0, plane, tail, b, s);
        if (rc) return rc;
        // ... then to the nearest voxel that is not of the class; its last pass reads the plane and leaves the signed value
        tail.mode = kEdtTailSigned;
        rc = edt_run("signed_sqdist_u8", labels, n, d, h, w, ids[i], 0, 0, plane, tail, b, s);
        if (rc) return rc;
    }
    return MRI3D_OK;
}

extern "C" size_t mri3d_softmax_boundary_workspace_bytes(void) { return (size_t)kIdxMaxBlocks * 2 * sizeof(double); }

extern "C" int mri3d_softmax_boundary_fwd(const Mri3dBoundaryGeom* g, const void* logits, const int32_t* map, float* loss, float* stats,
                                          void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    BdSlots slots;
    int rc = bd_check(g, "softmax_boundary_fwd", &slots);
    if (rc) return rc;
    MRI3D_REQUIRE(logits && map && loss && stats, MRI3D_EINVAL, "softmax_boundary_fwd: null pointer");
    rc = ws_check8("softmax_boundary_fwd", workspace, ws_bytes, mri3d_softmax_boundary_workspace_bytes());
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const IdxPlan plan = idx_plan(g->dtype, g->n, g->vox, g->c, g->x_ld, g->x_ld, false, ptr_align(logits), 0);
    double* part = static_cast<double*>(workspace);
#define CALL(CB)                                                                                                                 \
    hipLaunchKernelGGL((boundary_fwd_kernel<T, CB>), dim3(plan.blocks, g->n), dim3(256), 0, s, (const T*)logits, (const int*)map, part, \
                       g->vox, g->c, g->k, g->x_ld, plan.mode, slots)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { IDX_DISPATCH(plan.bucket, CALL); });
#undef CALL
    rc = check_launch("softmax_boundary_fwd");
    if (rc) return rc;
    hipLaunchKernelGGL(boundary_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)part, g->n * plan.blocks, stats, loss);
    return check_launch("softmax_boundary_fwd");
}

extern "C" int mri3d_softmax_boundary_bwd(const Mri3dBoundaryGeom* g, const void* logits, const int32_t* map, const float* stats,
                                          const float* dloss, void* dlogits, int32_t dx_ld, mri3d_stream_t stream) {
    BdSlots slots;
    int rc = bd_check(g, "softmax_boundary_bwd", &slots);
    if (rc) return rc;
    MRI3D_REQUIRE(dx_ld >= g->c, MRI3D_EINVAL, "softmax_boundary_bwd: gradient pitch %d < classes %d", dx_ld, g->c);
    MRI3D_REQUIRE(logits && map && stats && dloss && dlogits, MRI3D_EINVAL, "softmax_boundary_bwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const IdxPlan plan = idx_plan(g->dtype, g->n, g->vox, g->c, g->x_ld, dx_ld, true, ptr_align(logits, dlogits), 0);
#define CALL(CB)                                                                                                                 \
    hipLaunchKernelGGL((boundary_bwd_kernel<T, CB>), dim3(plan.blocks, g->n), dim3(256), 0, s, (const T*)logits, (const int*)map, stats, \
                       dloss, (T*)dlogits, g->vox, g->c, g->k, g->x_ld, dx_ld, plan.mode, slots)
    MRI3D_DISPATCH_DTYPE(g->dtype, T, { IDX_DISPATCH(plan.bucket, CALL); });
#undef CALL
    return check_launch("softmax_boundary_bwd");
}
