// conv_mfma_wgrad.hip — weight gradient of Conv3d 3x3x3 / stride 1 / pad 1 / dilation 1 on the MFMA, for the layers whose forward
// and data gradient are in conv_mfma.hip (fp32 tensors: v_mfma_f32_16x16x4_f32, exact fp32 fmaf chains; bf16 tensors: the same, or
// v_mfma_f32_16x16x32_bf16 in the two bf16 kernels).
//
//   wgrad     dW[co, ci, tap] = sum_v X[v + tap - 1, ci] * dY[v, co]                GEMM  M = (tap, ci), N = co, K = voxels
//
// GEMM view: dW(tap, ci; co) = sum over voxels.  One MFMA 16x16x4 takes A = X[4 voxels][16 rows] and B = dY[4 voxels][16 co]:
//   lane l supplies A[row = l&15][k = l>>4] and B[k = l>>4][col = l&15]; the 4 voxels of a k-step are consecutive in W.
//   rows of an M-tile:  CK=16: 16 input channels of one tap        (27 tap groups)
//                       CK= 8: 2 taps x 8 channels                 (14 tap groups, tap 27 = padding)
//                       CK= 1: 16 taps x the single input channel  ( 2 tap groups, taps 27..31 = padding)
// A workgroup (4 waves) is persistent over a contiguous range of 2x8x16-voxel tiles; it stages the X halo chunk and the
// dY tile (16 output channels) in LDS, each wave sweeps one quarter of the tile's voxels and keeps ALL tap groups of
// its (ci-tile, co-tile) pair in registers (27 x 4 VGPRs), so X and dY are read from LDS once per MFMA and from HBM/L2
// once per tile.  dbias rides along as one more accumulator fed with A = 1.  Partials are combined across the 4 waves
// through LDS in a fixed order, written once per workgroup (wgrad_combine_store), and summed by wgrad_mfma_reduce_kernel in a
// fixed order (deterministic: no float atomics).
//
// Six kernels, one per tuning round that is still the best for some layer; WgradKernel and mfma_wgrad_plan (below the kernels) say
// which layer takes which.  Activations are NDHWC (voxel pitch ld) as in conv_mfma.hip.
#include "common.h"
#include "conv_backends.h"
#include "mfma_util.h"
#include <stdlib.h>
#include <type_traits>

namespace mri3d {

constexpr int WTD = 2, WTH = 8, WTW = 16;
constexpr int WHD = WTD + 2, WHH = WTH + 2, WHW = WTW + 2;
constexpr int WHVOX = WHD * WHH * WHW;   // 720
constexpr int WVOX = WTD * WTH * WTW;    // 256

__host__ __device__ constexpr int wg_tap_groups(int CK) { return CK == 16 ? 27 : (CK == 8 ? 14 : 2); }

__device__ __forceinline__ int wg_tap_offset(int tap) {  // halo-voxel offset of a tap (clamped to tap 26 for padding)
    const int t = tap < 27 ? tap : 26;
    return ((t / 9) * WHH + (t / 3) % 3) * WHW + t % 3;
}

// ------------------------------------------------------------------ what the six kernels share
// The end of every kernel: combine the accumulators of the four waves through LDS in a FIXED order — wave 0 writes, waves 1..3 add,
// one barrier after each; the result is deterministic only through this order — and write the workgroup's partial.  The caller has
// put its barrier in front (every wave is done with the tile in `lds`, every DMA has landed): `lds` becomes the [TGA][256] buffer.
// Partial layout: part[P = gridDim.x][CIT = gridDim.y][COB = gridDim.z][TGA][256].  The 256 are an accumulator as the MFMA holds
// it, [row = 4*kq + r][col = li]: rows = the M-tile's (tap, ci) rows, columns = output channels.  TGA = the kernel's tap groups,
// plus one for dbias (the last) in the BIAS instantiations.
// tid, wv, li, kq: the kernel's own values (wv = tid >> 6 — a scalar in bf16t —, li = lane & 15, kq = lane >> 4).  They are
// passed in, not derived again: hipcc's schedule of the kernel in FRONT of the call moves with the form of this function, and
// this form left the hot kernels' loops as they were (compare the generated code before changing it).
template <int TGA>
__device__ __forceinline__ void wgrad_combine_store(const f32x4 (&acc)[TGA], float* lds, float* part, int tid, int wv, int li, int kq) {
    const int cit = blockIdx.y, cob = blockIdx.z;
    float* red = lds;  // [TGA][256]
    for (int w = 0; w < 4; ++w) {
        if (wv == w) {
#pragma unroll
            for (int t = 0; t < TGA; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = t * 256 + (4 * kq + r) * 16 + li;
                    red[o] = (w == 0) ? acc[t][r] : red[o] + acc[t][r];
                }
        }
        __syncthreads();
    }
    float* out = part + (((size_t)blockIdx.x * gridDim.y + cit) * gridDim.z + cob) * (TGA * 256);
    for (int i = tid; i < TGA * 256; i += 256) out[i] = red[i];
}

// conv over cat((x, x2), channels) in the transposed-tile kernels: a workgroup's 16-channel ci-tile (blockIdx.y) lives in ONE of the
// two tensors.  Which one, its pitch, the tile's first channel inside it and how many channels that tensor has (x2 == nullptr: x, Ci).
// Used by the two bf16 kernels; wgrad6 needs no channel count and has the same rebind written out (see there).
template <typename T>
struct CatTile { const T* x; int ld, c0, cn; };
template <typename T>
__device__ __forceinline__ CatTile<T> cat_tile(const T* x, int x_ld, int Ci, const T* x2, int x2_ld, int ksplit) {
    CatTile<T> t{x, x_ld, (int)blockIdx.y * 16, Ci};
    if (x2 != nullptr) {
        if (t.c0 >= ksplit) { t.x = x2; t.ld = x2_ld; t.c0 -= ksplit; t.cn = Ci - ksplit; }
        else t.cn = ksplit;
    }
    return t;
}

// Tile -> persistent-workgroup map shared by the wgrad kernels (speed only; see conv_mfma_fwd2_kernel): workgroups that
// land on the same XCD (linear block id mod 8) take CONSECUTIVE tiles of that XCD's contiguous tile range round-robin.
struct TileWalk { int first, stride, count; };
__device__ __forceinline__ TileWalk tile_walk(int ntiles) {
    const int P = gridDim.x;
    const int NX = P < 8 ? P : 8;
    const int off = (int)(((int64_t)P * (blockIdx.y + gridDim.y * blockIdx.z)) % NX);
    const int grp = ((int)blockIdx.x + off) % NX;
    const int p0 = (grp - off + NX) % NX;                 // first blockIdx.x of this XCD group in this (y, z) row
    const int slot = ((int)blockIdx.x - p0) / NX, members = (P - p0 + NX - 1) / NX;
    const int r_lo = (int)(((int64_t)ntiles * grp) / NX), r_hi = (int)(((int64_t)ntiles * (grp + 1)) / NX);
    TileWalk w;
    w.first = r_lo + slot;
    w.stride = members;
    w.count = w.first < r_hi ? (r_hi - w.first + members - 1) / members : 0;
    return w;
}

// Register staging of v3 and v4: a tile's 16-byte pieces (piece j of lane tid = piece j*256 + tid of the LDS image) are loaded from
// clamped addresses and bit j of a mask records whether piece j lies in the volume; wg_store_masked writes them to LDS, zeros where
// the bit is clear.  The clamped loads stay written out in both kernels: as a shared function they change hipcc's schedule of v3's
// tile loop (8 -> 16 layer 0.736 -> 0.742 ms).
struct WgTile { int n, d0, h0, w0; };
template <int NP>
__device__ __forceinline__ void wg_store_masked(float* dst, const float4 (&p)[NP], unsigned okbits, int tid) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const bool ok = (okbits >> j) & 1u;
        float4 v2;
        v2.x = ok ? p[j].x : 0.f; v2.y = ok ? p[j].y : 0.f; v2.z = ok ? p[j].z : 0.f; v2.w = ok ? p[j].w : 0.f;
        *reinterpret_cast<float4*>(dst + (j * 256 + tid) * 4) = v2;
    }
}

// ------------------------------------------------------------------ weight gradient of the first layer (Cin = 1; v1)
// The GEMM view above with 16 taps of the single input channel as the rows of an M-tile: two tap groups.  Synchronous staging (the
// tile is a 2.9 KB halo of X and 16 KB of dY).  T = storage type of x / dy (bf16 tensors are widened to fp32 when they are staged:
// the MFMA arithmetic is fp32 in every kernel of this file but the two bf16 ones).
constexpr int V1XBUF = (WHVOX + 3) & ~3;                                   // floats: X halo tile [WHVOX]
constexpr size_t V1LDS = (size_t)(V1XBUF + WVOX * 16) * sizeof(float);     // + dY tile [WVOX][16]

template <typename T, bool BIAS>
__global__ void __launch_bounds__(256, 2)
conv_mfma_wgrad_cin1_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part, int N, int D,
                            int H, int W, int Ci, int x_ld, int Co, int y_ld, int tilesD, int tilesH, int tilesW, int ntiles) {
    constexpr int TG = wg_tap_groups(1);
    constexpr int TGA = TG + (BIAS ? 1 : 0);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* xs = lds;             // [WHVOX]
    float* dys = lds + V1XBUF;   // [WVOX][16]

    const int cit = blockIdx.y, cob = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int dsel = wv >> 1, hsel = wv & 1;

    f32x4 acc[TGA];
#pragma unroll
    for (int t = 0; t < TGA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-lane A offsets that do not depend on the voxel
    int lane_aoff[TG];
#pragma unroll
    for (int tg = 0; tg < TG; ++tg) lane_aoff[tg] = wg_tap_offset(16 * tg + li);

    const int P = gridDim.x;
    const int t_lo = (int)(((int64_t)ntiles * blockIdx.x) / P), t_hi = (int)(((int64_t)ntiles * (blockIdx.x + 1)) / P);
    for (int tile = t_lo; tile < t_hi; ++tile) {
        int tt = tile;
        const int tw = tt % tilesW;
        tt /= tilesW;
        const int th = tt % tilesH;
        tt /= tilesH;
        const int td = tt % tilesD;
        const int n = tt / tilesD;
        const int w0 = tw * WTW, h0 = th * WTH, d0 = td * WTD;
        const T* xn = x + (int64_t)n * D * H * W * x_ld + cit;
        const T* dn = dy + (int64_t)n * D * H * W * y_ld + cob * 16;

        __syncthreads();
        for (int v = tid; v < WHVOX; v += 256) {
            const int wx = v % WHW;
            const int t2 = v / WHW;
            const int hy = t2 % WHH, dz = t2 / WHH;
            const int gd = d0 - 1 + dz, gh = h0 - 1 + hy, gw = w0 - 1 + wx;
            const bool ok = (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W;
            xs[v] = ok ? ldf(xn + (((int64_t)gd * H + gh) * W + gw) * x_ld) : 0.f;
        }
        for (int idx = tid; idx < WVOX * 4; idx += 256) {
            const int q = idx & 3, v = idx >> 2;
            const int wx = v % WTW;
            const int t2 = v / WTW;
            const int hy = t2 % WTH, dz = t2 / WTH;
            const int gd = d0 + dz, gh = h0 + hy, gw = w0 + wx;
            const bool ok = gd < D && gh < H && gw < W;
            const T* src = dn + (((int64_t)gd * H + gh) * W + gw) * y_ld + 4 * q;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            const int cbase = cob * 16 + 4 * q;
            if (ok) {
                if (cbase + 3 < Co && (y_ld & 3) == 0) {
                    val = ldf4(src);
                } else {
                    if (cbase + 0 < Co) val.x = ldf(src);
                    if (cbase + 1 < Co) val.y = ldf(src + 1);
                    if (cbase + 2 < Co) val.z = ldf(src + 2);
                    if (cbase + 3 < Co) val.w = ldf(src + 3);
                }
            }
            *reinterpret_cast<float4*>(dys + v * 16 + 4 * q) = val;
        }
        __syncthreads();

#pragma unroll 1
        for (int hr = 0; hr < 4; ++hr) {
            const int hy = hsel * 4 + hr;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int wx = ks * 4 + kq;
                const float b = dys[((dsel * WTH + hy) * WTW + wx) * 16 + li];
                const float* abase = xs + (dsel * WHH + hy) * WHW + wx;
#pragma unroll
                for (int tg = 0; tg < TG; ++tg) {
                    const float a = abase[lane_aoff[tg]];
                    acc[tg] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tg], 0, 0, 0);
                }
                if (BIAS) acc[TG] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b, acc[TG], 0, 0, 0);
            }
        }
    }

    __syncthreads();
    wgrad_combine_store(acc, lds, part, tid, wv, li, kq);
}

// ------------------------------------------------------------------ weight gradient, version 3 (Cin % 8 == 0: 8-channel chunks)
// v1 spends 2.3 of 5.1 ms of the 48->16 layer staging tiles while no MFMA runs (ablation: compute-only 130 TFLOP/s);
// the two resident workgroups of a CU run in lock-step, so nothing hides it.  v3 keeps v1's compute (all tap-group
// accumulators in registers, conflict-free 16-row M-tiles) and splits the staging T14-style: the NEXT tile's 16-byte
// pieces (6 of X + 4 of dY per lane) are fetched into registers before the current tile's 224 MFMAs per wave and
// written to LDS after them, so HBM/L2 latency is covered by MFMA work and only the LDS write pass stays exposed.
constexpr int V3NPX = (WHVOX * 2 + 255) / 256;   // X pieces per lane (6)
constexpr int V3NPY = WVOX * 4 / 256;            // dY pieces per lane (4)
constexpr int V3XBUF = V3NPX * 256 * 4;          // floats: X halo tile [WHVOX][8] (padded to whole pieces)
constexpr size_t V3LDS = (size_t)(V3XBUF + WVOX * 16) * sizeof(float);   // + dY tile [WVOX][16]

template <typename T, bool BIAS>
__global__ void __launch_bounds__(256, 2)
conv_mfma_wgrad3_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part, int N, int D,
                        int H, int W, int Ci, int x_ld, int Co, int y_ld, int tilesD, int tilesH, int tilesW, int ntiles) {
    constexpr int CK = 8, TG = wg_tap_groups(CK);
    constexpr int TGA = TG + (BIAS ? 1 : 0);
    constexpr int CP = CK;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* xs = lds;             // [WHVOX][CP] (+ padding)
    float* dys = lds + V3XBUF;   // [WVOX][16]

    const int cit = blockIdx.y, cob = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int dsel = wv >> 1, hsel = wv & 1;

    f32x4 acc[TGA];
#pragma unroll
    for (int t = 0; t < TGA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    int lane_aoff[TG];
#pragma unroll
    for (int tg = 0; tg < TG; ++tg) lane_aoff[tg] = wg_tap_offset(2 * tg + (li >> 3)) * CP + (li & 7);

    auto decode = [&](int tile) -> WgTile {
        WgTile r;
        r.w0 = (tile % tilesW) * WTW;
        tile /= tilesW;
        r.h0 = (tile % tilesH) * WTH;
        tile /= tilesH;
        r.d0 = (tile % tilesD) * WTD;
        r.n = tile / tilesD;
        return r;
    };
    float4 px[V3NPX], py[V3NPY];
    unsigned xok = 0, yok = 0;
    constexpr int XQ = CK / 4;
    // unconditional (clamped) loads; out-of-volume pieces are zeroed when they are written to LDS
    auto load_tile = [&](const WgTile& t) {
#pragma unroll
        for (int j = 0; j < V3NPX; ++j) {
            const int idx = j * 256 + tid;
            const int pv = idx < WHVOX * XQ ? idx : 0;
            const int q = pv % XQ, v = pv / XQ;
            const int wx = v % WHW, t2 = v / WHW;
            const int gd = t.d0 - 1 + t2 / WHH, gh = t.h0 - 1 + t2 % WHH, gw = t.w0 - 1 + wx;
            const bool ok = (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W;
            xok = ok ? (xok | (1u << j)) : (xok & ~(1u << j));
            const int cd = min(max(gd, 0), D - 1), chh = min(max(gh, 0), H - 1), cw = min(max(gw, 0), W - 1);
            px[j] = ldf4(x + ((((int64_t)t.n * D + cd) * H + chh) * W + cw) * x_ld + cit * CK + 4 * q);
        }
#pragma unroll
        for (int j = 0; j < V3NPY; ++j) {
            const int idx = j * 256 + tid;
            const int q = idx & 3, v = idx >> 2;
            const int wx = v % WTW, t2 = v / WTW;
            const int gd = t.d0 + t2 / WTH, gh = t.h0 + t2 % WTH, gw = t.w0 + wx;
            const int cb = cob * 16 + 4 * q;
            const bool ok = gd < D && gh < H && gw < W && cb < Co;   // host guarantees Co % 4 == 0
            yok = ok ? (yok | (1u << j)) : (yok & ~(1u << j));
            const int cd = min(gd, D - 1), chh = min(gh, H - 1), cw = min(gw, W - 1), cc = min(cb, Co - 4);
            py[j] = ldf4(dy + ((((int64_t)t.n * D + cd) * H + chh) * W + cw) * y_ld + cc);
        }
    };
    auto store_tile = [&]() {
        wg_store_masked(xs, px, xok, tid);
        wg_store_masked(dys, py, yok, tid);
    };

    const TileWalk tw = tile_walk(ntiles);
    if (tw.count > 0) {
        load_tile(decode(tw.first));
        store_tile();
        __syncthreads();
        for (int k = 0; k < tw.count; ++k) {
            const bool has_next = k + 1 < tw.count;
            if (has_next) load_tile(decode(tw.first + (k + 1) * tw.stride));   // global -> registers, in flight during the MFMAs
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
            for (int hr = 0; hr < 4; ++hr) {
                const int hy = hsel * 4 + hr;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int wx = ks * 4 + kq;
                    const float b = dys[((dsel * WTH + hy) * WTW + wx) * 16 + li];
                    const float* abase = xs + ((dsel * WHH + hy) * WHW + wx) * CP;
#pragma unroll
                    for (int tg = 0; tg < TG; ++tg) {
                        const float a = abase[lane_aoff[tg]];
                        acc[tg] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tg], 0, 0, 0);
                    }
                    if (BIAS) acc[TG] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b, acc[TG], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();                 // every wave is done reading this tile
            if (has_next) store_tile();      // registers -> LDS
            __syncthreads();
        }
    }

    __syncthreads();
    wgrad_combine_store(acc, lds, part, tid, wv, li, kq);
}

// ------------------------------------------------------------------ weight gradient, version 4 (bf16 tensors, Cin % 16 == 0)
// v3's overlap without its register bill: a 2x4x16-voxel tile (X halo 27 KB + dY 8 KB) is small enough to double-buffer
// in LDS with two workgroups per CU, and its 9 pieces per lane fit in registers next to the 27 tap accumulators.
// Per tile every wave runs 2 h-rows x 4 k-steps x 27 MFMAs: the next tile's pieces are fetched during row 0 and written
// to the OTHER buffer during row 1 — no exposed staging pass and a single barrier per tile.
// (bf16 tensors only — fp32 tensors with Cin % 16 == 0 take wgrad6 — and of those the ones whose channel counts or pitches the
// bf16 MFMA kernels cannot take.  The arithmetic is fp32 on the widened values, like v3's.)
constexpr int V4TH = 4, V4HH = V4TH + 2;
constexpr int V4HVOX = WHD * V4HH * WHW;           // 4 x 6 x 18 = 432 halo voxels
constexpr int V4VOX = WTD * V4TH * WTW;            // 128 output voxels
constexpr int V4NPX = (V4HVOX * 4 + 255) / 256;    // 7 X pieces per lane
constexpr int V4NPY = V4VOX * 4 / 256;             // 2 dY pieces per lane
constexpr int V4XBUF = V4NPX * 256 * 4;            // floats
constexpr int V4YBUF = V4VOX * 16;                 // floats
constexpr size_t V4LDS = (size_t)(2 * V4XBUF + 2 * V4YBUF) * sizeof(float);   // both double-buffered

__device__ __forceinline__ int v4_tap_offset(int tap) { return ((tap / 9) * V4HH + (tap / 3) % 3) * WHW + tap % 3; }

template <bool BIAS>
__global__ void __launch_bounds__(256, 2)
conv_mfma_wgrad4_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part, int N, int D,
                        int H, int W, int Ci, int x_ld, int Co, int y_ld, int tilesD, int tilesH, int tilesW, int ntiles) {
    constexpr int TG = 27, TGA = TG + (BIAS ? 1 : 0), CP = 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* xs = lds;                    // [2][V4XBUF]
    float* dys = lds + 2 * V4XBUF;      // [2][V4YBUF]

    const int cit = blockIdx.y, cob = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int dsel = wv >> 1, hsel = wv & 1;

    f32x4 acc[TGA];
#pragma unroll
    for (int t = 0; t < TGA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto decode = [&](int tile) -> WgTile {
        WgTile r;
        r.w0 = (tile % tilesW) * WTW;
        tile /= tilesW;
        r.h0 = (tile % tilesH) * V4TH;
        tile /= tilesH;
        r.d0 = (tile % tilesD) * WTD;
        r.n = tile / tilesD;
        return r;
    };
    float4 px[V4NPX], py[V4NPY];
    unsigned xok = 0, yok = 0;
    // Per-lane piece offsets relative to the tile's halo origin, computed ONCE: for an interior tile (the common case) a
    // piece's address is a wave-uniform base plus this 32-bit offset, i.e. no per-tile coordinate arithmetic at all.
    // The two workgroups of a CU run in lock-step, so every VALU instruction spent on addressing is time the MFMA pipe
    // idles (ablation: loads+stores alone 1.09 ms, MFMA alone 3.35 ms, together 4.26 ms on the 48->16 layer).
    unsigned xrel[V4NPX], yrel[V4NPY];
#pragma unroll
    for (int j = 0; j < V4NPX; ++j) {
        const int idx = j * 256 + tid;
        const int pv = idx < V4HVOX * 4 ? idx : 0;
        const int q = pv & 3, v = pv >> 2;
        const int wx = v % WHW, t2 = v / WHW;
        xrel[j] = (unsigned)((((t2 / V4HH) * H + t2 % V4HH) * W + wx) * x_ld + 4 * q);
    }
#pragma unroll
    for (int j = 0; j < V4NPY; ++j) {
        const int idx = j * 256 + tid;
        const int q = idx & 3, v = idx >> 2;
        const int wx = v % WTW, t2 = v / WTW;
        yrel[j] = (unsigned)((((t2 / V4TH) * H + t2 % V4TH) * W + wx) * y_ld + 4 * q);
    }
    const bool co_full = cob * 16 + 16 <= Co;
    auto load_tile = [&](const WgTile& t) {
        const bool interior = t.d0 >= 1 && t.d0 + WTD < D && t.h0 >= 1 && t.h0 + V4TH < H && t.w0 >= 1 && t.w0 + WTW < W &&
                              co_full;   // wave-uniform
        if (interior) {
            const bf16_t* xo = x + ((((int64_t)t.n * D + t.d0 - 1) * H + t.h0 - 1) * W + t.w0 - 1) * x_ld + cit * 16;
            const bf16_t* yo = dy + ((((int64_t)t.n * D + t.d0) * H + t.h0) * W + t.w0) * y_ld + cob * 16;
#pragma unroll
            for (int j = 0; j < V4NPX; ++j) px[j] = ldf4(xo + xrel[j]);
#pragma unroll
            for (int j = 0; j < V4NPY; ++j) py[j] = ldf4(yo + yrel[j]);
            xok = ~0u;
            yok = ~0u;
            return;
        }
        // border tiles: clamped addresses, zeroing happens at store time
#pragma unroll
        for (int j = 0; j < V4NPX; ++j) {
            const int idx = j * 256 + tid;
            const int pv = idx < V4HVOX * 4 ? idx : 0;
            const int q = pv & 3, v = pv >> 2;
            const int wx = v % WHW, t2 = v / WHW;
            const int gd = t.d0 - 1 + t2 / V4HH, gh = t.h0 - 1 + t2 % V4HH, gw = t.w0 - 1 + wx;
            const bool ok = (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W;
            xok = ok ? (xok | (1u << j)) : (xok & ~(1u << j));
            const int cd = min(max(gd, 0), D - 1), chh = min(max(gh, 0), H - 1), cw = min(max(gw, 0), W - 1);
            px[j] = ldf4(x + ((((int64_t)t.n * D + cd) * H + chh) * W + cw) * x_ld + cit * 16 + 4 * q);
        }
#pragma unroll
        for (int j = 0; j < V4NPY; ++j) {
            const int idx = j * 256 + tid;
            const int q = idx & 3, v = idx >> 2;
            const int wx = v % WTW, t2 = v / WTW;
            const int gd = t.d0 + t2 / V4TH, gh = t.h0 + t2 % V4TH, gw = t.w0 + wx;
            const int cb = cob * 16 + 4 * q;
            const bool ok = gd < D && gh < H && gw < W && cb < Co;   // host guarantees Co % 4 == 0
            yok = ok ? (yok | (1u << j)) : (yok & ~(1u << j));
            const int cd = min(gd, D - 1), chh = min(gh, H - 1), cw = min(gw, W - 1), cc = min(cb, Co - 4);
            py[j] = ldf4(dy + ((((int64_t)t.n * D + cd) * H + chh) * W + cw) * y_ld + cc);
        }
    };
    auto store_tile = [&](float* xb, float* yb) {
        if ((xok & yok) == ~0u) {   // interior tile (wave-uniform): no masking
#pragma unroll
            for (int j = 0; j < V4NPX; ++j) *reinterpret_cast<float4*>(xb + (j * 256 + tid) * 4) = px[j];
#pragma unroll
            for (int j = 0; j < V4NPY; ++j) *reinterpret_cast<float4*>(yb + (j * 256 + tid) * 4) = py[j];
            return;
        }
        wg_store_masked(xb, px, xok, tid);
        wg_store_masked(yb, py, yok, tid);
    };
    auto row = [&](const float* xb, const float* yb, int hr) {
        const int hy = hsel * 2 + hr;
        // a REAL loop over the 4 k-steps (one basic block each): unrolled, hipcc hoists all four k-steps' LDS reads
        // (108 VGPRs) on top of the 112 accumulators + 36 staging registers and spills (78 vs 96 TFLOP/s measured); a
        // ping-pong prefetch of the next k-step's fragments (2 x 28 VGPRs) spills as well.
#pragma unroll 1
        for (int ks = 0; ks < 4; ++ks) {
            const int wx = ks * 4 + kq;
            const float b = yb[((dsel * V4TH + hy) * WTW + wx) * 16 + li];
            const float* abase = xb + ((dsel * V4HH + hy) * WHW + wx) * CP + li;
#pragma unroll
            for (int tg = 0; tg < TG; ++tg) {
                const float a = abase[v4_tap_offset(tg) * CP];
                acc[tg] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tg], 0, 0, 0);
            }
            if (BIAS) acc[TG] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b, acc[TG], 0, 0, 0);
        }
    };

    const TileWalk tw = tile_walk(ntiles);
    if (tw.count > 0) {
        load_tile(decode(tw.first));
        store_tile(xs, dys);
        __syncthreads();
        for (int k = 0; k < tw.count; ++k) {
            const int cb = k & 1;
            const float* xb = xs + cb * V4XBUF;
            const float* yb = dys + cb * V4YBUF;
            const bool has_next = k + 1 < tw.count;
            if (has_next) load_tile(decode(tw.first + (k + 1) * tw.stride));        // global -> registers
            __builtin_amdgcn_sched_barrier(0);
            row(xb, yb, 0);                                   // 108 MFMAs per wave cover the loads
            if (has_next) store_tile(xs + (cb ^ 1) * V4XBUF, dys + (cb ^ 1) * V4YBUF);  // registers -> the OTHER buffer
            row(xb, yb, 1);
            __syncthreads();
        }
    }

    __syncthreads();
    wgrad_combine_store(acc, lds, part, tid, wv, li, kq);
}

// ------------------------------------------------------------------ weight gradient, transposed tiles (bf16 MFMA and fp32 v6)
// Both kernels below keep the tile TRANSPOSED in LDS, [channel][voxel]: the MFMA sums over voxels, and a lane's operand is a run
// of consecutive voxels of one channel.  Tile = 2 x 6 rows of TW voxels (TW = 32 bf16 / 16 fp32); X needs its (kd, kh) halo
// rows (4 x 8 rows), dY its 12 output rows.
//
// The kw taps:  dW[kd,kh,kw] = sum_v X[v + kw - 1] dY[v]  =  sum_u X[u] dY[u + 1 - kw].  The shift is applied to dY, not to X:
// per output row the three fragments dY[u+1], dY[u], dY[u-1] are built ONCE (register selection / v_alignbyte from the aligned
// fragment and its two neighbour voxels) and every (kd, kh) then costs ONE aligned X read for three MFMAs.  (Round 1 shifted X:
// one aligned read plus two neighbour reads per (kd, kh), 3-way bank-conflicted — PMC: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE =
// 0.64 in the bf16 kernel, which was LDS-bound at 18 % MFMA busy.)  The sums are re-partitioned between W-neighbouring tiles —
// a tile now takes the products of ITS X voxels, with dY[w0-1] and dY[w0+TW] read from the neighbours (zero outside the volume)
// — so X has no W halo at all and dY has a one-voxel W halo; the total over tiles is unchanged.
//
// LDS image: a (row, channel) line is 64 bytes = four 16-byte slots; logical slot q of channel c sits at physical slot
// (q + 2*(c >> 3)) & 3.  The hardware serves a ds_read_b128 in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...
// (MI355X_MICROARCH.md §LDS), i.e. channels 4..11 of a group read the NEXT k-group's slot; with unpadded 64-byte lines and the
// two-slot rotation of channels 8..15 all 16 lanes of every group hit different 4-bank slots (the 80-byte padded lines of round
// 1 cost 8 instead of 4 LDS cycles per read).
constexpr int BTD = 2, BTH = 6, BTW = 32;
constexpr int BHD = BTD + 2, BHH = BTH + 2;
constexpr int BXR = BHD * BHH;            // 32 X rows
constexpr int BYR = BTD * BTH;            // 12 dY rows
constexpr int DLS = 64;                   // bytes per (row, channel) line
constexpr int BXS = BXR * 16 * DLS;       // 32768 B  X
constexpr int BYS = BYR * 16 * DLS;       // 12288 B  dY
constexpr int BYH = BYR * 16 * 8;         //  1536 B  dY W-halo: per line {dword holding dY[w0-1], dword holding dY[w0+TW]}
constexpr size_t BLDS = (size_t)BXS + BYS + BYH;   // the tile of both kernels, in this order
// Sixteen zero bytes in device memory: what an out-of-volume 16-byte piece of a border tile loads.  Selecting the ADDRESS
// (piece or zeros) instead of the loaded VALUE (`ok ? loaded : 0`) keeps the staging wait-free: a select on loaded data makes
// hipcc wait for the load on the spot, i.e. the full memory latency in front of the tile's MFMAs.
__device__ const float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};

__device__ __forceinline__ int rot_slot(int q, int c) { return (q + 2 * ((c >> 3) & 1)) & 3; }

// eight voxels x eight channels (v[j] = the 16-byte channel vector of voxel j) -> out[c] = the 8 voxels of channel c
__device__ __forceinline__ void transpose8x8_bf16(const uint4 (&v)[8], uint4 (&out)[8]) {
    const unsigned* vw = reinterpret_cast<const unsigned*>(v);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int cd = c >> 1;
        const unsigned sel = (c & 1) ? 0x07060302u : 0x05040100u;   // high / low halves of (S1 = even voxel, S0 = odd voxel)
        out[c].x = __builtin_amdgcn_perm(vw[1 * 4 + cd], vw[0 * 4 + cd], sel);
        out[c].y = __builtin_amdgcn_perm(vw[3 * 4 + cd], vw[2 * 4 + cd], sel);
        out[c].z = __builtin_amdgcn_perm(vw[5 * 4 + cd], vw[4 * 4 + cd], sel);
        out[c].w = __builtin_amdgcn_perm(vw[7 * 4 + cd], vw[6 * 4 + cd], sel);
    }
}

// 16-byte load of bf16 data through an explicitly GLOBAL pointer (global_load_dwordx4: vmcnt only, never lgkmcnt)
__device__ __forceinline__ uint4 ldg4u(const bf16_t* p) {
    typedef unsigned gu32x4 __attribute__((ext_vector_type(4)));
    const gu32x4 v = *(const __attribute__((address_space(1))) gu32x4*)p;
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// v_mfma_f32_16x16x32_bf16 sums over K = 32 VOXELS with 8 consecutive k per lane.  Staging: each lane loads 8 consecutive
// voxels x 8 channels (8 x 16 B) and transposes them in registers (v_perm) into eight 16-byte LDS writes.
// Accumulators: 27 taps x (16 ci x 16 co) per wave (+1 for dbias, fed with A = 1).
template <bool BIAS>
__global__ void __launch_bounds__(256, 2)
conv_mfma_wgrad_bf16_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part, int N,
                            int D, int H, int W, int Ci, int x_ld, int Co, int y_ld, int tilesD, int tilesH, int tilesW,
                            int ntiles, const bf16_t* __restrict__ x2, int x2_ld, int ksplit) {
    constexpr int TG = 27, TGA = TG + (BIAS ? 1 : 0);
    const CatTile<bf16_t> ct = cat_tile(x, x_ld, Ci, x2, x2_ld, ksplit);
    x = ct.x, x_ld = ct.ld;
    const int xc0 = ct.c0, xcn = ct.cn;   // first channel of the tile inside its tensor, channels of that tensor
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char* xs = reinterpret_cast<char*>(lds);
    char* ys = xs + BXS;
    char* yh = ys + BYS;

    const int cob = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;

    f32x4 acc[TGA];
#pragma unroll
    for (int t = 0; t < TGA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging roles (fixed per lane)
    const int s_half = tid & 1, s_wg = (tid >> 1) & 3, s_row = tid >> 3;     // X: 32 rows x 4 w-groups x 2 channel halves
    const int h_half = tid & 1, h_side = (tid >> 1) & 1;   // dY halo voxels (lanes 128 .. 175)
    // per-lane operand addresses
    const int orow0 = wv * (BYR / 4);   // first of the wave's three output rows (same d-plane, consecutive h)
    const char* const xrow0 = xs + (((orow0 / BTH) * BHH + orow0 % BTH) * 16 + li) * DLS + 16 * rot_slot(kq, li);
    const int yline0 = orow0 * 16 + li;
    const char* const yrow0 = ys + yline0 * DLS + 16 * rot_slot(kq, li);
    // the dword holding the voxel before / after the lane's eight: last dword of the previous / first dword of the next k-group's
    // slot, or the W-halo entry of the line (k-groups 0 and 3)
    const char* const ypl0 = kq == 0 ? yh + yline0 * 8 : ys + yline0 * DLS + 16 * rot_slot(kq - 1, li) + 12;
    const char* const ynr0 = kq == 3 ? yh + yline0 * 8 + 4 : ys + yline0 * DLS + 16 * rot_slot(kq + 1, li);
    const int pl_step = kq == 0 ? 16 * 8 : 16 * DLS, nr_step = kq == 3 ? 16 * 8 : 16 * DLS;
    bf16x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16_t)1.0f;

    // The next tile's pieces are fetched into registers while the current tile is multiplied and transposed / written to the single
    // LDS tile between two barriers after it (as in wgrad6): the HBM latency of a tile is no longer exposed in front of its MFMAs
    // (round 1 staged synchronously: 18 % MFMA busy).
    uint4 vx[8], vy[8];
    uint4& vh = vy[0];   // the halo lanes (128 .. 175) stage no dY rows: their one piece shares a register with them
    const bool is_y = tid < BYR * 8, is_h = tid >= 128 && tid < 128 + BYR * 4;
    const int hy_row = (tid - 128) >> 2;   // dY halo row of lanes 128 .. 175
    // per-lane byte-free element offsets from the tile's origin voxels (X: (d0-1, h0-1, w0); dY: (d0, h0, w0); halo: (d0, h0, w0-1))
    const unsigned xrel = (unsigned)((((s_row / BHH) * H + s_row % BHH) * W + 8 * s_wg) * x_ld + 8 * s_half);
    const unsigned yrel = (unsigned)((((s_row / BTH) * H + s_row % BTH) * W + 8 * s_wg) * y_ld + 8 * s_half);
    const unsigned hrel = (unsigned)((((hy_row / BTH) * H + hy_row % BTH) * W + (h_side ? BTW + 1 : 0)) * y_ld + 8 * h_half);
    const bool ch_full = xc0 + 16 <= xcn && cob * 16 + 16 <= Co;
    auto load_tile = [&](int tile) {
        const int w0 = (tile % tilesW) * BTW;
        tile /= tilesW;
        const int d0 = (tile % tilesD) * BTD;
        tile /= tilesD;
        const int h0 = (tile % tilesH) * BTH;
        const int n = tile / tilesH;
        if (d0 >= 1 && d0 + BTD < D && h0 >= 1 && h0 + BTH < H && w0 >= 1 && w0 + BTW < W && ch_full) {
            // interior tile (wave-uniform): scalar bases + precomputed lane offsets, no coordinates, no masks
            const bf16_t* xb = x + ((((int64_t)n * D + d0 - 1) * H + h0 - 1) * W + w0) * x_ld + xc0;
            const bf16_t* yb = dy + ((((int64_t)n * D + d0) * H + h0) * W + w0) * y_ld + cob * 16;
#pragma unroll
            for (int j = 0; j < 8; ++j) vx[j] = ldg4u(xb + j * x_ld + xrel);
            if (is_y) {
#pragma unroll
                for (int j = 0; j < 8; ++j) vy[j] = ldg4u(yb + j * y_ld + yrel);
            }
            if (is_h) vh = ldg4u(yb - y_ld + hrel);
            return;
        }
        {   // ---- X: 8 voxels x 8 channels per lane
            const int gd = d0 - 1 + s_row / BHH, gh = h0 - 1 + s_row % BHH;
            const int c0 = xc0 + 8 * s_half;
            const bool rok = (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && c0 < xcn;
            const bf16_t* src = x + ((((int64_t)n * D + (rok ? gd : 0)) * H + (rok ? gh : 0)) * W) * x_ld + (c0 < xcn ? c0 : 0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int gw = w0 + 8 * s_wg + j;
                // unconditional, explicitly global; an out-of-volume piece reads g_zero16 (address select: no wait on the load here)
                vx[j] = ldg4u((rok && gw < W) ? src + (int64_t)gw * x_ld : reinterpret_cast<const bf16_t*>(g_zero16));
            }
        }
        if (is_y) {   // ---- dY: 12 rows x 4 w-groups x 2 channel halves
            const int gd = d0 + s_row / BTH, gh = h0 + s_row % BTH;
            const int c0 = cob * 16 + 8 * s_half;
            const bool rok = gd < D && gh < H && c0 < Co;       // host guarantees Co % 8 == 0
            const bf16_t* src = dy + ((((int64_t)n * D + (rok ? gd : 0)) * H + (rok ? gh : 0)) * W) * y_ld + (c0 < Co ? c0 : 0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int gw = w0 + 8 * s_wg + j;
                vy[j] = ldg4u((rok && gw < W) ? src + (int64_t)gw * y_ld : reinterpret_cast<const bf16_t*>(g_zero16));
            }
        }
        if (is_h) {   // ---- dY W-halo voxels w0 - 1 and w0 + 32
            const int gd = d0 + hy_row / BTH, gh = h0 + hy_row % BTH, gw = h_side ? w0 + BTW : w0 - 1;
            const int c0 = cob * 16 + 8 * h_half;
            const bool ok = gd < D && gh < H && (unsigned)gw < (unsigned)W && c0 < Co;
            vh = ldg4u(ok ? dy + ((((int64_t)n * D + gd) * H + gh) * W + gw) * y_ld + c0 : reinterpret_cast<const bf16_t*>(g_zero16));
        }
    };
    auto store_tile = [&]() {
        uint4 o[8];
        transpose8x8_bf16(vx, o);
        char* dline = xs + (s_row * 16 + 8 * s_half) * DLS + 16 * rot_slot(s_wg, 8 * s_half);   // 8 channels share a rotation
#pragma unroll
        for (int c = 0; c < 8; ++c) *reinterpret_cast<uint4*>(dline + c * DLS) = o[c];
        if (is_y) {
            transpose8x8_bf16(vy, o);
            char* yline = ys + (s_row * 16 + 8 * s_half) * DLS + 16 * rot_slot(s_wg, 8 * s_half);
#pragma unroll
            for (int c = 0; c < 8; ++c) *reinterpret_cast<uint4*>(yline + c * DLS) = o[c];
        } else if (is_h) {   // w0 - 1: high half of dword 0;  w0 + 32: low half of dword 1
            const unsigned* hw = reinterpret_cast<const unsigned*>(&vh);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const unsigned short val = (unsigned short)((c & 1) ? (hw[c >> 1] >> 16) : (hw[c >> 1] & 0xffffu));
                *reinterpret_cast<unsigned short*>(yh + (hy_row * 16 + 8 * h_half + c) * 8 + (h_side ? 4 : 2)) = val;
            }
        }
    };

    const TileWalk tw = tile_walk(ntiles);
    if (tw.count > 0) load_tile(tw.first);
    for (int k = 0; k < tw.count; ++k) {
        __syncthreads();   // the previous tile's MFMAs are done with the LDS tile
        store_tile();
        __syncthreads();
        if (k + 1 < tw.count) load_tile(tw.first + (k + 1) * tw.stride);
        __builtin_amdgcn_sched_barrier(0);

        // ---- 3 output rows per wave x 9 (kd, kh) x 3 kw MFMAs
        // the wave's three rows are consecutive in h: constant-stride row pointers, every tap an immediate offset
        const char* xrow = xrow0;
        const char* yrow = yrow0;
        const char* ypl = ypl0;
        const char* ynr = ynr0;
#pragma unroll 1
        for (int r = 0; r < BYR / 4; ++r, xrow += 16 * DLS, yrow += 16 * DLS, ypl += pl_step, ynr += nr_step) {
            const uint4 b1 = *reinterpret_cast<const uint4*>(yrow);            // dY[u], the lane's eight voxels
            const unsigned pl = *reinterpret_cast<const unsigned*>(ypl);        // high half = dY[first - 1]
            const unsigned nr = *reinterpret_cast<const unsigned*>(ynr);        // low half = dY[last + 1]
            uint4 bm, bp;   // dY[u - 1], dY[u + 1]
            bm.x = __builtin_amdgcn_alignbyte(b1.x, pl, 2);
            bm.y = __builtin_amdgcn_alignbyte(b1.y, b1.x, 2);
            bm.z = __builtin_amdgcn_alignbyte(b1.z, b1.y, 2);
            bm.w = __builtin_amdgcn_alignbyte(b1.w, b1.z, 2);
            bp.x = bm.y;
            bp.y = bm.z;
            bp.z = bm.w;
            bp.w = __builtin_amdgcn_alignbyte(nr, b1.w, 2);
            const bf16x8_t b0v = __builtin_bit_cast(bf16x8_t, bp), b1v = __builtin_bit_cast(bf16x8_t, b1),
                           b2v = __builtin_bit_cast(bf16x8_t, bm);
            if (BIAS) acc[TG] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, b1v, acc[TG], 0, 0, 0);
#pragma unroll
            for (int kdh = 0; kdh < 9; ++kdh) {
                const int lrow = ((kdh / 3) * BHH + kdh % 3) * 16;   // compile-time after unrolling
                const bf16x8_t g = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(xrow + lrow * DLS));
                acc[kdh * 3 + 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g, b0v, acc[kdh * 3 + 0], 0, 0, 0);   // X[u] dY[u+1]
                acc[kdh * 3 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g, b1v, acc[kdh * 3 + 1], 0, 0, 0);   // X[u] dY[u]
                acc[kdh * 3 + 2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g, b2v, acc[kdh * 3 + 2], 0, 0, 0);   // X[u] dY[u-1]
            }
        }
    }

    __syncthreads();
    wgrad_combine_store(acc, lds, part, tid, wv, li, kq);
}

// ------------------------------------------------------------------ bf16 weight gradient, marching along d, staged by LDS-DMA
// The tile kernel above re-reads its input 2.7x (a 2 x 6-row tile needs 4 x 8 rows of X) and is bound by what a CU can pull
// through its memory pipeline (MFMA busy 29 %).  Here a workgroup owns a COLUMN of the volume — 8 rows x 32 voxels
// — and marches through a segment of d planes with the last planes of X in an LDS ring: per output plane it fetches ONE new
// plane of X (10 rows) and one of dY (8 rows + the W halo).  Round 2 staged the column through registers (eight 16-byte loads
// with selected addresses, 32 v_perm of an 8x8 transpose and eight ds_write_b128 per staging lane and plane): ~100 vector
// instructions per plane which, beside the other workgroup's MFMAs, issue only each 14-28 cycles — 4 900 cycles
// per plane step for 1 800 cycles of MFMA work per SIMD (MFMA busy 0.30, 0.59 ms on 48 -> 16 at 2 x 160x192x160).
// Here NO vector instruction touches the data on its way in: the rows are copied as they lie in memory (channels last: one
// voxel = 32 bytes of a 16-channel tile) by LDS-DMA, and the transposition the MFMA needs — a lane's operand is a run of voxels
// of ONE channel — is done by the read: ds_read_b64_tr_b16 hands lane i of a 16-lane group channel i of four consecutive voxels
// (cdna_hip_programming.md T10).  With the address  row + 512*j + 8*lane  (j = 0, 1) a wave reads 512 contiguous bytes per
// instruction (conflict-free), and k-group kq of the K = 32 operand holds voxels 4kq..4kq+3 and 16+4kq..16+4kq+3 of the row —
// the same order in X and dY, so the sum over k is the sum over the row's 32 voxels.  The kw taps:
//   dW[kd,kh,kw] = sum_v X[v + kw - 1] dY[v]  =  sum_u X[u] dY[u + 1 - kw]
// i.e. dY read one voxel (32 bytes) to the left / right: an address, not a shuffle; the sums are re-partitioned between
// W-neighbouring columns — a column takes the products of ITS X voxels, with dY[w0-1] and dY[w0+32] read from the neighbours
// (zero outside the volume) — so X has no W halo and dY a one-voxel one.  Tasks = (sample, d-segment, column); accumulators
// (27 taps x (16 ci x 16 co) per wave, +1 for dbias fed with A = 1) and partial layout as in the tile kernel.
//   LDS: X planes (10 rows x 1 KiB) and dY planes (8 rows x 34 voxels, 1 088 B per row) in rings of four: the plane being
//   read + three in flight.  A wave keeps the X fragments of planes t-1 and t in REGISTERS from the steps that read them, so
//   LDS holds one live plane of each tensor instead of three + one: the same 78 KB carry three planes of lead instead of two —
//   on one-ci-tile layers the kernel's rate is (bytes in flight) / (loaded latency, ~3.7 us), DESIGN.md §4.4.
//   step t:  wait for the wave's pieces of step t-3 (counted vmcnt: those of steps t-2 and t-1 may still fly), barrier,
//            issue X plane t+4 and dY plane t+3 (19 pieces of 1 KiB per workgroup, 5 or 4 per wave, per-lane offsets constant
//            for the column; a plane outside the segment's range is a resource of zero records: zeros),
//            read the fragments of X plane t+1, multiply plane t (X planes t-1, t from registers, t+1; dY plane t).
// Measured against the register-staged kernel (tools/r03_wgt.sh, one box): 48 -> 16 0.590 -> 0.503 ms, 16 -> 16 0.232 -> 0.195,
// 8 -> 16 0.215 -> 0.180, 96 -> 32 at 80x96x80 0.358 -> 0.302, 16 -> 16 at 512 x 32^3 0.333 -> 0.287 with rings of five / three
// planes and two planes of lead; with the X fragments of two planes in registers and three planes of lead 0.457 / 0.186 / 0.168 /
// 0.291 / 0.26 ms.  What binds it is the
// fabric: with the MFMAs compiled out the 48 -> 16 layer still takes 0.415 ms (its three ci-tile workgroups each fetch dY: PMC
// 2.0x the algorithmic bytes, 5 TB/s), with the DMA compiled out 0.280 ms; with every workgroup on one L2-resident column the
// DMA alone runs at 14 TB/s.  (Workgroups of one task's ci-tiles share an XCD — tools/microbench/xcc_probe.hip — yet run in lock
// step and miss together; a start skew does not survive, the follower catches up.  One workgroup per CU taking all three ci-tiles
// against a single staging of dY — scatter form, dY in a five-plane ring, X triple-buffered, 138 KB of LDS — was built and is
// parity-green but slower: 0.72 ms with six waves of four rows (one or two waves per SIMD expose every fragment read and the
// step barrier), and twelve waves of two rows do not fit 170 registers: hipcc spills inside the MFMA loop.)
constexpr int MTH = 8, MXR = MTH + 2;                 // output rows / X rows per plane
constexpr int kMarchSeg = 40;                         // planes per task at most (5 fill steps per task); shorter for small volumes
constexpr int TXROW = BTW * 32;                       //  1 024 B  one X row: 32 voxels x 16 channels
constexpr int TXP = MXR * TXROW;                      // 10 240 B  one X plane
constexpr int TXSLOTS = 4;                            //           ring: the plane being read + three in flight
constexpr int TYROW = (BTW + 2) * 32;                 //  1 088 B  one dY row with its two W-halo voxels
constexpr int TYPIECES = (MTH * TYROW + 1023) / 1024; //  9 pieces of 1 KiB (the ninth: lanes 0..31)
constexpr int TYP = TYPIECES * 1024;                  //  9 216 B  one dY plane (8 704 used)
constexpr int TYSLOTS = 4;
constexpr size_t TLDS = TXSLOTS * TXP + TYSLOTS * TYP;   // 77 824 B: two workgroups per CU
constexpr int TNPC = (MXR + TYPIECES + 3) / 4;        // DMA pieces per wave and step at most (5)

typedef short s16x4_t __attribute__((ext_vector_type(4)));
// the K = 32 operand of the lane from a raw [voxel][16 channels] row: `a` = LDS byte address of the row + 8 * lane
__device__ __forceinline__ bf16x8_t tr_frag(unsigned a) {
    typedef __attribute__((address_space(3))) s16x4_t* lp;
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a + 512u));
    return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <bool BIAS>
__global__ void __launch_bounds__(256, 2)
conv_mfma_wgrad_bf16t_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part, int N,
                             int D, int H, int W, int Ci, int x_ld, int Co, int y_ld, int nseg, int tilesH, int tilesW,
                             int ntasks, const bf16_t* __restrict__ x2, int x2_ld, int ksplit, int segl) {
    constexpr int TG = 27, TGA = TG + (BIAS ? 1 : 0);
    const CatTile<bf16_t> ct = cat_tile(x, x_ld, Ci, x2, x2_ld, ksplit);
    x = ct.x, x_ld = ct.ld;
    const int xc0 = ct.c0, xcn = ct.cn;   // first channel of the tile inside its tensor, channels of that tensor
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const unsigned xs0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds), ys0 = xs0 + TXSLOTS * TXP;
    const int cob = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;

    f32x4 acc[TGA];
#pragma unroll
    for (int t = 0; t < TGA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16_t)1.0f;

    // operand addresses of the wave's two output rows (2 wv, 2 wv + 1): X rows 2 wv .. 2 wv + 3 of a plane, dY voxel u at + 32 (u + 1)
    const unsigned xfrag = xs0 + (unsigned)(2 * wv * TXROW + 8 * lane);        // + slot * TXP + row * TXROW
    const unsigned yfrag = ys0 + (unsigned)(2 * wv * TYROW + 32 + 8 * lane);   // + slot * TYP + row * TYROW + 32 * (1 - kw)

    const TileWalk tw = tile_walk(ntasks);
    for (int k = 0; k < tw.count; ++k) {
        int task = tw.first + k * tw.stride;
        const int w0 = (task % tilesW) * BTW;
        task /= tilesW;
        const int h0 = (task % tilesH) * MTH;
        task /= tilesH;
        const int seg = task % nseg, n = task / nseg;
        const int dA = seg * segl, dB = min(D, dA + segl);
        const int xlo = max(dA - 1, 0), xhi = min(dB, D - 1);   // X planes the segment consumes

        // the wave's pieces of a plane step: ids wv, wv + 4, ... < 19; id < 10 = X row id, else piece id - 10 of the dY plane.
        // Byte offset of the lane's 16 bytes from the plane's origin voxel, the out-of-volume value folded in: constant for the column.
        unsigned vof[TNPC];
#pragma unroll
        for (int i = 0; i < TNPC; ++i) {
            const int id = wv + 4 * i;
            vof[i] = kDmaOob;
            if (id < MXR) {   // wave-uniform
                const int vox = lane >> 1, half = lane & 1;
                const int gh = h0 - 1 + id, gw = w0 + vox;
                if ((unsigned)gh < (unsigned)H && gw < W && xc0 + 8 * half < xcn) vof[i] = (unsigned)(((id * W + vox) * x_ld + 8 * half) * 2);
            } else if (id < MXR + TYPIECES) {
                const int f = (id - MXR) * 64 + lane, row = f / (2 * (BTW + 2)), pc = f - row * (2 * (BTW + 2));
                const int vox = pc >> 1, half = pc & 1;
                const int gh = h0 + row, gw = w0 - 1 + vox;
                if (row < MTH && gh < H && (unsigned)gw < (unsigned)W && cob * 16 + 8 * half < Co)
                    vof[i] = (unsigned)(((row * W + vox) * y_ld + 8 * half) * 2);
            }
        }
        // plane origins: X at (h0 - 1, w0), dY at (h0, w0 - 1); a lane whose voxel lies outside the volume never dereferences them
        const int64_t xplane = (int64_t)H * W * x_ld * 2, yplane = (int64_t)H * W * y_ld * 2;
        const unsigned long long xorg = (unsigned long long)(x + ((((int64_t)n * D) * H + (h0 - 1)) * W + w0) * x_ld + xc0);
        const unsigned long long yorg = (unsigned long long)(dy + ((((int64_t)n * D) * H + h0) * W + (w0 - 1)) * y_ld + cob * 16);

        auto rsrc = [&](unsigned long long org, bool ok) {
            i32x4 rs;
            rs[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)(org & 0xffffffffu));
            rs[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)((org >> 32) & 0xffffu));
            rs[2] = ok ? (int)kDmaRecords : 0;
            rs[3] = 0x00020000;
            return rs;
        };
        // X fragments of planes t-1 and t stay in registers from the steps that read them: the LDS keeps ONE live plane of X and
        // of dY and three in flight of each (lead 3 instead of 2 in the same 78 KB)
        const int t0 = dA - 5;
        int sx = ((t0 + 4) % TXSLOTS + TXSLOTS) % TXSLOTS;   // ring slot of X plane t + 4
        int sy = ((t0 + 3) % TYSLOTS + TYSLOTS) % TYSLOTS;   // ring slot of dY plane t + 3
        bf16x8_t xfA[4], xfB[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xfA[i] = xfB[i] = ones;
        for (int t = t0; t < dB; ++t) {
            if (wv == 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            {
                const int qx = t + 4, qy = t + 3;
                const i32x4 rsx = rsrc(xorg + (unsigned long long)((int64_t)qx * xplane), qx >= xlo && qx <= xhi);
                const i32x4 rsy = rsrc(yorg + (unsigned long long)((int64_t)qy * yplane), qy >= dA && qy < dB);
                const unsigned xdst = xs0 + (unsigned)(sx * TXP), ydst = ys0 + (unsigned)(sy * TYP);
#pragma unroll
                for (int i = 0; i < TNPC; ++i) {
                    const int id = wv + 4 * i;
                    if (id < MXR) lds_dma16(vof[i], rsx, xdst + (unsigned)(id * 1024));
                    else if (id < MXR + TYPIECES - 1) lds_dma16(vof[i], rsy, ydst + (unsigned)((id - MXR) * 1024));
                    else if (id == MXR + TYPIECES - 1) {
                        if (lane < (MTH * TYROW - (TYPIECES - 1) * 1024) / 16) lds_dma16(vof[i], rsy, ydst + (unsigned)((id - MXR) * 1024));
                    }
                }
                sx = sx + 1 == TXSLOTS ? 0 : sx + 1;   // now the slot of plane t+5 = the slot of plane t+1
                sy = sy + 1 == TYSLOTS ? 0 : sy + 1;   // now the slot of plane t+4 = the slot of plane t
            }
            if (t >= dA - 2) {
                bf16x8_t xfC[4];
                const unsigned xb = xfrag + (unsigned)(sx * TXP);
#pragma unroll
                for (int i = 0; i < 4; ++i) xfC[i] = tr_frag(xb + (unsigned)(i * TXROW));
                if (t >= dA) {
                    const unsigned yb = yfrag + (unsigned)(sy * TYP);
                    bf16x8_t dyf[2][3];
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) dyf[r][kw] = tr_frag(yb + (unsigned)(r * TYROW + 32 * (1 - kw)));   // dY[u + 1 - kw]
                    if constexpr (BIAS) {
                        acc[TG] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, dyf[0][1], acc[TG], 0, 0, 0);
                        acc[TG] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, dyf[1][1], acc[TG], 0, 0, 0);
                    }
#pragma unroll
                    for (int kd = 0; kd < 3; ++kd)
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                                for (int kw = 0; kw < 3; ++kw) {
                                    const bf16x8_t a = kd == 0 ? xfA[r + kh] : kd == 1 ? xfB[r + kh] : xfC[r + kh];
                                    acc[(kd * 3 + kh) * 3 + kw] =
                                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, dyf[r][kw], acc[(kd * 3 + kh) * 3 + kw], 0, 0, 0);
                                }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) { xfA[i] = xfB[i]; xfB[i] = xfC[i]; }
            }
        }
    }
    // every DMA piece has landed (the last steps' zero planes too), every wave is done reading: the ring becomes the reduction buffer
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    wgrad_combine_store(acc, lds, part, tid, wv, li, kq);
}

// ------------------------------------------------------------------ weight gradient, version 6 (fp32, Cin % 16 == 0)
// The transposed tile for fp32: a line holds 16 voxels, and the MFMA K order is permuted so that k-group kq of the four k-steps
// of a row owns voxels 4kq..4kq+3 — ONE ds_read_b128 feeds four v_mfma_f32_16x16x4_f32 k-steps.  The kw = 0 / 2 taps take the
// same X fragment against dY shifted by one voxel: pure register selection from (left neighbour, fragment, right neighbour) of
// dY, done once per row.  A 2x6x16-voxel tile costs a wave 3 rows x (3 + 9) = 36 LDS reads for 324 MFMAs (v4 issued one 4-byte
// LDS read per MFMA, round 1's v6 84 reads); every non-MFMA instruction shows up as idle MFMA time.  Staging
// transposes 4 voxels x 4 channels per lane by register renaming.  Same accumulators and partial layout as v4.
constexpr int FTW = 16;   // voxels per line

// 16-byte load through an explicitly GLOBAL pointer (global_load_dwordx4: vmcnt only, never lgkmcnt)
__device__ __forceinline__ float4 ldg4(const float* p) {
    typedef float gf32x4 __attribute__((ext_vector_type(4)));
    const gf32x4 v = *(const __attribute__((address_space(1))) gf32x4*)p;
    return make_float4(v[0], v[1], v[2], v[3]);
}

//
// Eight-channel operands (Modified3DUNet's first level, modified_3dunet.py:33-55: 8 -> 8 twice, 16 -> 8) would leave half of a
// 16-row / 16-column operand empty.  CO8 (Co == 8): columns 8..15 of the dY operand carry the SAME eight channels for the next kw
// tap — lane li reads channel li & 7 and selects dY[u+1] (kw 0, columns 0..7) or dY[u] (kw 1, columns 8..15); a second operand
// carries kw 2: two MFMAs per (kd, kh) and k-step instead of three.  CI8 (Ci == 8): rows 8..15 of the X operand carry the same
// eight channels for the next (kd, kh) row pair — (kd,kh) = 2p + (li >> 3), five fragments instead of nine.  8 -> 8 then needs
// 10 MFMAs per k-step instead of the 27 of a half-empty 16 x 16 tile (and of the 14 of the older v3 kernel); the unused halves of
// the last pair / the kw-2 operand are duplicates that wgrad_mfma_reduce_kernel drops (accumulator -> tap map: wg6_tap()).
__host__ __device__ constexpr int wg6_groups(bool ci8, bool co8) { return (ci8 ? 5 : 9) * (co8 ? 2 : 3); }
// tap of element (row, col) of accumulator tg, or -1 (duplicate / padding)
__host__ __device__ inline int wg6_tap(bool ci8, bool co8, int tg, int row, int col) {
    const int nb = co8 ? 2 : 3, pa = tg / nb, q = tg % nb;
    int kdh = pa, kw = q;
    if (ci8) {
        kdh = 2 * pa + (row >> 3);
        if (kdh > 8) return -1;
    }
    if (co8) {
        kw = q == 0 ? (col >> 3) : 2;
        if (q == 1 && (col >> 3)) return -1;
    }
    return kdh * 3 + kw;
}

template <bool BIAS, bool CI8 = false, bool CO8 = false>
__global__ void __launch_bounds__(256, 2)
conv_mfma_wgrad6_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part, int N, int D,
                        int H, int W, int Ci, int x_ld, int Co, int y_ld, int tilesD, int tilesH, int tilesW, int ntiles,
                        const float* __restrict__ x2, int x2_ld, int ksplit) {
    constexpr int NA = CI8 ? 5 : 9, NB = CO8 ? 2 : 3;
    constexpr int TG = NA * NB, TGA = TG + (BIAS ? 1 : 0);
    // conv over cat((x, x2)) as in cat_tile (whole 16-channel tiles: no channel count).  Written out here: with the call, hipcc
    // schedules this kernel's tile loop differently and the 48 -> 16 layer measured 3.35 -> 3.39 ms.
    int xc0 = (int)blockIdx.y * 16;
    if (x2 != nullptr && xc0 >= ksplit) { x = x2; x_ld = x2_ld; xc0 -= ksplit; }
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char* xs = reinterpret_cast<char*>(lds);
    char* ys = xs + BXS;
    char* yh = ys + BYS;

    const int cob = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;

    f32x4 acc[TGA];
#pragma unroll
    for (int t = 0; t < TGA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging roles: a unit = 4 consecutive voxels x 4 channels; X has 32 rows x 4 w-groups x 4 quads = 512 units (2 per
    // lane), dY 12 rows x 4 x 4 = 192 units (lanes < 192), its W halo 12 rows x 2 sides x 4 quads = 96 voxels (lanes < 96)
    const int s_q = tid & 3, s_wg = (tid >> 2) & 3, s_row = tid >> 4;      // unit u = tid (+256): row = s_row (+16)
    const int h_q = tid & 3, h_side = (tid >> 2) & 1, h_row = tid >> 3;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int orow0 = wv * (BYR / 4);   // first of the wave's three output rows (same d-plane, consecutive h)
    const int ar = CI8 ? (li & 7) : li, ahs = CI8 ? (li >> 3) : 0;   // X operand row li: channel, (kd, kh) half
    const int bc = CO8 ? (li & 7) : li, bhs = CO8 ? (li >> 3) : 0;   // dY operand column li: channel, kw half
    const char* const xrow0 = xs + (((orow0 / BTH) * BHH + orow0 % BTH) * 16 + ar) * DLS + 16 * rot_slot(kq, ar);   // tap (kd,kh) = (0,0)
    int aoff[NA];   // CI8: the lane's line offset of pair p, (kd, kh) = 2p + ahs (the ninth has no partner: a duplicate)
#pragma unroll
    for (int pa = 0; pa < NA; ++pa) {
        const int kdh = CI8 ? (2 * pa + ahs < 9 ? 2 * pa + ahs : 8) : pa;
        aoff[pa] = ((kdh / 3) * BHH + kdh % 3) * 16 * DLS;
    }
    const int yline0 = orow0 * 16 + bc;
    const char* const yrow0 = ys + yline0 * DLS + 16 * rot_slot(kq, bc);
    // voxel before / after the lane's four: last float of the previous / first float of the next k-group's slot, or the W halo
    const char* const ypl0 = kq == 0 ? yh + yline0 * 8 : ys + yline0 * DLS + 16 * rot_slot(kq - 1, bc) + 12;
    const char* const ynr0 = kq == 3 ? yh + yline0 * 8 + 4 : ys + yline0 * DLS + 16 * rot_slot(kq + 1, bc);
    const int pl_step = kq == 0 ? 16 * 8 : 16 * DLS, nr_step = kq == 3 ? 16 * 8 : 16 * DLS;

    // next tile's pieces: fetched into registers while the current tile is multiplied (HBM/L2 latency hidden), written to
    // the single LDS tile between two barriers after it
    float4 vx[2][4], vh, vy[4];
    // Per-lane element offsets of its pieces from the tile's origin voxels, computed once: a piece's address is then a
    // wave-uniform tile base + a 32-bit lane offset, with no per-tile vector multiplies or 64-bit mads.
    // X origin = voxel (d0-1, h0-1, w0), dY origin = (d0, h0, w0).  Lanes without a piece (no such channel quad / row) read a
    // duplicate of an existing one and do not store it: EVERY lane issues the same 13 loads, unconditionally.
    // Two forms of the staging.  The 16-channel kernel keeps round 1's (load_tile_base): an interior tile is a scalar base plus
    // the lane offsets, wait-free; only border tiles (29 % at 160x192x160) select on loaded values, which makes hipcc wait for the
    // loads on the spot.  The eight-channel variants (load_tile_8) issue the same 13 loads in every lane, unconditionally —
    // lanes without a piece read a duplicate — and never look at a loaded value: out-of-volume pieces read a safe in-volume voxel,
    // their validity goes into a bit mask, and store_tile_8() zeroes them after the MFMAs (a load under a divergent `if` made
    // hipcc wait inside the interior path of these variants).  The same form for the 16-channel kernel measured 8 % SLOWER on the
    // 48 -> 16 layer (3.35 -> 3.63 ms): its per-lane 64-bit address arithmetic does not hide behind fp32 MFMAs.
    unsigned xrel[2], yrel;
    const int xq = CI8 ? (s_q & 1) : s_q, yq = CO8 ? (s_q & 1) : s_q, hq = CO8 ? (h_q & 1) : h_q;   // an existing channel quad
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int row = s_row + 16 * u;
        xrel[u] = (unsigned)((((row / BHH) * H + row % BHH) * W + 4 * s_wg) * x_ld + 4 * xq);
    }
    const unsigned xsafe = (unsigned)(((H + 1) * W) * x_ld);   // the tile's first output voxel (always in the volume)
    const bool yrow_ok = tid < BYR * 16, hrow_ok = tid < BYR * 8;
    yrel = yrow_ok ? (unsigned)((((s_row / BTH) * H + s_row % BTH) * W + 4 * s_wg) * y_ld + 4 * yq) : 0u;
    // halo voxel relative to (d0, h0, w0 - 1): never negative
    const unsigned hrel = hrow_ok ? (unsigned)((((h_row / BTH) * H + h_row % BTH) * W + (h_side ? FTW + 1 : 0)) * y_ld + 4 * hq) : (unsigned)y_ld;
    const bool co_full = CO8 || cob * 16 + 16 <= Co;
    const bool xon = !CI8 || s_q < 2, yon = yrow_ok && (!CO8 || s_q < 2), hon = hrow_ok && (!CO8 || h_q < 2);   // lanes that store
    unsigned okbits = ~0u;   // of the tile in the registers: bit 4u+j X piece (u, j), bit 8+j dY piece j, bit 12 the halo voxel
    bool border = false;     // ... and whether any lane has a zero bit (wave-uniform)
    auto load_tile_base = [&](int tile) {   // both operands 16 channels wide: the round-1 form, at the register limit as it is
        const int w0 = (tile % tilesW) * FTW;
        tile /= tilesW;
        const int d0 = (tile % tilesD) * BTD;
        tile /= tilesD;
        const int h0 = (tile % tilesH) * BTH;
        const int n = tile / tilesH;
        // wave-uniform bases; the X base may point before the tensor (d0 = 0 ...) and is only dereferenced at valid offsets
        const float* xb = x + ((((int64_t)n * D + d0 - 1) * H + h0 - 1) * W + w0) * x_ld + xc0;
        const int c0 = cob * 16 + 4 * s_q;
        const float* yb = dy + ((((int64_t)n * D + d0) * H + h0) * W + w0) * y_ld + cob * 16;
        // Interior tile (the common case; wave-uniform test on scalars): every piece is in the volume, so a piece's address is
        // a scalar base (tile origin + j voxels) plus the lane's precomputed 32-bit offset — no per-lane coordinates, no masks.
        // The general path below costs ~300 instructions per tile against the tile's 336 MFMAs per wave, and none of them hides
        // behind the fp32 MFMA.
        if (d0 >= 1 && d0 + BTD < D && h0 >= 1 && h0 + BTH < H && w0 >= 1 && w0 + FTW < W && co_full) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* xj = xb + j * x_ld;   // scalar
                vx[0][j] = ldg4(xj + xrel[0]);
                vx[1][j] = ldg4(xj + xrel[1]);
            }
            if (tid < BYR * 16) {
#pragma unroll
                for (int j = 0; j < 4; ++j) vy[j] = ldg4(yb + j * y_ld + yrel);
            }
            if (tid < BYR * 8) vh = ldg4(yb - y_ld + hrel);
            return;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {   // ---- X
            const int row = s_row + 16 * u;
            const int gd = d0 - 1 + row / BHH, gh = h0 - 1 + row % BHH;
            const bool rok = (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = rok && w0 + 4 * s_wg + j < W;
                // (the address-select form of the bf16 kernel — out-of-volume pieces read g_zero16, no wait here — costs this kernel
                // two more registers than it has: 2 spills, 48 -> 16 layer 3.33 -> 3.47 ms)
                const float4 t = ldg4(xb + (ok ? xrel[u] + (unsigned)(j * x_ld) : xsafe));
                vx[u][j] = ok ? t : zero4;
            }
        }
        if (tid < BYR * 16) {   // ---- dY
            const int gd = d0 + s_row / BTH, gh = h0 + s_row % BTH;
            const bool rok = gd < D && gh < H && c0 < Co;       // host guarantees Co % 4 == 0
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = rok && w0 + 4 * s_wg + j < W;
                const float4 t = ldg4(yb + (ok ? yrel + (unsigned)(j * y_ld) : 0u));
                vy[j] = ok ? t : zero4;
            }
        }
        if (tid < BYR * 8) {   // ---- dY W-halo voxels w0 - 1 / w0 + 16
            const int gd = d0 + h_row / BTH, gh = h0 + h_row % BTH, gw = h_side ? w0 + FTW : w0 - 1;
            const int hc = cob * 16 + 4 * h_q;
            const bool ok = gd < D && gh < H && (unsigned)gw < (unsigned)W && hc < Co;
            const float4 t = ldg4(dy + ((((int64_t)n * D + (ok ? gd : d0)) * H + (ok ? gh : h0)) * W + (ok ? gw : w0)) * y_ld + (ok ? hc : 0));
            vh = ok ? t : zero4;
        }
    };
    auto store_tile_base = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            char* dst = xs + ((s_row + 16 * u) * 16 + 4 * s_q) * DLS + 16 * rot_slot(s_wg, 4 * s_q);   // 4 channels share a rotation
            *reinterpret_cast<float4*>(dst) = make_float4(vx[u][0].x, vx[u][1].x, vx[u][2].x, vx[u][3].x);
            *reinterpret_cast<float4*>(dst + DLS) = make_float4(vx[u][0].y, vx[u][1].y, vx[u][2].y, vx[u][3].y);
            *reinterpret_cast<float4*>(dst + 2 * DLS) = make_float4(vx[u][0].z, vx[u][1].z, vx[u][2].z, vx[u][3].z);
            *reinterpret_cast<float4*>(dst + 3 * DLS) = make_float4(vx[u][0].w, vx[u][1].w, vx[u][2].w, vx[u][3].w);
        }
        if (tid < BYR * 16) {
            char* dst = ys + (s_row * 16 + 4 * s_q) * DLS + 16 * rot_slot(s_wg, 4 * s_q);
            *reinterpret_cast<float4*>(dst) = make_float4(vy[0].x, vy[1].x, vy[2].x, vy[3].x);
            *reinterpret_cast<float4*>(dst + DLS) = make_float4(vy[0].y, vy[1].y, vy[2].y, vy[3].y);
            *reinterpret_cast<float4*>(dst + 2 * DLS) = make_float4(vy[0].z, vy[1].z, vy[2].z, vy[3].z);
            *reinterpret_cast<float4*>(dst + 3 * DLS) = make_float4(vy[0].w, vy[1].w, vy[2].w, vy[3].w);
        }
        if (tid < BYR * 8) {
            char* dst = yh + (h_row * 16 + 4 * h_q) * 8 + 4 * h_side;
            *reinterpret_cast<float*>(dst) = vh.x;
            *reinterpret_cast<float*>(dst + 8) = vh.y;
            *reinterpret_cast<float*>(dst + 16) = vh.z;
            *reinterpret_cast<float*>(dst + 24) = vh.w;
        }
    };

    auto load_tile_8 = [&](int tile) {
        const int w0 = (tile % tilesW) * FTW;
        tile /= tilesW;
        const int d0 = (tile % tilesD) * BTD;
        tile /= tilesD;
        const int h0 = (tile % tilesH) * BTH;
        const int n = tile / tilesH;
        // wave-uniform bases; the X base may point before the tensor (d0 = 0 ...) and is only dereferenced at valid offsets
        const float* xb = x + ((((int64_t)n * D + d0 - 1) * H + h0 - 1) * W + w0) * x_ld + xc0;
        const float* yb = dy + ((((int64_t)n * D + d0) * H + h0) * W + w0) * y_ld + cob * 16;
        unsigned xo[2][4], yo[4], ho = hrel, bits = ~0u;
        // Interior tile (the common case; wave-uniform test on scalars): every piece is in the volume.  The general path costs
        // ~300 integer instructions per tile against the tile's 336 MFMAs per wave, and none of them hides behind the fp32 MFMA.
        const bool interior = d0 >= 1 && d0 + BTD < D && h0 >= 1 && h0 + BTH < H && w0 >= 1 && w0 + FTW < W && co_full;
        if (interior) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xo[0][j] = xrel[0] + (unsigned)(j * x_ld);
                xo[1][j] = xrel[1] + (unsigned)(j * x_ld);
                yo[j] = yrel + (unsigned)(j * y_ld);
            }
        } else {
            bits = 0u;
#pragma unroll
            for (int u = 0; u < 2; ++u) {   // ---- X
                const int row = s_row + 16 * u;
                const int gd = d0 - 1 + row / BHH, gh = h0 - 1 + row % BHH;
                const bool rok = (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = rok && w0 + 4 * s_wg + j < W;
                    xo[u][j] = ok ? xrel[u] + (unsigned)(j * x_ld) : xsafe;
                    bits |= ok ? 1u << (4 * u + j) : 0u;
                }
            }
            {   // ---- dY
                const int gd = d0 + s_row / BTH, gh = h0 + s_row % BTH;
                const bool rok = yrow_ok && gd < D && gh < H && cob * 16 + 4 * s_q < Co;       // host guarantees Co % 4 == 0
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = rok && w0 + 4 * s_wg + j < W;
                    yo[j] = ok ? yrel + (unsigned)(j * y_ld) : 0u;
                    bits |= ok ? 1u << (8 + j) : 0u;
                }
            }
            {   // ---- dY W-halo voxels w0 - 1 / w0 + 16
                const int gd = d0 + h_row / BTH, gh = h0 + h_row % BTH, gw = h_side ? w0 + FTW : w0 - 1;
                const bool ok = hrow_ok && gd < D && gh < H && (unsigned)gw < (unsigned)W && cob * 16 + 4 * h_q < Co;
                ho = ok ? hrel : (unsigned)y_ld;
                bits |= ok ? 1u << 12 : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            vx[0][j] = ldg4(xb + xo[0][j]);
            vx[1][j] = ldg4(xb + xo[1][j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) vy[j] = ldg4(yb + yo[j]);
        vh = ldg4(yb - y_ld + ho);
        okbits = bits;
        border = !interior;
    };
    auto store_tile_8 = [&]() {
        if (border) {   // wave-uniform; the loads landed long ago (a tile of MFMAs lies between load_tile and store_tile)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (!((okbits >> (4 * u + j)) & 1u)) vx[u][j] = zero4;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!((okbits >> (8 + j)) & 1u)) vy[j] = zero4;
            if (!((okbits >> 12) & 1u)) vh = zero4;
        }
        if (xon) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                char* dst = xs + ((s_row + 16 * u) * 16 + 4 * s_q) * DLS + 16 * rot_slot(s_wg, 4 * s_q);   // 4 channels share a rotation
                *reinterpret_cast<float4*>(dst) = make_float4(vx[u][0].x, vx[u][1].x, vx[u][2].x, vx[u][3].x);
                *reinterpret_cast<float4*>(dst + DLS) = make_float4(vx[u][0].y, vx[u][1].y, vx[u][2].y, vx[u][3].y);
                *reinterpret_cast<float4*>(dst + 2 * DLS) = make_float4(vx[u][0].z, vx[u][1].z, vx[u][2].z, vx[u][3].z);
                *reinterpret_cast<float4*>(dst + 3 * DLS) = make_float4(vx[u][0].w, vx[u][1].w, vx[u][2].w, vx[u][3].w);
            }
        }
        if (yon) {
            char* dst = ys + (s_row * 16 + 4 * s_q) * DLS + 16 * rot_slot(s_wg, 4 * s_q);
            *reinterpret_cast<float4*>(dst) = make_float4(vy[0].x, vy[1].x, vy[2].x, vy[3].x);
            *reinterpret_cast<float4*>(dst + DLS) = make_float4(vy[0].y, vy[1].y, vy[2].y, vy[3].y);
            *reinterpret_cast<float4*>(dst + 2 * DLS) = make_float4(vy[0].z, vy[1].z, vy[2].z, vy[3].z);
            *reinterpret_cast<float4*>(dst + 3 * DLS) = make_float4(vy[0].w, vy[1].w, vy[2].w, vy[3].w);
        }
        if (hon) {
            char* dst = yh + (h_row * 16 + 4 * h_q) * 8 + 4 * h_side;
            *reinterpret_cast<float*>(dst) = vh.x;
            *reinterpret_cast<float*>(dst + 8) = vh.y;
            *reinterpret_cast<float*>(dst + 16) = vh.z;
            *reinterpret_cast<float*>(dst + 24) = vh.w;
        }
    };

    auto load_tile = [&](int tile) {
        if constexpr (CI8 || CO8) load_tile_8(tile);
        else load_tile_base(tile);
    };
    auto store_tile = [&]() {
        if constexpr (CI8 || CO8) store_tile_8();
        else store_tile_base();
    };

    const TileWalk tw = tile_walk(ntiles);
    if (tw.count > 0) load_tile(tw.first);
    for (int k = 0; k < tw.count; ++k) {
        __syncthreads();   // the previous tile's MFMAs are done with the LDS tile
        store_tile();
        __syncthreads();
        load_tile(tw.first + (k + 1 < tw.count ? k + 1 : k) * tw.stride);   // (the last iteration re-reads its own tile: no branch)
        __builtin_amdgcn_sched_barrier(0);

        // ---- 3 output rows per wave x 9 (kd, kh) x 3 kw x 4 k-steps
        // the wave's three rows are consecutive in h (same d): row pointers advance by a constant, every tap is an
        // immediate offset — no per-row address arithmetic (each VALU instruction costs MFMA time)
        const char* xrow = xrow0;
        const char* yrow = yrow0;
        const char* ypl = ypl0;
        const char* ynr = ynr0;
#pragma unroll 1
        for (int r = 0; r < BYR / 4; ++r, xrow += 16 * DLS, yrow += 16 * DLS, ypl += pl_step, ynr += nr_step) {
            const float4 b = *reinterpret_cast<const float4*>(yrow);
            const float pl = *reinterpret_cast<const float*>(ypl);   // dY[first - 1]
            const float nr = *reinterpret_cast<const float*>(ynr);   // dY[last + 1]
            const float b0[4] = {b.y, b.z, b.w, nr}, b1[4] = {b.x, b.y, b.z, b.w}, b2[4] = {pl, b.x, b.y, b.z};   // dY[u+1], dY[u], dY[u-1]
            if (BIAS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[TG] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b1[j], acc[TG], 0, 0, 0);
            }
            float bp[4];   // CO8: kw 0 (columns 0..7) | kw 1 (columns 8..15)
#pragma unroll
            for (int j = 0; j < 4; ++j) bp[j] = bhs ? b1[j] : b0[j];
#pragma unroll
            for (int pa = 0; pa < NA; ++pa) {
                // the line offset is a compile-time constant after unrolling (CI8: one per-lane register per pair)
                const float4 g = *reinterpret_cast<const float4*>(xrow + (CI8 ? aoff[pa] : ((pa / 3) * BHH + pa % 3) * 16 * DLS));
                const float a[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (CO8) {
                        acc[pa * 2 + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bp[j], acc[pa * 2 + 0], 0, 0, 0);
                        acc[pa * 2 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b2[j], acc[pa * 2 + 1], 0, 0, 0);
                    } else {
                        acc[pa * 3 + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b0[j], acc[pa * 3 + 0], 0, 0, 0);
                        acc[pa * 3 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b1[j], acc[pa * 3 + 1], 0, 0, 0);
                        acc[pa * 3 + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b2[j], acc[pa * 3 + 2], 0, 0, 0);
                    }
                }
            }
        }
    }

    __syncthreads();
    wgrad_combine_store(acc, lds, part, tid, wv, li, kq);
}

// dw[co][ci][tap] = sum_p part[p][cit][cob][tg][row][col]   (+ dbias[co] from the extra accumulator of cit == 0); the partial
// layout is wgrad_combine_store's.
// Threads walk the partial layout itself (64 consecutive elements per wave => coalesced 256-byte reads of every
// partial), 4 partial-lanes per element combined through LDS in double; the (tiny) result is scattered into torch's
// (Co, Ci, 3,3,3) layout.
__global__ void __launch_bounds__(256)
wgrad_mfma_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ dbias, int P,
                         int CIT, int COB, int CK, int TG, int TGA, int Ci, int Co, int mode8) {
    __shared__ double red[256];
    const int el = threadIdx.x & 63, ql = threadIdx.x >> 6;
    const int nelem = CIT * COB * TGA * 256;
    const int e = blockIdx.x * 64 + el;
    const size_t pstride = (size_t)nelem;
    double s = 0.0;
    if (e < nelem) {
        double s1 = 0.0, s2 = 0.0, s3 = 0.0;   // four independent chains: more partial loads in flight
        int q = ql;
        for (; q + 12 < P; q += 16) {
            s += (double)part[(size_t)q * pstride + e];
            s1 += (double)part[(size_t)(q + 4) * pstride + e];
            s2 += (double)part[(size_t)(q + 8) * pstride + e];
            s3 += (double)part[(size_t)(q + 12) * pstride + e];
        }
        for (; q < P; q += 4) s += (double)part[(size_t)q * pstride + e];
        s = (s + s1) + (s2 + s3);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (ql != 0 || e >= nelem) return;
    s = red[el] + red[64 + el] + red[128 + el] + red[192 + el];
    const int col = e & 15, row = (e >> 4) & 15;
    int t = e >> 8;
    const int tg = t % TGA;
    t /= TGA;
    const int cob = t % COB, cit = t / COB;
    // mode8 (v6 with eight-channel operands; bit 0: Ci == 8, bit 1: Co == 8): rows / columns 8..15 repeat the channels for another tap
    const bool ci8 = mode8 & 1, co8 = mode8 & 2;
    const int co = co8 ? (col & 7) : cob * 16 + col;
    if (co >= Co) return;
    if (tg == TG) {  // bias accumulator (all rows equal): take row 0 of the first ci tile
        if (dbias != nullptr && cit == 0 && row == 0 && !(co8 && col >= 8)) dbias[co] = (float)s;
        return;
    }
    int ci, tap;
    if (mode8) {
        ci = ci8 ? (row & 7) : cit * 16 + row;
        tap = wg6_tap(ci8, co8, tg, row, col);
        if (tap < 0) return;
    } else if (CK == 16) { ci = cit * 16 + row; tap = tg; }
    else if (CK == 8) { ci = cit * 8 + (row & 7); tap = 2 * tg + (row >> 3); }
    else { ci = cit; tap = 16 * tg + row; }
    if (tap < 27 && ci < Ci) dw[((size_t)co * Ci + ci) * 27 + tap] = (float)s;
}

// The weight-gradient kernels of this file; mfma_wgrad_plan chooses one, and this list with the cascade there is the one
// description of that choice.
enum class WgradKernel {
    cin1,      // conv_mfma_wgrad_cin1_kernel: the first layer (Cin = 1: 16 taps per M-tile)
    wgrad3,    // conv_mfma_wgrad3_kernel: Cin % 8 == 0 (8-channel chunks), register prefetch
    wgrad4,    // conv_mfma_wgrad4_kernel: bf16 tensors the bf16 MFMA kernels cannot take, Cin % 16 == 0: small double-buffered tile
    bf16,      // conv_mfma_wgrad_bf16_kernel: bf16 tensors, Cin % 8 == 0: a 16-channel ci-tile whose upper half may be empty
    wgrad6,    // conv_mfma_wgrad6_kernel: fp32, Cin % 16 == 0, transposed tile: 110 / 104 / 102 TFLOP/s on 48->16 / 96->32 / 16->16 against wgrad4's 103 / 90 / 99
    bf16t      // conv_mfma_wgrad_bf16t_kernel: bf16, marching along d
};

struct MfmaWgradPlan {
    WgradKernel kernel;
    bool ci8, co8;   // wgrad6 with eight-channel operands: rows / columns 8..15 of a tile repeat the channels for another tap
    int CK, CIT, COB, TG, P, tilesD, tilesH, tilesW, ntiles, segl;
    int td, th, tw;   // the output tile (tasks of bf16t: td = segl planes of a column)
    size_t part_floats, smem;
    // the transposed-tile kernels are the only ones with a second operand; wgrad6 needs whole 16-channel chunks in it (the bf16
    // kernels' 8 follow from Cin % 8 == 0 and split % 16 == 0)
    bool takes_split() const { return kernel == WgradKernel::wgrad6 || kernel == WgradKernel::bf16 || kernel == WgradKernel::bf16t; }
    bool second_needs_16_channels() const { return kernel == WgradKernel::wgrad6; }
    bool needs_16_byte_alignment() const { return kernel == WgradKernel::bf16 || kernel == WgradKernel::bf16t; }
};

static bool mfma_wgrad_plan(const Mri3dConvGeom& g, MfmaWgradPlan& p) {
    if (!(g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 1 && g.ph == 1 &&
          g.pw == 1 && g.dd == 1 && g.dh == 1 && g.dw == 1))
        return false;
    const bool bf = g.dtype == MRI3D_BF16, f32 = g.dtype == MRI3D_F32;
    const bool quads = g.ci % 8 == 0 && g.co % 4 == 0 && g.y_ld % 4 == 0;
    p.ci8 = p.co8 = false;
    p.segl = 0;
    if (bf && g.ci % 8 == 0 && g.co % 8 == 0 && g.x_ld % 8 == 0 && g.y_ld % 8 == 0) {
        p.kernel = WgradKernel::bf16;
#ifndef MRI3D_BF16_WGRAD_MARCH_MIN_D
#define MRI3D_BF16_WGRAD_MARCH_MIN_D 8   // (tuning builds: a huge value keeps every bf16 layer on the tile kernel)
#endif
        // bf16, marching along d (conv_mfma_wgrad_bf16t_kernel): when the columns x segments give every workgroup at least three
        // tasks — segments of 40 planes, or 20 for smaller volumes (each task pays 4 staging-only fill steps; with 10-plane segments
        // the 32 -> 32 layer at 80x96x80 ran 0.132 ms against the tile kernel's 0.122)
        if (g.di >= MRI3D_BF16_WGRAD_MARCH_MIN_D) {
            const int pairs5 = cdiv(g.ci, 16) * cdiv(g.co, 16);
            const int P5 = std::max(1, 512 / std::max(1, pairs5));
            const int64_t cols = (int64_t)g.n * cdiv(g.hi, MTH) * cdiv(g.wi, BTW);
            for (int sl = kMarchSeg; sl >= 20 && p.segl == 0; sl /= 2)
                if (cols * cdiv(g.di, sl) >= (int64_t)3 * P5) p.segl = sl;
            if (p.segl) p.kernel = WgradKernel::bf16t;
        }
        // (The same structure for fp32 — tools/experiments/wgrad6m_kernel.hip, parity-green — measured no gain: 16 -> 16 1.20 -> 1.25 ms,
        // 48 -> 16 3.35 -> 3.40 ms, 96 -> 32 1.83 -> 1.81 ms, only 32^3 x 512 patches 2.21 -> 2.03 ms.  The fp32 kernel is MFMA-bound and
        // at its register limit; fewer staged bytes buy it nothing.)
    } else if (f32 && g.co == 8 && g.y_ld % 4 == 0 && g.x_ld % 4 == 0 && (g.ci % 16 == 0 || g.ci == 8)) {
        // wgrad6 with eight-channel operands: 16k -> 8 (dY columns paired over kw) and 8 -> 8 (X rows paired over (kd, kh) as well)
        p.kernel = WgradKernel::wgrad6;
        p.co8 = true, p.ci8 = g.ci == 8;
    } else if (quads && g.ci % 16 == 0) {
        p.kernel = f32 ? WgradKernel::wgrad6 : WgradKernel::wgrad4;
    } else if (quads) {
        p.kernel = WgradKernel::wgrad3;
    } else if (g.ci == 1) {
        // Conv3d(1, 8, 3) and the 1 -> 1 stencil have direct kernels in conv_generic.hip (conv_cin1_wgrad_kernel: 0.25 vs
        // 0.47 ms on 2 x 160x192x160; conv_c1c1_wgrad_kernel); Co = 16 stays here (0.22 vs 0.24 ms on 16 x 64^3)
        if ((g.co == 8 && g.y_ld % 4 == 0) || g.co == 1) return false;
        p.kernel = WgradKernel::cin1;
    } else return false;
    // per kernel: channels per chunk, tap groups, output tile (tasks = tiles), dynamic LDS without the reduction buffer (the
    // constant the kernel's own pointers are derived from)
    int td = WTD, th = WTH, tw = WTW;
    size_t lds = 0;
    p.CK = 16;
    p.TG = wg_tap_groups(16);
    switch (p.kernel) {
    case WgradKernel::cin1:
        p.CK = 1, p.TG = wg_tap_groups(1);
        lds = V1LDS;
        break;
    case WgradKernel::wgrad3:
        p.CK = 8, p.TG = wg_tap_groups(8);
        lds = V3LDS;
        break;
    case WgradKernel::wgrad4:
        th = V4TH;
        lds = V4LDS;
        break;
    case WgradKernel::bf16:
        td = BTD, th = BTH, tw = BTW;
        lds = BLDS;
        break;
    case WgradKernel::wgrad6:
        p.TG = wg6_groups(p.ci8, p.co8);
        td = BTD, th = BTH, tw = FTW;
        lds = BLDS;
        break;
    case WgradKernel::bf16t:   // tasks = (sample, segment of d, column): tilesD holds the segments
        td = p.segl, th = MTH, tw = BTW;
        lds = TLDS;
        break;
    }
    if (p.CK >= 4 && g.x_ld % 4 != 0) return false;
    p.CIT = cdiv(g.ci, p.CK);
    p.COB = cdiv(g.co, 16);
    p.td = td, p.th = th, p.tw = tw;
    p.tilesD = cdiv(g.di, td);
    p.tilesH = cdiv(g.hi, th);
    p.tilesW = cdiv(g.wi, tw);
    int64_t nt = (int64_t)g.n * p.tilesD * p.tilesH * p.tilesW;
    if (nt > 0x7fffffff) return false;
    p.ntiles = (int)nt;
    int pairs = p.CIT * p.COB;
    if (pairs > 65535) return false;
    int P = 512 / pairs;  // ~2 resident workgroups per CU in total
    if (P < 1) P = 1;
    if (P > p.ntiles) P = p.ntiles;
    p.P = P;
    p.part_floats = (size_t)P * p.CIT * p.COB * (p.TG + 1) * 256;
    p.smem = std::max(lds, (size_t)(p.TG + 1) * 256 * sizeof(float));   // the waves' partials are combined through the same LDS
    return true;
}

// ---- what conv_mfma.hip's queries over all passes answer with for the weight gradient: read from the plan the launch reads
// split > 0: ... and with that split operand (its own divisibility and pitch are checked by conv_mfma_cat_supported)
bool conv_mfma_wgrad_supported(const Mri3dConvGeom& g, int split, int /* second_ld: no kernel adds a condition on the pitch */) {
    MfmaWgradPlan q;
    if (!mfma_wgrad_plan(g, q)) return false;
    return split <= 0 || (q.takes_split() && (!q.second_needs_16_channels() || (g.ci - split) % 16 == 0));
}

size_t conv_mfma_wgrad_workspace_bytes(const Mri3dConvGeom& g) {
    MfmaWgradPlan q;
    return mfma_wgrad_plan(g, q) ? q.part_floats * sizeof(float) : 0;
}

// the kernel and the template arguments that select code in it (conv_mfma_route_name)
bool conv_mfma_wgrad_route_name(const Mri3dConvGeom& g, char* name, size_t name_bytes) {
    MfmaWgradPlan q;
    if (!mfma_wgrad_plan(g, q)) return false;
    switch (q.kernel) {
    case WgradKernel::cin1: snprintf(name, name_bytes, "cin1"); break;
    case WgradKernel::wgrad3: snprintf(name, name_bytes, "wgrad3"); break;
    case WgradKernel::wgrad4: snprintf(name, name_bytes, "wgrad4"); break;
    case WgradKernel::bf16: snprintf(name, name_bytes, "bf16"); break;
    case WgradKernel::wgrad6: snprintf(name, name_bytes, "wgrad6%s%s", q.ci8 ? " ci8" : "", q.co8 ? " co8" : ""); break;
    case WgradKernel::bf16t: snprintf(name, name_bytes, "bf16t"); break;
    }
    return true;
}

// the numbers of the launch (mri3d_conv3d_mfma_plan_query), from the plan the launch reads
bool conv_mfma_wgrad_plan_info(const Mri3dConvGeom& g, Mri3dConvMfmaPlanInfo& out) {
    MfmaWgradPlan q;
    if (!mfma_wgrad_plan(g, q)) return false;
    Mri3dConvMfmaPlanInfo o{};
    switch (q.kernel) {
    case WgradKernel::cin1: o.kernel = MRI3D_MFMA_CIN1; break;
    case WgradKernel::wgrad3: o.kernel = MRI3D_MFMA_WGRAD3; break;
    case WgradKernel::wgrad4: o.kernel = MRI3D_MFMA_WGRAD4; break;
    case WgradKernel::bf16: o.kernel = MRI3D_MFMA_BF16; break;
    case WgradKernel::wgrad6: o.kernel = MRI3D_MFMA_WGRAD6; break;
    case WgradKernel::bf16t: o.kernel = MRI3D_MFMA_BF16T; break;
    }
    o.ck = q.CK, o.chunks = q.CIT, o.partial_chunk = g.ci % q.CK != 0;
    o.tile_d = q.td, o.tile_h = q.th, o.tile_w = q.tw;
    o.tiles_d = q.tilesD, o.tiles_h = q.tilesH, o.tiles_w = q.tilesW, o.ntiles = q.ntiles, o.units = q.ntiles;
    o.cit = q.CIT, o.cob = q.COB, o.tg = q.TG, o.p = q.P, o.ci8 = q.ci8, o.co8 = q.co8, o.segl = q.segl;
    o.grid = q.P * q.CIT * q.COB;
    if (q.kernel == WgradKernel::cin1) {   // contiguous ranges [ntiles * b / P, ntiles * (b + 1) / P), not tile_walk
        o.max_tasks = 0, o.min_tasks = q.ntiles;
        for (int b = 0; b < q.P; ++b) {
            const int n = (int)(((int64_t)q.ntiles * (b + 1)) / q.P) - (int)(((int64_t)q.ntiles * b) / q.P);
            o.max_tasks = std::max(o.max_tasks, n), o.min_tasks = std::min(o.min_tasks, n);
        }
    } else {
        const WalkCounts wc = xcd_walk_counts(q.P, q.CIT * q.COB, q.ntiles);
        o.max_tasks = wc.max_tasks, o.min_tasks = wc.min_tasks;
    }
    // every wave owns a quarter of a tile's voxels (cin1, wgrad3, wgrad4: one of 2 x 2 (d, h) halves; the others: a quarter of the
    // rows), each one product of every accumulator element, padding included
    o.chain = (int)std::min<int64_t>((int64_t)o.max_tasks * q.td * q.th * q.tw / 4, 0x7fffffff);
    o.workspace_bytes = (int64_t)(q.part_floats * sizeof(float));
    out = o;
    return true;
}

// One launch for every weight-gradient kernel: the common arguments, then the kernel's own (`tail`).  The kernel's dynamic-LDS
// limit is set once per kernel (the static of this instantiation), not per launch.
template <auto kern, typename T, typename... Tail>
static void launch_wgrad(const MfmaWgradPlan& p, const Mri3dConvGeom& g, const T* x, const T* dy, float* part, hipStream_t s, Tail... tail) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.smem);
    (void)attr;
    hipLaunchKernelGGL(kern, dim3(p.P, p.CIT, p.COB), dim3(256), p.smem, s, x, dy, part, g.n, g.di, g.hi, g.wi, g.ci, g.x_ld, g.co, g.y_ld,
                       p.tilesD, p.tilesH, p.tilesW, p.ntiles, tail...);
}

// Calls f with std::true_type / std::false_type for `bias`: the kernel templates reserve the bias accumulator slot in the partial
// layout (TGA = TG + 1) only with BIAS.
template <typename F>
static void with_bias(bool bias, F f) {
    if (bias) f(std::true_type{});
    else f(std::false_type{});
}

// `if constexpr` keeps the kernels of the other storage type from being instantiated.  The bias is chosen per kernel, and the
// cases stand in the order in which the kernels have always been instantiated: that is their order in the code object.
template <typename T>
static void run_mfma_wgrad(const MfmaWgradPlan& p, const Mri3dConvGeom& g, const T* x, const T* dy, float* part, bool bias, hipStream_t s,
                           const ConvSplit& sp) {
    [[maybe_unused]] const T* x2 = static_cast<const T*>(sp.second);
    switch (p.kernel) {
    case WgradKernel::bf16t:
        if constexpr (sizeof(T) == 2) with_bias(bias, [&](auto B) { launch_wgrad<conv_mfma_wgrad_bf16t_kernel<B.value>>(p, g, x, dy, part, s, x2, sp.second_ld, sp.split, p.segl); });
        break;
    case WgradKernel::bf16:
        if constexpr (sizeof(T) == 2) with_bias(bias, [&](auto B) { launch_wgrad<conv_mfma_wgrad_bf16_kernel<B.value>>(p, g, x, dy, part, s, x2, sp.second_ld, sp.split); });
        break;
    case WgradKernel::wgrad6:
        if constexpr (sizeof(T) == 4) with_bias(bias, [&](auto B) {
            if (p.ci8 && p.co8) launch_wgrad<conv_mfma_wgrad6_kernel<B.value, true, true>>(p, g, x, dy, part, s, x2, sp.second_ld, sp.split);
            else if (p.co8) launch_wgrad<conv_mfma_wgrad6_kernel<B.value, false, true>>(p, g, x, dy, part, s, x2, sp.second_ld, sp.split);
            else if (p.ci8) launch_wgrad<conv_mfma_wgrad6_kernel<B.value, true, false>>(p, g, x, dy, part, s, x2, sp.second_ld, sp.split);
            else launch_wgrad<conv_mfma_wgrad6_kernel<B.value, false, false>>(p, g, x, dy, part, s, x2, sp.second_ld, sp.split);
        });
        break;
    case WgradKernel::wgrad4:   // fp32 tensors with Cin % 16 == 0 always take wgrad6
        if constexpr (sizeof(T) == 2) with_bias(bias, [&](auto B) { launch_wgrad<conv_mfma_wgrad4_kernel<B.value>>(p, g, x, dy, part, s); });
        break;
    case WgradKernel::wgrad3: with_bias(bias, [&](auto B) { launch_wgrad<conv_mfma_wgrad3_kernel<T, B.value>>(p, g, x, dy, part, s); }); break;
    case WgradKernel::cin1: with_bias(bias, [&](auto B) { launch_wgrad<conv_mfma_wgrad_cin1_kernel<T, B.value>>(p, g, x, dy, part, s); }); break;
    }
}

static int run_wgrad(const Mri3dConvGeom& g, const void* x, const void* dy, float* dw, float* dbias, void* ws, size_t ws_bytes,
                     hipStream_t s, ConvSplit sp) {
    MfmaWgradPlan p;
    MRI3D_REQUIRE(mfma_wgrad_plan(g, p), MRI3D_ENOTSUP, "conv3d_wgrad(mfma): unsupported geometry");
    MRI3D_REQUIRE(ws && ws_bytes >= p.part_floats * sizeof(float), MRI3D_EWORKSPACE,
                  "conv3d_wgrad(mfma): workspace %zu < %zu", ws_bytes, p.part_floats * sizeof(float));
    MRI3D_REQUIRE(aligned_vec4(g.dtype, x, dy), MRI3D_EINVAL, "conv3d_wgrad(mfma): x/dy must be aligned to 4 elements");
    MRI3D_REQUIRE(!p.needs_16_byte_alignment() || aligned16(x, dy), MRI3D_EINVAL, "conv3d_wgrad(bf16 mfma): x/dy must be 16-byte aligned");
    float* part = static_cast<float*>(ws);
    const bool bias = dbias != nullptr;
    MRI3D_REQUIRE(sp.second == nullptr || p.takes_split(), MRI3D_ENOTSUP, "conv3d_wgrad(mfma): split operands need the transposed-tile kernels");
    MRI3D_DISPATCH_DTYPE(g.dtype, T, { run_mfma_wgrad<T>(p, g, static_cast<const T*>(x), static_cast<const T*>(dy), part, bias, s, sp); });
    const int TGA = p.TG + (bias ? 1 : 0);
    const int nelem = p.CIT * p.COB * TGA * 256;
    hipLaunchKernelGGL(wgrad_mfma_reduce_kernel, dim3(cdiv(nelem, 64)), dim3(256), 0, s, part, dw, dbias, p.P, p.CIT,
                       p.COB, p.CK, p.TG, TGA, g.ci, g.co, (p.ci8 ? 1 : 0) | (p.co8 ? 2 : 0));
    return check_launch("conv3d_wgrad(mfma)");
}

int conv_mfma_wgrad(const Mri3dConvGeom& g, const void* x, const void* dy, float* dw, float* dbias, void* ws,
                    size_t ws_bytes, hipStream_t s) {
    return run_wgrad(g, x, dy, dw, dbias, ws, ws_bytes, s, ConvSplit{});
}

int conv_mfma_wgrad_cat(const Mri3dConvGeom& g, const void* x, const void* x2, int split, int x2_ld, const void* dy, float* dw,
                        float* dbias, void* ws, size_t ws_bytes, hipStream_t s) {
    return run_wgrad(g, x, dy, dw, dbias, ws, ws_bytes, s, ConvSplit{x2, split, x2_ld});
}

}  // namespace mri3d
