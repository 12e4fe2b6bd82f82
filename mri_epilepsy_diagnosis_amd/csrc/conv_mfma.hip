// conv_mfma.hip — implicit-GEMM Conv3d 3x3x3 / stride 1 / pad 1 / dilation 1 on the fp32-input MFMA
// (v_mfma_f32_16x16x4_f32: exact fp32 fmaf chains at 157 TFLOP/s peak, the fp32 roof of gfx950), for the hot layers
// of the U-Net: forward and data-gradient (the same kernel on flipped/transposed weights).  The weight gradient of the same
// layers is in conv_mfma_wgrad.hip.
//
//   forward   Y[v, co] = sum_{tap, ci} X[v + tap - 1, ci] * W[co, ci, tap]          GEMM  M = voxels, N = co, K = 27*ci
//   dgrad     dX[v, ci] = sum_{tap, co} dY[v + 1 - tap, co] * W[co, ci, tap]        same kernel, K = 27*co, N = ci
//
// Data layout in HBM: NDHWC activations (voxel pitch ld), so the K = ci fibre of a voxel is contiguous.
// LDS: one workgroup stages the (4+2) x (8+2) x (16+2) input halo tile of a 16- (or 8-) channel chunk, [voxel][ci].
// MFMA mapping (forward): an M-tile is 16 consecutive voxels along W; lane l supplies A[i = l&15][k-group = l>>4].
//   The K order inside a 16-channel chunk is permuted so that k-group g owns channels 4g..4g+3: one ds_read_b128 per
//   lane feeds four consecutive MFMA k-steps (step s takes element s).  The packed weight image applies the same
//   permutation, and is laid out so that each wave reads its B fragments as one contiguous 1 KiB global load.
//   With 8-channel chunks two taps share a k-step (k-groups 0,1 = tap 2t, k-groups 2,3 = tap 2t+1).
// A wave owns one d-plane of the tile = 8 M-tiles x NT N-tiles of 16 output channels (8*NT accumulators of 4 VGPRs),
// so every B fragment is reused 8x and every A fragment NT x.
//
// Roofline: compute-bound for Cin*Cout >= 8*16 (AI 72..270 FLOP/B vs ridge ~20): the bound is the fp32
// MFMA peak; algorithmic FLOPs = 2 * N*D*H*W * Cin * Cout * 27 per pass.
#include "common.h"
#include "conv_backends.h"
#include "mfma_util.h"
#include <stdlib.h>
#include <type_traits>

namespace mri3d {

constexpr int TD = 4, TH = 8, TW = 16;               // output tile (d, h, w)
constexpr int HD = TD + 2, HH = TH + 2, HW = TW + 2;  // halo tile
constexpr int HVOX = HD * HH * HW;                   // 1080 voxels

__host__ __device__ constexpr int tap_groups(int CK) { return CK == 16 ? 27 : 14; }

// Tap pairing of the two-taps-per-k-step kernels (8-channel fp32 chunks, 16-channel bf16 chunks): tap group tg carries taps
// pair_tap(tg, 0) in k-groups 0,1 and pair_tap(tg, 1) in k-groups 2,3 (27 = padding, zero weights).  The pairs are chosen so
// that the three groups of a CLASS differ only in kh, i.e. by ONE ROW of the halo tile:
//   groups 3c+kh (c = kd = 0..2):  (kd, kh, 0) | (kd, kh, 1)          groups 9+kh:  (0, kh, 2) | (1, kh, 2)
//   group 12:  (2, 0, 2) | (2, 1, 2)                                  group 13:     (2, 2, 2) | padding
// A-fragment (voxel rows) of group (class, kh), output row m == fragment of group (class, 0), row m + kh, so a wave needs 10
// LDS fragments per class instead of 3 x 8 (conv_mfma_fwd2_kernel, one N-tile): 56 instead of 112 ds_read_b128 per chunk.
// Group 13 is paired like this in the bf16 image only (one K = 32 step either way).  In the fp32 images it is a SINGLE group, as
// in conv_march.hip: the eight channels of tap (2, 2, 2) spread over all four k-groups, so the group is two K = 4 steps instead
// of four that are half zeros — 54 instead of 56 k-steps per row and chunk.  The MFMA adds its four products to the accumulator
// one after the other in k order, so WHICH channel sits in which k-group decides the bits of the sum: single_chan() keeps the
// order in which the paired form added the eight channels (0, 4, 1, 5, 2, 6, 3, 7; its zero products changed nothing), and the
// results stay what they were, bit for bit.
__host__ __device__ constexpr int pair_tap(int tg, int half) {
    return tg < 9 ? ((tg / 3) * 3 + tg % 3) * 3 + half
                  : (tg < 12 ? (half * 3 + (tg - 9)) * 3 + 2 : (tg == 12 ? (6 + half) * 3 + 2 : (half == 0 ? 26 : 27)));
}
// channel (within the 8-channel chunk) of k-group g in k-step s (0, 1) of the fp32 single group
__host__ __device__ constexpr int single_chan(int g, int s) { return 2 * s + (g >> 1) + 4 * (g & 1); }

// ------------------------------------------------------------------ weight packing
// Wp[chunk][tg][nt][lane][s]:  value = W'(tap, kc, nc) with
//   nc = nt*16 + (lane & 15)
//   CK == 16: tap = tg,                 kc = chunk*16 + 4*(lane>>4) + s
//   CK ==  8: tap = pair_tap(tg, lane>>5), kc = chunk*8  + 4*((lane>>4)&1) + s   (tap 27 -> 0)
//             tg == 13 (the single group): tap = 26, kc = chunk*8 + single_chan(lane>>4, s) for s < 2; s = 2, 3 are zero, never read
//   forward: W'(tap,kc,nc) = W[nc][kc][tap];  dgrad: W'(tap,kc,nc) = W[kc][nc][26 - tap]
__global__ void pack_w_mfma_kernel(const float* __restrict__ w, float* __restrict__ wp, int Co, int Ci, int dgrad,
                                   int CK, int NTT, int nchunks) {
    const int TG = tap_groups(CK);
    const int total = nchunks * TG * NTT * 256;
    const int Kc = dgrad ? Co : Ci, Nc = dgrad ? Ci : Co;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int s = i & 3, lane = (i >> 2) & 63;
        int t = i >> 8;
        int nt = t % NTT;
        t /= NTT;
        int tg = t % TG;
        int chunk = t / TG;
        int nc = nt * 16 + (lane & 15);
        int tap, kc;
        if (CK == 16) {
            tap = tg;
            kc = chunk * 16 + 4 * (lane >> 4) + s;
        } else if (tg == 13) {
            tap = s < 2 ? 26 : 27;
            kc = chunk * 8 + single_chan(lane >> 4, s & 1);
        } else {
            tap = pair_tap(tg, lane >> 5);
            kc = chunk * 8 + 4 * ((lane >> 4) & 1) + s;
        }
        float v = 0.f;
        if (tap < 27 && nc < Nc && kc < Kc) {
            v = dgrad ? w[((size_t)kc * Ci + nc) * 27 + (26 - tap)] : w[((size_t)nc * Ci + kc) * 27 + tap];
        }
        wp[i] = v;
    }
}

// bf16 image for the 16x16x32 MFMA (conv_mfma_fwd2_kernel<bf16_t>): a 32-byte voxel slice holds 16 channels, so a
// chunk is 16 channels and a lane's 16-byte fragment is 8 consecutive channels of one tap:
//   Wp[chunk][tg][nt][lane][s], s = 0..7:  tap = pair_tap(tg, lane>>5), kc = chunk*16 + 8*((lane>>4)&1) + s  (tap 27 -> 0)
__global__ void pack_w_mfma_bf16_kernel(const float* __restrict__ w, bf16_t* __restrict__ wp, int Co, int Ci, int dgrad,
                                        int NTT, int nchunks) {
    constexpr int TG = 14;
    const int total = nchunks * TG * NTT * 512;
    const int Kc = dgrad ? Co : Ci, Nc = dgrad ? Ci : Co;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int s = i & 7, lane = (i >> 3) & 63;
        int t = i >> 9;
        const int nt = t % NTT;
        t /= NTT;
        const int tg = t % TG, chunk = t / TG;
        const int nc = nt * 16 + (lane & 15);
        const int tap = pair_tap(tg, lane >> 5);
        const int kc = chunk * 16 + 8 * ((lane >> 4) & 1) + s;
        float v = 0.f;
        if (tap < 27 && nc < Nc && kc < Kc)
            v = dgrad ? w[((size_t)kc * Ci + nc) * 27 + (26 - tap)] : w[((size_t)nc * Ci + kc) * 27 + tap];
        wp[i] = (bf16_t)v;
    }
}

// Weight image of the 8-output-channel variant (conv_mfma_fwd2_kernel<.., N8>): Wp[chunk][group 0..9][lane][s].  Row li of the
// operand = channel li & 7 of row half hs = li >> 3; k-slot ks = lane >> 5 as in the images above.
//   groups 2u, 2u+1 (class u = 0..3: k-slot taps (kd, kw) = (u, ks) for u < 3, (ks, 2) for u = 3):
//       2u   (PAIR)   kh = hs         2u+1 (SINGLE) kh = 2, row half 0 only
//   group 8: taps (kd 2, kh ks, kw 2), group 9: tap 26 — row half 0 only (the old groups 12 and 13).  Group 9 holds tap 26 in
//   k-slot 0 in the bf16 image; in the fp32 image it is the single group of pack_w_mfma_kernel: elements s < 2 are channels
//   chunk*8 + single_chan(lane>>4, s), elements 2, 3 are zero
template <typename WT>
__global__ void pack_w_mfma_n8_kernel(const float* __restrict__ w, WT* __restrict__ wp, int Co, int Ci, int dgrad, int nchunks) {
    constexpr int PE = 16 / sizeof(WT);   // elements per lane fragment (4 fp32 / 8 bf16)
    const int total = nchunks * 10 * 64 * PE;
    const int Kc = dgrad ? Co : Ci;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int sidx = i % PE, lane = (i / PE) & 63;
        int t = i / (PE * 64);
        const int grp = t % 10, chunk = t / 10;
        const int li = lane & 15, nc = li & 7, hs = li >> 3, ks = lane >> 5;
        int kc = chunk * 2 * PE + PE * ((lane >> 4) & 1) + sidx;
        int tap = -1;
        if (grp < 8) {
            const int u = grp >> 1, single = grp & 1;
            const int kd = u < 3 ? u : ks, kw = u < 3 ? ks : 2;
            const int kh = single ? 2 : hs;
            if (!(single && hs)) tap = (kd * 3 + kh) * 3 + kw;
        } else if (grp == 8) {
            if (!hs) tap = (2 * 3 + ks) * 3 + 2;
        } else if constexpr (std::is_same<WT, float>::value) {
            if (!hs && sidx < 2) tap = 26;
            kc = chunk * 8 + single_chan(lane >> 4, sidx & 1);
        } else {
            if (!hs && ks == 0) tap = 26;
        }
        float v = 0.f;
        if (tap >= 0 && kc < Kc) v = dgrad ? w[((size_t)kc * Ci + nc) * 27 + (26 - tap)] : w[((size_t)nc * Ci + kc) * 27 + tap];
        wp[i] = (WT)v;
    }
}

#if defined(MRI3D_EXPERIMENT_STAMPS)   // tuning builds: in-kernel phase stamps of wave 0 of workgroup 0 (cdna_hip_programming.md §7)
__device__ unsigned long long g_stamps[8];
__device__ unsigned long long g_block_span[2 * 1024];   // per workgroup of the LAST launch: 100 MHz ticks at loop entry and exit
extern "C" void mri3d_debug_stamps(unsigned long long* out, int reset) {
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z));
    } else {
        (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 8);
    }
}
extern "C" void mri3d_debug_block_spans(unsigned long long* out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_block_span), sizeof(unsigned long long) * 2 * 1024);
}
// the phase sums stay in (scalar) registers until the kernel's end: a stamp must not add memory operations or waits to the loop
// (a stamp is pinned by scheduling barriers: s_memtime depends on nothing, and hipcc otherwise moves it across the MFMAs it brackets)
#define MRI3D_STAMP(var)                     \
    __builtin_amdgcn_sched_barrier(0);       \
    unsigned long long var = __builtin_readcyclecounter(); \
    __builtin_amdgcn_sched_barrier(0)
#define MRI3D_STAMP_ADD(slot, a, b) (stamp_acc[slot] += (b) - (a))
#else
#define MRI3D_STAMP(var)
#define MRI3D_STAMP_ADD(slot, a, b)
#endif

// ------------------------------------------------------------------ forward / dgrad kernel
// Persistent workgroups + double-buffered LDS + staging folded into the tap loop.
//   A first version (round 1, removed) alternated "stage a chunk" and "27 tap groups of MFMA" with a barrier pair in between; the two
//   workgroups resident on a CU ran in lock-step, so the staging time (1.0 of 4.1 ms on the 48->16 layer, measured by
//   ablation) was NOT hidden.  This kernel makes each workgroup self-overlapping:
//     * K is consumed in 8-channel chunks (two taps share an MFMA k-step: 14 tap groups per chunk), so TWO halo tiles
//       fit in LDS (2 x 34.5 KB) with two workgroups per CU;
//     * while chunk i is multiplied out of buffer i&1, every lane also fetches its 9 16-byte pieces of chunk i+1 (of the
//       same tile or the next one of this workgroup's range) — one global load per tap group, written to buffer
//       (i+1)&1 three tap groups later — so global latency, LDS writes and MFMAs overlap; one barrier per chunk;
//     * operands are passed to the MFMA as (weights, voxels): the accumulator then holds 4 consecutive output channels
//       of one voxel per lane and the epilogue is a fully coalesced 16-byte store per lane (1 KiB per wave).
constexpr int kStg = (HVOX * 2 + 255) / 256;  // 16-byte staging pieces per lane per 8-channel chunk (9)

#ifndef MRI3D_DMA_PPT
#define MRI3D_DMA_PPT 1   // DMA pieces issued per tap group (9 pieces per chunk)
#endif

// T = float: 8-channel chunks, four 16x16x4 fp32 MFMAs per tap group.  T = bf16_t: the SAME byte geometry (a 32-byte voxel
// slice = 16 channels, 16-byte pieces, identical staging and LDS addressing) with one v_mfma_f32_16x16x32_bf16 per tap
// group; the kernel is then bound by the LDS operand reads (the bf16 3x3x3 layers are memory-bound).
// `wp` is the packed weight image (fp32 or bf16), addressed in 16-byte fragments.
// STATS (forward only): the epilogue also accumulates, per output channel, sum(a) and sum(a^2) of the convolution result a
// WITHOUT its bias over the voxels of the volume — the BatchNorm batch statistics of y = a + bias (shift = bias), so that the
// statistics pass over y (one full read of every conv output, 0.5 ms per step of the U-Net) is not needed.  fp32 over a wave's
// 8 x 16 voxels of a tile, float64 from there on: per wave in LDS, one partial per workgroup in `stat_part`
// [gridDim.x][Nc][2], summed in a fixed order by norm_stats_finalize_kernel (deterministic: the tile -> workgroup map is static).
// N8 (exactly 8 output channels: the first level of Modified3DUNet, modified_3dunet.py:33-55, and the 8 -> 16 data gradient of
// the U-Net): a 16-row weight operand would be half zeros.  Its rows 8..15 take the SAME channels for the tap one halo row further
// (kh + 1) instead: with the voxel fragment of halo row i, rows 0..7 add to output row i (tap kh) and rows 8..15 to output row
// i - 1 (tap kh + 1).  A class of three tap groups (kh = 0, 1, 2: 3 x 8 row-MFMAs) becomes a PAIR group over halo rows 0..8 and
// a SINGLE group (kh = 2) over rows 2..9: 17 row-MFMAs; 84 instead of 112 per chunk.  Nine accumulators (halo rows 0..8); the
// epilogue adds the upper half of accumulator r + 1 (lanes 32..63) to the lower half of accumulator r (lanes 0..31).
// Packed weights: pack_w_mfma_n8_kernel, 10 groups per chunk.
template <typename T, int NT, bool STATS, bool N8 = false>
__global__ void __launch_bounds__(256, 2)
conv_mfma_fwd2_kernel(const T* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                      T* __restrict__ y, int N, int D, int H, int W, int Kc, int x_ld, int Nc, int y_ld, int NTT,
                      int gy, int tilesD, int tilesH, int tilesW, int ntiles, double* __restrict__ stat_part,
                      const T* __restrict__ x2, int x2_ld, int ksplit, T* __restrict__ y2, int y2_ld, int nsplit) {
    // x2 (forward of a conv over cat((x, x2), channels)): input channels >= ksplit live in the second tensor with its own pitch —
    // a chunk's DMA resource is simply based in the tensor that holds it, so torch.cat never materialises (unet.UNet decoder,
    // segmentation/routine.py:346-356).  y2 (its data gradient): output channels >= nsplit are written to the second tensor, so
    // both gradients come out dense.  ksplit, nsplit are multiples of 16; x2 = y2 = nullptr: one tensor each.
    constexpr bool kBf16 = sizeof(T) == 2;
    constexpr int CK = 32 / sizeof(T);   // channels per 32-byte chunk (8 fp32 / 16 bf16)
    constexpr int PE = 16 / sizeof(T);   // channels per 16-byte piece
    constexpr int CP = 8, TG = N8 ? 10 : 14;   // CP: LDS voxel pitch in floats (32 bytes); TG: weight fragments (groups) per chunk
    static_assert(!N8 || (NT == 1 && !STATS), "the 8-channel variant has one N-tile and no fused statistics");
    constexpr int AR = TH + (N8 ? 1 : 0);      // accumulator rows
    constexpr int BUF = kStg * 256 * 4;  // floats per LDS buffer: the halo tile rounded up to kStg 16-byte pieces per lane
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform BY CONSTRUCTION: told to hipcc, so that everything
                                                               // derived from it (output plane, tile base pointers) stays scalar
    const int li = lane & 15, kq = lane >> 4;
    const int nchunks = (Kc + CK - 1) / CK;   // bf16 with Kc % 16 == 8: the last chunk's upper piece is zero-filled
    // Tile -> workgroup map (speed only): blocks b and b+8 share an XCD (round-robin dispatch), so XCD k = b & 7 owns the
    // contiguous tile range [ntiles*k/8, ntiles*(k+1)/8) and its workgroups take those tiles round-robin: at any moment
    // the ~64 workgroups of an XCD work on ~64 CONSECUTIVE tiles, whose shared halo voxels then hit that XCD's L2
    // instead of being re-fetched over the fabric.
    const int NX = gridDim.x < 8 ? (int)gridDim.x : 8;                  // XCD groups that actually received a block
    const int xcd = blockIdx.x % NX, wslot = blockIdx.x / NX;
    const int wper = ((int)gridDim.x - xcd + NX - 1) / NX;             // workgroups living on this XCD
    const int r_lo = (int)(((int64_t)ntiles * xcd) / NX), r_hi = (int)(((int64_t)ntiles * (xcd + 1)) / NX);
    const int my_tiles = (r_hi - r_lo - wslot + wper - 1) / wper;      // tiles r_lo + wslot + k * wper < r_hi
    const int nitems = (r_lo + wslot < r_hi ? my_tiles : 0) * nchunks;
    double* const stat_lds = reinterpret_cast<double*>(lds + 2 * BUF);   // [4 waves][NTT * 16 channels][2]
    if constexpr (STATS) {
        if (nitems <= 0) {   // a workgroup without tiles still owns a partial: zeros
            for (int i = tid; i < Nc * 2; i += 256) stat_part[(size_t)blockIdx.x * Nc * 2 + i] = 0.0;
            return;
        }
        for (int i = tid; i < 4 * NTT * 16 * 2; i += 256) stat_lds[i] = 0.0;   // visible after the prologue's barrier
    }
    if (nitems <= 0) return;

    // per-lane staging geometry (independent of the item): piece j covers halo voxel (j*256+tid)>>1, channel quad &1
    // (pieces past the tile's end alias voxel 0 and land in the buffer's padding: no lane ever branches)
    int srel[kStg];  // packed (dz, hy, wx)
#pragma unroll
    for (int j = 0; j < kStg; ++j) {
        const int idx = j * 256 + tid;
        const int v = idx < HVOX * 2 ? idx >> 1 : 0;
        const int wx = v % HW, t2 = v / HW;
        srel[j] = ((t2 / HH) << 16) | ((t2 % HH) << 8) | wx;
    }
    // ... and its BYTE offset from the item's halo origin (voxel (d0-1, h0-1, w0-1), channel ch*CK): the DMA's buffer resource
    // is based at that origin, so an in-volume piece's offset is this per-lane constant — no per-piece integer multiplies,
    // clamps or 64-bit arithmetic — and an out-of-volume piece gets the out-of-range offset that makes the DMA write zeros.
    unsigned vrel[kStg];   // voxel index relative to the halo origin; byte offset = vrel * pitch bytes + the lane's piece (one v_mad)
#pragma unroll
    for (int j = 0; j < kStg; ++j) {
        const int r = srel[j];
        vrel[j] = (unsigned)(((r >> 16) * H + ((r >> 8) & 0xff)) * W + (r & 0xff));
    }
    const unsigned pieceb = (unsigned)(PE * (tid & 1)) * (unsigned)sizeof(T);

    struct Item { int n, d0, h0, w0, nt0, ch; };
    auto decode = [&](int it) -> Item {
        Item r;
        int tile = r_lo + wslot + (it / nchunks) * wper;
        r.ch = it % nchunks;
        r.nt0 = (tile % gy) * NT;
        tile /= gy;
        r.w0 = (tile % tilesW) * TW;
        tile /= tilesW;
        // tiles run w-fastest, then d, then h: the d-neighbours (which share 2 of 6 halo planes) are tilesW apart and run
        // side by side on one XCD; measured against (w, h, d): bf16 forward 48->16 0.658 -> 0.621 ms (profiles/r02_tile_order.txt)
        r.d0 = (tile % tilesD) * TD;
        tile /= tilesD;
        r.h0 = (tile % tilesH) * TH;
        r.n = tile / tilesH;

        return r;
    };
    // A workgroup's tiles are `wper` apart: the next tile's coordinates come from adding wper's mixed-radix digits (N-block, w, d,
    // h, n) with carries — ~15 scalar instructions instead of decode()'s five run-time divisions (~150).  Measured by ablation
    // (decode replaced by a constant): the divisions cost 5 % of the fp32 16 -> 16 forward, 12 % of 8 -> 16 and 22 % of the bf16
    // 16 -> 16 forward, whose tiles are a single chunk (one decode per item).
    int sdig[5];
    {
        int q = wper;
        sdig[0] = q % gy;
        q /= gy;
        sdig[1] = q % tilesW;
        q /= tilesW;
        sdig[2] = q % tilesD;
        q /= tilesD;
        sdig[3] = q % tilesH;
        sdig[4] = q / tilesH;
    }
    auto advance = [&](const Item& c) -> Item {   // chunk 0 of the tile `wper` after c's
        Item r;
        r.ch = 0;
        int a = c.nt0 / NT + sdig[0];
        int cy = a >= gy;
        r.nt0 = (a - (cy ? gy : 0)) * NT;
        a = c.w0 / TW + sdig[1] + cy;
        cy = a >= tilesW;
        r.w0 = (a - (cy ? tilesW : 0)) * TW;
        a = c.d0 / TD + sdig[2] + cy;
        cy = a >= tilesD;
        r.d0 = (a - (cy ? tilesD : 0)) * TD;
        a = c.h0 / TH + sdig[3] + cy;
        cy = a >= tilesH;
        r.h0 = (a - (cy ? tilesH : 0)) * TH;
        r.n = c.n + sdig[4] + cy;
        return r;
    };
    const unsigned lds_wave = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds + (unsigned)wv * 1024u);
    // Stage one item (a 32-byte channel chunk of a halo tile) into LDS buffer `bsel`: kStg DMA pieces per lane, piece j of lane
    // `tid` = 16-byte piece j*256 + tid of the [halo voxel][32 B] image — lane-linear, which is what an LDS-DMA writes.
    // Tiles whose halo lies inside the volume (70 % at 160x192x160) take the wave-uniform fast path: the offsets are the
    // per-lane constants, no VALU work at all.  (Pieces past the tile's end alias voxel 0 and land in the buffer's padding.)
    struct Stage { i32x4 rs; unsigned dst, ldb; bool interior, on; };
    auto stage_open = [&](const Item& it, int bsel, bool on) -> Stage {
        Stage st;
        const bool second = x2 != nullptr && it.ch * CK >= ksplit;   // wave-uniform: which tensor holds this chunk
        const T* xs = second ? x2 : x;
        const int ld = second ? x2_ld : x_ld, c0 = second ? it.ch * CK - ksplit : it.ch * CK;
        st.ldb = (unsigned)ld * (unsigned)sizeof(T);
        const unsigned long long org =
            (unsigned long long)(xs + (((((int64_t)it.n * D + it.d0 - 1) * H + it.h0 - 1) * W + it.w0 - 1) * ld + c0));
        // raw buffer resource: base (48 bits), stride 0, num_records, gfx9 raw-dword format
        st.rs[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)(org & 0xffffffffu));
        st.rs[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)((org >> 32) & 0xffffu));
        st.rs[2] = (int)kDmaRecords;
        st.rs[3] = 0x00020000;
        st.dst = lds_wave + (unsigned)bsel * (unsigned)(BUF * 4);
        st.interior = it.d0 >= 1 && it.d0 + TD < D && it.h0 >= 1 && it.h0 + TH < H && it.w0 >= 1 && it.w0 + TW < W &&
                      (it.ch + 1) * CK <= Kc;
        st.on = on;
        return st;
    };
    auto stage_piece = [&](const Item& it, const Stage& st, int j) {   // wave-uniform branches only
        if (!st.on) return;
        if (st.interior) {
            lds_dma16(__umul24(vrel[j], st.ldb) + pieceb, st.rs, st.dst + j * 4096);   // v_mad_u32_u24: both factors < 2^24
        } else {
            const int r = srel[j];
            const int gd = it.d0 - 1 + (r >> 16), gh = it.h0 - 1 + ((r >> 8) & 0xff), gw = it.w0 - 1 + (r & 0xff);
            const bool ok = (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W &&
                            it.ch * CK + PE * (tid & 1) < Kc;
            lds_dma16(ok ? __umul24(vrel[j], st.ldb) + pieceb : kDmaOob, st.rs, st.dst + j * 4096);
        }
    };
    // pieces issued in front of tap group tg: kPpt per group, so that a wave's issue slots (~60-180 cycles per piece) are
    // spread behind MFMAs instead of delaying the chunk's first fragments
    constexpr int kPpt = MRI3D_DMA_PPT;
    auto stage_group = [&](const Item& it, const Stage& st, int tg) {
#pragma unroll
        for (int j = tg * kPpt; j < (tg + 1) * kPpt && j < kStg; ++j) stage_piece(it, st, j);
    };
    auto weights_of = [&](const Item& it) -> const float* {
        return wp + ((size_t)it.ch * TG * NTT + it.nt0) * 256 + lane * 4;
    };
    const size_t wstep = (size_t)NTT * 256;

#if defined(MRI3D_EXPERIMENT_STAMPS)   // the clock the chip holds in this kernel: shader cycles / 100 MHz reference ticks
    const unsigned long long clk0 = __builtin_amdgcn_s_memtime(), ref0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    // prologue: item 0 -> buffer 0 (and, one N-tile: all 14 weight fragments of its chunk)
    Item cur = decode(0);
    f32x4 bqa[NT == 1 ? TG : 1];   // NT = 1: the weight fragments of the WHOLE chunk; fragment tg is re-loaded for the next item
                                   // right after tap group tg has used it — a full chunk of latency cover, and no weight load
                                   // ever queues behind the DMA pieces it does not depend on (VMEM returns in order)
    if constexpr (NT == 1) {
        const float* w0p = weights_of(cur);
#pragma unroll
        for (int tg = 0; tg < TG; ++tg) bqa[tg] = *reinterpret_cast<const f32x4*>(w0p + (size_t)tg * wstep);
    }
    {
        const Stage st0 = stage_open(cur, 0, true);
#pragma unroll
        for (int j = 0; j < kStg; ++j) stage_piece(cur, st0, j);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    f32x4 acc[AR][NT];
#pragma unroll
    for (int m = 0; m < AR; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[m][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 bias0[NT];   // the lane's bias quads when the kernel has one N-block (gy == 1: nt0 is always 0)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        bias0[nt] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int co = nt * 16 + 4 * kq;
        if (NT == 1 && bias && gy == 1 && co < Nc) {   // (two N-tiles: no registers to spare, the bias is loaded per tile)
            bias0[nt].x = bias[co];
            if (co + 1 < Nc) bias0[nt].y = bias[co + 1];
            if (co + 2 < Nc) bias0[nt].z = bias[co + 2];
            if (co + 3 < Nc) bias0[nt].w = bias[co + 3];
        }
    }
    // A-fragment LDS offsets of a tap group (k-groups 0,1 = pair_tap(tg, 0); k-groups 2,3 = pair_tap(tg, 1), tap 27 = zero weights)
    // fp32, group 13 (the single group, tap 26): k-group kq owns channels single_chan(kq, 0) and single_chan(kq, 1), two floats
    // apart (a_frag)
    auto a_off = [&](int tg) -> int {
        if (!kBf16 && tg == 13) return ((wv * HH) * HW + li + (2 * HH + 2) * HW + 2) * CP + single_chan(kq, 0);
        const int ta = pair_tap(tg, 0), tb = pair_tap(tg, 1) < 27 ? pair_tap(tg, 1) : 26;
        const int oa = ((ta / 9) * HH + (ta / 3) % 3) * HW + ta % 3;
        const int ob = ((tb / 9) * HH + (tb / 3) % 3) * HW + tb % 3;
        return ((wv * HH) * HW + li + ((kq >> 1) ? ob : oa)) * CP + 4 * (kq & 1);
    };
    // the voxel fragment of tap group tg at float offset `off` (a_off(tg) + rows) of a chunk's buffer: one ds_read_b128, or the
    // single group's two floats, one per k-step (elements 2, 3 of the result are never used): a ds_read2_b32, eight per wave and
    // chunk — the price of keeping the paired form's summation order (single_chan), against 8 x 16 MFMAs saved.
    auto a_frag = [&](const float* buf, int tg, int off) -> f32x4 {
        if (!kBf16 && tg == 13) {
            static_assert(single_chan(0, 1) - single_chan(0, 0) == 2 && single_chan(3, 1) - single_chan(3, 0) == 2, "k-step stride");
            return f32x4{buf[off], buf[off + 2], 0.f, 0.f};
        }
        return *reinterpret_cast<const f32x4*>(buf + off);
    };
    constexpr int kSingleSteps = kBf16 ? 4 : 2;   // fp32 k-steps of the single group (the bf16 paths do not use it)

    for (int it = 0; it < nitems; ++it) {
        MRI3D_STAMP(t_item);
        const float* bufc = lds + (it & 1) * BUF;
        const bool has_next = it + 1 < nitems;
        Item nxt = cur;
        // the next item is the next chunk of the same tile, or chunk 0 of this workgroup's next tile (advance(): digit adds)
        if (has_next) {
            if (cur.ch + 1 < nchunks) nxt.ch = cur.ch + 1;
            else nxt = advance(cur);
        }
        if constexpr (N8) {
            const Stage stn = stage_open(nxt, (it + 1) & 1, has_next);
            const float* wtn = weights_of(nxt);
            // units: four classes (a PAIR and a SINGLE group on one set of 10 row fragments), then the old groups 12 and 13
            constexpr int NU = 6;
            f32x4 fr[2][TH + 2];
            {
                const int o0 = a_off(0);
#pragma unroll
                for (int i = 0; i < TH + 2; ++i) fr[0][i] = *reinterpret_cast<const f32x4*>(bufc + o0 + i * HW * CP);
            }
#pragma unroll
            for (int g = 0; g < TG; ++g) {
                const int u = g < 8 ? g / 2 : g - 4, ng = u < 4 ? 2 : 1, gi = u < 4 ? g - 2 * u : 0;
                stage_group(nxt, stn, g);
                if (g >= 1) bqa[g - 1] = *reinterpret_cast<const f32x4*>(wtn + (size_t)(g - 1) * wstep);   // next item's
                if (u + 1 < NU) {   // this group's share of the next unit's fragments
                    const int nu = u + 1, nfirst = nu < 4 ? 3 * nu : nu + 8, nf = nu < 4 ? TH + 2 : TH;
                    const int on = a_off(nfirst);
#pragma unroll
                    for (int i = 0; i < TH + 2; ++i)
                        if (i >= gi * nf / ng && i < (gi + 1) * nf / ng) fr[nu & 1][i] = a_frag(bufc, nfirst, on + i * HW * CP);
                }
                __builtin_amdgcn_sched_barrier(0);  // keep the prefetches above this group's MFMAs
                // PAIR group: halo rows 0..8 -> accumulators 0..8; SINGLE group (kh = 2): halo rows 2..9 -> accumulators 0..7;
                // groups 8, 9: halo rows 0..7 -> accumulators 0..7
                const int r0 = (u < 4 && gi == 1) ? 2 : 0, nr = (u < 4 && gi == 0) ? TH + 1 : TH;
                if constexpr (kBf16) {
#pragma unroll
                    for (int m = 0; m < TH + 1; ++m)
                        if (m < nr)
                            acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bqa[g]),
                                                                                __builtin_bit_cast(bf16x8_t, fr[u & 1][m + r0]),
                                                                                acc[m][0], 0, 0, 0);
                } else {
#pragma unroll
                    for (int m = 0; m < TH; m += 2)
#pragma unroll
                        for (int s4 = 0; s4 < (g == 9 ? kSingleSteps : 4); ++s4) {   // group 9: the single group
                            acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(bqa[g][s4], fr[u & 1][m + r0][s4], acc[m][0], 0, 0, 0);
                            acc[m + 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(bqa[g][s4], fr[u & 1][m + 1 + r0][s4], acc[m + 1][0], 0, 0, 0);
                        }
                    if (nr == TH + 1) {
#pragma unroll
                        for (int s4 = 0; s4 < 4; ++s4)
                            acc[TH][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(bqa[g][s4], fr[u & 1][TH][s4], acc[TH][0], 0, 0, 0);
                    }
                }
            }
            bqa[TG - 1] = *reinterpret_cast<const f32x4*>(wtn + (size_t)(TG - 1) * wstep);
            if (cur.ch == nchunks - 1) {
                // fold: output row r = lower half of accumulator r + upper half (lanes 32..63 -> 0..31) of accumulator r + 1
#pragma unroll
                for (int m = 0; m < TH; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[m][0][r] += __shfl_down(acc[m + 1][0][r], 32, 64);
            }
        } else if constexpr (NT == 1) {
            // One N-tile: every A-fragment feeds a single MFMA chain, so the LDS reads are the largest non-MFMA cost.  The tap
            // groups come in UNITS: four classes of three groups that differ only by one halo row (pair_tap), then groups 12
            // and 13.  A class needs 10 row fragments (rows 0..9 of its kh = 0 group; group kh, output row m uses row m + kh)
            // instead of 3 x 8; the next unit's fragments are fetched while this unit is multiplied (two register sets).
            const Stage stn = stage_open(nxt, (it + 1) & 1, has_next);   // the next chunk: 9 DMA pieces per lane, landed by the barrier
            const float* wtn = weights_of(nxt);             // (the last item re-reads its own: the loads stay unconditional)
            constexpr int NU = 6;
            f32x4 fr[2][TH + 2];
            {
                const int o0 = a_off(0);
#pragma unroll
                for (int i = 0; i < TH + 2; ++i) fr[0][i] = *reinterpret_cast<const f32x4*>(bufc + o0 + i * HW * CP);
            }
#pragma unroll
            for (int tg = 0; tg < TG; ++tg) {
                const int u = tg < 12 ? tg / 3 : tg - 8, ufirst = u < 4 ? 3 * u : u + 8, ng = u < 4 ? 3 : 1;
                const int kh = tg - ufirst;   // row shift inside the class (0 for the single-group units)
                stage_group(nxt, stn, tg);
                if (tg >= 1) bqa[tg - 1] = *reinterpret_cast<const f32x4*>(wtn + (size_t)(tg - 1) * wstep);   // next item's
                if (u + 1 < NU) {   // this group's share of the next unit's fragments
                    const int nu = u + 1, nfirst = nu < 4 ? 3 * nu : nu + 8, nf = nu < 4 ? TH + 2 : TH;
                    const int on = a_off(nfirst);
#pragma unroll
                    for (int i = 0; i < TH + 2; ++i)
                        if (i >= kh * nf / ng && i < (kh + 1) * nf / ng) fr[nu & 1][i] = a_frag(bufc, nfirst, on + i * HW * CP);
                }
                __builtin_amdgcn_sched_barrier(0);  // keep the prefetches above this tap group's MFMAs
                if constexpr (kBf16) {
#pragma unroll
                    for (int m = 0; m < TH; ++m)
                        acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bqa[tg]),
                                                                            __builtin_bit_cast(bf16x8_t, fr[u & 1][m + kh]),
                                                                            acc[m][0], 0, 0, 0);
                } else {
                    // accumulator reuse distance 2 (two rows alternate over the four k-steps): the fp32 MFMA sustains its peak
                    // when an accumulator comes back after <= 3 or >= 16 instructions, not after 4..8 (tools/microbench); the
                    // single group's two k-steps keep that distance
#pragma unroll
                    for (int m = 0; m < TH; m += 2)
#pragma unroll
                        for (int s = 0; s < (tg == 13 ? kSingleSteps : 4); ++s) {
                            acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(bqa[tg][s], fr[u & 1][m + kh][s], acc[m][0], 0, 0, 0);
                            acc[m + 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(bqa[tg][s], fr[u & 1][m + 1 + kh][s], acc[m + 1][0], 0, 0, 0);
                        }
                }
            }
            bqa[TG - 1] = *reinterpret_cast<const f32x4*>(wtn + (size_t)(TG - 1) * wstep);
        } else {
        // Two N-tiles: a 3-deep ring of weight fragments (two tap groups of lead).  The ring is primed BEFORE the DMA pieces are
        // issued, so that the first tap group does not wait for them; the loads of tap groups 2.. queue behind the pieces,
        // which have two tap groups (fp32: 3 us) to land.
        const float* wt = weights_of(cur);
        f32x4 bq[3][NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            bq[0][nt] = *reinterpret_cast<const f32x4*>(wt + nt * 256);
            bq[1][nt] = *reinterpret_cast<const f32x4*>(wt + wstep + nt * 256);
        }
        const Stage stn = stage_open(nxt, (it + 1) & 1, has_next);
        f32x4 aq[2][TH];
        {
            const int o0 = a_off(0);
#pragma unroll
            for (int m = 0; m < TH; ++m) aq[0][m] = *reinterpret_cast<const f32x4*>(bufc + o0 + m * HW * CP);
        }
#pragma unroll
        for (int tg = 0; tg < TG; ++tg) {
            const int cb = tg % 3, nb = (tg + 2) % 3, ac = tg & 1, an = (tg + 1) & 1;
            stage_group(nxt, stn, tg);
            if (tg + 2 < TG) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    bq[nb][nt] = *reinterpret_cast<const f32x4*>(wt + (size_t)(tg + 2) * wstep + nt * 256);
            }
            if (tg + 1 < TG) {
                const int o1 = a_off(tg + 1);
#pragma unroll
                for (int m = 0; m < TH; ++m) aq[an][m] = a_frag(bufc, tg + 1, o1 + m * HW * CP);
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetches above this tap group's MFMAs
            if constexpr (kBf16) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int m = 0; m < TH; ++m)
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bq[cb][nt]),
                                                                             __builtin_bit_cast(bf16x8_t, aq[ac][m]),
                                                                             acc[m][nt], 0, 0, 0);
            } else {
#pragma unroll
                for (int s = 0; s < (tg == 13 ? kSingleSteps : 4); ++s)   // group 13: the single group
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int m = 0; m < TH; ++m)
                            acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[cb][nt][s], aq[ac][m][s], acc[m][nt], 0, 0, 0);
            }
        }
        }

        MRI3D_STAMP(t_mfma);
        MRI3D_STAMP_ADD(0, t_item, t_mfma);
        if (cur.ch == nchunks - 1) {
            // epilogue: lane holds channels 4*kq..4*kq+3 of voxel li of every 16x16 tile.  Everything that does not depend on the
            // lane is kept scalar — the output plane (wv is wave-uniform), which tensor an N-tile goes to, the tile's base pointer, the
            // row-in-volume tests — and the lane's own test (its channels and its voxel column exist) is made ONCE around the eight
            // rows: a one-chunk tile (every item of the 16-channel bf16 layers) pays this block per item.
            const int od = cur.d0 + wv;
            if (od < D) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int cob = (cur.nt0 + nt) * 16;   // wave-uniform
                    if (cob >= Nc) continue;
                    const bool second = y2 != nullptr && cob >= nsplit;   // nsplit % 16 == 0: an N-tile lives in one tensor
                    T* const yd = second ? y2 : y;
                    const int yld = second ? y2_ld : y_ld, cbase = second ? cob - nsplit : cob;
                    const int co = cob + 4 * kq;
                    const bool vec = (co + 3 < Nc) && ((yld & 3) == 0);
                    float4 bv = bias0[nt];   // one N-tile and one N-block: loaded once per kernel
                    if (bias && (NT > 1 || gy > 1) && co < Nc) {
                        bv = make_float4(0.f, 0.f, 0.f, 0.f);
                        bv.x = bias[co];
                        if (co + 1 < Nc) bv.y = bias[co + 1];
                        if (co + 2 < Nc) bv.z = bias[co + 2];
                        if (co + 3 < Nc) bv.w = bias[co + 3];
                    }
                    // consume the loads HERE on every path: a bias register still "pending" at the loop's back edge makes hipcc
                    // wait vmcnt(0) at its next reuse — at the top of the next item, right behind the freshly issued DMA pieces
                    if (bias && (NT > 1 || gy > 1)) asm volatile("" ::"v"(bv.x), "v"(bv.y), "v"(bv.z), "v"(bv.w));
                    // scalar 64-bit tile base + 32-bit lane / row offsets
                    T* const ytile = yd + (((((int64_t)cur.n * D + od) * H + cur.h0) * W + cur.w0) * yld + cbase);
                    const unsigned lane_off = (unsigned)(li * yld + 4 * kq), row_step = (unsigned)(W * yld);
                    if (co < Nc && cur.w0 + li < W) {
                        if ((Nc & 3) == 0 && (yld & 3) == 0) {   // wave-uniform: one vector store per row, nothing else
#pragma unroll
                            for (int m = 0; m < TH; ++m) {
                                if (cur.h0 + m < H) {   // wave-uniform
                                    const f32x4 a = acc[m][nt];
                                    stf4(ytile + (lane_off + (unsigned)m * row_step), make_float4(a[0] + bv.x, a[1] + bv.y, a[2] + bv.z, a[3] + bv.w));
                                }
                            }
                        } else {
#pragma unroll
                            for (int m = 0; m < TH; ++m) {
                                if (cur.h0 + m < H) {
                                    T* yp = ytile + (lane_off + (unsigned)m * row_step);
                                    const f32x4 a = acc[m][nt];
                                    if (vec) {
                                        stf4(yp, make_float4(a[0] + bv.x, a[1] + bv.y, a[2] + bv.z, a[3] + bv.w));
                                    } else {
                                        stf(yp, a[0] + bv.x);
                                        if (co + 1 < Nc) stf(yp + 1, a[1] + bv.y);
                                        if (co + 2 < Nc) stf(yp + 2, a[2] + bv.z);
                                        if (co + 3 < Nc) stf(yp + 3, a[3] + bv.w);
                                    }
                                }
                            }
                        }
                    }
                }
            }
            if constexpr (STATS) {
                const bool vok = cur.d0 + wv < D && cur.w0 + li < W;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int m = 0; m < TH; ++m) {
                        const bool ok = vok && cur.h0 + m < H;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float a = ok ? acc[m][nt][r] : 0.f;
                            s1[r] += a;
                            s2[r] += a * a;
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        s1[r] = row_sum16(s1[r]);
                        s2[r] = row_sum16(s2[r]);
                    }
                    if (li == 0) {   // one lane per k-group: channels 4*kq .. 4*kq+3 of this N-tile, this wave's own LDS slot
                        double* slot = stat_lds + ((size_t)wv * NTT * 16 + (cur.nt0 + nt) * 16 + 4 * kq) * 2;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            slot[2 * r] += (double)s1[r];
                            slot[2 * r + 1] += (double)s2[r];
                        }
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < AR; ++m)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[m][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // The DMA pieces of the next item are OLDER than the >= 12 weight loads issued after them in this iteration, and VMEM
        // returns in order: at most that many operations outstanding means every piece has landed in LDS.
        MRI3D_STAMP(t_epi);
        MRI3D_STAMP_ADD(1, t_mfma, t_epi);
        constexpr int kYounger = N8 ? 2 : 6;   // VMEM operations certainly issued after the last DMA piece (weight reloads)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kYounger) : "memory");
        MRI3D_STAMP(t_wait);
        MRI3D_STAMP_ADD(2, t_epi, t_wait);
        __syncthreads();  // buffer (it+1)&1 is complete; buffer it&1 may be overwritten from the next iteration on
        MRI3D_STAMP(t_bar);
        MRI3D_STAMP_ADD(3, t_wait, t_bar);
        MRI3D_STAMP_ADD(4, t_item, t_bar);
        MRI3D_STAMP_ADD(5, 0ull, 1ull);
        cur = nxt;
    }
#if defined(MRI3D_EXPERIMENT_STAMPS)
    {
        const unsigned long long clk1 = __builtin_amdgcn_s_memtime(), ref1 = __builtin_amdgcn_s_memrealtime();
        MRI3D_STAMP_ADD(6, clk0, clk1);
        MRI3D_STAMP_ADD(7, ref0, ref1);
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int i = 0; i < 8; ++i) g_stamps[i] += stamp_acc[i];
        if (threadIdx.x == 0 && blockIdx.x < 1024) {
            g_block_span[2 * blockIdx.x] = ref0;
            g_block_span[2 * blockIdx.x + 1] = ref1;
        }
    }
#endif
    if constexpr (STATS) {   // the loop ended with a barrier: combine the four waves in a fixed order, one partial per workgroup
        for (int i = tid; i < Nc * 2; i += 256) {
            const int c2 = i;   // (channel, stat) pair; LDS rows are NTT*16 channels wide
            double v = 0.0;
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) v += stat_lds[(size_t)w4 * NTT * 16 * 2 + c2];
            stat_part[(size_t)blockIdx.x * Nc * 2 + i] = v;
        }
    }
}

// ------------------------------------------------------------------ forward / dgrad without LDS: small volumes and strided layers
// The tiled kernel above needs thousands of 4x8x16 tiles to fill 512 workgroup slots and a stride of 1; the deep levels of
// Modified3DUNet (modified_3dunet.py:23-70: 64 -> 64 at 20x24x20, 128 -> 128 at 10x12x10, batch 1, and the four stride-2
// 3x3x3 layers between the levels), VoxResNet's stride-2 stem (cnn_model.py:49-81) and patch batches have neither, and ran on
// the direct (non-MFMA) kernels at 2 .. 13 TFLOP/s.  Here a WAVE is the unit: one M-tile of 16 voxels x NT N-tiles of 16 channels,
// the whole K = taps x Cin in one go, both operands straight from global memory (L2-resident at these sizes) — no LDS staging,
// no barriers, no tile waste.  Same operand order (weights, voxels), K permutation and epilogue as the tiled kernel; packed
// weights Wp[chunk16][tap][nt][lane][s] (pack_w_mfma_kernel, CK = 16).
//   MODE 0 (forward of a 3x3x3 / pad 1 / stride s layer; also the stride-1 data gradient = the forward of the flipped,
//           transposed weights on dY): the M-tile is 16 consecutive voxels of the flattened (n, od, oh, ow) OUTPUT index space;
//           tap (kd, kh, kw) reads input voxel (s*od - 1 + kd, ...), a constant element offset plus three range checks.
//   MODE 1 (data gradient of a stride-s layer, s > 1): dX[i] = sum over the taps with k = (i + 1) mod s of W[k] dY[(i + 1 - k)/s].
//           The M-tile is 16 input voxels of one (n, id, ih) row that share the residue of iw mod s, so the valid tap set —
//           1 .. 8 of the 27 — is wave-uniform: the tap loops just step by s and only the volume border is masked.
//   SPLIT: layers with fewer units than SIMDs give each unit to a whole workgroup: its four waves take the (kd, kh) pairs
//           round-robin and are summed through LDS in a fixed order (deterministic); otherwise a workgroup is four units.
// The loads of all kw taps of a (kd, kh) pair — up to 3 voxel fragments and 3 NT weight fragments per 16-channel chunk — are
// issued together before their MFMAs: a lone wave per SIMD then waits for L2 once per pair instead of once per MFMA group.
struct DirectGeom {
    int N, Di, Hi, Wi;   // the tensor the kernel READS (x, or dY for the gradients)
    int Do, Ho, Wo;      // the tensor it WRITES
    int s, Kc, in_ld, Nc, out_ld, NTT, gy, nmt, wbn;
};

template <typename T, int NT, int MODE, bool SPLIT>
__global__ void __launch_bounds__(256)
conv_mfma_direct_kernel(const T* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
                        T* __restrict__ out, const DirectGeom q) {
    __shared__ float red[SPLIT ? 3 * NT * 256 : 1];
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4, wv = threadIdx.x >> 6;
    const int unit = SPLIT ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    if (unit >= q.nmt * q.gy) return;   // SPLIT: whole workgroup; otherwise the wave (no barrier follows)
    const int ntb = unit % q.gy, mt = unit / q.gy;
    const int s = q.s;

    // the lane's voxel: where it writes, and the read-side coordinates of its taps
    bool vok;
    int64_t out_off;           // element offset of the lane's output voxel
    int n, c_d, c_h, c_w;      // MODE 0: input coordinates of tap (0,0,0); MODE 1: the input-gradient voxel (id, ih, iw)
    if (MODE == 0) {
        const int64_t nvox = (int64_t)q.N * q.Do * q.Ho * q.Wo;
        const int64_t v = (int64_t)mt * 16 + li;
        vok = v < nvox;
        const int64_t vc = vok ? v : nvox - 1;
        const int ow = (int)(vc % q.Wo);
        int64_t t = vc / q.Wo;
        const int oh = (int)(t % q.Ho);
        t /= q.Ho;
        const int od = (int)(t % q.Do);
        n = (int)(t / q.Do);
        c_d = od * s - 1, c_h = oh * s - 1, c_w = ow * s - 1;
        out_off = vc * q.out_ld;
    } else {
        int r = mt / q.wbn;
        const int wb = mt % q.wbn;
        const int rw = r % s;
        r /= s;
        c_h = r % q.Ho;
        r /= q.Ho;
        c_d = r % q.Do;
        n = r / q.Do;
        c_w = rw + s * (wb * 16 + li);
        vok = c_w < q.Wo;
        out_off = ((((int64_t)n * q.Do + c_d) * q.Ho + c_h) * q.Wo + (vok ? c_w : 0)) * q.out_ld;
    }
    const T* const in_n = in + (int64_t)n * q.Di * q.Hi * q.Wi * q.in_ld;   // sample base: always readable (Kc >= 8)
    const int nchunks = (q.Kc + 15) / 16;
    const int nt0 = ntb * NT;
    const float* const wbase = wp + (size_t)nt0 * 256 + lane * 4;
    const size_t wtap = (size_t)q.NTT * 256, wchunk = (size_t)27 * q.NTT * 256;

    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // (kd, kh) pairs of this wave; MODE 1 starts at the residue tap and steps by the stride
    const int kd0 = MODE == 0 ? 0 : (c_d + 1) % s, kh0 = MODE == 0 ? 0 : (c_h + 1) % s, kstep = MODE == 0 ? 1 : s;
    int pair = 0;
#pragma unroll 1
    for (int kd = kd0; kd < 3; kd += kstep) {
        int rd;   // read-side d coordinate
        if (MODE == 0) rd = c_d + kd;
        else {
            const int nd = c_d + 1 - kd;
            rd = nd >= 0 ? nd / s : -1;
        }
        const bool okd = (unsigned)rd < (unsigned)q.Di;   // MODE 1: wave-uniform
#pragma unroll 1
        for (int kh = kh0; kh < 3; kh += kstep, ++pair) {
            if (SPLIT && (pair & 3) != wv) continue;
            int rh;
            if (MODE == 0) rh = c_h + kh;
            else {
                const int nh = c_h + 1 - kh;
                rh = nh >= 0 ? nh / s : -1;
            }
            const bool okh = okd && (unsigned)rh < (unsigned)q.Hi;
            if (MODE == 1 && !okh) continue;   // wave-uniform in MODE 1
            // the kw taps of this pair: source pointer (clamped to the sample base when masked), mask, weight tap
            const T* src[3];
            bool okw[3];
            int wtapi[3];
            int nkw = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                int kw, rwc;
                bool have;
                if (MODE == 0) {
                    kw = j;
                    have = true;
                    rwc = c_w + kw;
                } else {
                    kw = (c_w + 1) % s + j * s;   // wave-uniform: c_w mod s is the M-tile's residue
                    have = kw < 3;
                    const int nw = c_w + 1 - kw;
                    rwc = nw >= 0 ? nw / s : -1;
                }
                const bool ok = have && vok && okh && (unsigned)rwc < (unsigned)q.Wi;
                okw[j] = ok;
                src[j] = ok ? in_n + (((int64_t)rd * q.Hi + rh) * q.Wi + rwc) * q.in_ld : in_n;
                const int tap = (kd * 3 + kh) * 3 + (have ? kw : 0);
                wtapi[j] = MODE == 0 ? tap : 26 - tap;   // MODE 1 reads the gradient image (pack_w_mfma_kernel dgrad = 1: 26 - tap)
                if (have) nkw = j + 1;
            }
#pragma unroll 1
            for (int ch = 0; ch < nchunks; ++ch) {
                const bool cok = ch * 16 + 4 * kq < q.Kc;   // Kc % 4 == 0 (host)
                float4 a[3];
                f32x4 b[3][NT];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (j < nkw) {
                        a[j] = ldf4((okw[j] && cok) ? src[j] + ch * 16 + 4 * kq : in_n);
                        if (!(okw[j] && cok)) a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            b[j][nt] = *reinterpret_cast<const f32x4*>(wbase + (size_t)wtapi[j] * wtap + (size_t)ch * wchunk + nt * 256);
                    }
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (j < nkw) {
                        const float av[4] = {a[j].x, a[j].y, a[j].z, a[j].w};
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                            for (int s4 = 0; s4 < 4; ++s4)
                                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j][nt][s4], av[s4], acc[nt], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (SPLIT) {   // waves 1..3 -> LDS, wave 0 adds them in a fixed order
        if (wv > 0) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[((wv - 1) * NT + nt) * 256 + r * 64 + lane] = acc[nt][r];
        }
        __syncthreads();
        if (wv > 0) return;
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[nt][r] += red[(w * NT + nt) * 256 + r * 64 + lane];
    }
    if (!vok) return;
    T* yv = out + out_off;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = (nt0 + nt) * 16 + 4 * kq;
        if (co >= q.Nc) continue;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (co + r < q.Nc) bv[r] = bias[co + r];
        }
        if (co + 3 < q.Nc && (q.out_ld & 3) == 0) {
            stf4(yv + co, make_float4(acc[nt][0] + bv[0], acc[nt][1] + bv[1], acc[nt][2] + bv[2], acc[nt][3] + bv[3]));
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (co + r < q.Nc) stf(yv + co + r, acc[nt][r] + bv[r]);
        }
    }
}

// ------------------------------------------------------------------ host side
// Plan of the tiled kernel (conv_mfma_fwd2_kernel): 3x3x3, stride 1, pad 1, dilation 1.
struct MfmaFwdPlan {
    int CK, NT, NTT, gy, nchunks, tilesD, tilesH, tilesW, ntiles, grid;
    size_t wp_floats, smem, stat_smem;   // packed-weight image, halo buffers, float64 statistics of the STATS variant
};

// Plan of the LDS-free kernel (conv_mfma_direct_kernel): 3x3x3, pad 1, dilation 1, one stride s for the three axes.
struct DirectPlan {
    DirectGeom q;
    int nt, mode, split, units;
    size_t wp_floats;
    int grid() const { return split ? units : cdiv(units, 4); }
};

static bool direct_plan(const Mri3dConvGeom& g, bool dgrad, DirectPlan& p) {
    if (!(g.kd == 3 && g.kh == 3 && g.kw == 3 && g.pd == 1 && g.ph == 1 && g.pw == 1 && g.dd == 1 && g.dh == 1 && g.dw == 1 &&
          g.sd == g.sh && g.sh == g.sw && g.sd >= 1 && g.sd <= 3))
        return false;
    const int Kc = dgrad ? g.co : g.ci, Nc = dgrad ? g.ci : g.co;
    const int in_ld = dgrad ? g.y_ld : g.x_ld, out_ld = dgrad ? g.x_ld : g.y_ld;
    if (Kc % 4 != 0 || Kc < 8 || in_ld % 4 != 0 || Nc < 8) return false;   // 4-channel fragments; tiny outputs stay on the gather kernels
    DirectGeom& q = p.q;
    q.N = g.n;
    q.s = g.sd;
    p.mode = (dgrad && g.sd > 1) ? 1 : 0;
    if (!dgrad) {            // reads x (di..), writes y (dout..)
        q.Di = g.di, q.Hi = g.hi, q.Wi = g.wi, q.Do = g.dout, q.Ho = g.ho, q.Wo = g.wo;
    } else if (p.mode == 1) {   // reads dY (dout..), writes dX (di..)
        q.Di = g.dout, q.Hi = g.ho, q.Wi = g.wo, q.Do = g.di, q.Ho = g.hi, q.Wo = g.wi;
    } else {                 // stride 1: the gradient is the forward of the flipped weights on dY, same extents
        q.Di = g.dout, q.Hi = g.ho, q.Wi = g.wo, q.Do = g.di, q.Ho = g.hi, q.Wo = g.wi;
    }
    q.Kc = Kc, q.in_ld = in_ld, q.Nc = Nc, q.out_ld = out_ld;
    q.NTT = cdiv(Nc, 16);
    const int64_t nvox_out = (int64_t)q.N * q.Do * q.Ho * q.Wo;
    int64_t nmt;
    if (p.mode == 0) {
        q.wbn = 1;
        nmt = (nvox_out + 15) / 16;
    } else {
        q.wbn = cdiv(cdiv(q.Wo, q.s), 16);
        nmt = (int64_t)q.N * q.Do * q.Ho * q.s * q.wbn;
    }
    if (nmt * q.NTT > 0x3fffffff || nvox_out > 0x7fffffff || (int64_t)q.N * q.Di * q.Hi * q.Wi > 0x7fffffff) return false;
    q.nmt = (int)nmt;
    // enough waves for ~4 per SIMD where the layer allows it: narrower N-blocks when there are few M-tiles
    p.nt = (q.NTT % 4 == 0) ? 4 : ((q.NTT % 2 == 0) ? 2 : 1);
    while (p.nt > 1 && nmt * (q.NTT / p.nt) < 4096) p.nt >>= 1;
    q.gy = q.NTT / p.nt;
    p.units = q.nmt * q.gy;
    p.split = p.units < 1024 ? 1 : 0;   // fewer units than SIMDs: a workgroup per unit, its waves split the taps
    p.wp_floats = (size_t)cdiv(Kc, 16) * 27 * q.NTT * 256;   // [chunk16][tap][nt][lane][s]
    return true;
}

template <typename T>
static void launch_direct(const DirectPlan& p, const T* in, const float* wp, const float* bias, T* out, hipStream_t s) {
#define MRI3D_DIRECT_CASE(NTv, MODEv, SPv)                                                                            \
    if (p.nt == NTv && p.mode == MODEv && p.split == SPv)                                                             \
        hipLaunchKernelGGL((conv_mfma_direct_kernel<T, NTv, MODEv, (SPv != 0)>), dim3(p.grid()), dim3(256), 0, s, in, wp, bias, out, p.q);
#define MRI3D_DIRECT_NT(MODEv, SPv) MRI3D_DIRECT_CASE(1, MODEv, SPv) MRI3D_DIRECT_CASE(2, MODEv, SPv) MRI3D_DIRECT_CASE(4, MODEv, SPv)
    MRI3D_DIRECT_NT(0, 0)
    MRI3D_DIRECT_NT(0, 1)
    MRI3D_DIRECT_NT(1, 0)
    MRI3D_DIRECT_NT(1, 1)
#undef MRI3D_DIRECT_NT
#undef MRI3D_DIRECT_CASE
}

static bool mfma_fwd_plan(const Mri3dConvGeom& g, bool dgrad, MfmaFwdPlan& p) {
    if (!(g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 1 && g.ph == 1 &&
          g.pw == 1 && g.dd == 1 && g.dh == 1 && g.dw == 1))
        return false;
    const bool bf = g.dtype == MRI3D_BF16;
    const int Kc = dgrad ? g.co : g.ci, Nc = dgrad ? g.ci : g.co;
    const int in_ld = dgrad ? g.y_ld : g.x_ld;
    if (Kc % 8 != 0 || in_ld % (bf ? 8 : 4) != 0) return false;   // 16-byte staging pieces
    if (Nc < 8) return false;  // tiny outputs (e.g. 16->2) stay on the direct kernel
    p.CK = bf ? 16 : 8;
    p.NTT = cdiv(Nc, 16);
    // NT (16-channel N-tiles per wave) is capped by registers: 8*NT accumulators + 2-deep A / 3-deep B rings + the staging
    // ring (NT <= 2).  Wider outputs are split over gy passes of the same tile.
    p.NT = (p.NTT % 2 == 0) ? 2 : 1;
    p.gy = p.NTT / p.NT;
    p.nchunks = cdiv(Kc, p.CK);
    p.tilesD = cdiv(g.di, TD);
    p.tilesH = cdiv(g.hi, TH);
    p.tilesW = cdiv(g.wi, TW);
    int64_t nt = (int64_t)g.n * p.tilesD * p.tilesH * p.tilesW;
    if (nt > 0x7fffffff) return false;
    p.ntiles = (int)nt;
    p.wp_floats = (size_t)p.nchunks * 14 * p.NTT * 256;   // 1 KiB per (chunk, tap group, N-tile)
    p.smem = (size_t)2 * kStg * 256 * 16;
    p.stat_smem = (size_t)4 * p.NTT * 16 * 2 * sizeof(double);   // per-wave float64 statistics of the STATS variant
    int64_t st = (int64_t)p.ntiles * p.gy;  // (spatial tile, n-tile block) work units
    if (st > 0x7fffffff) return false;
    p.grid = (int)std::min<int64_t>(st, 512);  // 2 resident workgroups per CU x 256 CUs
    return true;
}

// What the LDS-free kernel is to a geometry; the reasons are rows 1, 3, 5 and 6 of the table on fwd_route.  preferred / few_units:
// a small volume of 256 work units or more / of fewer; strided: it is the only kernel of this file with a stride.
enum class DirectUse { no, preferred, few_units, narrow, strided };

// `tiled`: the tiled kernel's plan where mfma_fwd_plan accepts, else nullptr.  dp is filled unless the answer is `no`.
static DirectUse direct_use(const Mri3dConvGeom& g, bool dgrad, const MfmaFwdPlan* tiled, DirectPlan& dp) {
    if (g.sd > 1 || g.sh > 1 || g.sw > 1) return direct_plan(g, dgrad, dp) ? DirectUse::strided : DirectUse::no;
    if (g.dtype == MRI3D_BF16 || tiled == nullptr) return DirectUse::no;   // bf16 tensors stay on the bf16 MFMA
    if (g.wi <= 8) return direct_plan(g, dgrad, dp) ? DirectUse::narrow : DirectUse::no;
#ifndef MRI3D_SMALL_UNITS
#define MRI3D_SMALL_UNITS 512   // one work unit per workgroup slot or fewer.  Measured (tools/small_units_ab.sh, variants -DMRI3D_SMALL_UNITS=N): 256 -> 512 moves 32 -> 32
#endif                          // @ 40x48x40 x 2 from 64 to 72 and 64 -> 64 @ 40x48x40 from 68 to 80 TFLOP/s; 1024 loses on 32 -> 64 (85 -> 79)
    const int st = tiled->ntiles * tiled->gy;   // (spatial tile, n-tile block) work units of the tiled kernel
    const int64_t in_bytes = (int64_t)g.n * g.di * g.hi * g.wi * (dgrad ? g.co : g.ci) * 4;
    if (st >= MRI3D_SMALL_UNITS || in_bytes > ((int64_t)32 << 20) || !direct_plan(g, dgrad, dp)) return DirectUse::no;
    return st < 256 ? DirectUse::few_units : DirectUse::preferred;
}

enum class FwdKernel { none, march, direct, tiled, tiled_n8 };   // conv_march_kernel, conv_mfma_direct_kernel, conv_mfma_fwd2_kernel<.., N8>

struct FwdRoute {
    FwdKernel kernel = FwdKernel::none;   // none: not served
    int grid = 0;                         // workgroups of the kernel = statistics partials when it fuses the statistics
    size_t wp_bytes = 0;                  // its packed-weight image at the head of the workspace
    MfmaFwdPlan tiled{};                  // kernel == tiled / tiled_n8  (the marching kernel keeps its MarchPlan in conv_march.hip)
    DirectPlan direct{};                  // kernel == direct
};

// THE forward / data-gradient decision of this file: which kernel runs, on what grid, with how much workspace.  The launch
// (run_mfma_fwd) and every query (conv_mfma_supported, conv_mfma_cat_supported, conv_mfma_fwd_stat_blocks) read this one answer,
// so they cannot disagree about the kernel or its grid.  `stats`: BatchNorm statistics fused into the forward; `sp`: a split
// operand (sp.split > 0).  First matching row wins:
//
//   1  any stride > 1                                          direct if direct_plan accepts, no stats and no split; otherwise none
//   2  mfma_fwd_plan refuses                                   none
//   3  a split, and row 5's `narrow` or `few units`            none (the LDS-free kernel has no second operand)
//   4  conv_march.hip takes it by choice, and no split or      march: the layers the marching kernel is faster on (bf16 tensors on
//      (split % 16 == 0 and second_ld % 8 == 0)                a chip-filling grid); the tiled kernel takes the other pitches
//   5  fp32, direct_plan accepts, no stats, no split, and      direct
//      narrow (wi <= 8) or small (see below)
//   6  stats, and more than 128 output channels or narrow      none: LDS statistics slots for up to 128 channels
//   7  exactly 8 output channels, no stats                     tiled_n8: the row-paired variant (10 tap groups per chunk)
//   8  otherwise                                               tiled
//
// Small volumes: no more work units than workgroup slots (fewer than MRI3D_SMALL_UNITS) — the wave-per-M-tile kernel fills the chip
// instead.  Its operands come from L2 / the Infinity Cache, so it is only used while the input is small (<= 32 MB).  With 256 units
// or more (`preferred`) that is a preference only: split operands and fused statistics still take the tiled kernel.
// Narrow volumes, at most half a tile row wide (the 8^3 level of the patch CNN, cnn_model.py:104-175, batch 512): a 16-voxel tile row
// would be half padding.  The LDS-free kernel's M-tiles are 16 consecutive voxels of the flattened index space (two rows of eight),
// nothing is wasted: 64 -> 64 @ 8^3 x 512 forward 61 -> 90, data gradient 65 -> 97 TFLOP/s.  (No fused BatchNorm statistics there:
// row 6, and the statistics pass reads the small output once.)
// Rows 2 and 3 stand before the marching kernel because the dispatcher (api.hip) has always asked conv_mfma_supported /
// conv_mfma_cat_supported first, which answered by them.
static FwdRoute fwd_route(const Mri3dConvGeom& g, bool dgrad, bool stats, const ConvSplit& sp) {
    FwdRoute r;
    const bool split = sp.split > 0;
    DirectPlan dp;
    MfmaFwdPlan p;
    const bool tiled_ok = mfma_fwd_plan(g, dgrad, p);   // (refuses a stride at once)
    const DirectUse du = direct_use(g, dgrad, tiled_ok ? &p : nullptr, dp);
    const auto direct = [&] {
        r.kernel = FwdKernel::direct, r.grid = dp.grid(), r.wp_bytes = dp.wp_floats * sizeof(float), r.direct = dp;
        return r;
    };
    if (du == DirectUse::strided) return (stats || split) ? r : direct();                                  // 1
    if (!tiled_ok) return r;                                                                               // 2
    if (split && (du == DirectUse::few_units || du == DirectUse::narrow)) return r;                        // 3
    const MarchNeeds march = conv_march_needs(g, dgrad, stats, false);
    if (march.grid > 0 && (!split || (sp.split % 16 == 0 && sp.second_ld % 8 == 0))) {                     // 4
        r.kernel = FwdKernel::march, r.grid = march.grid, r.wp_bytes = march.wp_bytes;
        return r;
    }
    if (du != DirectUse::no && !stats && !split) return direct();                                          // 5
    if (stats && (p.NTT > 8 || du == DirectUse::narrow)) return r;                                         // 6
    const bool n8 = (dgrad ? g.ci : g.co) == 8 && !stats;                                                  // 7, 8
    r.kernel = n8 ? FwdKernel::tiled_n8 : FwdKernel::tiled, r.grid = p.grid, r.tiled = p;
    // n8: 10 x 16-byte fragments x 64 lanes per chunk; both storage types: 256 floats == 512 bf16 per (chunk, tap group, N-tile)
    r.wp_bytes = (n8 ? (size_t)p.nchunks * 10 * 256 : p.wp_floats) * sizeof(float);
    return r;
}

// grid of a weight-packing kernel (grid-stride over the image's elements)
static dim3 pack_blocks(int elements) { return dim3(std::min(cdiv(elements, 256), 2048)); }

// The workspace must hold the chosen kernel's packed-weight image (callers size it with conv_mfma_workspace_bytes, a maximum over
// the kernel families, so this is never the stricter of the two).
static int run_mfma_fwd(const Mri3dConvGeom& g, bool dgrad, const void* in_v, const float* w, const float* bias,
                        void* out_v, void* ws, size_t ws_bytes, hipStream_t s, double* stat_part = nullptr,
                        ConvSplit sp = ConvSplit{}) {
    const FwdRoute r = fwd_route(g, dgrad, stat_part != nullptr, sp);
    MRI3D_REQUIRE(r.kernel != FwdKernel::none && (sp.second != nullptr) == (sp.split > 0), MRI3D_ENOTSUP,
                  "conv3d(mfma): geometry, fused statistics or split operand not served");
    MRI3D_REQUIRE(ws && ws_bytes >= r.wp_bytes, MRI3D_EWORKSPACE, "conv3d(mfma): workspace %zu < %zu", ws_bytes, r.wp_bytes);
    MRI3D_REQUIRE(aligned16(in_v, out_v, ws), MRI3D_EINVAL, "conv3d(mfma): input/output/workspace must be 16-byte aligned");
    float* wp = static_cast<float*>(ws);
    const int Kc = dgrad ? g.co : g.ci, Nc = dgrad ? g.ci : g.co;
    const int in_ld = dgrad ? g.y_ld : g.x_ld, out_ld = dgrad ? g.x_ld : g.y_ld;
    const bool bf = g.dtype == MRI3D_BF16;
    const MfmaFwdPlan& p = r.tiled;
    const int wp_floats = (int)(r.wp_bytes / sizeof(float));   // fp32 images: elements; the tiled kernels' bf16 images: two elements each
    switch (r.kernel) {
    case FwdKernel::none: return MRI3D_ENOTSUP;
    case FwdKernel::march: return conv_march_run(g, dgrad, false, in_v, w, bias, out_v, ws, ws_bytes, s, stat_part, sp);
    case FwdKernel::direct:
        hipLaunchKernelGGL(pack_w_mfma_kernel, pack_blocks(wp_floats), dim3(256), 0, s, w, wp, g.co, g.ci, dgrad ? 1 : 0, 16, r.direct.q.NTT, cdiv(Kc, 16));
        MRI3D_DISPATCH_DTYPE(g.dtype, T, { launch_direct<T>(r.direct, (const T*)in_v, wp, bias, (T*)out_v, s); });
        return check_launch(dgrad ? "conv3d_dgrad(mfma direct)" : "conv3d_fwd(mfma direct)");
    case FwdKernel::tiled_n8:
        if (bf)
            hipLaunchKernelGGL(pack_w_mfma_n8_kernel<bf16_t>, pack_blocks(2 * wp_floats), dim3(256), 0, s, w, reinterpret_cast<bf16_t*>(wp), g.co, g.ci,
                               dgrad ? 1 : 0, p.nchunks);
        else
            hipLaunchKernelGGL(pack_w_mfma_n8_kernel<float>, pack_blocks(wp_floats), dim3(256), 0, s, w, wp, g.co, g.ci, dgrad ? 1 : 0, p.nchunks);
        break;
    case FwdKernel::tiled:
        if (bf)
            hipLaunchKernelGGL(pack_w_mfma_bf16_kernel, pack_blocks(2 * wp_floats), dim3(256), 0, s, w, reinterpret_cast<bf16_t*>(wp), g.co, g.ci,
                               dgrad ? 1 : 0, p.NTT, p.nchunks);
        else
            hipLaunchKernelGGL(pack_w_mfma_kernel, pack_blocks(wp_floats), dim3(256), 0, s, w, wp, g.co, g.ci, dgrad ? 1 : 0, 8, p.NTT, p.nchunks);
        break;
    }
    const bool n8 = r.kernel == FwdKernel::tiled_n8;
    const int st = p.ntiles * p.gy;
    const size_t smem = p.smem + (stat_part ? p.stat_smem : 0);
    constexpr int kMaxSmem = 2 * kStg * 256 * 16 + 4 * 8 * 16 * 2 * 8;   // two halo buffers + float64 statistics of up to 128 channels
    // forward: the split is on the input (K) side; data gradient: on the output (N) side
    const void* x2 = dgrad ? nullptr : sp.second;
    void* y2 = dgrad ? const_cast<void*>(sp.second) : nullptr;
    const int x2_ld = dgrad ? 0 : sp.second_ld, ksplit = dgrad ? 0 : sp.split, y2_ld = dgrad ? sp.second_ld : 0, nsplit = dgrad ? sp.split : 0;
#define MRI3D_FWD2_CASE(NTv, STv, N8v)                                                                                \
    if (p.NT == NTv && (stat_part != nullptr) == STv && n8 == N8v) {                                                  \
        auto kern = conv_mfma_fwd2_kernel<T, NTv, STv, N8v>;                                                          \
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                       \
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, kMaxSmem);     \
        (void)attr;   /* once per kernel, not per launch */                                                          \
        hipLaunchKernelGGL(kern, dim3(r.grid), dim3(256), smem, s, (const T*)in_v, wp, bias, (T*)out_v, g.n, g.di,    \
                           g.hi, g.wi, Kc, in_ld, Nc, out_ld, p.NTT, p.gy, p.tilesD, p.tilesH, p.tilesW, st,         \
                           stat_part, (const T*)x2, x2_ld, ksplit, (T*)y2, y2_ld, nsplit);                           \
    }
    MRI3D_DISPATCH_DTYPE(g.dtype, T, {
        MRI3D_FWD2_CASE(1, false, false)
        MRI3D_FWD2_CASE(2, false, false)
        MRI3D_FWD2_CASE(1, true, false)
        MRI3D_FWD2_CASE(2, true, false)
        MRI3D_FWD2_CASE(1, false, true)
    });
#undef MRI3D_FWD2_CASE
    return check_launch(dgrad ? "conv3d_dgrad(mfma)" : "conv3d_fwd(mfma)");
}

int conv_mfma_fwd(const Mri3dConvGeom& g, const void* x, const float* w, const float* bias, void* y, void* ws,
                  size_t ws_bytes, hipStream_t s) {
    return run_mfma_fwd(g, false, x, w, bias, y, ws, ws_bytes, s);
}

// number of per-workgroup statistics partials the forward kernel writes for this geometry (0: no fused statistics);
// split / second_ld: those of a split operand (conv_mfma_fwd_cat), split 0: one tensor
int conv_mfma_fwd_stat_blocks(const Mri3dConvGeom& g, int split, int second_ld) {
    return fwd_route(g, false, true, ConvSplit{nullptr, split, second_ld}).grid;
}

int conv_mfma_fwd_stats(const Mri3dConvGeom& g, const void* x, const float* w, const float* bias, void* y, double* stat_part,
                        void* ws, size_t ws_bytes, hipStream_t s) {
    MRI3D_REQUIRE(stat_part != nullptr, MRI3D_EINVAL, "conv3d_fwd_stats: null partial buffer");
    return run_mfma_fwd(g, false, x, w, bias, y, ws, ws_bytes, s, stat_part);
}

int conv_mfma_dgrad(const Mri3dConvGeom& g, const void* dy, const float* w, const float* bias, void* dx, void* ws,
                    size_t ws_bytes, hipStream_t s) {
    return run_mfma_fwd(g, true, dy, w, bias, dx, ws, ws_bytes, s);
}

// ---- split operands (conv over cat((x, x2), channels)): which kernels take them is fwd_route's answer (weight gradient:
// conv_mfma_wgrad_supported's), what the operand itself must satisfy is in conv_mfma_cat_supported; the second tensor 16-byte aligned with a pitch like the first's
int conv_mfma_fwd_cat(const Mri3dConvGeom& g, const void* x, const void* x2, int split, int x2_ld, const float* w, const float* bias,
                      void* y, double* stat_part, void* ws, size_t ws_bytes, hipStream_t s) {
    return run_mfma_fwd(g, false, x, w, bias, y, ws, ws_bytes, s, stat_part, ConvSplit{x2, split, x2_ld});
}

int conv_mfma_dgrad_cat(const Mri3dConvGeom& g, const void* dy, const float* w, void* dx, void* dx2, int split, int dx2_ld, void* ws,
                        size_t ws_bytes, hipStream_t s) {
    return run_mfma_fwd(g, true, dy, w, nullptr, dx, ws, ws_bytes, s, nullptr, ConvSplit{dx2, split, dx2_ld});
}

// ------------------------------------------------------------------ queries over all three passes
// (the weight gradient's answers come from conv_mfma_wgrad.hip)
// the split operand's own divisibility checks, then: does a kernel take it (fwd_route / conv_mfma_wgrad_supported)
bool conv_mfma_cat_supported(const Mri3dConvGeom& g, int split, int second_ld, int pass) {
    const bool bf = g.dtype == MRI3D_BF16;
    if (split <= 0 || split >= g.ci || split % 16 != 0 || second_ld % (bf ? 8 : 4) != 0 || second_ld < g.ci - split) return false;
    const ConvSplit sp{nullptr, split, second_ld};
    if (pass == MRI3D_PASS_FWD) return (g.ci - split) % 8 == 0 && fwd_route(g, false, false, sp).kernel != FwdKernel::none;
    if (pass == MRI3D_PASS_DGRAD) return (g.ci - split) % 4 == 0 && fwd_route(g, true, false, sp).kernel != FwdKernel::none;   // N side: 16-channel tiles
    if (pass == MRI3D_PASS_WGRAD) return conv_mfma_wgrad_supported(g, split, second_ld);
    return false;
}

bool conv_mfma_supported(const Mri3dConvGeom& g, int pass) {
    if (pass == MRI3D_PASS_FWD || pass == MRI3D_PASS_DGRAD) return fwd_route(g, pass == MRI3D_PASS_DGRAD, false, ConvSplit{}).kernel != FwdKernel::none;
    return pass == MRI3D_PASS_WGRAD && conv_mfma_wgrad_supported(g);
}

// What run_mfma_fwd / the weight gradient launch for the pass, by name: the kernel and the template arguments that select code in
// it (no grids, no plan values that are run-time arguments).  Read from the same fwd_route / weight-gradient plan as the launch.
bool conv_mfma_route_name(const Mri3dConvGeom& g, int pass, bool stats, bool bias, const ConvSplit& sp, char* name, size_t name_bytes) {
    if (pass == MRI3D_PASS_WGRAD) return conv_mfma_wgrad_route_name(g, name, name_bytes);
    if (pass != MRI3D_PASS_FWD && pass != MRI3D_PASS_DGRAD) return false;
    const FwdRoute r = fwd_route(g, pass == MRI3D_PASS_DGRAD, stats, sp);
    switch (r.kernel) {
    case FwdKernel::none: return false;
    case FwdKernel::march: snprintf(name, name_bytes, "march%s%s", stats ? " stats" : "", bias ? " bias" : ""); break;
    case FwdKernel::direct: snprintf(name, name_bytes, "direct nt%d mode%d split%d", r.direct.nt, r.direct.mode, r.direct.split); break;
    case FwdKernel::tiled: snprintf(name, name_bytes, "tiled nt%d%s", r.tiled.NT, stats ? " stats" : ""); break;
    case FwdKernel::tiled_n8: snprintf(name, name_bytes, "tiled_n8"); break;
    }
    return true;
}

// The numbers run_mfma_fwd launches by (mri3d_conv3d_mfma_plan_query), from the same fwd_route answer; the weight gradient's come
// from its own plan.  The marching kernel is not of this file: false.
bool conv_mfma_plan_info(const Mri3dConvGeom& g, int pass, bool stats, const ConvSplit& sp, Mri3dConvMfmaPlanInfo& out) {
    if (pass == MRI3D_PASS_WGRAD) return conv_mfma_wgrad_plan_info(g, out);
    if (pass != MRI3D_PASS_FWD && pass != MRI3D_PASS_DGRAD) return false;
    const bool dgrad = pass == MRI3D_PASS_DGRAD;
    const FwdRoute r = fwd_route(g, dgrad, stats, sp);
    if (r.kernel == FwdKernel::none || r.kernel == FwdKernel::march) return false;
    const int Kc = dgrad ? g.co : g.ci;
    Mri3dConvMfmaPlanInfo o{};
    o.grid = r.grid;
    o.workspace_bytes = (int64_t)r.wp_bytes;
    o.stats_blocks = stats ? r.grid : 0;
    if (r.kernel == FwdKernel::direct) {
        const DirectPlan& d = r.direct;
        o.kernel = MRI3D_MFMA_DIRECT;
        o.ck = 16, o.chunks = cdiv(Kc, 16), o.partial_chunk = Kc % 16 != 0;
        o.nt = d.nt, o.ntt = d.q.NTT, o.gy = d.q.gy;
        o.tile_d = o.tile_h = 1, o.tile_w = 16;
        o.ntiles = d.q.nmt, o.units = d.units;
        o.mode = d.mode, o.split = d.split, o.wbn = d.q.wbn;
        o.max_tasks = o.min_tasks = 1;
    } else {
        const MfmaFwdPlan& p = r.tiled;
        o.kernel = r.kernel == FwdKernel::tiled_n8 ? MRI3D_MFMA_TILED_N8 : MRI3D_MFMA_TILED;
        o.ck = p.CK, o.chunks = p.nchunks, o.partial_chunk = Kc % p.CK != 0;
        o.nt = p.NT, o.ntt = p.NTT, o.gy = p.gy;
        o.tile_d = TD, o.tile_h = TH, o.tile_w = TW;
        o.tiles_d = p.tilesD, o.tiles_h = p.tilesH, o.tiles_w = p.tilesW, o.ntiles = p.ntiles;
        o.units = p.ntiles * p.gy;
        const WalkCounts wc = xcd_walk_counts(r.grid, 1, o.units);
        o.max_tasks = wc.max_tasks, o.min_tasks = wc.min_tasks;
    }
    out = o;
    return true;
}

// Forward / data gradient: the caller asks before it knows whether statistics or a split operand will be requested, and
// mri3d_conv3d_{fwd,dgrad}_march is documented to size its workspace with this query too.  So the answer is not the need of one
// route but the maximum over the kernel families that accept the geometry at all: the tiled kernel's image where mfma_fwd_plan
// accepts (also for narrow volumes, which no route takes there), the LDS-free kernel's where a direct route exists, and the forced
// marching plan's.
size_t conv_mfma_workspace_bytes(const Mri3dConvGeom& g, int pass) {
    MfmaFwdPlan p;
    DirectPlan dp;
    if (pass == MRI3D_PASS_WGRAD) return conv_mfma_wgrad_workspace_bytes(g);
    if (!conv_mfma_supported(g, pass)) return 0;
    const bool dgrad = pass == MRI3D_PASS_DGRAD;
    size_t bytes = conv_march_needs(g, dgrad, false, true).wp_bytes;
    const bool tiled_ok = mfma_fwd_plan(g, dgrad, p);
    if (tiled_ok) bytes = std::max(bytes, p.wp_floats * sizeof(float));
    if (direct_use(g, dgrad, tiled_ok ? &p : nullptr, dp) != DirectUse::no) bytes = std::max(bytes, dp.wp_floats * sizeof(float));
    return bytes;
}

}  // namespace mri3d
