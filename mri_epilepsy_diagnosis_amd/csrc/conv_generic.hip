// conv_generic.hip — direct NDHWC Conv3d forward / data-gradient / weight-gradient for ANY kernel size,
// stride, padding and dilation (separable (k,1,1) convs of AE_model.py:9-26, strided convs of
// modified_3dunet.py:23-38, dilated convs of cnn_model.py:212-240, 1x1x1 classifier of unet.UNet).
// The 3x3x3 stride-1 hot layers take the MFMA implicit-GEMM path in conv_mfma.hip / conv_mfma_wgrad.hip instead.
//
// Roofline: these layers have arithmetic intensity of a few FLOP/byte (separable convs AI~6) and are
// HBM-bound; the design goal is one coalesced pass over x and y with weights on the scalar path.
#include "common.h"
#include "conv_backends.h"

namespace mri3d {

// sum over the 64 lanes of a wave, the same value in every lane: xor-1 / xor-2 inside quads, half-mirror and mirror inside
// the 16-lane DPP rows, then the four row sums through readlane
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    const int vi = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 48));
    return (r0 + r1) + (r2 + r3);
}

// ------------------------------------------------------------------ weight repack
// torch (Co, Ci, kd, kh, kw)  ->  forward (dgrad = 0)        Wf[tap][ci][coP]   (P = coP: Co rounded up to the cout tile)
//                             ->  data gradient (dgrad = 1)  Wd[tap][co][ciP]   (P = ciP)
__global__ void repack_w_kernel(const float* __restrict__ w, float* __restrict__ wp, int Co, int Ci, int taps, int P, int dgrad) {
    const int M = dgrad ? Co : Ci, N = dgrad ? Ci : Co;   // channels summed over, channels tiled (N padded to P)
    int total = taps * M * P;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int p = i % P;
        int m = (i / P) % M;
        int tap = i / (P * M);
        const int co = dgrad ? m : p, ci = dgrad ? p : m;
        wp[i] = (p < N) ? w[((size_t)co * Ci + ci) * taps + tap] : 0.f;
    }
}

// ------------------------------------------------------------------ index arithmetic the kernels share
// Shared is what leaves every kernel's gfx950 code instruction-identical to the same text written out in place: the two index
// decodes (here and decode_tile below).  A helper that takes a thread's arrays by reference (acc[], the tap tables) changes the
// code of the kernels that use it, so those pieces stay written out in each kernel, marked "written out".

// flat voxel index -> (n, d, h, w) of n volumes of D x H x W
__device__ __forceinline__ void decode_voxel(int64_t v, int D, int H, int W, int& n, int& d, int& h, int& w) {
    w = (int)(v % W);
    int64_t t = v / W;
    h = (int)(t % H);
    t /= H;
    d = (int)(t % D);
    n = (int)(t / D);
}

// ------------------------------------------------------------------ forward
// One thread = one output voxel x COT output channels.  Weights are wave-uniform -> scalar loads.
template <typename T, int COT, bool VEC4>
__global__ void __launch_bounds__(256)
conv_fwd_generic_kernel(Mri3dConvGeom g, const T* __restrict__ x, const float* __restrict__ wp,
                        const float* __restrict__ bias, T* __restrict__ y, int CoP) {
    const int cot = blockIdx.y * COT;
    const int64_t nvox = (int64_t)g.n * g.dout * g.ho * g.wo;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
        int n, od, oh, ow;
        decode_voxel(v, g.dout, g.ho, g.wo, n, od, oh, ow);
        // (bias initialisation, tap FMAs and tile store are written out in each of the six kernels of this kind: shared, the code changed)
        float acc[COT];
#pragma unroll
        for (int j = 0; j < COT; ++j) acc[j] = (bias != nullptr && cot + j < g.co) ? bias[cot + j] : 0.f;
        int tap = 0;
        for (int kd = 0; kd < g.kd; ++kd) {
            int id = od * g.sd - g.pd + kd * g.dd;
            for (int kh = 0; kh < g.kh; ++kh) {
                int ih = oh * g.sh - g.ph + kh * g.dh;
                for (int kw = 0; kw < g.kw; ++kw, ++tap) {
                    int iw = ow * g.sw - g.pw + kw * g.dw;
                    bool valid = (unsigned)id < (unsigned)g.di && (unsigned)ih < (unsigned)g.hi &&
                                 (unsigned)iw < (unsigned)g.wi;
                    const T* xp = x + ((((int64_t)n * g.di + (valid ? id : 0)) * g.hi + (valid ? ih : 0)) * g.wi +
                                           (valid ? iw : 0)) * g.x_ld;
                    const float* wt = wp + (size_t)tap * g.ci * CoP + cot;
                    if (VEC4) {
                        for (int ci = 0; ci < g.ci; ci += 4) {
                            float4 xv = valid ? ldf4(xp + ci) : make_float4(0, 0, 0, 0);
                            const float* w0 = wt + (size_t)ci * CoP;
#pragma unroll
                            for (int j = 0; j < COT; ++j) {
                                acc[j] = fmaf(xv.x, w0[j], acc[j]);
                                acc[j] = fmaf(xv.y, w0[CoP + j], acc[j]);
                                acc[j] = fmaf(xv.z, w0[2 * CoP + j], acc[j]);
                                acc[j] = fmaf(xv.w, w0[3 * CoP + j], acc[j]);
                            }
                        }
                    } else {
                        for (int ci = 0; ci < g.ci; ++ci) {
                            float xv = valid ? ldf(xp + ci) : 0.f;
                            const float* w0 = wt + (size_t)ci * CoP;
#pragma unroll
                            for (int j = 0; j < COT; ++j) acc[j] = fmaf(xv, w0[j], acc[j]);
                        }
                    }
                }
            }
        }
        T* yp = y + v * g.y_ld + cot;
#pragma unroll
        for (int j = 0; j < COT; ++j)
            if (cot + j < g.co) stf(yp + j, acc[j]);
    }
}

// ------------------------------------------------------------------ forward, few taps (separable convs of the autoencoder)
// Same arithmetic and thread = (output voxel, COT output channels) as the kernel above, for filters of <= 8 taps on input channels in
// multiples of 4 (AE_model.py:9-26, 74-91: (6,1,1)/(1,6,1)/(1,1,6) stride 2 and (3,1,1)/(1,3,1)/(1,1,3)).  There every tap's load
// sits inside nested run-time loops behind `valid ? load : 0`, so it gets its own wait (12 serial round trips per voxel of the 8 -> 8
// layer) and each voxel pays three 64-bit divisions.  Here voxels are walked slab-wise with 32-bit arithmetic and, per input-channel
// quad, the loads of ALL taps are issued together (clamped address, masked afterwards) before their FMAs.
// CV = input channels per load: 4 (Ci % 4 == 0, 16-byte loads) or 1 (any Ci; the autoencoder's first conv has Ci = 1)
template <typename T, int COT, int NTAPS, int CV>
__global__ void __launch_bounds__(256)
conv_fwd_taps_kernel(Mri3dConvGeom g, const T* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                     T* __restrict__ y, int CoP, int hch) {
    const int taps = g.kd * g.kh * g.kw;
    const int cot = blockIdx.y * COT;
    int tdd[NTAPS], tdh[NTAPS], tdw[NTAPS];   // tap offsets in voxels per axis, and as one element offset (all wave-uniform; the table of
                                              // conv_wgrad_quads_kernel, written out in both: shared, the code changed)
    int64_t tdelta[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) {
        const int tt = t < taps ? t : 0;
        tdw[t] = (tt % g.kw) * g.dw, tdh[t] = ((tt / g.kw) % g.kh) * g.dh, tdd[t] = (tt / (g.kw * g.kh)) * g.dd;
        tdelta[t] = (((int64_t)tdd[t] * g.hi + tdh[t]) * g.wi + tdw[t]) * g.x_ld;
    }
    const int hchunks = (g.ho + hch - 1) / hch;
    const int slabs = g.n * g.dout * hchunks;
    for (int slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
        const int hc = slab % hchunks, nd = slab / hchunks;
        const int n = nd / g.dout, od = nd - n * g.dout;
        const int h0 = hc * hch, hn = min(hch, g.ho - h0);
        const unsigned inner = (unsigned)hn * g.wo;
        const T* xn = x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld;
        T* yn = y + (((int64_t)nd * g.ho + h0) * g.wo) * g.y_ld + cot;
        for (unsigned e = threadIdx.x; e < inner; e += blockDim.x) {
            const int ow = e % g.wo, oh = h0 + e / g.wo;
            // a tap's address = the voxel's base offset + a wave-uniform delta (one add); a tap outside the volume re-reads a valid
            // element (`safe`: the sample's first voxel) and is masked
            const int id0 = od * g.sd - g.pd, ih0 = oh * g.sh - g.ph, iw0 = ow * g.sw - g.pw;
            const int64_t base = (((int64_t)id0 * g.hi + ih0) * g.wi + iw0) * g.x_ld;
            int64_t off[NTAPS];
            unsigned okm = 0;
#pragma unroll
            for (int t = 0; t < NTAPS; ++t) {
                const bool ok = t < taps && (unsigned)(id0 + tdd[t]) < (unsigned)g.di && (unsigned)(ih0 + tdh[t]) < (unsigned)g.hi &&
                                (unsigned)(iw0 + tdw[t]) < (unsigned)g.wi;
                okm |= ok ? (1u << t) : 0u;
                off[t] = ok ? base + tdelta[t] : 0;
            }
            // (bias initialisation, batched tap FMAs and tile store are written out: shared with the other few-taps kernel, the code changed)
            float acc[COT];
#pragma unroll
            for (int j = 0; j < COT; ++j) acc[j] = (bias != nullptr && cot + j < g.co) ? bias[cot + j] : 0.f;
            for (int ci = 0; ci < g.ci; ci += CV) {
                float xv[NTAPS][CV];
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) {
                    if constexpr (CV == 4) {
                        const float4 q = ldf4(xn + off[t] + ci);
                        xv[t][0] = q.x, xv[t][1] = q.y, xv[t][2] = q.z, xv[t][3] = q.w;
                    } else {
                        xv[t][0] = ldf(xn + off[t] + ci);
                    }
                }
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) {
                    if (t < taps) {   // uniform
                        const bool ok = (okm >> t) & 1u;
                        const float* w0 = wp + ((size_t)t * g.ci + ci) * CoP + cot;
#pragma unroll
                        for (int c = 0; c < CV; ++c) {
                            const float xc = ok ? xv[t][c] : 0.f;
#pragma unroll
                            for (int j = 0; j < COT; ++j) acc[j] = fmaf(xc, w0[c * CoP + j], acc[j]);
                        }
                    }
                }
            }
            T* yp = yn + (int64_t)e * g.y_ld;
            if (COT % 4 == 0 && cot + COT <= g.co && (g.y_ld & 3) == 0) {
#pragma unroll
                for (int j = 0; j < COT; j += 4) stf4(yp + j, make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]));
            } else {
#pragma unroll
                for (int j = 0; j < COT; ++j)
                    if (cot + j < g.co) stf(yp + j, acc[j]);
            }
        }
    }
}

// ------------------------------------------------------------------ data gradient (also ConvTranspose3d forward)
// One thread = one input voxel x CIT input channels; gather over the output voxels that read it.
template <typename T, int CIT, bool VEC4>
__global__ void __launch_bounds__(256)
conv_dgrad_generic_kernel(Mri3dConvGeom g, const T* __restrict__ dy, const float* __restrict__ wp,
                          const float* __restrict__ bias, T* __restrict__ dx, int CiP) {
    const int cit = blockIdx.y * CIT;
    const int64_t nvox = (int64_t)g.n * g.di * g.hi * g.wi;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
        int n, id, ih, iw;
        decode_voxel(v, g.di, g.hi, g.wi, n, id, ih, iw);
        // (bias initialisation, tap FMAs and tile store are written out in each of the six kernels of this kind: shared, the code changed)
        float acc[CIT];
#pragma unroll
        for (int j = 0; j < CIT; ++j) acc[j] = (bias != nullptr && cit + j < g.ci) ? bias[cit + j] : 0.f;
        int tap = 0;
        for (int kd = 0; kd < g.kd; ++kd) {
            int nd = id + g.pd - kd * g.dd;
            int od = nd / g.sd;
            bool vd = nd >= 0 && (nd - od * g.sd) == 0 && od < g.dout;
            for (int kh = 0; kh < g.kh; ++kh) {
                int nh = ih + g.ph - kh * g.dh;
                int oh = nh / g.sh;
                bool vh = nh >= 0 && (nh - oh * g.sh) == 0 && oh < g.ho;
                for (int kw = 0; kw < g.kw; ++kw, ++tap) {
                    int nw = iw + g.pw - kw * g.dw;
                    int ow = nw / g.sw;
                    bool valid = vd && vh && nw >= 0 && (nw - ow * g.sw) == 0 && ow < g.wo;
                    const T* yp = dy + ((((int64_t)n * g.dout + (valid ? od : 0)) * g.ho + (valid ? oh : 0)) * g.wo +
                                            (valid ? ow : 0)) * g.y_ld;
                    const float* wt = wp + (size_t)tap * g.co * CiP + cit;
                    if (VEC4) {
                        for (int co = 0; co < g.co; co += 4) {
                            float4 gv = valid ? ldf4(yp + co) : make_float4(0, 0, 0, 0);
                            const float* w0 = wt + (size_t)co * CiP;
#pragma unroll
                            for (int j = 0; j < CIT; ++j) {
                                acc[j] = fmaf(gv.x, w0[j], acc[j]);
                                acc[j] = fmaf(gv.y, w0[CiP + j], acc[j]);
                                acc[j] = fmaf(gv.z, w0[2 * CiP + j], acc[j]);
                                acc[j] = fmaf(gv.w, w0[3 * CiP + j], acc[j]);
                            }
                        }
                    } else {
                        for (int co = 0; co < g.co; ++co) {
                            float gv = valid ? ldf(yp + co) : 0.f;
                            const float* w0 = wt + (size_t)co * CiP;
#pragma unroll
                            for (int j = 0; j < CIT; ++j) acc[j] = fmaf(gv, w0[j], acc[j]);
                        }
                    }
                }
            }
        }
        T* xp = dx + v * g.x_ld + cit;
#pragma unroll
        for (int j = 0; j < CIT; ++j)
            if (cit + j < g.ci) stf(xp + j, acc[j]);
    }
}

// ------------------------------------------------------------------ data gradient, few taps (separable convs of the autoencoder)
// The gather above with slab-wise 32-bit voxel arithmetic and, per output-channel quad, the dy loads of ALL taps issued together
// (clamped address, masked afterwards: taps that do not reach this input voxel — wrong stride residue, outside the volume — cost a
// cached load instead of a branch with its own wait).  <= 8 taps, Co in multiples of 4.
// CV = output channels per dy load: 4 (Co % 4 == 0) or 1 (Co = 1: the 8 -> 1 convs in front of the autoencoder's last block)
template <typename T, int CIT, int NTAPS, int CV>
__global__ void __launch_bounds__(256)
conv_dgrad_taps_kernel(Mri3dConvGeom g, const T* __restrict__ dy, const float* __restrict__ wp, const float* __restrict__ bias,
                       T* __restrict__ dx, int CiP, int hch) {
    const int taps = g.kd * g.kh * g.kw;
    const int cit = blockIdx.y * CIT;
    int tkd[NTAPS], tkh[NTAPS], tkw[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) {
        const int tt = t < taps ? t : 0;
        tkw[t] = tt % g.kw, tkh[t] = (tt / g.kw) % g.kh, tkd[t] = tt / (g.kw * g.kh);
    }
    const int hchunks = (g.hi + hch - 1) / hch;
    const int slabs = g.n * g.di * hchunks;
    for (int slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
        const int hc = slab % hchunks, nd_ = slab / hchunks;
        const int n = nd_ / g.di, id = nd_ - n * g.di;
        const int h0 = hc * hch, hn = min(hch, g.hi - h0);
        const unsigned inner = (unsigned)hn * g.wi;
        const T* yn = dy + (int64_t)n * g.dout * g.ho * g.wo * g.y_ld;
        T* xn = dx + (((int64_t)nd_ * g.hi + h0) * g.wi) * g.x_ld + cit;
        for (unsigned e = threadIdx.x; e < inner; e += blockDim.x) {
            const int iw = e % g.wi, ih = h0 + e / g.wi;   // (incremental counters instead of this division pair: measured, no gain)
            int64_t off[NTAPS];
            unsigned okm = 0;
#pragma unroll
            for (int t = 0; t < NTAPS; ++t) {
                // (launched for unit strides only — launch_dgrad — so the output voxel of a tap is the shifted input voxel: no
                // run-time integer divisions, which were most of this kernel's instructions)
                const int od = id + g.pd - tkd[t] * g.dd, oh = ih + g.ph - tkh[t] * g.dh, ow = iw + g.pw - tkw[t] * g.dw;
                const bool ok = t < taps && (unsigned)od < (unsigned)g.dout && (unsigned)oh < (unsigned)g.ho && (unsigned)ow < (unsigned)g.wo;
                okm |= ok ? (1u << t) : 0u;
                const int cd = min(max(od, 0), g.dout - 1), chh = min(max(oh, 0), g.ho - 1), cw = min(max(ow, 0), g.wo - 1);
                off[t] = (((int64_t)cd * g.ho + chh) * g.wo + cw) * g.y_ld;
            }
            // (bias initialisation, batched tap FMAs and tile store are written out: shared with the other few-taps kernel, the code changed)
            float acc[CIT];
#pragma unroll
            for (int j = 0; j < CIT; ++j) acc[j] = (bias != nullptr && cit + j < g.ci) ? bias[cit + j] : 0.f;
            for (int co = 0; co < g.co; co += CV) {
                float gv[NTAPS][CV];
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) {
                    if constexpr (CV == 4) {
                        const float4 q = ldf4(yn + off[t] + co);
                        gv[t][0] = q.x, gv[t][1] = q.y, gv[t][2] = q.z, gv[t][3] = q.w;
                    } else {
                        gv[t][0] = ldf(yn + off[t] + co);
                    }
                }
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) {
                    if (t < taps) {   // uniform
                        const bool ok = (okm >> t) & 1u;
                        const float* w0 = wp + ((size_t)t * g.co + co) * CiP + cit;
#pragma unroll
                        for (int c = 0; c < CV; ++c) {
                            const float gc = ok ? gv[t][c] : 0.f;
#pragma unroll
                            for (int j = 0; j < CIT; ++j) acc[j] = fmaf(gc, w0[c * CiP + j], acc[j]);
                        }
                    }
                }
            }
            T* xp = xn + (int64_t)e * g.x_ld;
            if (CIT % 4 == 0 && cit + CIT <= g.ci && (g.x_ld & 3) == 0) {
#pragma unroll
                for (int j = 0; j < CIT; j += 4) stf4(xp + j, make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]));
            } else {
#pragma unroll
                for (int j = 0; j < CIT; ++j)
                    if (cit + j < g.ci) stf(xp + j, acc[j]);
            }
        }
    }
}

// ------------------------------------------------------------------ data gradient, strided convs
// Data gradient of a STRIDED convolution (dilation 1): only the taps with k = (i + pad) mod stride reach an input voxel i, i.e.
// 1 .. 8 of the 27 taps of a 3x3x3 / stride-2 layer (modified_3dunet.py:23-38, cnn_model.py:49-81).  The gather kernel above
// walks all taps and masks (8x wasted FMAs: 6 TFLOP/s on the 8 -> 16 stride-2 layer at 80x96x80).  Here one WAVE owns one
// (n, id, ih, w-parity) row segment: the valid tap set is wave-uniform, so the tap loops just step by the stride, the weights
// stay on the scalar path and nothing is masked except the volume border.
template <typename T, int CIT, bool VEC4>
__global__ void __launch_bounds__(64)
conv_dgrad_strided_kernel(Mri3dConvGeom g, const T* __restrict__ dy, const float* __restrict__ wp,
                          const float* __restrict__ bias, T* __restrict__ dx, int CiP) {
    int u = blockIdx.x;
    const int rw = u % g.sw;   // residue of iw modulo the W stride handled by this wave
    u /= g.sw;
    const int ih = u % g.hi;
    u /= g.hi;
    const int id = u % g.di;
    const int n = u / g.di;
    const int cit = blockIdx.y * CIT;
    const int kd0 = (id + g.pd) % g.sd, kh0 = (ih + g.ph) % g.sh, kw0 = (rw + g.pw) % g.sw;
    for (int iw = rw + (int)threadIdx.x * g.sw; iw < g.wi; iw += 64 * g.sw) {
        // (bias initialisation, tap FMAs and tile store are written out in each of the six kernels of this kind: shared, the code changed)
        float acc[CIT];
#pragma unroll
        for (int j = 0; j < CIT; ++j) acc[j] = (bias != nullptr && cit + j < g.ci) ? bias[cit + j] : 0.f;
        for (int kd = kd0; kd < g.kd; kd += g.sd) {
            const int nd = id + g.pd - kd;
            if (nd < 0) break;
            const int od = nd / g.sd;
            if (od >= g.dout) continue;
            for (int kh = kh0; kh < g.kh; kh += g.sh) {
                const int nh = ih + g.ph - kh;
                if (nh < 0) break;
                const int oh = nh / g.sh;
                if (oh >= g.ho) continue;
                for (int kw = kw0; kw < g.kw; kw += g.sw) {
                    const int nw = iw + g.pw - kw;
                    const int ow = nw / g.sw;
                    const bool valid = nw >= 0 && ow < g.wo;
                    const T* yp = dy + ((((int64_t)n * g.dout + od) * g.ho + oh) * g.wo + (valid ? ow : 0)) * g.y_ld;
                    const float* wt = wp + (size_t)((kd * g.kh + kh) * g.kw + kw) * g.co * CiP + cit;
                    if (VEC4) {
                        for (int co = 0; co < g.co; co += 4) {
                            const float4 gv = valid ? ldf4(yp + co) : make_float4(0.f, 0.f, 0.f, 0.f);
                            const float* w0 = wt + (size_t)co * CiP;
#pragma unroll
                            for (int j = 0; j < CIT; ++j) {
                                acc[j] = fmaf(gv.x, w0[j], acc[j]);
                                acc[j] = fmaf(gv.y, w0[CiP + j], acc[j]);
                                acc[j] = fmaf(gv.z, w0[2 * CiP + j], acc[j]);
                                acc[j] = fmaf(gv.w, w0[3 * CiP + j], acc[j]);
                            }
                        }
                    } else {
                        for (int co = 0; co < g.co; ++co) {
                            const float gv = valid ? ldf(yp + co) : 0.f;
                            const float* w0 = wt + (size_t)co * CiP;
#pragma unroll
                            for (int j = 0; j < CIT; ++j) acc[j] = fmaf(gv, w0[j], acc[j]);
                        }
                    }
                }
            }
        }
        T* xp = dx + ((((int64_t)n * g.di + id) * g.hi + ih) * g.wi + iw) * g.x_ld + cit;
#pragma unroll
        for (int j = 0; j < CIT; ++j)
            if (cit + j < g.ci) stf(xp + j, acc[j]);
    }
}

// The same wave-per-(n, id, ih, w-residue) decomposition with the valid taps ENUMERATED first (they are wave-uniform: at most NT of
// them) and, per output-channel quad, their dy loads issued together before the FMAs — in the kernel above every tap's load sits in
// a run-time loop behind `valid ? load : 0` and gets its own wait (6 serial round trips per voxel of the (1,6,1) stride-2 layer).
// Slots past the last valid tap re-read slot 0 (cached) and are masked: no branch around a load.
template <typename T, int CIT, int NT>
__global__ void __launch_bounds__(64)
conv_dgrad_strided_taps_kernel(Mri3dConvGeom g, const T* __restrict__ dy, const float* __restrict__ wp,
                               const float* __restrict__ bias, T* __restrict__ dx, int CiP) {
    int u = blockIdx.x;
    const int rw = u % g.sw;
    u /= g.sw;
    const int ih = u % g.hi;
    u /= g.hi;
    const int id = u % g.di;
    const int n = u / g.di;
    const int cit = blockIdx.y * CIT;
    const int kd0 = (id + g.pd) % g.sd, kh0 = (ih + g.ph) % g.sh, kw0 = (rw + g.pw) % g.sw;
    // enumerate the taps that reach this row (uniform): dy row base, kw, packed-weight tap index
    int64_t rowoff[NT];
    int tkw[NT], ttap[NT];
    int ntap = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) { rowoff[t] = 0; tkw[t] = kw0; ttap[t] = 0; }
    for (int kd = kd0; kd < g.kd; kd += g.sd) {
        const int nd = id + g.pd - kd;
        if (nd < 0) break;
        const int od = nd / g.sd;
        if (od >= g.dout) continue;
        for (int kh = kh0; kh < g.kh; kh += g.sh) {
            const int nh = ih + g.ph - kh;
            if (nh < 0) break;
            const int oh = nh / g.sh;
            if (oh >= g.ho) continue;
            for (int kw = kw0; kw < g.kw; kw += g.sw) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t == ntap) {
                        rowoff[t] = ((((int64_t)n * g.dout + od) * g.ho + oh) * g.wo) * g.y_ld;
                        tkw[t] = kw;
                        ttap[t] = (kd * g.kh + kh) * g.kw + kw;
                    }
                ++ntap;   // host guarantees <= NT
            }
        }
    }
    // input voxel iw = rw + k * sw: its tap kw (kw = (rw + pw) mod sw, enumerated above) reaches output voxel k + (rw + pw - kw) / sw —
    // an exact, wave-uniform quotient per tap, so the voxel loop has no integer division
    int tq[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) tq[t] = (rw + g.pw - tkw[t]) / g.sw;
    int k = (int)threadIdx.x;
    for (int iw = rw + (int)threadIdx.x * g.sw; iw < g.wi; iw += 64 * g.sw, k += 64) {
        // (bias initialisation, tap FMAs and tile store are written out in each of the six kernels of this kind: shared, the code changed)
        float acc[CIT];
#pragma unroll
        for (int j = 0; j < CIT; ++j) acc[j] = (bias != nullptr && cit + j < g.ci) ? bias[cit + j] : 0.f;
        int64_t off[NT];
        unsigned okm = 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int ow = k + tq[t];
            const bool ok = t < ntap && (unsigned)ow < (unsigned)g.wo;
            okm |= ok ? (1u << t) : 0u;
            off[t] = rowoff[t] + (int64_t)(ok ? ow : 0) * g.y_ld;
        }
        for (int co = 0; co < g.co; co += 4) {
            float4 gv[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) gv[t] = ldf4(dy + off[t] + co);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bool ok = (okm >> t) & 1u;
                const float g0 = ok ? gv[t].x : 0.f, g1 = ok ? gv[t].y : 0.f, g2 = ok ? gv[t].z : 0.f, g3 = ok ? gv[t].w : 0.f;
                const float* w0 = wp + ((size_t)ttap[t] * g.co + co) * CiP + cit;
#pragma unroll
                for (int j = 0; j < CIT; ++j) {
                    acc[j] = fmaf(g0, w0[j], acc[j]);
                    acc[j] = fmaf(g1, w0[CiP + j], acc[j]);
                    acc[j] = fmaf(g2, w0[2 * CiP + j], acc[j]);
                    acc[j] = fmaf(g3, w0[3 * CiP + j], acc[j]);
                }
            }
        }
        T* xp = dx + ((((int64_t)n * g.di + id) * g.hi + ih) * g.wi + iw) * g.x_ld + cit;
        if (CIT % 4 == 0 && cit + CIT <= g.ci && (g.x_ld & 3) == 0) {
#pragma unroll
            for (int j = 0; j < CIT; j += 4) stf4(xp + j, make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]));
        } else {
#pragma unroll
            for (int j = 0; j < CIT; ++j)
                if (cit + j < g.ci) stf(xp + j, acc[j]);
        }
    }
}

// ------------------------------------------------------------------ weight gradient
// grid = (voxel-chunk blocks, taps, item groups).  A block stages CH output voxels of dy and the tap-shifted x
// rows in LDS, and each thread owns a 4(ci) x 4(co) register tile of dW (or, for tiny Ci*Co, a voxel sub-group of
// it that is reduced through LDS at the end).  Per-block partials go to the workspace and are summed by
// wgrad_reduce_kernel in a fixed order (deterministic, no float atomics).
constexpr int kWgCH = 64;   // output voxels per chunk
constexpr int kWgIPT = 4;   // 4x4 items per thread (when Ci4*Co4 > 256)

template <typename T>
__global__ void __launch_bounds__(256)
conv_wgrad_generic_kernel(Mri3dConvGeom g, const T* __restrict__ x, const T* __restrict__ dy,
                          float* __restrict__ part, float* __restrict__ bias_part, int Ci4, int Co4, int nitems,
                          int vsplit) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int CiP = Ci4 * 4, CoP = Co4 * 4;
    float* dy_s = smem;                       // [CH][CoP]
    float* x_s = dy_s + kWgCH * CoP;          // [CH][CiP]
    int64_t* off_s = reinterpret_cast<int64_t*>(x_s + kWgCH * CiP);  // [CH] input voxel offset or -1
    float* red_s = reinterpret_cast<float*>(off_s + kWgCH);          // [256][16] (vsplit > 1 only)

    const int tap = blockIdx.y;
    const int kw_ = tap % g.kw, kh_ = (tap / g.kw) % g.kh, kd_ = tap / (g.kw * g.kh);
    const int tid = threadIdx.x;
    const int64_t nvox = (int64_t)g.n * g.dout * g.ho * g.wo;
    const int64_t nchunks = (nvox + kWgCH - 1) / kWgCH;

    // item ownership
    int my_item[kWgIPT];
    int vg = 0;
    if (vsplit > 1) {
        my_item[0] = tid % nitems;
        vg = tid / nitems;
        if (vg >= vsplit) my_item[0] = -1;
#pragma unroll
        for (int j = 1; j < kWgIPT; ++j) my_item[j] = -1;
    } else {
#pragma unroll
        for (int j = 0; j < kWgIPT; ++j) {
            int it = blockIdx.z * (256 * kWgIPT) + j * 256 + tid;
            my_item[j] = it < nitems ? it : -1;
        }
    }
    float acc[kWgIPT][16];
#pragma unroll
    for (int j = 0; j < kWgIPT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    float bsum = 0.f;
    const bool do_bias = (bias_part != nullptr) && tap == 0 && blockIdx.z == 0;

    for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int64_t v0 = ch * kWgCH;
        if (tid < kWgCH) {
            int64_t v = v0 + tid;
            int64_t off = -1;
            if (v < nvox) {
                int n, od, oh, ow;
                decode_voxel(v, g.dout, g.ho, g.wo, n, od, oh, ow);
                int id = od * g.sd - g.pd + kd_ * g.dd;
                int ih = oh * g.sh - g.ph + kh_ * g.dh;
                int iw = ow * g.sw - g.pw + kw_ * g.dw;
                if ((unsigned)id < (unsigned)g.di && (unsigned)ih < (unsigned)g.hi && (unsigned)iw < (unsigned)g.wi)
                    off = ((((int64_t)n * g.di + id) * g.hi + ih) * g.wi + iw) * g.x_ld;
            }
            off_s[tid] = off;
        }
        __syncthreads();
        for (int i = tid; i < kWgCH * CoP; i += 256) {
            int vv = i / CoP, c = i - vv * CoP;
            int64_t v = v0 + vv;
            dy_s[i] = (v < nvox && c < g.co) ? ldf(dy + v * g.y_ld + c) : 0.f;
        }
        for (int i = tid; i < kWgCH * CiP; i += 256) {
            int vv = i / CiP, c = i - vv * CiP;
            int64_t off = off_s[vv];
            x_s[i] = (off >= 0 && c < g.ci) ? ldf(x + off + c) : 0.f;
        }
        __syncthreads();
        if (do_bias && tid < g.co) {
            float s = 0.f;
            for (int vv = 0; vv < kWgCH; ++vv) s += dy_s[vv * CoP + tid];
            bsum += s;
        }
#pragma unroll
        for (int j = 0; j < kWgIPT; ++j) {
            if (my_item[j] < 0) continue;
            const int ci4 = my_item[j] / Co4, co4 = my_item[j] - ci4 * Co4;
            for (int vv = vg; vv < kWgCH; vv += vsplit) {
                float4 xv = *reinterpret_cast<const float4*>(x_s + vv * CiP + ci4 * 4);
                float4 gv = *reinterpret_cast<const float4*>(dy_s + vv * CoP + co4 * 4);
                acc[j][0] = fmaf(xv.x, gv.x, acc[j][0]);
                acc[j][1] = fmaf(xv.x, gv.y, acc[j][1]);
                acc[j][2] = fmaf(xv.x, gv.z, acc[j][2]);
                acc[j][3] = fmaf(xv.x, gv.w, acc[j][3]);
                acc[j][4] = fmaf(xv.y, gv.x, acc[j][4]);
                acc[j][5] = fmaf(xv.y, gv.y, acc[j][5]);
                acc[j][6] = fmaf(xv.y, gv.z, acc[j][6]);
                acc[j][7] = fmaf(xv.y, gv.w, acc[j][7]);
                acc[j][8] = fmaf(xv.z, gv.x, acc[j][8]);
                acc[j][9] = fmaf(xv.z, gv.y, acc[j][9]);
                acc[j][10] = fmaf(xv.z, gv.z, acc[j][10]);
                acc[j][11] = fmaf(xv.z, gv.w, acc[j][11]);
                acc[j][12] = fmaf(xv.w, gv.x, acc[j][12]);
                acc[j][13] = fmaf(xv.w, gv.y, acc[j][13]);
                acc[j][14] = fmaf(xv.w, gv.z, acc[j][14]);
                acc[j][15] = fmaf(xv.w, gv.w, acc[j][15]);
            }
        }
        __syncthreads();
    }

    // partial layout: part[blockIdx.x][tap][ciP][coP]
    const int taps = g.kd * g.kh * g.kw;
    float* my_part = part + ((size_t)blockIdx.x * taps + tap) * CiP * CoP;
    if (vsplit > 1) {
#pragma unroll
        for (int e = 0; e < 16; ++e) red_s[tid * 16 + e] = acc[0][e];
        __syncthreads();
        if (vg == 0 && my_item[0] >= 0) {
            const int ci4 = my_item[0] / Co4, co4 = my_item[0] - ci4 * Co4;
            float s[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            for (int q = 0; q < vsplit; ++q)
#pragma unroll
                for (int e = 0; e < 16; ++e) s[e] += red_s[(q * nitems + my_item[0]) * 16 + e];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) my_part[(ci4 * 4 + a) * CoP + co4 * 4 + b] = s[a * 4 + b];
        }
    } else {
#pragma unroll
        for (int j = 0; j < kWgIPT; ++j) {
            if (my_item[j] < 0) continue;
            const int ci4 = my_item[j] / Co4, co4 = my_item[j] - ci4 * Co4;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) my_part[(ci4 * 4 + a) * CoP + co4 * 4 + b] = acc[j][a * 4 + b];
        }
    }
    if (do_bias && tid < g.co) bias_part[(size_t)blockIdx.x * g.co + tid] = bsum;
}

// dw[co][ci][tap] = sum_b part[b][tap][ci][co]; dbias[co] = sum_b bias_part[b][co]
// 32 lanes per output element stride over the per-block partials; lane sums are combined in a fixed order (double).
__global__ void __launch_bounds__(256)
wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias_part, float* __restrict__ dw,
                    float* __restrict__ dbias, int nb, int taps, int Ci, int Co, int CiP, int CoP) {
    __shared__ double red[256];
    const int el = threadIdx.x >> 5, ql = threadIdx.x & 31;
    const int nw = Co * Ci * taps, ntot = nw + (dbias != nullptr ? Co : 0);
    const int i = blockIdx.x * 8 + el;
    double s = 0.0;
    if (i < nw) {
        const int tap = i % taps, ci = (i / taps) % Ci, co = i / (taps * Ci);
        const float* p = part + ((size_t)tap * CiP + ci) * CoP + co;
        const size_t stride = (size_t)taps * CiP * CoP;
        for (int b = ql; b < nb; b += 32) s += (double)p[b * stride];
    } else if (i < ntot) {
        for (int b = ql; b < nb; b += 32) s += (double)bias_part[(size_t)b * Co + (i - nw)];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (ql == 0 && i < ntot) {
        double t = 0.0;
        for (int k = 0; k < 32; ++k) t += red[el * 32 + k];
        if (i < nw) dw[i] = (float)t;
        else dbias[i - nw] = (float)t;
    }
}

// ------------------------------------------------------------------ weight gradient, few-taps variant
// Separable (k,1,1)/(1,k,1)/(1,1,k) convs (k <= 8 taps) with narrow channels are pure HBM streams: AI ~ 6 FLOP/B.  The
// chunked kernel above spends its time on per-chunk barriers there (147 GB/s on the 6x1x1 1->8 layer).  Here a thread
// owns (voxel lane, input channel): it walks output voxels grid-stride, reads dy[v][0..8) and its x value at every tap,
// and keeps a taps x 8 block of dW in registers; lanes are combined through LDS (double) once per block, one partial
// per block in the layout wgrad_reduce_kernel expects, fixed-order final sum => deterministic.
constexpr int kSmTaps = 8, kSmCo = 8;

template <typename T>
__global__ void __launch_bounds__(256)
conv_wgrad_small_kernel(Mri3dConvGeom g, const T* __restrict__ x, const T* __restrict__ dy,
                        float* __restrict__ part, float* __restrict__ bias_part, int CiL, int CiP, int CoP) {
    __shared__ float red[256 * kSmCo];
    const int taps = g.kd * g.kh * g.kw;
    const int tid = threadIdx.x;
    const int cil = tid % CiL, vl = tid / CiL, VL = 256 / CiL;
    const int ci = blockIdx.z * CiL + cil;
    const int co0 = blockIdx.y * kSmCo;
    const bool ci_ok = ci < g.ci;
    const bool vec_dy = co0 + kSmCo <= g.co && (g.y_ld & 3) == 0 && ((uintptr_t)dy & (4 * sizeof(T) - 1)) == 0;
    float acc[kSmTaps][kSmCo], bsum[kSmCo];
#pragma unroll
    for (int t = 0; t < kSmTaps; ++t)
#pragma unroll
        for (int c = 0; c < kSmCo; ++c) acc[t][c] = 0.f;
#pragma unroll
    for (int c = 0; c < kSmCo; ++c) bsum[c] = 0.f;
    const int64_t per_n = (int64_t)g.dout * g.ho * g.wo;
    const int64_t nvox = (int64_t)g.n * per_n;
    for (int64_t v = (int64_t)blockIdx.x * VL + vl; v < nvox; v += (int64_t)gridDim.x * VL) {
        const int n = (int)(v / per_n);   // (this decode is written out here and in the other per-sample walk: shared, the code changed)
        unsigned r = (unsigned)(v - (int64_t)n * per_n);
        const int ow = r % g.wo;
        r /= g.wo;
        const int oh = r % g.ho, od = r / g.ho;
        float gv[kSmCo];
        if (vec_dy) {
            const T* q = dy + v * g.y_ld + co0;
            const float4 a = ldf4(q), b = ldf4(q + 4);
            gv[0] = a.x, gv[1] = a.y, gv[2] = a.z, gv[3] = a.w, gv[4] = b.x, gv[5] = b.y, gv[6] = b.z, gv[7] = b.w;
        } else {
#pragma unroll
            for (int c = 0; c < kSmCo; ++c) gv[c] = (co0 + c < g.co) ? ldf(dy + v * g.y_ld + co0 + c) : 0.f;
        }
        if (cil == 0) {
#pragma unroll
            for (int c = 0; c < kSmCo; ++c) bsum[c] += gv[c];
        }
        const T* xn = x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld + ci;
#pragma unroll
        for (int t = 0; t < kSmTaps; ++t) {
            if (t < taps) {
                const int kw = t % g.kw, kh = (t / g.kw) % g.kh, kd = t / (g.kw * g.kh);
                const int id = od * g.sd - g.pd + kd * g.dd, ih = oh * g.sh - g.ph + kh * g.dh, iw = ow * g.sw - g.pw + kw * g.dw;
                const bool ok = ci_ok && (unsigned)id < (unsigned)g.di && (unsigned)ih < (unsigned)g.hi &&
                                (unsigned)iw < (unsigned)g.wi;
                const float xv = ok ? ldf(xn + (((int64_t)id * g.hi + ih) * g.wi + iw) * g.x_ld) : 0.f;
#pragma unroll
                for (int c = 0; c < kSmCo; ++c) acc[t][c] = fmaf(xv, gv[c], acc[t][c]);
            }
        }
    }
    // combine the VL voxel lanes of every (tap, ci) through LDS, in double, in a fixed order
    for (int t = 0; t < taps; ++t) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kSmCo; ++c) {
            float val = 0.f;
#pragma unroll
            for (int tt = 0; tt < kSmTaps; ++tt)
                if (tt == t) val = acc[tt][c];
            red[tid * kSmCo + c] = val;
        }
        __syncthreads();
        for (int o = tid; o < CiL * kSmCo; o += 256) {
            const int c = o % kSmCo, cl = o / kSmCo;
            double sdbl = 0.0;
            for (int l = 0; l < VL; ++l) sdbl += (double)red[(l * CiL + cl) * kSmCo + c];
            const int cig = blockIdx.z * CiL + cl;
            if (cig < g.ci && co0 + c < g.co)
                part[(((size_t)blockIdx.x * taps + t) * CiP + cig) * CoP + co0 + c] = (float)sdbl;
        }
    }
    if (bias_part != nullptr && blockIdx.z == 0) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kSmCo; ++c) red[tid * kSmCo + c] = (cil == 0) ? bsum[c] : 0.f;
        __syncthreads();
        if (tid < kSmCo && co0 + tid < g.co) {
            double sdbl = 0.0;
            for (int l = 0; l < VL; ++l) sdbl += (double)red[(l * CiL) * kSmCo + tid];
            bias_part[(size_t)blockIdx.x * g.co + co0 + tid] = (float)sdbl;
        }
    }
}

// ------------------------------------------------------------------ weight gradient, few taps, channel QUADS
// The encoder's separable convs (AE_model.py:9-26: (6,1,1)/(1,6,1)/(1,1,6) stride 2, 8 -> 8 ... 32 -> 32) have Ci, Co in multiples
// of 4.  In the per-channel kernel above the 8 lanes of a voxel each fetch ONE 4-byte x value per tap and all re-read the same 32
// bytes of dy: 8 load instructions per lane for 56 bytes (0.84 TB/s on 8 -> 8 (1,6,1) at 80x96x160).  Here a lane owns (voxel,
// input-channel quad, output-channel quad): one 16-byte x load per tap, one 16-byte dy load, a taps x 4 x 4 register block.
// Voxels are walked slab-wise — (n, od, h-chunk) per workgroup iteration, 32-bit arithmetic per element — instead of decoding a
// 64-bit flat index per voxel.  Lanes are combined through LDS (double) once per workgroup: same partial layout and final
// fixed-order sum as above (deterministic).
// NTAPS = 4, 6 or 8 accumulator slots (the smallest that holds the filter: fewer registers, more resident waves to cover the latency)
// CIV = input channels per lane: 4 (Ci % 4 == 0) or 1 (Ci = 1: the autoencoder's first conv, (6,1,1) 1 -> 8)
template <typename T, int NTAPS, int CIV>
__global__ void __launch_bounds__(256)
conv_wgrad_quads_kernel(Mri3dConvGeom g, const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part,
                        float* __restrict__ bias_part, int QI, int QO, int hch, int CiP, int CoP) {
    __shared__ float red[256 * 16];
    const int taps = g.kd * g.kh * g.kw;
    const int tid = threadIdx.x;
    const int PV = QI * QO, VL = 256 / PV;           // lanes per voxel, voxel lanes per workgroup (PV divides 256: host)
    const int pq = tid % PV, vl = tid / PV;
    const int iq = pq % QI, oq = pq / QI;
    float acc[NTAPS][CIV][4], bsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NTAPS; ++t)
#pragma unroll
        for (int a = 0; a < CIV; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[t][a][b] = 0.f;
    // tap offsets in voxels per axis and as ONE element offset (all wave-uniform): a tap's address is the voxel's base offset plus
    // a scalar — no clamps, no multiplications per tap (they were 230 of the 330 instructions per voxel of the 8 -> 8 layer)
    // (the table of conv_fwd_taps_kernel, written out in both: shared, the code changed)
    int tdd[NTAPS], tdh[NTAPS], tdw[NTAPS];
    int64_t tdelta[NTAPS];
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) {
        const int tt = t < taps ? t : 0;
        tdw[t] = (tt % g.kw) * g.dw, tdh[t] = ((tt / g.kw) % g.kh) * g.dh, tdd[t] = (tt / (g.kw * g.kh)) * g.dd;
        tdelta[t] = (((int64_t)tdd[t] * g.hi + tdh[t]) * g.wi + tdw[t]) * g.x_ld;
    }
    const int hchunks = (g.ho + hch - 1) / hch;
    const int slabs = g.n * g.dout * hchunks;
    for (int slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
        const int hc = slab % hchunks, nd = slab / hchunks;
        const int n = nd / g.dout, od = nd - n * g.dout;
        const int h0 = hc * hch, hn = min(hch, g.ho - h0);
        const unsigned inner = (unsigned)hn * g.wo;
        const T* xn = x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld + CIV * iq;
        const T* yn = dy + (((int64_t)nd * g.ho + h0) * g.wo) * g.y_ld + 4 * oq;
        // ALL tap loads of a voxel first, unconditional (clamped address, masked afterwards; taps past the filter re-read tap 0):
        // a load inside `if (ok)` / `if (t < taps)` is followed by its own s_waitcnt and the taps become serial round trips to
        // L2 (7 per voxel: 0.51 ms on the (1,6,1) 8 -> 8 layer at 80x96x160, waves waiting 73 % of their cycles; batched 0.31 ms).
        auto fetch = [&](unsigned e, float4& gv, float (&xv)[NTAPS][CIV], unsigned& okm) {
            const bool live = e < inner;
            const unsigned ec = live ? e : inner - 1;
            const int ow = ec % g.wo, oh = h0 + ec / g.wo;
            gv = ldf4(yn + (int64_t)ec * g.y_ld);
            okm = 0;
            const int id0 = od * g.sd - g.pd, ih0 = oh * g.sh - g.ph, iw0 = ow * g.sw - g.pw;
            const int64_t base = (((int64_t)id0 * g.hi + ih0) * g.wi + iw0) * g.x_ld;
#pragma unroll
            for (int t = 0; t < NTAPS; ++t) {
                const bool ok = live && t < taps && (unsigned)(id0 + tdd[t]) < (unsigned)g.di && (unsigned)(ih0 + tdh[t]) < (unsigned)g.hi &&
                                (unsigned)(iw0 + tdw[t]) < (unsigned)g.wi;
                okm |= ok ? (1u << t) : 0u;
                const T* xp = xn + (ok ? base + tdelta[t] : 0);   // a tap outside the volume re-reads the sample's first voxel and is masked
                if constexpr (CIV == 4) {
                    const float4 q4 = ldf4(xp);
                    xv[t][0] = q4.x, xv[t][1] = q4.y, xv[t][2] = q4.z, xv[t][3] = q4.w;
                } else {
                    xv[t][0] = ldf(xp);
                }
            }
            if (!live) gv = make_float4(0.f, 0.f, 0.f, 0.f);
        };
        auto consume = [&](const float4& gv, const float (&xv)[NTAPS][CIV], unsigned okm) {
            const float gq[4] = {gv.x, gv.y, gv.z, gv.w};
            if (iq == 0) {
#pragma unroll
                for (int b = 0; b < 4; ++b) bsum[b] += gq[b];
            }
#pragma unroll
            for (int t = 0; t < NTAPS; ++t) {
                const bool ok = (okm >> t) & 1u;
#pragma unroll
                for (int a = 0; a < CIV; ++a) {
                    const float xa = ok ? xv[t][a] : 0.f;
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[t][a][b] = fmaf(xa, gq[b], acc[t][a][b]);
                }
            }
        };
        // (a second register set for the next voxel's loads was measured: with 128 accumulators it pushes the kernel to 256 VGPRs
        //  and 80 spilled SGPRs and is slower, 0.50 vs 0.31 ms; fewer accumulator slots and more waves hide the latency instead)
        for (unsigned e = vl; e < inner; e += VL) {
            float4 gv;
            float xv[NTAPS][CIV];
            unsigned okm;
            fetch(e, gv, xv, okm);
            consume(gv, xv, okm);
        }
    }
    // combine the VL voxel lanes of every (tap, ci, co) through LDS, in double, in a fixed order
    for (int t = 0; t < taps; ++t) {
        __syncthreads();
#pragma unroll
        for (int a = 0; a < CIV; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float val = 0.f;
#pragma unroll
                for (int tt = 0; tt < NTAPS; ++tt)
                    if (tt == t) val = acc[tt][a][b];
                red[tid * 16 + a * 4 + b] = val;
            }
        __syncthreads();
        for (int o = tid; o < PV * (CIV * 4); o += 256) {
            const int ab = o % (CIV * 4), q = o / (CIV * 4);
            double sdbl = 0.0;
            for (int l = 0; l < VL; ++l) sdbl += (double)red[(l * PV + q) * 16 + ab];
            const int ci = (q % QI) * CIV + ab / 4, co = (q / QI) * 4 + ab % 4;
            if (ci < g.ci && co < g.co) part[(((size_t)blockIdx.x * taps + t) * CiP + ci) * CoP + co] = (float)sdbl;
        }
    }
    if (bias_part != nullptr) {
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 4; ++b) red[tid * 4 + b] = (iq == 0) ? bsum[b] : 0.f;
        __syncthreads();
        if (tid < g.co) {
            double sdbl = 0.0;
            for (int l = 0; l < VL; ++l) sdbl += (double)red[((l * PV) + (tid / 4) * QI) * 4 + (tid % 4)];
            bias_part[(size_t)blockIdx.x * g.co + tid] = (float)sdbl;
        }
    }
}

// ------------------------------------------------------------------ weight gradient, few taps, ONE output channel
// The decoder's last separable convs end in a single channel (8 -> 1 and 1 -> 1 with (3,1,1)/(1,3,1)/(1,1,3) kernels at full
// resolution, AE_model.py:110-160).  In the kernel above a lane owns one input channel and reads it 4 bytes at a time while 7 of
// its 8 output-channel slots stay empty (1.32 ms for 8 -> 1 on 4 x 160x192x160, 536 GB/s).  Here a lane owns a VOXEL: one dy
// value, CI input channels per tap as 16-byte loads, taps x CI accumulators; lanes are combined with DPP wave sums.
template <typename T, int CI>
__global__ void __launch_bounds__(256)
conv_wgrad_co1_kernel(Mri3dConvGeom g, const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part,
                      float* __restrict__ bias_part) {
    __shared__ float red[4][kSmTaps * CI + 1];
    const int taps = g.kd * g.kh * g.kw;
    const int tid = threadIdx.x;
    float acc[kSmTaps][CI], bsum = 0.f;
#pragma unroll
    for (int t = 0; t < kSmTaps; ++t)
#pragma unroll
        for (int c = 0; c < CI; ++c) acc[t][c] = 0.f;
    const int64_t per_n = (int64_t)g.dout * g.ho * g.wo;
    const int64_t nvox = (int64_t)g.n * per_n;
    for (int64_t v = (int64_t)blockIdx.x * 256 + tid; v < nvox; v += (int64_t)gridDim.x * 256) {
        const int n = (int)(v / per_n);   // (this decode is written out here and in the other per-sample walk: shared, the code changed)
        unsigned r = (unsigned)(v - (int64_t)n * per_n);
        const int ow = r % g.wo;
        r /= g.wo;
        const int oh = r % g.ho, od = r / g.ho;
        const float gv = ldf(dy + v * g.y_ld);
        bsum += gv;
        const T* xn = x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld;
#pragma unroll
        for (int t = 0; t < kSmTaps; ++t) {
            if (t < taps) {
                const int kw = t % g.kw, kh = (t / g.kw) % g.kh, kd = t / (g.kw * g.kh);
                const int id = od * g.sd - g.pd + kd * g.dd, ih = oh * g.sh - g.ph + kh * g.dh, iw = ow * g.sw - g.pw + kw * g.dw;
                const bool ok = (unsigned)id < (unsigned)g.di && (unsigned)ih < (unsigned)g.hi && (unsigned)iw < (unsigned)g.wi;
                const T* xp = xn + (((int64_t)min(max(id, 0), g.di - 1) * g.hi + min(max(ih, 0), g.hi - 1)) * g.wi +
                                    min(max(iw, 0), g.wi - 1)) * g.x_ld;
                const float gm = ok ? gv : 0.f;
                if constexpr (CI == 1) {
                    acc[t][0] = fmaf(ldf(xp), gm, acc[t][0]);
                } else {
#pragma unroll
                    for (int c = 0; c < CI; c += 4) {
                        const float4 q = ldf4(xp + c);
                        acc[t][c] = fmaf(q.x, gm, acc[t][c]);
                        acc[t][c + 1] = fmaf(q.y, gm, acc[t][c + 1]);
                        acc[t][c + 2] = fmaf(q.z, gm, acc[t][c + 2]);
                        acc[t][c + 3] = fmaf(q.w, gm, acc[t][c + 3]);
                    }
                }
            }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int t = 0; t < kSmTaps; ++t)
#pragma unroll
        for (int c = 0; c < CI; ++c) {
            const float vsum = wave_sum_dpp(acc[t][c]);
            if (lane == 0) red[wave][t * CI + c] = vsum;
        }
    {
        const float vsum = wave_sum_dpp(bsum);
        if (lane == 0) red[wave][kSmTaps * CI] = vsum;
    }
    __syncthreads();
    if (tid < taps * CI)   // part[blk][tap][ci][co = 0]
        part[(size_t)blockIdx.x * taps * CI + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    else if (tid == kSmTaps * CI && bias_part)
        bias_part[blockIdx.x] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

constexpr int kCo1Blocks = 1024;

static bool wgrad_co1_ok(const Mri3dConvGeom& g) {
    static const int off = tuning_knob("MRI3D_CO1_OFF", 0);   // tuning aid (A/B)
    return !off && g.co == 1 && g.kd * g.kh * g.kw <= kSmTaps && (g.ci == 1 || ((g.ci == 4 || g.ci == 8 || g.ci == 16) && g.x_ld % 4 == 0)) &&
           (int64_t)g.dout * g.ho * g.wo < 0x7fffffffLL;
}

// ------------------------------------------------------------------ first layer: 3x3x3, stride 1, pad 1, ONE input channel
// unet.UNet / Modified3DUNet / CNN all start with Conv3d(1, 8|16, 3, padding=1) on the whole volume.  With Cin = 1 there is
// no GEMM to speak of (K = 27): forward reads 4 B and writes 4*Co B per voxel, the weight gradient reads both, and 27*Co
// FMAs per voxel keep the VALUs about as busy as HBM (~0.05 ms each per 2 x 160x192x160 volumes).  The generic forward
// kernel needs 0.39 ms there and the CK = 1 MFMA weight gradient 0.47 ms; these two take 0.18 and 0.25 ms:
//   forward: a 4 x 8 x (8*VPT) voxel tile of x (+halo) sits in LDS, a lane owns VPT consecutive voxels along W and all Co
//            outputs; per (kd, kh) it reads its VPT+2 inputs once and reuses them for the 3 kw taps; weights are broadcast
//            LDS reads.
//   wgrad:   the same tile, but a workgroup owns ONE kd plane of the filter (9*Co accumulators per lane instead of 27*Co) and
//            walks its share of the tiles; the three kd workgroups of a share sit next to each other on one XCD so that dy is
//            fetched from HBM once.  Lanes are combined by wave shuffles + LDS in a fixed order, one partial per
//            workgroup, then wgrad_reduce_kernel (deterministic).
constexpr int C1D = 4, C1H = 8, C1WQ = 8;   // tile: 4 x 8 x (8*VPT) voxels, 256 lanes

template <int CO> struct Cin1 { static constexpr int VPT = CO <= 8 ? 4 : 2; };
typedef float f32x2 __attribute__((ext_vector_type(2)));

// tile index -> sample and origin of a C1D x C1H x TW voxel tile
__device__ __forceinline__ void decode_tile(int t, int tilesD, int tilesH, int tilesW, int TW, int& n, int& d0, int& h0, int& w0) {
    w0 = (t % tilesW) * TW;
    t /= tilesW;
    h0 = (t % tilesH) * C1H;
    t /= tilesH;
    d0 = (t % tilesD) * C1D;
    n = t / tilesD;
}

// stage rows [dlo, dlo+ND) x (C1H+2) x (TW+2) of the zero-padded input around tile origin (d0, h0, w0) into LDS
template <typename T, int TW, int ND, int NTHR = 256>
__device__ __forceinline__ void cin1_stage(float* xs, const T* __restrict__ xn, const Mri3dConvGeom& g, int dlo, int h0,
                                           int w0, int tid) {
    constexpr int PW = TW + 4, NE = ND * (C1H + 2) * (TW + 2);
    for (int e = tid; e < NE; e += NTHR) {
        const int fw = e % (TW + 2), r = e / (TW + 2);
        const int fh = r % (C1H + 2), fd = r / (C1H + 2);
        const int id = dlo + fd, ih = h0 - 1 + fh, iw = w0 - 1 + fw;
        const bool ok = (unsigned)id < (unsigned)g.di && (unsigned)ih < (unsigned)g.hi && (unsigned)iw < (unsigned)g.wi;
        const int cd = min(max(id, 0), g.di - 1), ch = min(max(ih, 0), g.hi - 1), cw = min(max(iw, 0), g.wi - 1);
        const float v = ldf(xn + (((int64_t)cd * g.hi + ch) * g.wi + cw) * g.x_ld);
        xs[(fd * (C1H + 2) + fh) * PW + fw] = ok ? v : 0.f;
    }
}

template <typename T, int CO>
__global__ void __launch_bounds__(256)
conv_cin1_fwd_kernel(Mri3dConvGeom g, const T* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                     T* __restrict__ y, int tilesD, int tilesH, int tilesW, int ntiles) {
    // wp = repacked weights [tap][co].  They live in LDS and are re-read (broadcast) per (kd, kh) row through a pointer the
    // compiler cannot see through: left to itself it hoists all 27*Co loop-invariant weights out of the tile loop
    // (398 VGPRs+AGPRs, one wave per SIMD; as scalar loads: spilled to VGPR lanes, 722 v_readlane per tile).
    constexpr int VPT = Cin1<CO>::VPT, TW = C1WQ * VPT, PW = TW + 4;
    __shared__ __attribute__((aligned(16))) float xs[(C1D + 2) * (C1H + 2) * PW];
    __shared__ __attribute__((aligned(16))) float wsh[27 * CO];
    const int tid = threadIdx.x;
    for (int e = tid; e < 27 * CO; e += 256) wsh[e] = wp[e];
    const int wq = tid % C1WQ, hl = (tid / C1WQ) % C1H, dl = tid / (C1WQ * C1H);
    float bv[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) bv[c] = bias ? bias[c] : 0.f;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int n, d0, h0, w0;
        decode_tile(tile, tilesD, tilesH, tilesW, TW, n, d0, h0, w0);
        __syncthreads();
        cin1_stage<T, TW, C1D + 2>(xs, x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld, g, d0 - 1, h0, w0, tid);
        __syncthreads();
        f32x2 acc[VPT][CO / 2];   // channel pairs: v_pk_fma_f32
#pragma unroll
        for (int v = 0; v < VPT; ++v)
#pragma unroll
            for (int c = 0; c < CO / 2; ++c) acc[v][c] = f32x2{bv[2 * c], bv[2 * c + 1]};
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const float* row = xs + ((dl + kd) * (C1H + 2) + hl + kh) * PW + wq * VPT;
                float r[VPT + 2];
#pragma unroll
                for (int i = 0; i < VPT + 2; ++i) r[i] = row[i];
                int woff = (kd * 3 + kh) * 3 * CO;
                asm volatile("" : "+v"(woff));              // opaque offset: the weight reads stay inside the tile loop ...
                __builtin_amdgcn_sched_barrier(0);          // ... and inside their (kd, kh) group
                const float* wrow = wsh + woff;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float* wt = wrow + kw * CO;
#pragma unroll
                    for (int c = 0; c < CO / 2; ++c) {
                        const f32x2 wv = f32x2{wt[2 * c], wt[2 * c + 1]};
#pragma unroll
                        for (int v = 0; v < VPT; ++v)
                            acc[v][c] = __builtin_elementwise_fma(f32x2{r[v + kw], r[v + kw]}, wv, acc[v][c]);
                    }
                }
            }
        // results are pinned here: otherwise the compiler sinks each voxel's 27*Co FMAs into its bounds-checked store below
        // and keeps every weight and input row of the tile alive across all of them (256 VGPRs + AGPR traffic)
#pragma unroll
        for (int v = 0; v < VPT; ++v)
#pragma unroll
            for (int c = 0; c < CO / 2; ++c) asm volatile("" : "+v"(acc[v][c]));
        const int od = d0 + dl, oh = h0 + hl;
        if (od < g.dout && oh < g.ho) {
            T* yo = y + ((((int64_t)n * g.dout + od) * g.ho + oh) * g.wo + w0 + wq * VPT) * g.y_ld;
#pragma unroll
            for (int v = 0; v < VPT; ++v)
                if (w0 + wq * VPT + v < g.wo) {
#pragma unroll
                    for (int c = 0; c < CO; c += 4)
                        stf4(yo + (int64_t)v * g.y_ld + c,
                             make_float4(acc[v][c / 2].x, acc[v][c / 2].y, acc[v][c / 2 + 1].x, acc[v][c / 2 + 1].y));
                }
        }
    }
}

template <typename T, int CO>
__global__ void __launch_bounds__(768)
conv_cin1_wgrad_kernel(Mri3dConvGeom g, const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part,
                       float* __restrict__ bias_part, int tilesD, int tilesH, int tilesW, int ntiles, int nshares) {
    constexpr int VPT = Cin1<CO>::VPT, TW = C1WQ * VPT, PW = TW + 4, NA = 9 * CO + CO;
    __shared__ __attribute__((aligned(16))) float xs[(C1D + 2) * (C1H + 2) * PW];
    __shared__ float red[12][NA];
    // One workgroup of 12 waves per share: waves 4 kd .. 4 kd + 3 take the taps of plane kd of the SAME tile — x is staged once for
    // the three of them and their dy loads, issued within microseconds of each other on one CU, are served from its L1 / L2 (as three
    // workgroups per share each of them fetched dy: 3 x the gradient tensor, 0.23 ms for 2 x 160x192x160 fp32).
    const int kd = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);
    const int tid = threadIdx.x & 255;
    // blockIdx -> share, consecutive shares inside one XCD's contiguous range (gridDim.x = nshares, a multiple of 8)
    const int per_xcd = gridDim.x / 8;
    const int share = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    const int wq = tid % C1WQ, hl = (tid / C1WQ) % C1H, dl = tid / (C1WQ * C1H);
    f32x2 acc[3][3][CO / 2];   // channel pairs: v_pk_fma_f32
    float bsum[CO];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int c = 0; c < CO / 2; ++c) acc[a][b][c] = f32x2{0.f, 0.f};
#pragma unroll
    for (int c = 0; c < CO; ++c) bsum[c] = 0.f;
    for (int tile = share; tile < ntiles; tile += nshares) {
        int n, d0, h0, w0;
        decode_tile(tile, tilesD, tilesH, tilesW, TW, n, d0, h0, w0);
        __syncthreads();
        cin1_stage<T, TW, C1D + 2, 768>(xs, x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld, g, d0 - 1, h0, w0, (int)threadIdx.x);
        // this lane's VPT output voxels of dy (zero outside the volume)
        const int od = d0 + dl, oh = h0 + hl;
        f32x2 gy[VPT][CO / 2];
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int ow = w0 + wq * VPT + v;
            const bool ok = od < g.dout && oh < g.ho && ow < g.wo;
            const T* dp = dy + ((((int64_t)n * g.dout + min(od, g.dout - 1)) * g.ho + min(oh, g.ho - 1)) * g.wo +
                                min(ow, g.wo - 1)) * g.y_ld;
#pragma unroll
            for (int c = 0; c < CO; c += 4) {
                const float4 q = ldf4(dp + c);
                gy[v][c / 2] = f32x2{ok ? q.x : 0.f, ok ? q.y : 0.f};
                gy[v][c / 2 + 1] = f32x2{ok ? q.z : 0.f, ok ? q.w : 0.f};
            }
        }
        __syncthreads();
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const float* row = xs + ((dl + kd) * (C1H + 2) + hl + kh) * PW + wq * VPT;
            float r[VPT + 2];
#pragma unroll
            for (int i = 0; i < VPT + 2; ++i) r[i] = row[i];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int v = 0; v < VPT; ++v)
#pragma unroll
                    for (int c = 0; c < CO / 2; ++c)
                        acc[kh][kw][c] = __builtin_elementwise_fma(f32x2{r[v + kw], r[v + kw]}, gy[v][c], acc[kh][kw][c]);
        }
        if (kd == 1) {
#pragma unroll
            for (int v = 0; v < VPT; ++v)
#pragma unroll
                for (int c = 0; c < CO / 2; ++c) { bsum[2 * c] += gy[v][c].x; bsum[2 * c + 1] += gy[v][c].y; }
        }
    }
    // lanes -> wave with DPP adds inside the 16-lane rows + the four row sums (fixed order), waves -> workgroup through LDS
    // (ds_bpermute shuffles here cost 480 LDS round trips per workgroup, 40 % of its run time)
    const int lane = tid & 63, wave = (int)threadIdx.x >> 6;   // 0 .. 11; waves 4 kd .. 4 kd + 3 hold plane kd's taps
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                const float vsum = wave_sum_dpp((c & 1) ? acc[a][b][c / 2].y : acc[a][b][c / 2].x);
                if (lane == 0) red[wave][(a * 3 + b) * CO + c] = vsum;
            }
#pragma unroll
    for (int c = 0; c < CO; ++c) {
        const float vsum = wave_sum_dpp(bsum[c]);
        if (lane == 0) red[wave][9 * CO + c] = vsum;
    }
    __syncthreads();
    const int w0_ = 4 * kd;
    if (tid < 9 * CO) {
        const float t4 = (red[w0_][tid] + red[w0_ + 1][tid]) + (red[w0_ + 2][tid] + red[w0_ + 3][tid]);
        part[((size_t)share * 27 + kd * 9 + tid / CO) * CO + tid % CO] = t4;   // part[share][tap][ci = 0][co]
    } else if (tid < NA && kd == 1 && bias_part) {
        const int c = tid - 9 * CO;
        bias_part[(size_t)share * CO + c] = (red[w0_][tid] + red[w0_ + 1][tid]) + (red[w0_ + 2][tid] + red[w0_ + 3][tid]);
    }
}

// ------------------------------------------------------------------ first layer + its activation (no normalisation in between)
// unet.UNet's first ConvolutionalBlock is Conv3d(1, 8, 3, padding=1) + PReLU: as four launches z and its gradient cross HBM five
// times (conv -> z; z -> a; (z, da) -> dz; (x, dz) -> dW).  The two kernels below are conv_cin1_fwd_kernel and
// conv_cin1_wgrad_kernel with the activation folded in: every FMA chain and every summation order is theirs, so z, a, dW and db
// keep their bits, and the gradient of z exists in registers only.
//   a  = apply_act(fmaf(z, 1, 0), act, alpha)                  norm_act_fwd_kernel for mode none (scale 1, shift 0: -0 -> +0)
//   dz = z > 0 ? da : da * alpha                               norm_act_bwd_reduce_body's du; its (gm * is) * du is du for scale 1
//   dalpha = sum over z <= 0 of (double)da * (double)z         float64 per lane -> wave -> workgroup -> one pass, fixed order
struct Cin1Act {
    const float* alpha;   // PReLU's slopes (alpha_n of them: 1 or Co); not read for the other kinds
    int alpha_n, act;     // MRI3D_ACT_RELU | _LEAKY | _PRELU
    float slope;          // LeakyReLU
};

template <int CO>
__global__ void __launch_bounds__(256)
conv_cin1_act_fwd_kernel(Mri3dConvGeom g, const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                         Cin1Act pa, float* __restrict__ z, float* __restrict__ a, int a_ld, int tilesD, int tilesH, int tilesW,
                         int ntiles) {
    // tile, lane mapping and FMA chain of conv_cin1_fwd_kernel (see there for the two pins on the compiler).  The stores differ:
    // a lane's 4 x 8 (2 x 16) results are 128 contiguous bytes, and stored from the lane that computed them one instruction
    // writes 16 bytes per lane at a 128-byte stride (2.4 TB/s).  Each wave turns its 8 rows of 1 KB through LDS, four rows at a
    // time, so that one store instruction writes one whole row: lane l holds the l-th 16 bytes of it.
    constexpr int VPT = Cin1<CO>::VPT, TW = C1WQ * VPT, PW = TW + 4;
    constexpr int Q = CO / 4;             // 16-byte pieces per voxel
    constexpr int LS = VPT * CO + 4;      // floats between two lanes' results in the turn buffer (+16 B: the b128 writes hit distinct banks)
    constexpr int RS = C1WQ * LS;         // ... and between two rows
    __shared__ __attribute__((aligned(16))) float xs[(C1D + 2) * (C1H + 2) * PW];
    __shared__ __attribute__((aligned(16))) float wsh[27 * CO];
    __shared__ __attribute__((aligned(16))) float turn[C1D][4 * RS];
    const int tid = threadIdx.x;
    for (int e = tid; e < 27 * CO; e += 256) wsh[e] = wp[e];
    const int wq = tid % C1WQ, hl = (tid / C1WQ) % C1H, dl = tid / (C1WQ * C1H);   // dl = the wave
    float bv[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) bv[c] = bias ? bias[c] : 0.f;
    // after the turn: this lane's channel quad and its voxel along W in every row
    const int lane = tid & 63, tq = lane % Q, tv = lane / Q;
    const int toff = (tv / VPT) * LS + (tv % VPT) * CO + tq * 4;
    float al[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) al[j] = (pa.act == MRI3D_ACT_PRELU) ? pa.alpha[pa.alpha_n == 1 ? 0 : tq * 4 + j] : pa.slope;
    float sc = 1.f, sh = 0.f;             // norm_act_fwd_kernel's scale and shift without statistics, as run-time values: a real fma
    asm volatile("" : "+v"(sc), "+v"(sh));
    float* tw = turn[dl];
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int n, d0, h0, w0;
        decode_tile(tile, tilesD, tilesH, tilesW, TW, n, d0, h0, w0);
        __syncthreads();
        cin1_stage<float, TW, C1D + 2>(xs, x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld, g, d0 - 1, h0, w0, tid);
        __syncthreads();
        f32x2 acc[VPT][CO / 2];   // channel pairs: v_pk_fma_f32
#pragma unroll
        for (int v = 0; v < VPT; ++v)
#pragma unroll
            for (int c = 0; c < CO / 2; ++c) acc[v][c] = f32x2{bv[2 * c], bv[2 * c + 1]};
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const float* row = xs + ((dl + kd) * (C1H + 2) + hl + kh) * PW + wq * VPT;
                float r[VPT + 2];
#pragma unroll
                for (int i = 0; i < VPT + 2; ++i) r[i] = row[i];
                int woff = (kd * 3 + kh) * 3 * CO;
                asm volatile("" : "+v"(woff));
                __builtin_amdgcn_sched_barrier(0);
                const float* wrow = wsh + woff;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float* wt = wrow + kw * CO;
#pragma unroll
                    for (int c = 0; c < CO / 2; ++c) {
                        const f32x2 wv = f32x2{wt[2 * c], wt[2 * c + 1]};
#pragma unroll
                        for (int v = 0; v < VPT; ++v)
                            acc[v][c] = __builtin_elementwise_fma(f32x2{r[v + kw], r[v + kw]}, wv, acc[v][c]);
                    }
                }
            }
#pragma unroll
        for (int v = 0; v < VPT; ++v)
#pragma unroll
            for (int c = 0; c < CO / 2; ++c) asm volatile("" : "+v"(acc[v][c]));
        const int od = d0 + dl;
        // the turn buffer is the wave's own and a wave's LDS accesses complete in order: no workgroup barrier
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if ((hl >> 2) == half) {
                float* dst = tw + (hl & 3) * RS + wq * LS;
#pragma unroll
                for (int v = 0; v < VPT; ++v)
#pragma unroll
                    for (int c = 0; c < CO; c += 4)
                        *reinterpret_cast<float4*>(dst + v * CO + c) =
                            make_float4(acc[v][c / 2].x, acc[v][c / 2].y, acc[v][c / 2 + 1].x, acc[v][c / 2 + 1].y);
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 zq = *reinterpret_cast<const float4*>(tw + j * RS + toff);
                const int oh = h0 + half * 4 + j, ow = w0 + tv;
                if (od < g.dout && oh < g.ho && ow < g.wo) {
                    const int64_t vox = (((int64_t)n * g.dout + od) * g.ho + oh) * g.wo + ow;
                    stf4(z + vox * g.y_ld + tq * 4, zq);
                    stf4(a + vox * a_ld + tq * 4,
                         make_float4(apply_act(fmaf(zq.x, sc, sh), pa.act, al[0]), apply_act(fmaf(zq.y, sc, sh), pa.act, al[1]),
                                     apply_act(fmaf(zq.z, sc, sh), pa.act, al[2]), apply_act(fmaf(zq.w, sc, sh), pa.act, al[3])));
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

template <int CO>
__global__ void __launch_bounds__(768)
conv_cin1_act_bwd_kernel(Mri3dConvGeom g, const float* __restrict__ x, const float* __restrict__ z, const float* __restrict__ da,
                         int da_ld, Cin1Act pa, float* __restrict__ part, float* __restrict__ bias_part,
                         double* __restrict__ alpha_part, int tilesD, int tilesH, int tilesW, int ntiles, int nshares) {
    // conv_cin1_wgrad_kernel (see there) with dz = act'(z) * da where it read dy: same lanes, same accumulators, same order.
    // What differs is how the gradient reaches the lanes.  There every lane loads its own 128 bytes, 16 at a time, and the three
    // kd groups each load all of them: 64 cache lines per load instruction, 6144 line requests per tile, which is what the kernel
    // waits for (6 us per tile).  Here the twelve waves load z and da once, one whole 1 KB row per instruction, form dz and the
    // products for dalpha once per element, and hand dz to the compute lanes through LDS (conv_cin1_act_fwd_kernel's turn, the
    // other way round).  alpha_part[share][co] (may be NULL): this workgroup's float64 sum for dalpha.
    constexpr int VPT = Cin1<CO>::VPT, TW = C1WQ * VPT, PW = TW + 4, NA = 9 * CO + CO;
    constexpr int Q = CO / 4, LS = VPT * CO + 4, RS = C1WQ * LS, NROW = C1D * C1H, RPW = (NROW + 11) / 12;   // rows per wave
    __shared__ __attribute__((aligned(16))) float xs[(C1D + 2) * (C1H + 2) * PW];
    __shared__ __attribute__((aligned(16))) float dzs[NROW * RS];
    __shared__ float red[12][NA];
    __shared__ double ared[12][CO];
    const int kd = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);
    const int tid = threadIdx.x & 255;
    const int per_xcd = gridDim.x / 8;
    const int share = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    const int wq = tid % C1WQ, hl = (tid / C1WQ) % C1H, dl = tid / (C1WQ * C1H);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // 0 .. 11
    // as a loader: this lane's channel quad and its voxel along W in every row it loads
    const int tq = lane % Q, tv = lane / Q;
    const int toff = (tv / VPT) * LS + (tv % VPT) * CO + tq * 4;
    float al[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        al[j] = (pa.act == MRI3D_ACT_PRELU) ? pa.alpha[pa.alpha_n == 1 ? 0 : tq * 4 + j] : (pa.act == MRI3D_ACT_LEAKY ? pa.slope : 0.f);
    f32x2 acc[3][3][CO / 2];   // channel pairs: v_pk_fma_f32
    float bsum[CO];
    double asum[4];            // channels 4 tq .. 4 tq + 3
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int c = 0; c < CO / 2; ++c) acc[a][b][c] = f32x2{0.f, 0.f};
#pragma unroll
    for (int c = 0; c < CO; ++c) bsum[c] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) asum[j] = 0.0;
    const bool want_alpha = alpha_part != nullptr;
    for (int tile = share; tile < ntiles; tile += nshares) {
        int n, d0, h0, w0;
        decode_tile(tile, tilesD, tilesH, tilesW, TW, n, d0, h0, w0);
        // rows wave, wave + 12, wave + 24 of the tile's 32 (d, h) rows: in flight while x is staged
        float4 zq[RPW], dq[RPW];
        bool ok[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int row = wave + 12 * i, od = d0 + row / C1H, oh = h0 + row % C1H, ow = w0 + tv;
            ok[i] = row < NROW && od < g.dout && oh < g.ho && ow < g.wo;
            zq[i] = dq[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok[i]) {
                const int64_t vox = (((int64_t)n * g.dout + od) * g.ho + oh) * g.wo + ow;
                zq[i] = ldf4(z + vox * g.y_ld + tq * 4);
                dq[i] = ldf4(da + vox * da_ld + tq * 4);
            }
        }
        __syncthreads();   // the last tile's readers of xs and dzs are through
        cin1_stage<float, TW, C1D + 2, 768>(xs, x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld, g, d0 - 1, h0, w0, (int)threadIdx.x);
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int row = wave + 12 * i;
            if (row < NROW) {   // (uniform in the wave)
                const float zv[4] = {zq[i].x, zq[i].y, zq[i].z, zq[i].w}, dv[4] = {dq[i].x, dq[i].y, dq[i].z, dq[i].w};
                float du[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool pos = zv[j] > 0.f;
                    du[j] = ok[i] ? (pos ? dv[j] : dv[j] * al[j]) : 0.f;   // zero outside the volume
                    if (want_alpha) asum[j] += (pos || !ok[i]) ? 0.0 : (double)dv[j] * (double)zv[j];
                }
                *reinterpret_cast<float4*>(dzs + row * RS + toff) = make_float4(du[0], du[1], du[2], du[3]);
            }
        }
        __syncthreads();
        // this lane's VPT output voxels of dz
        f32x2 gy[VPT][CO / 2];
        {
            const float* gp = dzs + (dl * C1H + hl) * RS + wq * LS;
#pragma unroll
            for (int v = 0; v < VPT; ++v)
#pragma unroll
                for (int c = 0; c < CO; c += 4) {
                    const float4 q = *reinterpret_cast<const float4*>(gp + v * CO + c);
                    gy[v][c / 2] = f32x2{q.x, q.y};
                    gy[v][c / 2 + 1] = f32x2{q.z, q.w};
                }
        }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const float* row = xs + ((dl + kd) * (C1H + 2) + hl + kh) * PW + wq * VPT;
            float r[VPT + 2];
#pragma unroll
            for (int i = 0; i < VPT + 2; ++i) r[i] = row[i];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int v = 0; v < VPT; ++v)
#pragma unroll
                    for (int c = 0; c < CO / 2; ++c)
                        acc[kh][kw][c] = __builtin_elementwise_fma(f32x2{r[v + kw], r[v + kw]}, gy[v][c], acc[kh][kw][c]);
        }
        if (kd == 1) {
#pragma unroll
            for (int v = 0; v < VPT; ++v)
#pragma unroll
                for (int c = 0; c < CO / 2; ++c) { bsum[2 * c] += gy[v][c].x; bsum[2 * c + 1] += gy[v][c].y; }
        }
    }
    // waves 4 kd .. 4 kd + 3 hold plane kd's taps
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                const float vsum = wave_sum_dpp((c & 1) ? acc[a][b][c / 2].y : acc[a][b][c / 2].x);
                if (lane == 0) red[wave][(a * 3 + b) * CO + c] = vsum;
            }
#pragma unroll
    for (int c = 0; c < CO; ++c) {
        const float vsum = wave_sum_dpp(bsum[c]);
        if (lane == 0) red[wave][9 * CO + c] = vsum;
    }
    if (want_alpha) {
        // lanes of one channel quad (lane % Q) -> wave: a butterfly over the other lane bits, the same order in every run
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v = asum[j];
#pragma unroll
            for (int m = 32; m >= Q; m >>= 1) v += __shfl_xor(v, m, 64);
            if (lane < Q) ared[wave][lane * 4 + j] = v;
        }
    }
    __syncthreads();
    const int w0_ = 4 * kd;
    if (tid < 9 * CO) {
        const float t4 = (red[w0_][tid] + red[w0_ + 1][tid]) + (red[w0_ + 2][tid] + red[w0_ + 3][tid]);
        part[((size_t)share * 27 + kd * 9 + tid / CO) * CO + tid % CO] = t4;   // part[share][tap][ci = 0][co]
    } else if (tid < NA && kd == 1 && bias_part) {
        const int c = tid - 9 * CO;
        bias_part[(size_t)share * CO + c] = (red[w0_][tid] + red[w0_ + 1][tid]) + (red[w0_ + 2][tid] + red[w0_ + 3][tid]);
    }
    if (want_alpha && (int)threadIdx.x < CO) {   // the twelve waves in order
        double t = 0.0;
#pragma unroll
        for (int wv = 0; wv < 12; ++wv) t += ared[wv][tid];
        alpha_part[(size_t)share * CO + tid] = t;
    }
}

// dalpha from the per-share float64 sums, rounded as norm_act_bwd_sums_kernel + norm_act_bwd_params_block round theirs: one fp32
// value per channel first, then (one alpha for all channels) the float64 sum of those in channel order.  One workgroup.
__global__ void __launch_bounds__(256)
cin1_act_dalpha_kernel(const double* __restrict__ alpha_part, int nshares, int CO, int alpha_n, float* __restrict__ dalpha) {
    __shared__ double r[256];
    __shared__ float sums[16];
    const int L = 256 / CO, c = threadIdx.x / L, ql = threadIdx.x % L;   // CO = 8 | 16
    double t = 0.0;
    for (int q = ql; q < nshares; q += L) t += alpha_part[(size_t)q * CO + c];
    r[threadIdx.x] = t;
    __syncthreads();
    if (ql == 0) {
        t = 0.0;
        for (int q = 0; q < L; ++q) t += r[c * L + q];
        sums[c] = (float)t;
    }
    __syncthreads();
    if (alpha_n > 1) {
        if ((int)threadIdx.x < CO) dalpha[threadIdx.x] = (float)(double)sums[threadIdx.x];
    } else if (threadIdx.x == 0) {
        t = 0.0;
        for (int q = 0; q < CO; ++q) t += (double)sums[q];
        dalpha[0] = (float)t;
    }
}

// ------------------------------------------------------------------ 3x3x3 stencil: ONE input and ONE output channel
// The autoencoder's last layer `vox = Conv3d(1, 1, 3, padding=1)` (AE_model.py:160) on the whole reconstructed volume: 8 bytes of
// traffic and 27 FMAs per voxel.  The generic kernels spend 0.55 / 0.82 / 0.72 ms (fwd / dgrad / wgrad, 4 x 160x192x160) on it,
// 200-300 GB/s.  Same LDS tile as the first-layer kernels above; the 27 weights sit in SGPRs; dgrad = the same stencil with the
// taps reversed, applied to dy; wgrad keeps 27 accumulators per lane.
template <typename T>
__global__ void __launch_bounds__(256)
conv_c1c1_stencil_kernel(Mri3dConvGeom g, const T* __restrict__ x, int x_ld, const float* __restrict__ w, const float* __restrict__ bias,
                         int flip, T* __restrict__ y, int y_ld, int tilesD, int tilesH, int tilesW, int ntiles) {
    constexpr int VPT = 4, TW = C1WQ * VPT, PW = TW + 4;
    __shared__ __attribute__((aligned(16))) float xs[(C1D + 2) * (C1H + 2) * PW];
    const int tid = threadIdx.x;
    const int wq = tid % C1WQ, hl = (tid / C1WQ) % C1H, dl = tid / (C1WQ * C1H);
    float wt[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) wt[t] = w[flip ? 26 - t : t];   // uniform -> scalar registers
    const float b0 = bias ? bias[0] : 0.f;
    Mri3dConvGeom gs = g;
    gs.x_ld = x_ld;   // cin1_stage reads its source pitch from the geometry
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int n, d0, h0, w0;
        decode_tile(tile, tilesD, tilesH, tilesW, TW, n, d0, h0, w0);
        __syncthreads();
        cin1_stage<T, TW, C1D + 2>(xs, x + (int64_t)n * g.di * g.hi * g.wi * x_ld, gs, d0 - 1, h0, w0, tid);
        __syncthreads();
        float acc[VPT];
#pragma unroll
        for (int v = 0; v < VPT; ++v) acc[v] = b0;
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const float* row = xs + ((dl + kd) * (C1H + 2) + hl + kh) * PW + wq * VPT;
                float r[VPT + 2];
#pragma unroll
                for (int i = 0; i < VPT + 2; ++i) r[i] = row[i];
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int v = 0; v < VPT; ++v) acc[v] = fmaf(r[v + kw], wt[(kd * 3 + kh) * 3 + kw], acc[v]);
            }
#pragma unroll
        for (int v = 0; v < VPT; ++v) asm volatile("" : "+v"(acc[v]));
        const int od = d0 + dl, oh = h0 + hl;
        if (od < g.di && oh < g.hi) {
            T* yo = y + ((((int64_t)n * g.di + od) * g.hi + oh) * g.wi + w0 + wq * VPT) * y_ld;
#pragma unroll
            for (int v = 0; v < VPT; ++v)
                if (w0 + wq * VPT + v < g.wi) stf(yo + (int64_t)v * y_ld, acc[v]);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
conv_c1c1_wgrad_kernel(Mri3dConvGeom g, const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part,
                       float* __restrict__ bias_part, int tilesD, int tilesH, int tilesW, int ntiles) {
    constexpr int VPT = 4, TW = C1WQ * VPT, PW = TW + 4;
    __shared__ __attribute__((aligned(16))) float xs[(C1D + 2) * (C1H + 2) * PW];
    __shared__ float red[4][28];
    const int tid = threadIdx.x;
    const int wq = tid % C1WQ, hl = (tid / C1WQ) % C1H, dl = tid / (C1WQ * C1H);
    float acc[27], bsum = 0.f;
#pragma unroll
    for (int t = 0; t < 27; ++t) acc[t] = 0.f;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int n, d0, h0, w0;
        decode_tile(tile, tilesD, tilesH, tilesW, TW, n, d0, h0, w0);
        __syncthreads();
        cin1_stage<T, TW, C1D + 2>(xs, x + (int64_t)n * g.di * g.hi * g.wi * g.x_ld, g, d0 - 1, h0, w0, tid);
        const int od = d0 + dl, oh = h0 + hl;
        float gy[VPT];
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int ow = w0 + wq * VPT + v;
            const bool ok = od < g.dout && oh < g.ho && ow < g.wo;
            const float q = ldf(dy + ((((int64_t)n * g.dout + min(od, g.dout - 1)) * g.ho + min(oh, g.ho - 1)) * g.wo +
                                      min(ow, g.wo - 1)) * g.y_ld);
            gy[v] = ok ? q : 0.f;
            bsum += gy[v];
        }
        __syncthreads();
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const float* row = xs + ((dl + kd) * (C1H + 2) + hl + kh) * PW + wq * VPT;
                float r[VPT + 2];
#pragma unroll
                for (int i = 0; i < VPT + 2; ++i) r[i] = row[i];
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int v = 0; v < VPT; ++v) acc[(kd * 3 + kh) * 3 + kw] = fmaf(r[v + kw], gy[v], acc[(kd * 3 + kh) * 3 + kw]);
            }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int t = 0; t < 27; ++t) {
        const float vsum = wave_sum_dpp(acc[t]);
        if (lane == 0) red[wave][t] = vsum;
    }
    {
        const float vsum = wave_sum_dpp(bsum);
        if (lane == 0) red[wave][27] = vsum;
    }
    __syncthreads();
    if (tid < 27) part[(size_t)blockIdx.x * 27 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    else if (tid == 27 && bias_part) bias_part[blockIdx.x] = (red[0][27] + red[1][27]) + (red[2][27] + red[3][27]);
}

constexpr int kC1C1Blocks = 1024;

// ------------------------------------------------------------------ 1 -> 1 channel, few taps (the autoencoder's last separable convs)
// Conv3d(1, 1, (1,3,1) / (1,1,3) ...) at full resolution (AE_model.py:110-160): a one-channel tensor is a dense float array, so a lane
// takes FOUR consecutive voxels of a row as one 16-byte access and a tap is the same access shifted by a wave-uniform element
// offset (4-byte aligned: global dwordx4 loads do not need more).  Forward and stride-1 data gradient are the same stencil (the
// gradient walks the taps with the opposite sign); the weight gradient is taps + 1 dot products reduced per wave (DPP), per
// workgroup (LDS, double) and across workgroups (wgrad_reduce_kernel: fixed order).  fp32, stride 1, <= 8 taps, W % 4 == 0.
// The gather kernels spent 0.11 - 0.18 ms per pass on 4 x 160x192x160 (1 TB/s) on 64-bit index arithmetic per voxel.
constexpr int kC1TBlocks = 1024;

// sign = +1: y[o] = b + sum_t w[t] x[o - p + k_t d]   (forward);   sign = -1: dx[i] = sum_t w[t] dy[i + p - k_t d]   (data gradient)
template <int NT>   // tap slots: 3 (the autoencoder's (3,1,1) / (1,3,1) / (1,1,3) filters) or kSmTaps
__global__ void __launch_bounds__(256)
conv_c1_taps_kernel(Mri3dConvGeom g, const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ bias,
                    float* __restrict__ dst, int sign, int sD, int sH, int sW, int oD, int oH, int oW) {
    const int taps = g.kd * g.kh * g.kw;
    const unsigned W4 = (unsigned)oW >> 2;
    const unsigned nitems = (unsigned)g.n * oD * oH * W4;   // < 2^31 (c1_taps_ok): 32-bit index arithmetic per item
    const float b0 = bias != nullptr ? bias[0] : 0.f;
    for (unsigned item = blockIdx.x * blockDim.x + threadIdx.x; item < nitems; item += gridDim.x * blockDim.x) {
        const unsigned q = item % W4;
        unsigned r = item / W4;
        const int oh = (int)(r % (unsigned)oH);
        r /= (unsigned)oH;
        const int od = (int)(r % (unsigned)oD), n = (int)(r / (unsigned)oD);
        const int ow = 4 * (int)q;
        const float* sn = src + (int64_t)n * sD * sH * sW;
        float4 xv[NT];
        unsigned vm[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int tt = t < taps ? t : 0;
            const int kw = tt % g.kw, kh = (tt / g.kw) % g.kh, kd = tt / (g.kw * g.kh);
            const int sd_ = od + sign * (kd * g.dd - g.pd), sh_ = oh + sign * (kh * g.dh - g.ph), sw_ = ow + sign * (kw * g.dw - g.pw);
            const bool rowok = t < taps && (unsigned)sd_ < (unsigned)sD && (unsigned)sh_ < (unsigned)sH;
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) m |= (rowok && (unsigned)(sw_ + j) < (unsigned)sW) ? (1u << j) : 0u;
            vm[t] = m;
            const float* p = sn + ((int64_t)(rowok ? sd_ : 0) * sH + (rowok ? sh_ : 0)) * sW;
            if (m == 15u) {
                xv[t] = *reinterpret_cast<const float4*>(p + sw_);          // 4-byte aligned 16-byte load
            } else {   // row ends / outside: element-wise (a handful of lanes per row)
                xv[t].x = (m & 1u) ? p[sw_] : 0.f;
                xv[t].y = (m & 2u) ? p[sw_ + 1] : 0.f;
                xv[t].z = (m & 4u) ? p[sw_ + 2] : 0.f;
                xv[t].w = (m & 8u) ? p[sw_ + 3] : 0.f;
            }
        }
        float4 acc = make_float4(b0, b0, b0, b0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t < taps) {
                const float wt = w[t];
                acc.x = fmaf(xv[t].x, wt, acc.x);
                acc.y = fmaf(xv[t].y, wt, acc.y);
                acc.z = fmaf(xv[t].z, wt, acc.z);
                acc.w = fmaf(xv[t].w, wt, acc.w);
            }
        }
        *reinterpret_cast<float4*>(dst + (((int64_t)n * oD + od) * oH + oh) * oW + ow) = acc;
    }
}

// part[b][t] = sum over the workgroup's voxels of x[o - p + k_t d] * dy[o];  bias_part[b] = sum dy
template <int NT>
__global__ void __launch_bounds__(256)
conv_c1_taps_wgrad_kernel(Mri3dConvGeom g, const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
                          float* __restrict__ bias_part) {
    __shared__ double red[4][NT + 1];
    const int taps = g.kd * g.kh * g.kw;
    const unsigned W4 = (unsigned)g.wo >> 2;
    const unsigned nitems = (unsigned)g.n * g.dout * g.ho * W4;   // < 2^31 (c1_taps_ok)
    float acc[NT + 1];
#pragma unroll
    for (int t = 0; t <= NT; ++t) acc[t] = 0.f;
    for (unsigned item = blockIdx.x * blockDim.x + threadIdx.x; item < nitems; item += gridDim.x * blockDim.x) {
        const unsigned q = item % W4;
        unsigned r = item / W4;
        const int oh = (int)(r % (unsigned)g.ho);
        r /= (unsigned)g.ho;
        const int od = (int)(r % (unsigned)g.dout), n = (int)(r / (unsigned)g.dout);
        const int ow = 4 * (int)q;
        const float4 gv = *reinterpret_cast<const float4*>(dy + (((int64_t)n * g.dout + od) * g.ho + oh) * g.wo + ow);
        acc[NT] += (gv.x + gv.y) + (gv.z + gv.w);
        const float* xn = x + (int64_t)n * g.di * g.hi * g.wi;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int tt = t < taps ? t : 0;
            const int kw = tt % g.kw, kh = (tt / g.kw) % g.kh, kd = tt / (g.kw * g.kh);
            const int id = od - g.pd + kd * g.dd, ih = oh - g.ph + kh * g.dh, iw = ow - g.pw + kw * g.dw;
            const bool rowok = t < taps && (unsigned)id < (unsigned)g.di && (unsigned)ih < (unsigned)g.hi;
            const float* p = xn + ((int64_t)(rowok ? id : 0) * g.hi + (rowok ? ih : 0)) * g.wi;
            float4 xv;
            if (rowok && iw >= 0 && iw + 3 < g.wi) {
                xv = *reinterpret_cast<const float4*>(p + iw);
            } else {
                xv.x = (rowok && (unsigned)iw < (unsigned)g.wi) ? p[iw] : 0.f;
                xv.y = (rowok && (unsigned)(iw + 1) < (unsigned)g.wi) ? p[iw + 1] : 0.f;
                xv.z = (rowok && (unsigned)(iw + 2) < (unsigned)g.wi) ? p[iw + 2] : 0.f;
                xv.w = (rowok && (unsigned)(iw + 3) < (unsigned)g.wi) ? p[iw + 3] : 0.f;
            }
            acc[t] = fmaf(xv.x, gv.x, fmaf(xv.y, gv.y, fmaf(xv.z, gv.z, fmaf(xv.w, gv.w, acc[t]))));
        }
    }
    // wave sums (fixed butterfly), then the four waves in double through LDS
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t <= NT; ++t) {
        float v = acc[t];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wv][t] = (double)v;
    }
    __syncthreads();
    if (threadIdx.x <= NT) {
        const double sdbl = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if ((int)threadIdx.x < taps) part[(size_t)blockIdx.x * taps + threadIdx.x] = (float)sdbl;
        if (threadIdx.x == NT && bias_part != nullptr) bias_part[blockIdx.x] = (float)sdbl;
    }
}

static bool c1_taps_ok(const Mri3dConvGeom& g) {
    return g.dtype == MRI3D_F32 && g.ci == 1 && g.co == 1 && g.kd * g.kh * g.kw <= kSmTaps && g.sd == 1 && g.sh == 1 && g.sw == 1 &&
           g.x_ld == 1 && g.y_ld == 1 && g.wo % 4 == 0 && g.wi % 4 == 0 && !(g.kd == 3 && g.kh == 3 && g.kw == 3) &&
           (int64_t)g.n * g.dout * g.ho * g.wo < 0x7fffffffLL && (int64_t)g.n * g.di * g.hi * g.wi < 0x7fffffffLL;
}

// forward (sign +1: src = x) and stride-1 data gradient (sign -1: src = dy) of the 1 -> 1 few-taps stencil
static void launch_c1_taps(const Mri3dConvGeom& g, int nt, const float* src, const float* w, const float* bias, float* dst, int sign,
                           hipStream_t s) {
    const int sD = sign > 0 ? g.di : g.dout, sH = sign > 0 ? g.hi : g.ho, sW = sign > 0 ? g.wi : g.wo;
    const int oD = sign > 0 ? g.dout : g.di, oH = sign > 0 ? g.ho : g.hi, oW = sign > 0 ? g.wo : g.wi;
    const int64_t items = (int64_t)g.n * oD * oH * (oW / 4);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(items, 256), 8192));
    if (nt == 3)
        hipLaunchKernelGGL(conv_c1_taps_kernel<3>, dim3(grid), dim3(256), 0, s, g, src, w, bias, dst, sign, sD, sH, sW, oD, oH, oW);
    else
        hipLaunchKernelGGL(conv_c1_taps_kernel<kSmTaps>, dim3(grid), dim3(256), 0, s, g, src, w, bias, dst, sign, sD, sH, sW, oD, oH, oW);
}

// the 4 x 8 x (8*vpt) voxel tiles of the cin1 / c1c1 kernels over n volumes of D x H x W (the count in 64 bits: the _ok tests bound it)
struct C1Tiles { int tilesD, tilesH, tilesW; int64_t ntiles; };
static C1Tiles c1_tiles(int n, int D, int H, int W, int vpt) {
    C1Tiles t;
    t.tilesD = cdiv(D, C1D), t.tilesH = cdiv(H, C1H), t.tilesW = cdiv(W, C1WQ * vpt);
    t.ntiles = (int64_t)n * t.tilesD * t.tilesH * t.tilesW;
    return t;
}

static bool c1c1_ok(const Mri3dConvGeom& g) {
    static const int off = tuning_knob("MRI3D_C1C1_OFF", 0);   // tuning aid (A/B)
    return !off && g.ci == 1 && g.co == 1 && g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sd == 1 && g.sh == 1 && g.sw == 1 &&
           g.dd == 1 && g.dh == 1 && g.dw == 1 && g.pd == 1 && g.ph == 1 && g.pw == 1 &&
           c1_tiles(g.n, g.dout, g.ho, g.wo, 4).ntiles < 0x7fffffffLL;
}

template <typename T>
static void launch_c1c1_stencil(const Mri3dConvGeom& g, const T* src, int src_ld, const float* w, const float* bias, int flip,
                                T* dst, int dst_ld, hipStream_t s) {
    const C1Tiles t = c1_tiles(g.n, g.di, g.hi, g.wi, 4);
    hipLaunchKernelGGL(conv_c1c1_stencil_kernel<T>, dim3(std::min((int)t.ntiles, 256 * 8)), dim3(256), 0, s, g, src, src_ld, w, bias, flip,
                       dst, dst_ld, t.tilesD, t.tilesH, t.tilesW, (int)t.ntiles);
}

static const int g_cin1_off = tuning_knob("MRI3D_CIN1_OFF", 0);   // tuning aid (A/B)
constexpr int kCin1Shares = 256;   // 3 * 256 = 768 workgroups = 3 per CU

static bool cin1_ok(const Mri3dConvGeom& g) {
    return !g_cin1_off && g.ci == 1 && (g.co == 8 || g.co == 16) && g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sd == 1 &&
           g.sh == 1 && g.sw == 1 && g.dd == 1 && g.dh == 1 && g.dw == 1 && g.pd == 1 && g.ph == 1 && g.pw == 1 &&
           g.y_ld % 4 == 0 && c1_tiles(g.n, g.dout, g.ho, g.wo, 2).ntiles < 0x7fffffffLL;   // (the Co = 16 tiles: the larger count)
}
static C1Tiles cin1_tiles(const Mri3dConvGeom& g) { return c1_tiles(g.n, g.dout, g.ho, g.wo, g.co <= 8 ? 4 : 2); }   // Cin1<CO>::VPT

static bool wgrad_small_ok(const Mri3dConvGeom& g) {
    const int taps = g.kd * g.kh * g.kw;
    return taps <= kSmTaps && g.ci <= 64 && g.co <= 64 && (int64_t)g.dout * g.ho * g.wo < 0x7fffffffLL;
}

// the channel-quad variant: Ci, Co multiples of 4 with QI * QO lanes per voxel dividing 256 (<= 64), 16-byte aligned rows
static bool wgrad_quads_ok(const Mri3dConvGeom& g) {
    const int taps = g.kd * g.kh * g.kw;
    const int pv = (g.ci / 4) * (g.co / 4);
    if (g.ci == 1)   // one input channel: a lane owns (voxel, co quad)
        return taps <= kSmTaps && g.co % 4 == 0 && g.co >= 4 && g.co <= 64 && 256 % (g.co / 4) == 0 && g.y_ld % 4 == 0 &&
               (int64_t)g.ho * g.wo < 0x7fffffffLL && (int64_t)g.n * g.dout * g.ho < 0x7fffffffLL && !cin1_ok(g);
    return taps <= kSmTaps && g.ci % 4 == 0 && g.co % 4 == 0 && g.ci >= 4 && g.co >= 4 && pv <= 64 && 256 % pv == 0 &&
           g.x_ld % 4 == 0 && g.y_ld % 4 == 0 && (int64_t)g.ho * g.wo < 0x7fffffffLL &&
           (int64_t)g.n * g.dout * g.ho < 0x7fffffffLL;
}

// ------------------------------------------------------------------ host side
static int pick_tile(int c) { return c >= 16 ? 16 : (c > 4 ? 8 : (c > 2 ? 4 : 2)); }
static int pad_to_tile(int c) { return cdiv(c, pick_tile(c)) * pick_tile(c); }
// forward / data gradient: the repacked weights [tap][channels summed over][tiled channels, padded to the tile], in the workspace
static size_t packed_w_bytes(const Mri3dConvGeom& g, int pass) {
    const int taps = g.kd * g.kh * g.kw;
    return pass == MRI3D_PASS_FWD ? (size_t)taps * g.ci * pad_to_tile(g.co) * sizeof(float)
                                  : (size_t)taps * g.co * pad_to_tile(g.ci) * sizeof(float);
}

// ------------------------------------------------------------------ THE decision of each pass
// Which kernel and instantiation a pass launches, from the geometry and the alignment (ptr_align) of its two activation tensors:
// ax = that of x (forward, weight gradient) / dx (data gradient), ay = that of y / dy.  conv_generic_fwd / _dgrad / _wgrad launch
// from it and conv_generic_route_name prints it.  The plan of a weight gradient also OWNS the layout of its workspace — where the
// partials of dw end and those of the bias begin, how wgrad_reduce_kernel strides through them, the grid that fills them: the
// launch carves the workspace by the plan and conv_generic_workspace_bytes sizes it by the plan, neither has a size of its own.
enum class GenKernel { c1c1, c1taps, cin1, taps, gather, strided_taps, strided, co1, quads, small, lds };
struct GenericPlan {
    GenKernel kernel = GenKernel::gather;
    int tl = 0;           // taps / gather / strided_taps / strided: channel tile of a thread, the padding of the packed weights
    int nt = 0;           // tap slots: c1taps 3 | 8, taps 3 | 4 | 6 | 8, strided_taps 3 | 4 | 8, quads 4 | 6 | 8
    int cv = 0;           // taps: channels per load (4 | 1)
    int vec = 0;          // gather / strided: 16-byte loads (1 | 0)
    int civ = 0;          // quads: input channels per lane, the kernel's CIV (4 | 1)
    int co_inst = 0;      // cin1: the CO instance (8 | 16)
    int ci_inst = 0;      // co1: the CI instance (1 | 4 | 8 | 16)
    int cp = 0;           // taps / gather / strided*: channels of the packed weights (Co or Ci rounded up to tl)
    size_t ws_bytes = 0;  // workspace the launch requires: the packed weights, or (part_floats + bias_floats) floats
    // weight gradient: the workspace is part[slots][taps][CiP][CoP] (c1taps and co1: [slots][slot of their widest instance]), then
    // bias_part[slots][Co]; a launch fills the first nb <= slots of each and wgrad_reduce_kernel sums those
    int slots = 0;                              // partials the workspace holds = the most workgroups (x) a launch may use
    size_t part_floats = 0, bias_floats = 0;    // part_floats is also the offset of bias_part
    int CiP = 0, CoP = 0;                       // channel pitches of a partial (taps, Ci, Co: the geometry's)
    // the family's own grid data (grid x = slots in all three)
    struct { int QI = 0, QO = 0, hch = 0; } quads;          // channel quads per voxel, output rows per slab
    struct { int CiL = 0, gy = 1, gz = 1; } small;          // input channels per workgroup; grid (slots, gy, gz)
    struct { int Ci4 = 0, Co4 = 0, nitems = 0, vsplit = 0, gz = 1; size_t smem = 0; } lds;   // channel quads, 4x4 items, voxel split
                                                            // of a small item set; grid (slots, taps, gz); dynamic LDS bytes
};

static GenericPlan generic_fwd_plan(const Mri3dConvGeom& g, int ax, int ay) {
    GenericPlan p;
    const int taps = g.kd * g.kh * g.kw;
    if (c1c1_ok(g)) { p.kernel = GenKernel::c1c1; return p; }
    if (c1_taps_ok(g) && align16(ay)) { p.kernel = GenKernel::c1taps, p.nt = taps <= 3 ? 3 : kSmTaps; return p; }
    p.ws_bytes = packed_w_bytes(g, MRI3D_PASS_FWD);
    if (cin1_ok(g) && align_vec4(g.dtype, ay)) { p.kernel = GenKernel::cin1, p.co_inst = g.co == 8 ? 8 : 16; return p; }   // [27][1][Co]: the tile of 8 | 16 pads nothing
    p.tl = pick_tile(g.co), p.cp = pad_to_tile(g.co);
    const bool vec = (g.ci % 4 == 0) && (g.x_ld % 4 == 0) && align_vec4(g.dtype, ax);
    if ((vec || g.ci == 1) && taps <= 8 && align_vec4(g.dtype, ay) && (int64_t)g.ho * g.wo < 0x7fffffffLL && (int64_t)g.n * g.dout * g.ho < 0x7fffffffLL) {
        // tap slots = the filter's taps where an instance exists (3: the decoder's k = 3 filters, 6: the encoder's k = 6 ones): a
        // slot past the filter still costs its address arithmetic and a (cached) load
        p.kernel = GenKernel::taps, p.cv = vec ? 4 : 1;
        p.nt = vec ? (taps <= 3 ? 3 : (taps <= 4 ? 4 : (taps <= 6 ? 6 : 8))) : (taps <= 3 ? 3 : (taps <= 6 ? 6 : 8));
        return p;
    }
    p.kernel = GenKernel::gather, p.vec = vec ? 1 : 0;
    return p;
}

// (ax: dx, ay: dy)
static GenericPlan generic_dgrad_plan(const Mri3dConvGeom& g, int ax, int ay) {
    GenericPlan p;
    const int taps = g.kd * g.kh * g.kw;
    if (c1c1_ok(g)) { p.kernel = GenKernel::c1c1; return p; }
    if (c1_taps_ok(g) && align16(ax)) { p.kernel = GenKernel::c1taps, p.nt = taps <= 3 ? 3 : kSmTaps; return p; }
    p.tl = pick_tile(g.ci), p.cp = pad_to_tile(g.ci);
    p.ws_bytes = packed_w_bytes(g, MRI3D_PASS_DGRAD);
    const bool vec = (g.co % 4 == 0) && (g.y_ld % 4 == 0) && align_vec4(g.dtype, ay);
    const bool unit_stride = g.sd == 1 && g.sh == 1 && g.sw == 1;   // strided layers: the wave-uniform tap sets below are faster (0.29 vs 0.33 ms)
    if ((vec || g.co == 1) && unit_stride && taps <= 8 && align_vec4(g.dtype, ax) && (int64_t)g.hi * g.wi < 0x7fffffffLL && (int64_t)g.n * g.di * g.hi < 0x7fffffffLL) {
        p.kernel = GenKernel::taps, p.cv = vec ? 4 : 1;
        p.nt = vec ? (taps <= 3 ? 3 : (taps <= 4 ? 4 : (taps <= 6 ? 6 : 8))) : (taps <= 3 ? 3 : 8);
        return p;
    }
    const int64_t rows = (int64_t)g.n * g.di * g.hi * g.sw;
    if ((g.sd > 1 || g.sh > 1 || g.sw > 1) && g.dd == 1 && g.dh == 1 && g.dw == 1 && rows <= 0x7fffffff) {
        // valid taps per input voxel: ceil(k / s) per axis; up to 4 (the separable stride-2 filters: 3) or 8 take the batched kernel
        const int vt = cdiv(g.kd, g.sd) * cdiv(g.kh, g.sh) * cdiv(g.kw, g.sw);
        if (vec && vt <= 8 && align_vec4(g.dtype, ax)) {
            p.kernel = GenKernel::strided_taps, p.nt = vt <= 3 ? 3 : (vt <= 4 ? 4 : 8);
            return p;
        }
        p.kernel = GenKernel::strided, p.vec = vec ? 1 : 0;
        return p;
    }
    p.kernel = GenKernel::gather, p.vec = vec ? 1 : 0;
    return p;
}

// the three families whose grid follows the volume: each sets its slots (grid x), channel pitches and grid data
static void wgrad_quads_plan(const Mri3dConvGeom& g, GenericPlan& p) {
    const int taps = g.kd * g.kh * g.kw;
    auto& q = p.quads;
    p.civ = g.ci == 1 ? 1 : 4, p.nt = g.ci == 1 ? 8 : (taps <= 4 ? 4 : (taps <= 6 ? 6 : 8));
    q.QI = g.ci == 1 ? 1 : g.ci / 4, q.QO = g.co / 4;
    const int VL = 256 / (q.QI * q.QO);
    // ~16 voxels per lane and slab
    q.hch = (int)std::max<int64_t>(1, std::min<int64_t>(g.ho, (int64_t)16 * VL / std::max(g.wo, 1)));
    const int64_t slabs = (int64_t)g.n * g.dout * cdiv(g.ho, q.hch);
    // one resident round: 4 / 3 / 2 workgroups per CU with 4 / 6 / 8 accumulator slots (112 / 161 / 209 VGPRs)
    const int resident = 256 * (taps <= 4 ? 4 : (taps <= 6 ? 3 : 2));
    p.slots = (int)std::max<int64_t>(1, std::min<int64_t>(slabs, resident));
}

static void wgrad_small_plan(const Mri3dConvGeom& g, GenericPlan& p) {
    auto& q = p.small;
    int cil = 1;
    while (cil < g.ci && cil < 16) cil <<= 1;
    q.CiL = cil;
    q.gz = cdiv(g.ci, cil);
    q.gy = cdiv(g.co, kSmCo);
    p.CiP = cdiv(g.ci, 4) * 4;
    p.CoP = cdiv(g.co, 4) * 4;
    const int64_t nvox = (int64_t)g.n * g.dout * g.ho * g.wo;
    int64_t want = cdiv64(nvox, (int64_t)(256 / cil) * 8);
    int cap = 2048 / (q.gy * q.gz);
    if (cap < 8) cap = 8;
    p.slots = (int)std::max<int64_t>(1, std::min<int64_t>(want, cap));
}

static void wgrad_lds_plan(const Mri3dConvGeom& g, GenericPlan& p) {
    const int taps = g.kd * g.kh * g.kw;
    auto& q = p.lds;
    q.Ci4 = cdiv(g.ci, 4);
    q.Co4 = cdiv(g.co, 4);
    p.CiP = q.Ci4 * 4, p.CoP = q.Co4 * 4;
    q.nitems = q.Ci4 * q.Co4;
    q.vsplit = q.nitems >= 256 ? 1 : (256 / q.nitems);
    if (q.vsplit > kWgCH) q.vsplit = kWgCH;
    q.gz = q.vsplit > 1 ? 1 : cdiv(q.nitems, 256 * kWgIPT);
    int64_t nvox = (int64_t)g.n * g.dout * g.ho * g.wo;
    int64_t nchunks = cdiv64(nvox, kWgCH);
    int gx = 2048 / (taps * q.gz);
    if (gx < 8) gx = 8;
    if (gx > 256) gx = 256;
    if (gx > nchunks) gx = (int)nchunks;
    if (gx < 1) gx = 1;
    p.slots = gx;
    q.smem = (size_t)kWgCH * (q.Ci4 + q.Co4) * 4 * sizeof(float) + kWgCH * sizeof(int64_t) +
             (q.vsplit > 1 ? 256 * 16 * sizeof(float) : 0);
}

// (ax: x, ay: dy)
static GenericPlan generic_wgrad_plan(const Mri3dConvGeom& g, int ax, int ay) {
    GenericPlan p;
    const int taps = g.kd * g.kh * g.kw;
    p.CiP = g.ci, p.CoP = g.co;   // small and lds round them up to quads
    size_t slot_floats = 0;       // floats of one partial of dw; 0: taps * CiP * CoP
    if (c1c1_ok(g)) {
        p.kernel = GenKernel::c1c1, p.slots = kC1C1Blocks;
    } else if (c1_taps_ok(g) && align16(ay)) {
        p.kernel = GenKernel::c1taps, p.nt = taps <= 3 ? 3 : kSmTaps, p.slots = kC1TBlocks, slot_floats = kSmTaps;
    } else if (cin1_ok(g) && align_vec4(g.dtype, ay)) {
        p.kernel = GenKernel::cin1, p.co_inst = g.co == 8 ? 8 : 16, p.slots = kCin1Shares;
    } else if (wgrad_co1_ok(g) && align_vec4(g.dtype, ax)) {
        p.kernel = GenKernel::co1, p.ci_inst = (g.ci == 1 || g.ci == 4 || g.ci == 8) ? g.ci : 16;
        p.slots = kCo1Blocks, slot_floats = kSmTaps * 16;
    } else if (wgrad_quads_ok(g) && align_vec4(g.dtype, ay) && (g.ci == 1 || align_vec4(g.dtype, ax))) {
        p.kernel = GenKernel::quads, wgrad_quads_plan(g, p);
    } else if (wgrad_small_ok(g)) {
        p.kernel = GenKernel::small, wgrad_small_plan(g, p);
    } else {
        p.kernel = GenKernel::lds, wgrad_lds_plan(g, p);
    }
    p.part_floats = (size_t)p.slots * (slot_floats ? slot_floats : (size_t)taps * p.CiP * p.CoP);
    p.bias_floats = (size_t)p.slots * g.co;
    p.ws_bytes = (p.part_floats + p.bias_floats) * sizeof(float);
    return p;
}

bool conv_generic_route_name(const Mri3dConvGeom& g, int pass, bool bias, int ax, int ay, char* name, size_t name_bytes) {
    const GenericPlan p = pass == MRI3D_PASS_FWD ? generic_fwd_plan(g, ax, ay)
                                                 : (pass == MRI3D_PASS_DGRAD ? generic_dgrad_plan(g, ax, ay) : generic_wgrad_plan(g, ax, ay));
    // the bias of a data gradient (the forward of a ConvTranspose3d) is part of the name, as in the MFMA file's names
    const char* b = (bias && pass == MRI3D_PASS_DGRAD) ? " bias" : "";
    int len = 0;
    switch (p.kernel) {
    case GenKernel::c1c1: len = snprintf(name, name_bytes, "generic c1c1%s", b); break;
    case GenKernel::c1taps: len = snprintf(name, name_bytes, "generic c1taps nt%d%s", p.nt, b); break;
    case GenKernel::cin1: len = snprintf(name, name_bytes, "generic cin1 co%d", p.co_inst); break;
    case GenKernel::taps: len = snprintf(name, name_bytes, "generic taps tl%d nt%d cv%d%s", p.tl, p.nt, p.cv, b); break;
    case GenKernel::gather: len = snprintf(name, name_bytes, "generic gather tl%d vec%d%s", p.tl, p.vec, b); break;
    case GenKernel::strided_taps: len = snprintf(name, name_bytes, "generic staps tl%d nt%d%s", p.tl, p.nt, b); break;
    case GenKernel::strided: len = snprintf(name, name_bytes, "generic strided tl%d vec%d%s", p.tl, p.vec, b); break;
    case GenKernel::co1: len = snprintf(name, name_bytes, "generic co1 ci%d", p.ci_inst); break;
    case GenKernel::quads: len = snprintf(name, name_bytes, "generic quads nt%d civ%d", p.nt, p.civ); break;
    case GenKernel::small: len = snprintf(name, name_bytes, "generic small"); break;
    case GenKernel::lds: len = snprintf(name, name_bytes, "generic lds"); break;
    }
    return len > 0 && (size_t)len < name_bytes;
}

size_t conv_generic_workspace_bytes(const Mri3dConvGeom& g, int pass) {
    // forward / data gradient: the packed weights, also where the plan ends at a kernel that reads the weights as they are
    if (pass != MRI3D_PASS_WGRAD) return packed_w_bytes(g, pass);
    // the weight gradient falls through a chain of `geometry && alignment` tests whose kernels lay their partials out differently:
    // the largest need of the kernels the chain can end at, over the alignments x and dy may have
    size_t a = 0;
    for (int ax : {16, 8, 4})
        for (int ay : {16, 8, 4}) a = std::max(a, generic_wgrad_plan(g, ax, ay).ws_bytes);
    return a;
}

template <int TL>
static void launch_fwd(const Mri3dConvGeom& g, const GenericPlan& p, const void* x, const float* wp, const float* bias, void* y,
                       hipStream_t s) {
    const int CoP = p.cp;
    int64_t nvox = (int64_t)g.n * g.dout * g.ho * g.wo;
    dim3 grid((unsigned)std::min<int64_t>(cdiv64(nvox, 256), 8192), CoP / TL);
    if (p.kernel == GenKernel::taps) {
        // few taps: slab walk + batched tap loads (conv_fwd_taps_kernel)
        const int hch = (int)std::max<int64_t>(1, std::min<int64_t>(g.ho, (int64_t)2048 / std::max(g.wo, 1)));
        const int64_t slabs = (int64_t)g.n * g.dout * cdiv(g.ho, hch);
        dim3 tgrid((unsigned)std::min<int64_t>(slabs, 4096), CoP / TL);
#define MRI3D_FT(NTv, CVv) hipLaunchKernelGGL((conv_fwd_taps_kernel<T, TL, NTv, CVv>), tgrid, dim3(256), 0, s, g, (const T*)x, wp, bias, (T*)y, CoP, hch)
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            if (p.cv == 4) { if (p.nt == 3) MRI3D_FT(3, 4); else if (p.nt == 4) MRI3D_FT(4, 4); else if (p.nt == 6) MRI3D_FT(6, 4); else MRI3D_FT(8, 4); }
            else { if (p.nt == 3) MRI3D_FT(3, 1); else if (p.nt == 6) MRI3D_FT(6, 1); else MRI3D_FT(8, 1); }
        });
#undef MRI3D_FT
        return;
    }
    MRI3D_DISPATCH_DTYPE(g.dtype, T, {
        if (p.vec)
            hipLaunchKernelGGL((conv_fwd_generic_kernel<T, TL, true>), grid, dim3(256), 0, s, g, (const T*)x, wp, bias, (T*)y, CoP);
        else
            hipLaunchKernelGGL((conv_fwd_generic_kernel<T, TL, false>), grid, dim3(256), 0, s, g, (const T*)x, wp, bias, (T*)y, CoP);
    });
}

int conv_generic_fwd(const Mri3dConvGeom& g, const void* x, const float* w, const float* bias, void* y, void* ws,
                     size_t ws_bytes, hipStream_t s) {
    const GenericPlan p = generic_fwd_plan(g, ptr_align(x), ptr_align(y));
    if (p.kernel == GenKernel::c1c1) {
        MRI3D_DISPATCH_DTYPE(g.dtype, T, { launch_c1c1_stencil<T>(g, (const T*)x, g.x_ld, w, bias, 0, (T*)y, g.y_ld, s); });
        return check_launch("conv3d_fwd(1->1 stencil)");
    }
    if (p.kernel == GenKernel::c1taps) {
        launch_c1_taps(g, p.nt, (const float*)x, w, bias, (float*)y, 1, s);
        return check_launch("conv3d_fwd(1->1 taps)");
    }
    MRI3D_REQUIRE(ws != nullptr && ws_bytes >= p.ws_bytes, MRI3D_EWORKSPACE, "conv3d_fwd: workspace %zu < %zu", ws_bytes, p.ws_bytes);
    float* wp = static_cast<float*>(ws);
    const int taps = g.kd * g.kh * g.kw;
    if (p.kernel == GenKernel::cin1) {
        hipLaunchKernelGGL(repack_w_kernel, dim3(1), dim3(256), 0, s, w, wp, g.co, 1, 27, g.co, 0);
        const C1Tiles t = cin1_tiles(g);
        const int grid = std::min((int)t.ntiles, 256 * 8);
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            if (p.co_inst == 8)
                hipLaunchKernelGGL((conv_cin1_fwd_kernel<T, 8>), dim3(grid), dim3(256), 0, s, g, (const T*)x, wp, bias, (T*)y,
                                   t.tilesD, t.tilesH, t.tilesW, (int)t.ntiles);
            else
                hipLaunchKernelGGL((conv_cin1_fwd_kernel<T, 16>), dim3(grid), dim3(256), 0, s, g, (const T*)x, wp, bias, (T*)y,
                                   t.tilesD, t.tilesH, t.tilesW, (int)t.ntiles);
        });
        return check_launch("conv3d_fwd(cin1)");
    }
    const int TL = p.tl, CoP = p.cp;
    int total = taps * g.ci * CoP;
    hipLaunchKernelGGL(repack_w_kernel, dim3(std::min(cdiv(total, 256), 1024)), dim3(256), 0, s, w, wp, g.co, g.ci, taps, CoP, 0);
    switch (TL) {
        case 16: launch_fwd<16>(g, p, x, wp, bias, y, s); break;
        case 8: launch_fwd<8>(g, p, x, wp, bias, y, s); break;
        case 4: launch_fwd<4>(g, p, x, wp, bias, y, s); break;
        default: launch_fwd<2>(g, p, x, wp, bias, y, s); break;
    }
    return check_launch("conv3d_fwd(generic)");
}

template <int TL>
static void launch_dgrad(const Mri3dConvGeom& g, const GenericPlan& p, const void* dy, const float* wp, const float* bias, void* dx,
                         hipStream_t s) {
    const int CiP = p.cp;
    int64_t nvox = (int64_t)g.n * g.di * g.hi * g.wi;
    dim3 grid((unsigned)std::min<int64_t>(cdiv64(nvox, 256), 8192), CiP / TL);
    if (p.kernel == GenKernel::taps) {
        // few taps, stride 1: slab walk + batched tap loads (conv_dgrad_taps_kernel)
        const int hch = (int)std::max<int64_t>(1, std::min<int64_t>(g.hi, (int64_t)2048 / std::max(g.wi, 1)));
        const int64_t slabs = (int64_t)g.n * g.di * cdiv(g.hi, hch);
        dim3 tgrid((unsigned)std::min<int64_t>(slabs, 4096), CiP / TL);
#define MRI3D_DT(NTv, CVv) hipLaunchKernelGGL((conv_dgrad_taps_kernel<T, TL, NTv, CVv>), tgrid, dim3(256), 0, s, g, (const T*)dy, wp, bias, (T*)dx, CiP, hch)
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            if (p.cv == 4) { if (p.nt == 3) MRI3D_DT(3, 4); else if (p.nt == 4) MRI3D_DT(4, 4); else if (p.nt == 6) MRI3D_DT(6, 4); else MRI3D_DT(8, 4); }
            else { if (p.nt == 3) MRI3D_DT(3, 1); else MRI3D_DT(8, 1); }
        });
#undef MRI3D_DT
        return;
    }
    if (p.kernel == GenKernel::strided_taps || p.kernel == GenKernel::strided) {
        dim3 sgrid((unsigned)((int64_t)g.n * g.di * g.hi * g.sw), CiP / TL);
        if (p.kernel == GenKernel::strided_taps) {
            MRI3D_DISPATCH_DTYPE(g.dtype, T, {
                if (p.nt == 3)
                    hipLaunchKernelGGL((conv_dgrad_strided_taps_kernel<T, TL, 3>), sgrid, dim3(64), 0, s, g, (const T*)dy, wp, bias, (T*)dx, CiP);
                else if (p.nt == 4)
                    hipLaunchKernelGGL((conv_dgrad_strided_taps_kernel<T, TL, 4>), sgrid, dim3(64), 0, s, g, (const T*)dy, wp, bias, (T*)dx, CiP);
                else
                    hipLaunchKernelGGL((conv_dgrad_strided_taps_kernel<T, TL, 8>), sgrid, dim3(64), 0, s, g, (const T*)dy, wp, bias, (T*)dx, CiP);
            });
            return;
        }
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            if (p.vec)
                hipLaunchKernelGGL((conv_dgrad_strided_kernel<T, TL, true>), sgrid, dim3(64), 0, s, g, (const T*)dy, wp, bias, (T*)dx, CiP);
            else
                hipLaunchKernelGGL((conv_dgrad_strided_kernel<T, TL, false>), sgrid, dim3(64), 0, s, g, (const T*)dy, wp, bias, (T*)dx, CiP);
        });
        return;
    }
    MRI3D_DISPATCH_DTYPE(g.dtype, T, {
        if (p.vec)
            hipLaunchKernelGGL((conv_dgrad_generic_kernel<T, TL, true>), grid, dim3(256), 0, s, g, (const T*)dy, wp, bias, (T*)dx, CiP);
        else
            hipLaunchKernelGGL((conv_dgrad_generic_kernel<T, TL, false>), grid, dim3(256), 0, s, g, (const T*)dy, wp, bias, (T*)dx, CiP);
    });
}

int conv_generic_dgrad(const Mri3dConvGeom& g, const void* dy, const float* w, const float* bias, void* dx, void* ws,
                       size_t ws_bytes, hipStream_t s) {
    const GenericPlan p = generic_dgrad_plan(g, ptr_align(dx), ptr_align(dy));
    if (p.kernel == GenKernel::c1c1) {
        // dx = the same stencil with reversed taps, applied to dy (pad 1, stride 1: the transposed conv is a conv)
        MRI3D_DISPATCH_DTYPE(g.dtype, T, { launch_c1c1_stencil<T>(g, (const T*)dy, g.y_ld, w, bias, 1, (T*)dx, g.x_ld, s); });
        return check_launch("conv3d_dgrad(1->1 stencil)");
    }
    if (p.kernel == GenKernel::c1taps) {
        launch_c1_taps(g, p.nt, (const float*)dy, w, bias, (float*)dx, -1, s);
        return check_launch("conv3d_dgrad(1->1 taps)");
    }
    const int taps = g.kd * g.kh * g.kw;
    const int TL = p.tl, CiP = p.cp;
    MRI3D_REQUIRE(ws != nullptr && ws_bytes >= p.ws_bytes, MRI3D_EWORKSPACE, "conv3d_dgrad: workspace %zu < %zu", ws_bytes, p.ws_bytes);
    float* wp = static_cast<float*>(ws);
    int total = taps * g.co * CiP;
    hipLaunchKernelGGL(repack_w_kernel, dim3(std::min(cdiv(total, 256), 1024)), dim3(256), 0, s, w, wp, g.co, g.ci, taps, CiP, 1);
    switch (TL) {
        case 16: launch_dgrad<16>(g, p, dy, wp, bias, dx, s); break;
        case 8: launch_dgrad<8>(g, p, dy, wp, bias, dx, s); break;
        case 4: launch_dgrad<4>(g, p, dy, wp, bias, dx, s); break;
        default: launch_dgrad<2>(g, p, dy, wp, bias, dx, s); break;
    }
    return check_launch("conv3d_dgrad(generic)");
}

int conv_generic_wgrad(const Mri3dConvGeom& g, const void* x, const void* dy, float* dw, float* dbias, void* ws,
                       size_t ws_bytes, hipStream_t s) {
    const GenericPlan p = generic_wgrad_plan(g, ptr_align(x), ptr_align(dy));
    MRI3D_REQUIRE(ws != nullptr && ws_bytes >= p.ws_bytes, MRI3D_EWORKSPACE, "conv3d_wgrad: workspace %zu < %zu", ws_bytes, p.ws_bytes);
    float* part = static_cast<float*>(ws);
    float* bias_part = dbias ? part + p.part_floats : nullptr;
    const int taps = g.kd * g.kh * g.kw;
    const int64_t nvox = (int64_t)g.n * g.dout * g.ho * g.wo;
    int nb = p.slots;   // workgroups (x) = partials written; c1c1, c1taps and co1 use fewer on small volumes
    const char* what = "conv3d_wgrad(generic)";
    switch (p.kernel) {
    case GenKernel::c1c1: {
        const C1Tiles t = c1_tiles(g.n, g.dout, g.ho, g.wo, 4);
        nb = std::min((int)t.ntiles, kC1C1Blocks), what = "conv3d_wgrad(1->1 stencil)";
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            hipLaunchKernelGGL(conv_c1c1_wgrad_kernel<T>, dim3(nb), dim3(256), 0, s, g, (const T*)x, (const T*)dy, part, bias_part,
                               t.tilesD, t.tilesH, t.tilesW, (int)t.ntiles);
        });
        break;
    }
    case GenKernel::c1taps: {
        const int64_t items = (int64_t)g.n * g.dout * g.ho * (g.wo / 4);
        nb = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(items, 256 * 4), kC1TBlocks)), what = "conv3d_wgrad(1->1 taps)";
        if (p.nt == 3)
            hipLaunchKernelGGL(conv_c1_taps_wgrad_kernel<3>, dim3(nb), dim3(256), 0, s, g, (const float*)x, (const float*)dy, part, bias_part);
        else
            hipLaunchKernelGGL(conv_c1_taps_wgrad_kernel<kSmTaps>, dim3(nb), dim3(256), 0, s, g, (const float*)x, (const float*)dy, part, bias_part);
        break;
    }
    case GenKernel::cin1: {
        const C1Tiles t = cin1_tiles(g);
        what = "conv3d_wgrad(cin1)";
        // every (share, kd) workgroup writes its slots, also when its share of the tiles is empty (zeros)
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            if (p.co_inst == 8)
                hipLaunchKernelGGL((conv_cin1_wgrad_kernel<T, 8>), dim3(nb), dim3(768), 0, s, g, (const T*)x,
                                   (const T*)dy, part, bias_part, t.tilesD, t.tilesH, t.tilesW, (int)t.ntiles, nb);
            else
                hipLaunchKernelGGL((conv_cin1_wgrad_kernel<T, 16>), dim3(nb), dim3(768), 0, s, g, (const T*)x,
                                   (const T*)dy, part, bias_part, t.tilesD, t.tilesH, t.tilesW, (int)t.ntiles, nb);
        });
        break;
    }
    case GenKernel::co1: {
        nb = (int)std::min<int64_t>(cdiv64(nvox, 256), kCo1Blocks), what = "conv3d_wgrad(co1)";
#define MRI3D_CO1(CIv) hipLaunchKernelGGL((conv_wgrad_co1_kernel<T, CIv>), dim3(nb), dim3(256), 0, s, g, (const T*)x, (const T*)dy, part, bias_part)
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            switch (p.ci_inst) {
                case 1: MRI3D_CO1(1); break;
                case 4: MRI3D_CO1(4); break;
                case 8: MRI3D_CO1(8); break;
                default: MRI3D_CO1(16); break;
            }
        });
#undef MRI3D_CO1
        break;
    }
    case GenKernel::quads: {
        what = "conv3d_wgrad(quads)";
#define MRI3D_WGQ(NTv, CIVv)                                                                                           \
    hipLaunchKernelGGL((conv_wgrad_quads_kernel<T, NTv, CIVv>), dim3(nb), dim3(256), 0, s, g, (const T*)x, (const T*)dy,  \
                       part, bias_part, p.quads.QI, p.quads.QO, p.quads.hch, p.CiP, p.CoP)
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            if (p.civ == 1) MRI3D_WGQ(8, 1);
            else if (p.nt == 4) MRI3D_WGQ(4, 4);
            else if (p.nt == 6) MRI3D_WGQ(6, 4);
            else MRI3D_WGQ(8, 4);
        });
#undef MRI3D_WGQ
        break;
    }
    case GenKernel::small: {
        what = "conv3d_wgrad(small)";
        // partial slots of padded channels are never written by the kernel and never read by the reduce
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            hipLaunchKernelGGL(conv_wgrad_small_kernel<T>, dim3(nb, p.small.gy, p.small.gz), dim3(256), 0, s, g, (const T*)x,
                               (const T*)dy, part, bias_part, p.small.CiL, p.CiP, p.CoP);
        });
        break;
    }
    case GenKernel::lds: {
        const auto& q = p.lds;
        MRI3D_REQUIRE(q.smem <= 160 * 1024, MRI3D_ENOTSUP, "conv3d_wgrad: Ci=%d Co=%d needs %zu B of LDS", g.ci, g.co, q.smem);
        MRI3D_DISPATCH_DTYPE(g.dtype, T, {
            // the kernel's dynamic-LDS limit is raised once (to the CU's 160 KB), not per launch
            static const hipError_t attr_ = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wgrad_generic_kernel<T>),
                                                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            (void)attr_;
            hipLaunchKernelGGL(conv_wgrad_generic_kernel<T>, dim3(nb, taps, q.gz), dim3(256), q.smem, s, g, (const T*)x,
                               (const T*)dy, part, bias_part, q.Ci4, q.Co4, q.nitems, q.vsplit);
        });
        break;
    }
    case GenKernel::taps: case GenKernel::gather: case GenKernel::strided_taps: case GenKernel::strided:   // forward / data gradient only
        MRI3D_REQUIRE(false, MRI3D_EINVAL, "conv3d_wgrad: no weight-gradient kernel in the plan");
    }
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(g.co * g.ci * taps + g.co, 8)), dim3(256), 0, s, part, bias_part, dw, dbias, nb,
                       taps, g.ci, g.co, p.CiP, p.CoP);
    return check_launch(what);
}

// ------------------------------------------------------------------ first layer + its activation: host side
// THE decision of mri3d_conv_cin1_act_supported / _workspace_bytes / _route / _fwd / _bwd.  g: the convolution (y_ld = z's pitch);
// a_ld: the pitch of a (forward) or of da (backward); align: ptr_align of every tensor the pass touches.  fp32 only (bf16 streaming
// passes are instruction-bound and keep the separate launches).  The backward is conv_cin1_wgrad_kernel's sum order, so it is
// offered only where the plain weight gradient of the layer is that kernel: eight output channels (sixteen go to the MFMA file).
bool conv_cin1_act_supported(const Mri3dConvGeom& g, int a_ld, int act, int alpha_n, int pass, int align) {
    if (pass != MRI3D_PASS_FWD && pass != MRI3D_PASS_WGRAD) return false;
    if (g.dtype != MRI3D_F32 || !cin1_ok(g)) return false;   // (cin1_ok: y_ld % 4 == 0, tile count below 2^31)
    if (act != MRI3D_ACT_RELU && act != MRI3D_ACT_LEAKY && act != MRI3D_ACT_PRELU) return false;
    if (act == MRI3D_ACT_PRELU && alpha_n != 1 && alpha_n != g.co) return false;
    if (a_ld < g.co || a_ld % 4 != 0 || align < 16) return false;
    return pass == MRI3D_PASS_FWD || g.co == 8;
}

struct Cin1ActPlan {
    size_t part_floats, bias_floats, alpha_doubles;   // backward: the partials of dW, db and dalpha, in this order in the workspace
    size_t ws_bytes;
};

static Cin1ActPlan cin1_act_plan(const Mri3dConvGeom& g, int pass) {
    Cin1ActPlan p{0, 0, 0, 0};
    if (pass == MRI3D_PASS_FWD) {
        p.ws_bytes = (size_t)27 * g.co * sizeof(float);   // the repacked weights [tap][co]
        return p;
    }
    p.part_floats = (size_t)kCin1Shares * 27 * g.co, p.bias_floats = (size_t)kCin1Shares * g.co;
    p.alpha_doubles = (size_t)kCin1Shares * g.co;
    p.ws_bytes = (p.part_floats + p.bias_floats) * sizeof(float) + p.alpha_doubles * sizeof(double);   // (the floats: a multiple of 8 bytes)
    return p;
}

size_t conv_cin1_act_workspace_bytes(const Mri3dConvGeom& g, int pass) { return cin1_act_plan(g, pass).ws_bytes; }

bool conv_cin1_act_route_name(const Mri3dConvGeom& g, int a_ld, int act, int alpha_n, int pass, int align, char* name, size_t name_bytes) {
    const int len = conv_cin1_act_supported(g, a_ld, act, alpha_n, pass, align)
                        ? snprintf(name, name_bytes, "cin1 act %s co%d", pass == MRI3D_PASS_FWD ? "fwd" : "bwd", g.co)
                        : snprintf(name, name_bytes, "none");
    return len > 0 && (size_t)len < name_bytes;
}

int conv_cin1_act_fwd(const Mri3dConvGeom& g, int a_ld, int act, int alpha_n, float slope, const float* x, const float* w,
                      const float* bias, const float* alpha, float* z, float* a, void* ws, size_t ws_bytes, hipStream_t s) {
    MRI3D_REQUIRE(conv_cin1_act_supported(g, a_ld, act, alpha_n, MRI3D_PASS_FWD, ptr_align(z, a, ws)), MRI3D_ENOTSUP,
                  "conv_cin1_act_fwd: geometry / activation / alignment not served (query mri3d_conv_cin1_act_supported)");
    const Cin1ActPlan p = cin1_act_plan(g, MRI3D_PASS_FWD);
    MRI3D_REQUIRE(ws != nullptr && ws_bytes >= p.ws_bytes, MRI3D_EWORKSPACE, "conv_cin1_act_fwd: workspace %zu < %zu", ws_bytes, p.ws_bytes);
    float* wp = static_cast<float*>(ws);
    hipLaunchKernelGGL(repack_w_kernel, dim3(1), dim3(256), 0, s, w, wp, g.co, 1, 27, g.co, 0);
    const C1Tiles t = cin1_tiles(g);
    const int grid = std::min((int)t.ntiles, 256 * 8);
    const Cin1Act pa{alpha, alpha_n, act, slope};
    if (g.co == 8)
        hipLaunchKernelGGL(conv_cin1_act_fwd_kernel<8>, dim3(grid), dim3(256), 0, s, g, x, wp, bias, pa, z, a, a_ld, t.tilesD, t.tilesH,
                           t.tilesW, (int)t.ntiles);
    else
        hipLaunchKernelGGL(conv_cin1_act_fwd_kernel<16>, dim3(grid), dim3(256), 0, s, g, x, wp, bias, pa, z, a, a_ld, t.tilesD, t.tilesH,
                           t.tilesW, (int)t.ntiles);
    return check_launch("conv_cin1_act_fwd");
}

int conv_cin1_act_bwd(const Mri3dConvGeom& g, int da_ld, int act, int alpha_n, float slope, const float* x, const float* z,
                      const float* da, const float* alpha, float* dw, float* dbias, float* dalpha, void* ws, size_t ws_bytes,
                      hipStream_t s) {
    MRI3D_REQUIRE(conv_cin1_act_supported(g, da_ld, act, alpha_n, MRI3D_PASS_WGRAD, ptr_align(z, da, ws)), MRI3D_ENOTSUP,
                  "conv_cin1_act_bwd: geometry / activation / alignment not served (query mri3d_conv_cin1_act_supported)");
    const Cin1ActPlan p = cin1_act_plan(g, MRI3D_PASS_WGRAD);
    MRI3D_REQUIRE(ws != nullptr && ws_bytes >= p.ws_bytes, MRI3D_EWORKSPACE, "conv_cin1_act_bwd: workspace %zu < %zu", ws_bytes, p.ws_bytes);
    float* part = static_cast<float*>(ws);
    float* bias_part = dbias ? part + p.part_floats : nullptr;
    double* alpha_part = (dalpha && act == MRI3D_ACT_PRELU) ? reinterpret_cast<double*>(part + p.part_floats + p.bias_floats) : nullptr;
    const C1Tiles t = cin1_tiles(g);
    const Cin1Act pa{alpha, alpha_n, act, slope};
    // every workgroup writes its slots, also when its share of the tiles is empty (zeros)
    hipLaunchKernelGGL(conv_cin1_act_bwd_kernel<8>, dim3(kCin1Shares), dim3(768), 0, s, g, x, z, da, da_ld, pa, part, bias_part,
                       alpha_part, t.tilesD, t.tilesH, t.tilesW, (int)t.ntiles, kCin1Shares);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(g.co * 27 + g.co, 8)), dim3(256), 0, s, part, bias_part, dw, dbias, kCin1Shares,
                       27, 1, g.co, 1, g.co);
    if (alpha_part)
        hipLaunchKernelGGL(cin1_act_dalpha_kernel, dim3(1), dim3(256), 0, s, alpha_part, kCin1Shares, g.co, alpha_n, dalpha);
    return check_launch("conv_cin1_act_bwd");
}

}  // namespace mri3d
