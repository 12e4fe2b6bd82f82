// mc_stats.hip — Monte-Carlo predictive statistics over sampled forward passes (UNet3D(bayes=True), Dropout3d models).
// accumulate: per draw and voxel softmax(logits) -> state += (p_c, p_c^2, sum_c p_c log p_c); finalize: state -> mean prediction,
// population variance, predictive entropy, mutual information and the arg-max mask of the mean.  Both are HBM-bound streaming
// kernels like bayes.hip and elementwise.hip (stream_grid, 256 lanes).  The file is compiled with -ffp-contract=off and says fmaf
// where it wants one, so the vector path, the scalar path and a `reps` call against separate calls round identically.
//
// State (fp32, opaque to the caller), three planes, each starting on a multiple of 4 floats:
//     sum_p [nvox][c]    sum_p2 [nvox][c]    sum_plogp [nvox]
// Vector path (c == 2, dense logits, 16-byte aligned pointers and draws): a lane owns 4 consecutive voxels = 16 B of every plane
// access (two dwordx4 per [nvox][2] plane, one for [nvox]) and 32 B (fp32) / 16 B (bf16) of logits per draw; the nvox % 4 tail
// voxels take the scalar code in the same launch.  Scalar path: one voxel per lane, three passes over its c logits.
#include "common.h"

namespace mri3d {

constexpr int kMcMaxC = 32;
constexpr int kMcVox = 4;   // voxels per lane on the vector path

// V consecutive elements as floats (V = 4 or 8), 16 bytes per access (bf16: V = 8 only); p is 16-byte aligned
template <int V> __device__ __forceinline__ void mc_ld(const float* p, float (&r)[V]) {
#pragma unroll
    for (int k = 0; k < V; k += 4) {
        const float4 t = ldf4(p + k);
        r[k] = t.x, r[k + 1] = t.y, r[k + 2] = t.z, r[k + 3] = t.w;
    }
}
template <int V> __device__ __forceinline__ void mc_ld(const bf16_t* p, float (&r)[V]) {
    static_assert(V == 8, "one 16-byte access");
    const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (float)v[k];
}
template <int V> __device__ __forceinline__ void mc_st(float* p, const float (&r)[V]) {
#pragma unroll
    for (int k = 0; k < V; k += 4) stf4(p + k, make_float4(r[k], r[k + 1], r[k + 2], r[k + 3]));
}

struct McLayout {
    int64_t p2, plogp, total;   // float offsets of the sum_p2 and sum_plogp planes (sum_p is at 0), and the state's length
};

__host__ __device__ inline McLayout mc_layout(int64_t nvox, int c) {
    const int64_t plane = (nvox * c + 3) / 4 * 4;
    McLayout l;
    l.p2 = plane;
    l.plogp = 2 * plane;
    l.total = 2 * plane + (nvox + 3) / 4 * 4;
    return l;
}

// One draw of one voxel held in registers: z -> (sp, sq, sl) += (p, p^2, sum p log p).  log p comes from the logits, so a class
// whose probability underflows to 0 adds 0 * (finite) = 0.
// TWIN: mc_accumulate_voxel below is this arithmetic for a runtime class count.  The two must stay the same sequence of rounded
// operations (max left to right; S = 0 + e_0 + e_1 ...; p = e / S; sp + p; fmaf(p, p, sq); t = fmaf(p, (z - m) - lS, t) from 0;
// sl + t): a C = 2 call takes one or the other by alignment alone and promises the same bits
// (tests/test_mc_gpu.py::test_alignment_fallbacks_leave_the_same_bits, ::test_reps_call_leaves_the_bits_of_separate_calls).
template <int C> __device__ __forceinline__ void mc_draw(const float (&z)[C], float (&sp)[C], float (&sq)[C], float& sl) {
    float m = z[0];
#pragma unroll
    for (int j = 1; j < C; ++j) m = fmaxf(m, z[j]);
    float e[C], S = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        e[j] = expf(z[j] - m);
        S += e[j];
    }
    const float lS = logf(S);
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const float p = e[j] / S;
        sp[j] += p;
        sq[j] = fmaf(p, p, sq[j]);
        t = fmaf(p, (z[j] - m) - lS, t);
    }
    sl += t;
}

// The same arithmetic for a runtime class count: one voxel, its logits re-read per pass (they stay in L1), the state read and
// written once.  z points at draw 0 of the voxel; draw r is rep_elems elements further.
// TWIN: mc_draw above; change both or neither.
template <typename T>
__device__ __forceinline__ void mc_accumulate_voxel(const T* __restrict__ z0, int C, int reps, int64_t rep_elems, int first,
                                                    float* __restrict__ sp, float* __restrict__ sq, float* __restrict__ slp) {
    float sl = first ? 0.f : *slp;
    for (int r = 0; r < reps; ++r) {
        const T* z = z0 + r * rep_elems;
        float m = ldf(z);
        for (int j = 1; j < C; ++j) m = fmaxf(m, ldf(z + j));
        float S = 0.f;
        for (int j = 0; j < C; ++j) S += expf(ldf(z + j) - m);
        const float lS = logf(S);
        float t = 0.f;
        for (int j = 0; j < C; ++j) {
            const float d = ldf(z + j) - m;
            const float p = expf(d) / S;
            // the state is the accumulator: draw 0 of a `first` call starts from 0 instead of what the buffer holds
            const float a = (first && r == 0) ? 0.f : sp[j];
            const float b = (first && r == 0) ? 0.f : sq[j];
            sp[j] = a + p;
            sq[j] = fmaf(p, p, b);
            t = fmaf(p, d - lS, t);
        }
        sl += t;
    }
    *slp = sl;
}

template <typename T, bool VEC>
__device__ __forceinline__ void mc_accumulate_body(const T* __restrict__ logits, int64_t nvox, int C, int ld, int reps,
                                                   int64_t rep_stride, int first, float* __restrict__ state) {
    const McLayout lay = mc_layout(nvox, C);
    float* __restrict__ SP = state;
    float* __restrict__ SQ = state + lay.p2;
    float* __restrict__ SL = state + lay.plogp;
    const int64_t groups = VEC ? nvox / kMcVox : 0;       // lanes' worth of whole 4-voxel groups
    const int64_t items = groups + (nvox - groups * kMcVox);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        if (VEC && i < groups) {
            // C == 2, ld == 2: 8 logits, 8 + 8 + 4 state floats
            float sp[kMcVox][2], sq[kMcVox][2], sl[kMcVox];
            float* gp = SP + i * (kMcVox * 2);
            float* gq = SQ + i * (kMcVox * 2);
            float* gl = SL + i * kMcVox;
            if (first) {
#pragma unroll
                for (int k = 0; k < kMcVox; ++k) sp[k][0] = sp[k][1] = sq[k][0] = sq[k][1] = sl[k] = 0.f;
            } else {
                float a[8], b[8], l[4];
                mc_ld<8>(gp, a), mc_ld<8>(gq, b), mc_ld<4>(gl, l);
#pragma unroll
                for (int k = 0; k < kMcVox; ++k)
                    sp[k][0] = a[2 * k], sp[k][1] = a[2 * k + 1], sq[k][0] = b[2 * k], sq[k][1] = b[2 * k + 1], sl[k] = l[k];
            }
            for (int r = 0; r < reps; ++r) {
                float z[8];
                mc_ld<8>(logits + (r * rep_stride + i * kMcVox) * 2, z);
#pragma unroll
                for (int k = 0; k < kMcVox; ++k) {
                    const float zz[2] = {z[2 * k], z[2 * k + 1]};
                    mc_draw<2>(zz, sp[k], sq[k], sl[k]);
                }
            }
            float a[8], b[8];
#pragma unroll
            for (int k = 0; k < kMcVox; ++k)
                a[2 * k] = sp[k][0], a[2 * k + 1] = sp[k][1], b[2 * k] = sq[k][0], b[2 * k + 1] = sq[k][1];
            mc_st<8>(gp, a), mc_st<8>(gq, b), mc_st<4>(gl, sl);
        } else {
            const int64_t v = groups * kMcVox + (i - groups);
            mc_accumulate_voxel(logits + v * ld, C, reps, rep_stride * ld, first, SP + v * C, SQ + v * C, SL + v);
        }
    }
}

// One voxel of finalize from its sums in registers.  The mask takes the first maximal mean with argmax_u8_kernel's rule
// (loss.hip), on the floats that go to mean_p.
// TWIN: mc_finalize_voxel below is this arithmetic for a runtime class count, operation for operation; change both or neither
// (tests/test_mc_gpu.py::test_alignment_fallbacks_leave_the_same_bits compares the two bit for bit).
template <int C>
__device__ __forceinline__ void mc_final(const float (&sp)[C], const float (&sq)[C], float sl, float T, float (&mean)[C],
                                         float (&var)[C], float& ent, float& mi, uint8_t& mask) {
    float h = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        mean[j] = sp[j] / T;
        var[j] = fmaxf(fmaf(-mean[j], mean[j], sq[j] / T), 0.f);
        if (mean[j] > 0.f) h = fmaf(mean[j], logf(mean[j]), h);
    }
    ent = -h;
    mi = fmaxf(ent + sl / T, 0.f);
    float best = mean[0];
    int bi = 0;
#pragma unroll
    for (int j = 1; j < C; ++j) {
        const float t = mean[j];
        if ((t > best && best == best) || (t != t && best == best)) { best = t, bi = j; }
    }
    mask = (uint8_t)bi;
}

struct McOut {
    float* mean;
    float* var;
    float* ent;
    float* mi;
    uint8_t* mask;
};

// TWIN: mc_final above.
__device__ __forceinline__ void mc_finalize_voxel(const float* __restrict__ sp, const float* __restrict__ sq, float sl, int C,
                                                  float T, int64_t v, const McOut& o) {
    float h = 0.f, best = 0.f;
    int bi = 0;
    for (int j = 0; j < C; ++j) {
        const float mean = sp[j] / T;
        if (o.mean) o.mean[v * C + j] = mean;
        if (o.var) o.var[v * C + j] = fmaxf(fmaf(-mean, mean, sq[j] / T), 0.f);
        if (mean > 0.f) h = fmaf(mean, logf(mean), h);
        if (j == 0) best = mean;
        else if ((mean > best && best == best) || (mean != mean && best == best)) { best = mean, bi = j; }
    }
    const float ent = -h;
    if (o.ent) o.ent[v] = ent;
    if (o.mi) o.mi[v] = fmaxf(ent + sl / T, 0.f);
    if (o.mask) o.mask[v] = (uint8_t)bi;
}

template <bool VEC>
__device__ __forceinline__ void mc_finalize_body(const float* __restrict__ state, int64_t nvox, int C, float T, const McOut& o) {
    const McLayout lay = mc_layout(nvox, C);
    const float* __restrict__ SP = state;
    const float* __restrict__ SQ = state + lay.p2;
    const float* __restrict__ SL = state + lay.plogp;
    const int64_t groups = VEC ? nvox / kMcVox : 0;
    const int64_t items = groups + (nvox - groups * kMcVox);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        if (VEC && i < groups) {
            float a[8], b[8], l[4] = {0.f, 0.f, 0.f, 0.f};
            mc_ld<8>(SP + i * (kMcVox * 2), a);
            if (o.var) {
                mc_ld<8>(SQ + i * (kMcVox * 2), b);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) b[k] = 0.f;
            }
            if (o.mi) mc_ld<4>(SL + i * kMcVox, l);
            float mean[8], var[8], ent[4], mi[4];
            uchar4 mk;
            uint8_t* mkp = reinterpret_cast<uint8_t*>(&mk);
#pragma unroll
            for (int k = 0; k < kMcVox; ++k) {
                const float sp[2] = {a[2 * k], a[2 * k + 1]}, sq[2] = {b[2 * k], b[2 * k + 1]};
                float mn[2], vr[2];
                mc_final<2>(sp, sq, l[k], T, mn, vr, ent[k], mi[k], mkp[k]);
                mean[2 * k] = mn[0], mean[2 * k + 1] = mn[1], var[2 * k] = vr[0], var[2 * k + 1] = vr[1];
            }
            if (o.mean) mc_st<8>(o.mean + i * (kMcVox * 2), mean);
            if (o.var) mc_st<8>(o.var + i * (kMcVox * 2), var);
            if (o.ent) mc_st<4>(o.ent + i * kMcVox, ent);
            if (o.mi) mc_st<4>(o.mi + i * kMcVox, mi);
            if (o.mask) *reinterpret_cast<uchar4*>(o.mask + i * kMcVox) = mk;
        } else {
            const int64_t v = groups * kMcVox + (i - groups);
            mc_finalize_voxel(SP + v * C, SQ + v * C, SL[v], C, T, v, o);
        }
    }
}

// The two kernels, each under one name per path, so that a profile or a test sees which one a call took.
template <typename T>
__global__ void __launch_bounds__(256)
mc_accumulate_vec_kernel(const T* __restrict__ logits, int64_t nvox, int C, int ld, int reps, int64_t rep_stride, int first,
                         float* __restrict__ state) {
    mc_accumulate_body<T, true>(logits, nvox, C, ld, reps, rep_stride, first, state);
}
template <typename T>
__global__ void __launch_bounds__(256)
mc_accumulate_scalar_kernel(const T* __restrict__ logits, int64_t nvox, int C, int ld, int reps, int64_t rep_stride, int first,
                            float* __restrict__ state) {
    mc_accumulate_body<T, false>(logits, nvox, C, ld, reps, rep_stride, first, state);
}
__global__ void __launch_bounds__(256)
mc_finalize_vec_kernel(const float* __restrict__ state, int64_t nvox, int C, float T, McOut o) {
    mc_finalize_body<true>(state, nvox, C, T, o);
}
__global__ void __launch_bounds__(256)
mc_finalize_scalar_kernel(const float* __restrict__ state, int64_t nvox, int C, float T, McOut o) {
    mc_finalize_body<false>(state, nvox, C, T, o);
}

}  // namespace mri3d

using namespace mri3d;

static inline bool mc_classes_ok(int c) { return c >= 2 && c <= kMcMaxC; }

extern "C" size_t mri3d_mc_state_bytes(int64_t nvox, int32_t c) {
    if (nvox <= 0 || !mc_classes_ok(c)) return 0;
    return (size_t)mc_layout(nvox, c).total * sizeof(float);
}

extern "C" int mri3d_mc_accumulate(const void* logits, int64_t nvox, int32_t c, int32_t ld, int32_t dtype, int32_t reps,
                                   int64_t rep_stride, int32_t first, void* state, size_t state_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(dtype == MRI3D_F32 || dtype == MRI3D_BF16, MRI3D_ENOTSUP, "mc_accumulate: unknown dtype %d", dtype);
    MRI3D_REQUIRE(mc_classes_ok(c), MRI3D_ENOTSUP, "mc_accumulate: c = %d outside 2..%d", c, kMcMaxC);
    MRI3D_REQUIRE(logits && state && nvox > 0, MRI3D_EINVAL, "mc_accumulate: bad arguments");
    MRI3D_REQUIRE(ld >= c, MRI3D_EINVAL, "mc_accumulate: ld %d < c %d", ld, c);
    MRI3D_REQUIRE(reps >= 1 && (reps == 1 || rep_stride >= nvox), MRI3D_EINVAL,
                  "mc_accumulate: reps %d with rep_stride %lld (needs reps >= 1 and draws that do not overlap)", reps,
                  (long long)rep_stride);
    MRI3D_REQUIRE(state_bytes >= mri3d_mc_state_bytes(nvox, c) && (reinterpret_cast<uintptr_t>(state) & 3) == 0, MRI3D_EINVAL,
                  "mc_accumulate: state of %zu bytes < %zu, or not 4-byte aligned", state_bytes, mri3d_mc_state_bytes(nvox, c));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every draw's first logit 16-byte aligned: draw r starts r * rep_stride * 2 elements in
    const int64_t draw_bytes = rep_stride * 2 * (int64_t)dtype_size(dtype);
    const bool vec = c == 2 && ld == 2 && aligned16(logits, state) && (reps == 1 || draw_bytes % 16 == 0);
    const int64_t items = vec ? nvox / kMcVox + nvox % kMcVox : nvox;
    const int grid = stream_grid(items, 256);
    MRI3D_DISPATCH_DTYPE(dtype, T, {
        if (vec)
            hipLaunchKernelGGL(mc_accumulate_vec_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)logits, nvox, c, ld, reps,
                               rep_stride, first, (float*)state);
        else
            hipLaunchKernelGGL(mc_accumulate_scalar_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)logits, nvox, c, ld, reps,
                               rep_stride, first, (float*)state);
    });
    return check_launch("mc_accumulate");
}

extern "C" int mri3d_mc_finalize(const void* state, size_t state_bytes, int64_t nvox, int32_t c, int32_t samples, float* mean_p,
                                 float* variance, float* entropy, float* mutual_info, uint8_t* mask, mri3d_stream_t stream) {
    MRI3D_REQUIRE(mc_classes_ok(c), MRI3D_ENOTSUP, "mc_finalize: c = %d outside 2..%d", c, kMcMaxC);
    MRI3D_REQUIRE(state && nvox > 0, MRI3D_EINVAL, "mc_finalize: bad arguments");
    MRI3D_REQUIRE(samples >= 1, MRI3D_EINVAL, "mc_finalize: samples %d < 1", samples);
    MRI3D_REQUIRE(mean_p || variance || entropy || mutual_info || mask, MRI3D_EINVAL, "mc_finalize: no output requested");
    MRI3D_REQUIRE(state_bytes >= mri3d_mc_state_bytes(nvox, c) && (reinterpret_cast<uintptr_t>(state) & 3) == 0, MRI3D_EINVAL,
                  "mc_finalize: state of %zu bytes < %zu, or not 4-byte aligned", state_bytes, mri3d_mc_state_bytes(nvox, c));
    MRI3D_REQUIRE(((reinterpret_cast<uintptr_t>(mean_p) | reinterpret_cast<uintptr_t>(variance) |
                    reinterpret_cast<uintptr_t>(entropy) | reinterpret_cast<uintptr_t>(mutual_info)) & 3) == 0,
                  MRI3D_EINVAL, "mc_finalize: a float output is not 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec = c == 2 && aligned16(state, mean_p, variance) && aligned16(entropy, mutual_info) &&
                     (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    const int64_t items = vec ? nvox / kMcVox + nvox % kMcVox : nvox;
    const int grid = stream_grid(items, 256);
    const McOut o = {mean_p, variance, entropy, mutual_info, mask};
    if (vec) hipLaunchKernelGGL(mc_finalize_vec_kernel, dim3(grid), dim3(256), 0, s, (const float*)state, nvox, c, (float)samples, o);
    else hipLaunchKernelGGL(mc_finalize_scalar_kernel, dim3(grid), dim3(256), 0, s, (const float*)state, nvox, c, (float)samples, o);
    return check_launch("mc_finalize");
}
