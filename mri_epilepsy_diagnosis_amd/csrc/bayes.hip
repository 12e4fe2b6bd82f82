// bayes.hip — the passes of BayesConv3d (variational dropout, reference segmentation/models/3d_bayes_layers.py:195-232) that are
// not convolutions: the weight transform (mu, logsigma) -> (w_mean, w_var, log_alpha) with its backward, x^2, the sampling
// y = mu_out + eps * sqrt(1e-4 + var_out) with its backward, and dx = dx_mean + 2 x dx_var.  The two convolutions and their
// gradients run on the convolution kernels; the noise eps is an INPUT (fp32, drawn by the caller), nothing here is random.
// The volume kernels are HBM-bound streaming kernels like elementwise.hip: 16 B per lane in the storage type when the channel
// count, pitches and pointers allow it (4 floats / 8 bf16), one element per lane otherwise.
#include "common.h"

namespace mri3d {

constexpr float kBayesLogEps = 1e-8f;   // log(mu^2 + 1e-8)
constexpr float kBayesVarEps = 1e-4f;   // sqrt(1e-4 + var_out)

// ---------------------------------------------------------------- V consecutive elements as floats (V = 1, 4 or 8)
template <int V, typename T> __device__ __forceinline__ void ldv(const T* p, float (&r)[V]) {
    if constexpr (V == 1) {
        r[0] = ldf(p);
    } else if constexpr (V == 8 && sizeof(T) == 2) {
        const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = (float)v[k];
    } else {
#pragma unroll
        for (int k = 0; k < V; k += 4) {
            const float4 t = ldf4(p + k);
            r[k] = t.x, r[k + 1] = t.y, r[k + 2] = t.z, r[k + 3] = t.w;
        }
    }
}

template <int V, typename T> __device__ __forceinline__ void stv(T* p, const float (&r)[V]) {
    if constexpr (V == 1) {
        stf(p, r[0]);
    } else if constexpr (V == 8 && sizeof(T) == 2) {
        bf16x8_t o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (bf16_t)r[k];
        *reinterpret_cast<bf16x8_t*>(p) = o;
    } else {
#pragma unroll
        for (int k = 0; k < V; k += 4) stf4(p + k, make_float4(r[k], r[k + 1], r[k + 2], r[k + 3]));
    }
}

// ---------------------------------------------------------------- weight transform
struct BayesW {
    float alpha, ea, v, q;   // clamp(raw, -5, 5), exp(alpha), mu^2 exp(alpha), mu^2 + 1e-8
    bool in, keep;           // raw inside the closed clamp interval; eval-mode mask alpha < threshold (true in train mode)
};

__device__ __forceinline__ BayesW bayes_w(float mu, float ls, int eval, float threshold) {
    BayesW r;
    r.q = fmaf(mu, mu, kBayesLogEps);
    const float raw = ls - logf(r.q);
    r.in = raw >= -5.f && raw <= 5.f;
    r.alpha = fminf(fmaxf(raw, -5.f), 5.f);
    r.ea = expf(r.alpha);
    r.v = mu * mu * r.ea;
    r.keep = !eval || r.alpha < threshold;
    return r;
}

__global__ void __launch_bounds__(256)
bayes_weights_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ ls, int64_t n, int eval, float threshold,
                         float* __restrict__ w_mean, float* __restrict__ w_var, float* __restrict__ log_alpha) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float m = mu[i];
        const BayesW r = bayes_w(m, ls[i], eval, threshold);
        w_var[i] = r.keep ? r.v : 0.f;
        log_alpha[i] = r.alpha;
        if (eval) w_mean[i] = r.keep ? m : 0.f;
    }
}

// dmu, dlogsigma from the gradients of w_mean, w_var and log_alpha (each pointer may be null: no such gradient).  With
// q = mu^2 + 1e-8 and `in` the clamp's pass-through:  d alpha / d logsigma = in,  d alpha / d mu = -in 2 mu / q,
// d v / d logsigma = in v,  d v / d mu = 2 mu e^alpha (1 - in mu^2 / q) = 2 mu e^alpha (in ? 1e-8 / q : 1)  — the last form has
// no cancellation.  The eval-mode mask multiplies the two weight gradients and carries none itself.
__global__ void __launch_bounds__(256)
bayes_weights_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ ls, int64_t n, int eval, float threshold,
                         const float* __restrict__ d_w_mean, const float* __restrict__ d_w_var,
                         const float* __restrict__ d_log_alpha, float* __restrict__ dmu, float* __restrict__ dls) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float m = mu[i];
        const BayesW r = bayes_w(m, ls[i], eval, threshold);
        const float gm = (d_w_mean && r.keep) ? d_w_mean[i] : 0.f;
        const float gv = (d_w_var && r.keep) ? d_w_var[i] : 0.f;
        const float ga = (d_log_alpha && r.in) ? d_log_alpha[i] : 0.f;
        const float two_mu = 2.f * m;
        const float dv_dmu = two_mu * r.ea * (r.in ? kBayesLogEps / r.q : 1.f);
        dmu[i] = gm + gv * dv_dmu - ga * (two_mu / r.q);
        dls[i] = r.in ? fmaf(gv, r.v, ga) : 0.f;
    }
}

// ---------------------------------------------------------------- volume passes
template <typename T, int V>
__global__ void __launch_bounds__(256)
bayes_square_kernel(const T* __restrict__ x, T* __restrict__ x2, int64_t nvox, int C, int x_ld, int x2_ld) {
    const int CV = C / V;
    const int64_t total = nvox * CV;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV) * V;
        const int64_t v = i / CV;
        float a[V];
        ldv<V>(x + v * x_ld + c, a);
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] *= a[k];
        stv<V>(x2 + v * x2_ld + c, a);
    }
}

// y may be mu_out itself (each lane reads its elements before it writes them): no __restrict__ on the two
template <typename T, int V>
__global__ void __launch_bounds__(256)
bayes_sample_fwd_kernel(const T* mu_out, const T* __restrict__ var_out, const float* __restrict__ eps, T* y, int64_t nvox,
                        int C, int mu_ld, int var_ld, int eps_ld, int y_ld) {
    const int CV = C / V;
    const int64_t total = nvox * CV;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV) * V;
        const int64_t v = i / CV;
        float m[V], s[V], e[V];
        ldv<V>(mu_out + v * mu_ld + c, m);
        ldv<V>(var_out + v * var_ld + c, s);
        ldv<V>(eps + v * eps_ld + c, e);
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = fmaf(e[k], sqrtf(kBayesVarEps + s[k]), m[k]);
        stv<V>(y + v * y_ld + c, m);
    }
}

template <typename T, int V>
__global__ void __launch_bounds__(256)
bayes_sample_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ var_out, const float* __restrict__ eps,
                        T* __restrict__ dvar, int64_t nvox, int C, int dy_ld, int var_ld, int eps_ld, int dvar_ld) {
    const int CV = C / V;
    const int64_t total = nvox * CV;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV) * V;
        const int64_t v = i / CV;
        float g[V], s[V], e[V];
        ldv<V>(dy + v * dy_ld + c, g);
        ldv<V>(var_out + v * var_ld + c, s);
        ldv<V>(eps + v * eps_ld + c, e);
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = g[k] * e[k] / (2.f * sqrtf(kBayesVarEps + s[k]));
        stv<V>(dvar + v * dvar_ld + c, g);
    }
}

// dx may be dx_mean itself
template <typename T, int V>
__global__ void __launch_bounds__(256)
bayes_dx_kernel(const T* dx_mean, const T* __restrict__ dx_var, const T* __restrict__ x, T* dx, int64_t nvox, int C, int m_ld,
                int v_ld, int x_ld, int dx_ld) {
    const int CV = C / V;
    const int64_t total = nvox * CV;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV) * V;
        const int64_t v = i / CV;
        float a[V], b[V], xx[V];
        ldv<V>(dx_mean + v * m_ld + c, a);
        ldv<V>(dx_var + v * v_ld + c, b);
        ldv<V>(x + v * x_ld + c, xx);
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] = fmaf(2.f * xx[k], b[k], a[k]);
        stv<V>(dx + v * dx_ld + c, a);
    }
}

}  // namespace mri3d

using namespace mri3d;

static inline bool known_dtype(int d) { return d == MRI3D_F32 || d == MRI3D_BF16; }

// Elements per lane: 16 bytes of the storage type (4 floats, 8 bf16) when the channel count and every pitch are multiples of it
// and every pointer is 16-byte aligned (an fp32 eps beside bf16 tensors is then read as two 16-byte pieces); else 1.
static int bayes_vec(int dtype, int c, const int* lds, int n_ld, const void* p0, const void* p1, const void* p2, const void* p3) {
    const int v = dtype == MRI3D_BF16 ? 8 : 4;
    if (c % v) return 1;
    for (int i = 0; i < n_ld; ++i)
        if (lds[i] % v) return 1;
    return (aligned16(p0, p1, p2) && aligned16(p3)) ? v : 1;
}

// Launch `kernel<T, V>` with T from dtype and V from `vec` (fp32: 4 or 1; bf16: 8 or 1).
#define MRI3D_BAYES_LAUNCH(kernel, dtype, vec, grid, s, ...)                                               \
    do {                                                                                                   \
        if ((dtype) == MRI3D_BF16) {                                                                       \
            using T = ::mri3d::bf16_t;                                                                     \
            if ((vec) == 8) hipLaunchKernelGGL((kernel<T, 8>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);  \
            else hipLaunchKernelGGL((kernel<T, 1>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);             \
        } else {                                                                                           \
            using T = float;                                                                               \
            if ((vec) == 4) hipLaunchKernelGGL((kernel<T, 4>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);  \
            else hipLaunchKernelGGL((kernel<T, 1>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);             \
        }                                                                                                  \
    } while (0)

extern "C" int mri3d_bayes_weights_fwd(const float* mu, const float* logsigma, int64_t n, int32_t eval, float threshold,
                                       float* w_mean, float* w_var, float* log_alpha, mri3d_stream_t stream) {
    MRI3D_REQUIRE(mu && logsigma && w_var && log_alpha && n > 0, MRI3D_EINVAL, "bayes_weights_fwd: bad arguments");
    MRI3D_REQUIRE(!eval || w_mean, MRI3D_EINVAL, "bayes_weights_fwd: eval mode needs w_mean");
    hipLaunchKernelGGL(bayes_weights_fwd_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), mu,
                       logsigma, n, eval, threshold, w_mean, w_var, log_alpha);
    return check_launch("bayes_weights_fwd");
}

extern "C" int mri3d_bayes_weights_bwd(const float* mu, const float* logsigma, int64_t n, int32_t eval, float threshold,
                                       const float* d_w_mean, const float* d_w_var, const float* d_log_alpha, float* dmu,
                                       float* dlogsigma, mri3d_stream_t stream) {
    MRI3D_REQUIRE(mu && logsigma && dmu && dlogsigma && n > 0, MRI3D_EINVAL, "bayes_weights_bwd: bad arguments");
    hipLaunchKernelGGL(bayes_weights_bwd_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), mu,
                       logsigma, n, eval, threshold, d_w_mean, d_w_var, d_log_alpha, dmu, dlogsigma);
    return check_launch("bayes_weights_bwd");
}

extern "C" int mri3d_bayes_square(const void* x, void* x2, int64_t nvox, int32_t c, int32_t x_ld, int32_t x2_ld, int32_t dtype,
                                  mri3d_stream_t stream) {
    MRI3D_REQUIRE(known_dtype(dtype), MRI3D_ENOTSUP, "bayes_square: unknown dtype %d", dtype);
    MRI3D_REQUIRE(x && x2 && nvox > 0 && c > 0 && x_ld >= c && x2_ld >= c, MRI3D_EINVAL, "bayes_square: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lds[] = {x_ld, x2_ld};
    const int vec = bayes_vec(dtype, c, lds, 2, x, x2, nullptr, nullptr);
    const int grid = stream_grid(nvox * (c / vec), 256);
    MRI3D_BAYES_LAUNCH(bayes_square_kernel, dtype, vec, grid, s, (const T*)x, (T*)x2, nvox, c, x_ld, x2_ld);
    return check_launch("bayes_square");
}

extern "C" int mri3d_bayes_sample_fwd(const void* mu_out, const void* var_out, const float* eps, void* y, int64_t nvox,
                                      int32_t c, int32_t mu_ld, int32_t var_ld, int32_t eps_ld, int32_t y_ld, int32_t dtype,
                                      mri3d_stream_t stream) {
    MRI3D_REQUIRE(known_dtype(dtype), MRI3D_ENOTSUP, "bayes_sample_fwd: unknown dtype %d", dtype);
    MRI3D_REQUIRE(mu_out && var_out && eps && y && nvox > 0 && c > 0 && mu_ld >= c && var_ld >= c && eps_ld >= c && y_ld >= c,
                  MRI3D_EINVAL, "bayes_sample_fwd: bad arguments");
    MRI3D_REQUIRE(y != mu_out || y_ld == mu_ld, MRI3D_EINVAL, "bayes_sample_fwd: in place needs y_ld == mu_ld");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lds[] = {mu_ld, var_ld, eps_ld, y_ld};
    const int vec = bayes_vec(dtype, c, lds, 4, mu_out, var_out, eps, y);
    const int grid = stream_grid(nvox * (c / vec), 256);
    MRI3D_BAYES_LAUNCH(bayes_sample_fwd_kernel, dtype, vec, grid, s, (const T*)mu_out, (const T*)var_out, eps, (T*)y, nvox, c,
                       mu_ld, var_ld, eps_ld, y_ld);
    return check_launch("bayes_sample_fwd");
}

extern "C" int mri3d_bayes_sample_bwd(const void* dy, const void* var_out, const float* eps, void* dvar, int64_t nvox,
                                      int32_t c, int32_t dy_ld, int32_t var_ld, int32_t eps_ld, int32_t dvar_ld, int32_t dtype,
                                      mri3d_stream_t stream) {
    MRI3D_REQUIRE(known_dtype(dtype), MRI3D_ENOTSUP, "bayes_sample_bwd: unknown dtype %d", dtype);
    MRI3D_REQUIRE(dy && var_out && eps && dvar && nvox > 0 && c > 0 && dy_ld >= c && var_ld >= c && eps_ld >= c && dvar_ld >= c,
                  MRI3D_EINVAL, "bayes_sample_bwd: bad arguments");
    MRI3D_REQUIRE(dvar != dy && dvar != var_out && dvar != (const void*)eps, MRI3D_EINVAL, "bayes_sample_bwd: dvar aliases an input");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lds[] = {dy_ld, var_ld, eps_ld, dvar_ld};
    const int vec = bayes_vec(dtype, c, lds, 4, dy, var_out, eps, dvar);
    const int grid = stream_grid(nvox * (c / vec), 256);
    MRI3D_BAYES_LAUNCH(bayes_sample_bwd_kernel, dtype, vec, grid, s, (const T*)dy, (const T*)var_out, eps, (T*)dvar, nvox, c,
                       dy_ld, var_ld, eps_ld, dvar_ld);
    return check_launch("bayes_sample_bwd");
}

extern "C" int mri3d_bayes_dx(const void* dx_mean, const void* dx_var, const void* x, void* dx, int64_t nvox, int32_t c,
                              int32_t dx_mean_ld, int32_t dx_var_ld, int32_t x_ld, int32_t dx_ld, int32_t dtype,
                              mri3d_stream_t stream) {
    MRI3D_REQUIRE(known_dtype(dtype), MRI3D_ENOTSUP, "bayes_dx: unknown dtype %d", dtype);
    MRI3D_REQUIRE(dx_mean && dx_var && x && dx && nvox > 0 && c > 0 && dx_mean_ld >= c && dx_var_ld >= c && x_ld >= c && dx_ld >= c,
                  MRI3D_EINVAL, "bayes_dx: bad arguments");
    MRI3D_REQUIRE(dx != dx_mean || dx_ld == dx_mean_ld, MRI3D_EINVAL, "bayes_dx: in place needs dx_ld == dx_mean_ld");
    MRI3D_REQUIRE(dx != dx_var && dx != x, MRI3D_EINVAL, "bayes_dx: dx aliases dx_var or x");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lds[] = {dx_mean_ld, dx_var_ld, x_ld, dx_ld};
    const int vec = bayes_vec(dtype, c, lds, 4, dx_mean, dx_var, x, dx);
    const int grid = stream_grid(nvox * (c / vec), 256);
    MRI3D_BAYES_LAUNCH(bayes_dx_kernel, dtype, vec, grid, s, (const T*)dx_mean, (const T*)dx_var, (const T*)x, (T*)dx, nvox, c,
                       dx_mean_ld, dx_var_ld, x_ld, dx_ld);
    return check_launch("bayes_dx");
}
