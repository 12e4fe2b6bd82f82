// api.hip — C-ABI entry points that are not tied to one kernel file: version, error string, and the Conv3d
// dispatcher (generic direct kernels vs. the MFMA implicit-GEMM path for 3x3x3 stride-1 layers).
#include "common.h"
#include "conv_backends.h"
#include <string.h>

namespace mri3d {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// (the aligned16 tests of the entry points below: the MFMA kernels move 16-byte pieces, so a pitched channel slice whose base is
// not 16-byte aligned, legal for the generic kernels, must not be routed to them)
// first_ci >= 0: the input is split over two tensors (the *_cat entry points) and x_ld is the pitch of the first, which holds
// first_ci channels
static int conv_check(const Mri3dConvGeom* g, const char* who, int first_ci = -1) {
    MRI3D_REQUIRE(g != nullptr, MRI3D_EINVAL, "%s: null geometry", who);
    MRI3D_REQUIRE(g->dtype == MRI3D_F32 || g->dtype == MRI3D_BF16, MRI3D_ENOTSUP, "%s: unknown dtype %d", who, g->dtype);
    MRI3D_REQUIRE(g->n > 0 && g->di > 0 && g->hi > 0 && g->wi > 0 && g->ci > 0 && g->dout > 0 && g->ho > 0 && g->wo > 0 &&
                      g->co > 0,
                  MRI3D_EINVAL, "%s: empty tensor", who);
    MRI3D_REQUIRE(g->kd > 0 && g->kh > 0 && g->kw > 0 && g->sd > 0 && g->sh > 0 && g->sw > 0 && g->dd > 0 && g->dh > 0 &&
                      g->dw > 0 && g->pd >= 0 && g->ph >= 0 && g->pw >= 0,
                  MRI3D_EINVAL, "%s: bad kernel/stride/padding/dilation", who);
    MRI3D_REQUIRE(g->x_ld >= (first_ci >= 0 ? first_ci : g->ci) && g->y_ld >= g->co, MRI3D_EINVAL, "%s: pitch smaller than channel count", who);
    // torch: out = floor((in + 2p - d(k-1) - 1)/s) + 1
    int ed = (g->di + 2 * g->pd - g->dd * (g->kd - 1) - 1) / g->sd + 1;
    int eh = (g->hi + 2 * g->ph - g->dh * (g->kh - 1) - 1) / g->sh + 1;
    int ew = (g->wi + 2 * g->pw - g->dw * (g->kw - 1) - 1) / g->sw + 1;
    MRI3D_REQUIRE(ed == g->dout && eh == g->ho && ew == g->wo, MRI3D_EINVAL,
                  "%s: output dims (%d,%d,%d) do not match conv arithmetic (%d,%d,%d)", who, g->dout, g->ho, g->wo, ed, eh,
                  ew);
    return MRI3D_OK;
}

// THE backend decision of the Conv3d entry points: mri3d_conv3d_fwd / _fwd_stats / _dgrad / _wgrad (split == 0), the *_cat entry
// points (split > 0) and the route query mri3d_conv3d_route all read it, so the query names what the entry point launches.
// Forward tries the MFMA file before the pointwise kernels, the gradients the pointwise kernels first; whatever neither takes goes
// to the generic kernels.  Fused statistics and split operands exist only in the MFMA file: `none` = the entry point refuses.
// align_mfma: common alignment in bytes (ptr_align) of the tensors and the workspace the MFMA kernels move in 16-byte pieces;
// align_pw: that of the tensor the pointwise kernels access four elements at a time.
enum class ConvBackend { none, generic, pointwise, mfma };

static ConvBackend conv_backend(const Mri3dConvGeom& g, int pass, bool stats, int split, int second_ld, int align_mfma, int align_pw) {
    const bool mfma_aligned = align_mfma >= 16;                                  // aligned16
    const bool pw_aligned = align_pw >= (g.dtype == MRI3D_BF16 ? 8 : 16);        // aligned_vec4
    if (split > 0) {
        if (!(conv_mfma_cat_supported(g, split, second_ld, pass) && mfma_aligned)) return ConvBackend::none;
        return (stats && conv_mfma_fwd_stat_blocks(g, split, second_ld) <= 0) ? ConvBackend::none : ConvBackend::mfma;
    }
    if (stats)
        return (pass == MRI3D_PASS_FWD && conv_mfma_supported(g, MRI3D_PASS_FWD) && conv_mfma_fwd_stat_blocks(g) > 0 && mfma_aligned)
                   ? ConvBackend::mfma : ConvBackend::none;
    if (pass == MRI3D_PASS_FWD) {
        if (conv_mfma_supported(g, pass) && mfma_aligned) return ConvBackend::mfma;
        if (conv_pointwise_supported(g, pass) && pw_aligned) return ConvBackend::pointwise;
        return ConvBackend::generic;
    }
    if (conv_pointwise_supported(g, pass) && pw_aligned) return ConvBackend::pointwise;
    if (conv_mfma_supported(g, pass) && mfma_aligned) return ConvBackend::mfma;
    return ConvBackend::generic;
}

}  // namespace mri3d

using namespace mri3d;

extern "C" int mri3d_version(void) { return 100; }  // 0.1.0
extern "C" const char* mri3d_last_error(void) { return g_err; }

extern "C" size_t mri3d_conv3d_workspace_bytes(const Mri3dConvGeom* g, int pass) {
    if (!g) return 0;
    size_t a = conv_generic_workspace_bytes(*g, pass);
    size_t b = conv_mfma_supported(*g, pass) ? conv_mfma_workspace_bytes(*g, pass) : 0;
    size_t c = conv_pointwise_supported(*g, pass) ? conv_pointwise_workspace_bytes(*g, pass) : 0;
    a = a > b ? a : b;
    return align_up(a > c ? a : c, 256);
}

extern "C" int mri3d_conv3d_fwd(const Mri3dConvGeom* g, const void* x, const void* w, const void* bias, void* y,
                                void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_fwd");
    if (rc) return rc;
    MRI3D_REQUIRE(x && w && y, MRI3D_EINVAL, "conv3d_fwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (conv_backend(*g, MRI3D_PASS_FWD, false, 0, 0, ptr_align(x, y, workspace), ptr_align(x))) {
    case ConvBackend::mfma: return conv_mfma_fwd(*g, x, (const float*)w, (const float*)bias, y, workspace, ws_bytes, s);
    case ConvBackend::pointwise: return conv_pointwise_fwd(*g, x, (const float*)w, (const float*)bias, y, s);
    default: return conv_generic_fwd(*g, x, (const float*)w, (const float*)bias, y, workspace, ws_bytes, s);
    }
}

extern "C" int32_t mri3d_conv3d_fwd_stats_blocks(const Mri3dConvGeom* g) {
    if (!g || conv_check(g, "conv3d_fwd_stats_blocks") != MRI3D_OK) return 0;
    return conv_mfma_supported(*g, MRI3D_PASS_FWD) ? conv_mfma_fwd_stat_blocks(*g) : 0;
}

extern "C" int mri3d_conv3d_fwd_stats(const Mri3dConvGeom* g, const void* x, const void* w, const void* bias, void* y,
                                      double* stat_partials, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_fwd_stats");
    if (rc) return rc;
    MRI3D_REQUIRE(x && w && y && stat_partials, MRI3D_EINVAL, "conv3d_fwd_stats: null pointer");
    MRI3D_REQUIRE(conv_backend(*g, MRI3D_PASS_FWD, true, 0, 0, ptr_align(x, y, workspace), ptr_align(x)) == ConvBackend::mfma,
                  MRI3D_ENOTSUP, "conv3d_fwd_stats: geometry not served by the MFMA forward kernel (query mri3d_conv3d_fwd_stats_blocks)");
    return conv_mfma_fwd_stats(*g, x, (const float*)w, (const float*)bias, y, stat_partials, workspace, ws_bytes,
                               static_cast<hipStream_t>(stream));
}

extern "C" int mri3d_conv3d_dgrad(const Mri3dConvGeom* g, const void* dy, const void* w, const void* bias, void* dx,
                                  void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_dgrad");
    if (rc) return rc;
    MRI3D_REQUIRE(dy && w && dx, MRI3D_EINVAL, "conv3d_dgrad: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (conv_backend(*g, MRI3D_PASS_DGRAD, false, 0, 0, ptr_align(dy, dx, workspace), ptr_align(dx))) {
    case ConvBackend::pointwise: return conv_pointwise_dgrad(*g, dy, (const float*)w, (const float*)bias, dx, s);
    case ConvBackend::mfma: return conv_mfma_dgrad(*g, dy, (const float*)w, (const float*)bias, dx, workspace, ws_bytes, s);
    default: return conv_generic_dgrad(*g, dy, (const float*)w, (const float*)bias, dx, workspace, ws_bytes, s);
    }
}

// ---- convolution over torch.cat((x, x2), dim=1) without the concatenation (unet.UNet decoder: cat((skip, upsampled)))
extern "C" int32_t mri3d_conv3d_cat_supported(const Mri3dConvGeom* g, int32_t split, int32_t second_ld, int32_t pass) {
    if (!g || split <= 0 || conv_check(g, "conv3d_cat_supported", split) != MRI3D_OK) return 0;
    return conv_mfma_cat_supported(*g, split, second_ld, pass) ? 1 : 0;
}

extern "C" int32_t mri3d_conv3d_fwd_cat_stats_blocks(const Mri3dConvGeom* g, int32_t split, int32_t second_ld) {
    if (!g || split <= 0 || conv_check(g, "conv3d_fwd_cat_stats_blocks", split) != MRI3D_OK) return 0;
    return conv_mfma_cat_supported(*g, split, second_ld, MRI3D_PASS_FWD) ? conv_mfma_fwd_stat_blocks(*g, split, second_ld) : 0;
}

extern "C" int mri3d_conv3d_fwd_cat(const Mri3dConvGeom* g, const void* x, const void* x2, int32_t split, int32_t x2_ld,
                                    const void* w, const void* bias, void* y, double* stat_partials, void* workspace,
                                    size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_fwd_cat", split);
    if (rc) return rc;
    MRI3D_REQUIRE(x && x2 && w && y, MRI3D_EINVAL, "conv3d_fwd_cat: null pointer");
    MRI3D_REQUIRE(conv_backend(*g, MRI3D_PASS_FWD, false, split, x2_ld, ptr_align(x, y, workspace, x2), 0) == ConvBackend::mfma,
                  MRI3D_ENOTSUP, "conv3d_fwd_cat: geometry / alignment not served (query mri3d_conv3d_cat_supported)");
    MRI3D_REQUIRE(stat_partials == nullptr || conv_mfma_fwd_stat_blocks(*g, split, x2_ld) > 0, MRI3D_ENOTSUP,
                  "conv3d_fwd_cat: no fused statistics for this geometry (query mri3d_conv3d_fwd_cat_stats_blocks)");
    return conv_mfma_fwd_cat(*g, x, x2, split, x2_ld, (const float*)w, (const float*)bias, y, stat_partials, workspace, ws_bytes,
                             static_cast<hipStream_t>(stream));
}

extern "C" int mri3d_conv3d_dgrad_cat(const Mri3dConvGeom* g, const void* dy, const void* w, void* dx, void* dx2, int32_t split,
                                      int32_t dx2_ld, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_dgrad_cat", split);
    if (rc) return rc;
    MRI3D_REQUIRE(dy && w && dx && dx2, MRI3D_EINVAL, "conv3d_dgrad_cat: null pointer");
    MRI3D_REQUIRE(conv_backend(*g, MRI3D_PASS_DGRAD, false, split, dx2_ld, ptr_align(dy, dx, workspace, dx2), 0) == ConvBackend::mfma,
                  MRI3D_ENOTSUP, "conv3d_dgrad_cat: geometry / alignment not served (query mri3d_conv3d_cat_supported)");
    return conv_mfma_dgrad_cat(*g, dy, (const float*)w, dx, dx2, split, dx2_ld, workspace, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int mri3d_conv3d_wgrad_cat(const Mri3dConvGeom* g, const void* x, const void* x2, int32_t split, int32_t x2_ld,
                                      const void* dy, void* dw, void* dbias, void* workspace, size_t ws_bytes,
                                      mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_wgrad_cat", split);
    if (rc) return rc;
    MRI3D_REQUIRE(x && x2 && dy && dw, MRI3D_EINVAL, "conv3d_wgrad_cat: null pointer");
    MRI3D_REQUIRE(conv_backend(*g, MRI3D_PASS_WGRAD, false, split, x2_ld, ptr_align(x, dy, workspace, x2), 0) == ConvBackend::mfma,
                  MRI3D_ENOTSUP, "conv3d_wgrad_cat: geometry / alignment not served (query mri3d_conv3d_cat_supported)");
    return conv_mfma_wgrad_cat(*g, x, x2, split, x2_ld, dy, (float*)dw, (float*)dbias, workspace, ws_bytes,
                               static_cast<hipStream_t>(stream));
}

// ---- the d-marching forward / data-gradient kernel by name (conv_march.hip).  The plain entry points above choose it themselves for
// the layers it is faster on; these take EVERY geometry it can compute, so that parity tests reach it with small volumes.
extern "C" int32_t mri3d_conv3d_march_supported(const Mri3dConvGeom* g, int32_t pass) {
    if (!g || (pass != MRI3D_PASS_FWD && pass != MRI3D_PASS_DGRAD) || conv_check(g, "conv3d_march_supported") != MRI3D_OK) return 0;
    return conv_march_needs(*g, pass == MRI3D_PASS_DGRAD, false, true).grid > 0 ? 1 : 0;
}

extern "C" int32_t mri3d_conv3d_march_stats_blocks(const Mri3dConvGeom* g) {
    if (!g || conv_check(g, "conv3d_march_stats_blocks") != MRI3D_OK) return 0;
    return conv_march_needs(*g, false, true, true).grid;
}

// the numbers those entry points launch by: the same conv_march_plan(.., force = true, ..), host only
extern "C" int32_t mri3d_conv3d_march_plan_query(const Mri3dConvGeom* g, int32_t pass, int32_t stats, Mri3dMarchPlanInfo* out) {
    MRI3D_REQUIRE(g && out, MRI3D_EINVAL, "conv3d_march_plan_query: null pointer");
    int rc = conv_check(g, "conv3d_march_plan_query");
    if (rc) return rc;
    MRI3D_REQUIRE(pass == MRI3D_PASS_FWD || pass == MRI3D_PASS_DGRAD, MRI3D_EINVAL, "conv3d_march_plan_query: pass %d", pass);
    MRI3D_REQUIRE(!stats || pass == MRI3D_PASS_FWD, MRI3D_EINVAL, "conv3d_march_plan_query: statistics outside the forward");
    Mri3dMarchPlanInfo info;
    MRI3D_REQUIRE(conv_march_plan_info(*g, pass == MRI3D_PASS_DGRAD, stats != 0, info), MRI3D_ENOTSUP,
                  "conv3d_march_plan_query: geometry not served (see mri3d_conv3d_march_supported; statistics: at most 8 output blocks)");
    *out = info;
    return MRI3D_OK;
}

extern "C" int mri3d_conv3d_fwd_march(const Mri3dConvGeom* g, const void* x, const void* x2, int32_t split, int32_t x2_ld,
                                      const void* w, const void* bias, void* y, double* stat_partials, void* workspace,
                                      size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_fwd_march", x2 ? split : -1);
    if (rc) return rc;
    MRI3D_REQUIRE(x && w && y, MRI3D_EINVAL, "conv3d_fwd_march: null pointer");
    MRI3D_REQUIRE(x2 == nullptr || (split > 0 && split < g->ci && x2_ld >= g->ci - split), MRI3D_EINVAL, "conv3d_fwd_march: bad split");
    return conv_march_run(*g, false, true, x, (const float*)w, (const float*)bias, y, workspace, ws_bytes,
                          static_cast<hipStream_t>(stream), stat_partials, ConvSplit{x2, split, x2_ld});
}

extern "C" int mri3d_conv3d_dgrad_march(const Mri3dConvGeom* g, const void* dy, const void* w, void* dx, void* dx2, int32_t split,
                                        int32_t dx2_ld, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_dgrad_march", dx2 ? split : -1);
    if (rc) return rc;
    MRI3D_REQUIRE(dy && w && dx, MRI3D_EINVAL, "conv3d_dgrad_march: null pointer");
    MRI3D_REQUIRE(dx2 == nullptr || (split > 0 && split < g->ci && dx2_ld >= g->ci - split), MRI3D_EINVAL, "conv3d_dgrad_march: bad split");
    return conv_march_run(*g, true, true, dy, (const float*)w, nullptr, dx, workspace, ws_bytes, static_cast<hipStream_t>(stream),
                          nullptr, ConvSplit{dx2, split, dx2_ld});
}

extern "C" int mri3d_conv3d_wgrad(const Mri3dConvGeom* g, const void* x, const void* dy, void* dw, void* dbias,
                                  void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv3d_wgrad");
    if (rc) return rc;
    MRI3D_REQUIRE(x && dy && dw, MRI3D_EINVAL, "conv3d_wgrad: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (conv_backend(*g, MRI3D_PASS_WGRAD, false, 0, 0, ptr_align(x, dy, workspace), ptr_align(x))) {
    case ConvBackend::pointwise: return conv_pointwise_wgrad(*g, x, dy, (float*)dw, (float*)dbias, workspace, ws_bytes, s);
    case ConvBackend::mfma: return conv_mfma_wgrad(*g, x, dy, (float*)dw, (float*)dbias, workspace, ws_bytes, s);
    default: return conv_generic_wgrad(*g, x, dy, (float*)dw, (float*)dbias, workspace, ws_bytes, s);
    }
}

// ---- the first layer with its activation folded in: Conv3d(1, 8|16, 3, padding=1) + PReLU / LeakyReLU / ReLU (conv_generic.hip)
static bool cin1_act_ok(const Mri3dConvGeom* g, int32_t a_ld, int32_t act, int32_t alpha_n, int32_t pass, int32_t align, const char* who) {
    if (!g || conv_check(g, who) != MRI3D_OK) return false;
    if (!conv_cin1_act_supported(*g, a_ld, act, alpha_n, pass, align)) return false;
    // the backward keeps the bits of the layer's plain weight gradient only where that runs conv_generic.hip's kernel
    return pass == MRI3D_PASS_FWD || conv_backend(*g, MRI3D_PASS_WGRAD, false, 0, 0, align, align) == ConvBackend::generic;
}

extern "C" int32_t mri3d_conv_cin1_act_supported(const Mri3dConvGeom* g, int32_t a_ld, int32_t act, int32_t alpha_n, int32_t pass,
                                                 int32_t align) {
    return cin1_act_ok(g, a_ld, act, alpha_n, pass, align, "conv_cin1_act_supported") ? 1 : 0;
}

extern "C" size_t mri3d_conv_cin1_act_workspace_bytes(const Mri3dConvGeom* g, int32_t pass) {
    if (!g || (pass != MRI3D_PASS_FWD && pass != MRI3D_PASS_WGRAD)) return 0;
    return conv_cin1_act_workspace_bytes(*g, pass);   // exactly what the pass asks for
}

extern "C" int mri3d_conv_cin1_act_route(const Mri3dConvGeom* g, int32_t a_ld, int32_t act, int32_t alpha_n, int32_t pass,
                                         int32_t align, char* name, size_t name_bytes) {
    int rc = conv_check(g, "conv_cin1_act_route");
    if (rc) return rc;
    MRI3D_REQUIRE(name != nullptr && name_bytes >= 32, MRI3D_EINVAL, "conv_cin1_act_route: name buffer of at least 32 bytes required");
    MRI3D_REQUIRE(pass == MRI3D_PASS_FWD || pass == MRI3D_PASS_WGRAD, MRI3D_EINVAL, "conv_cin1_act_route: pass %d", pass);
    if (!cin1_act_ok(g, a_ld, act, alpha_n, pass, align, "conv_cin1_act_route")) {
        snprintf(name, name_bytes, "none");
        return MRI3D_OK;
    }
    MRI3D_REQUIRE(conv_cin1_act_route_name(*g, a_ld, act, alpha_n, pass, align, name, name_bytes), MRI3D_EINVAL,
                  "conv_cin1_act_route: name buffer too small");
    return MRI3D_OK;
}

extern "C" int mri3d_conv_cin1_act_fwd(const Mri3dConvGeom* g, int32_t a_ld, int32_t act, int32_t alpha_n, float slope, const void* x,
                                       const void* w, const void* bias, const void* alpha, void* z, void* a, void* workspace,
                                       size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv_cin1_act_fwd");
    if (rc) return rc;
    MRI3D_REQUIRE(x && w && z && a, MRI3D_EINVAL, "conv_cin1_act_fwd: null pointer");
    MRI3D_REQUIRE(act != MRI3D_ACT_PRELU || alpha, MRI3D_EINVAL, "conv_cin1_act_fwd: PReLU needs alpha");
    MRI3D_REQUIRE(cin1_act_ok(g, a_ld, act, alpha_n, MRI3D_PASS_FWD, ptr_align(z, a, workspace), "conv_cin1_act_fwd"), MRI3D_ENOTSUP,
                  "conv_cin1_act_fwd: geometry / activation / alignment not served (query mri3d_conv_cin1_act_supported)");
    return conv_cin1_act_fwd(*g, a_ld, act, alpha_n, slope, (const float*)x, (const float*)w, (const float*)bias, (const float*)alpha,
                             (float*)z, (float*)a, workspace, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int mri3d_conv_cin1_act_bwd(const Mri3dConvGeom* g, int32_t da_ld, int32_t act, int32_t alpha_n, float slope, const void* x,
                                       const void* z, const void* da, const void* alpha, void* dw, void* dbias, void* dalpha,
                                       void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    int rc = conv_check(g, "conv_cin1_act_bwd");
    if (rc) return rc;
    MRI3D_REQUIRE(x && z && da && dw, MRI3D_EINVAL, "conv_cin1_act_bwd: null pointer");
    MRI3D_REQUIRE(act != MRI3D_ACT_PRELU || alpha, MRI3D_EINVAL, "conv_cin1_act_bwd: PReLU needs alpha");
    MRI3D_REQUIRE(cin1_act_ok(g, da_ld, act, alpha_n, MRI3D_PASS_WGRAD, ptr_align(z, da, workspace), "conv_cin1_act_bwd"), MRI3D_ENOTSUP,
                  "conv_cin1_act_bwd: geometry / activation / alignment not served (query mri3d_conv_cin1_act_supported)");
    return conv_cin1_act_bwd(*g, da_ld, act, alpha_n, slope, (const float*)x, (const float*)z, (const float*)da, (const float*)alpha,
                             (float*)dw, (float*)dbias, (float*)dalpha, workspace, ws_bytes, static_cast<hipStream_t>(stream));
}

// ---- which kernel would run (host only): the backend decision above, then the chosen file's own plan by name
extern "C" int mri3d_conv3d_route(const Mri3dConvGeom* g, int32_t pass, int32_t stats, int32_t bias, int32_t split, int32_t second_ld,
                                  int32_t align_x, int32_t align_y, char* name, size_t name_bytes) {
    int rc = conv_check(g, "conv3d_route", split > 0 ? split : -1);
    if (rc) return rc;
    MRI3D_REQUIRE(name != nullptr && name_bytes >= 32, MRI3D_EINVAL, "conv3d_route: name buffer of at least 32 bytes required");
    MRI3D_REQUIRE(pass == MRI3D_PASS_FWD || pass == MRI3D_PASS_DGRAD || pass == MRI3D_PASS_WGRAD, MRI3D_EINVAL, "conv3d_route: unknown pass %d", pass);
    MRI3D_REQUIRE(split >= 0 && (!stats || pass == MRI3D_PASS_FWD), MRI3D_EINVAL, "conv3d_route: negative split, or statistics outside the forward");
    const ConvSplit sp{nullptr, split, second_ld};
    // mri3d_conv3d_dgrad_cat takes no bias; the weight gradient has none to add
    const bool with_bias = bias != 0 && pass != MRI3D_PASS_WGRAD && !(split > 0 && pass == MRI3D_PASS_DGRAD);
    // the MFMA kernels move both tensors in 16-byte pieces; the pointwise kernels need only the x-side tensor aligned
    switch (conv_backend(*g, pass, stats != 0, split, second_ld, align_x < align_y ? align_x : align_y, align_x)) {
    case ConvBackend::none: snprintf(name, name_bytes, "none"); break;
    case ConvBackend::generic:
        MRI3D_REQUIRE(conv_generic_route_name(*g, pass, with_bias, align_x, align_y, name, name_bytes), MRI3D_EINVAL,
                      "conv3d_route: name buffer too small");
        break;
    case ConvBackend::pointwise:
        MRI3D_REQUIRE(conv_pointwise_route_name(*g, pass, with_bias, align_x, align_y, name, name_bytes), MRI3D_EINVAL,
                      "conv3d_route: name buffer too small");
        break;
    case ConvBackend::mfma:
        MRI3D_REQUIRE(conv_mfma_route_name(*g, pass, stats != 0, with_bias, sp, name, name_bytes), MRI3D_ENOTSUP,
                      "conv3d_route: the MFMA file names no kernel for a pass it supports");
        break;
    }
    return MRI3D_OK;
}

// ---- the numbers of that launch where the 3x3x3 MFMA files serve it (host only): the same backend decision, then their plan.
// `bias` is part of the call the query describes (as in mri3d_conv3d_route); no plan number of these kernels depends on it.
extern "C" int32_t mri3d_conv3d_mfma_plan_query(const Mri3dConvGeom* g, int32_t pass, int32_t stats, int32_t /* bias */, int32_t split,
                                                int32_t second_ld, int32_t align_x, int32_t align_y, Mri3dConvMfmaPlanInfo* out) {
    int rc = conv_check(g, "conv3d_mfma_plan_query", split > 0 ? split : -1);
    if (rc) return rc;
    MRI3D_REQUIRE(out != nullptr, MRI3D_EINVAL, "conv3d_mfma_plan_query: null pointer");
    MRI3D_REQUIRE(pass == MRI3D_PASS_FWD || pass == MRI3D_PASS_DGRAD || pass == MRI3D_PASS_WGRAD, MRI3D_EINVAL, "conv3d_mfma_plan_query: unknown pass %d", pass);
    MRI3D_REQUIRE(split >= 0 && (!stats || pass == MRI3D_PASS_FWD), MRI3D_EINVAL, "conv3d_mfma_plan_query: negative split, or statistics outside the forward");
    MRI3D_REQUIRE(conv_backend(*g, pass, stats != 0, split, second_ld, align_x < align_y ? align_x : align_y, align_x) == ConvBackend::mfma,
                  MRI3D_ENOTSUP, "conv3d_mfma_plan_query: the call is not served by the MFMA files (see mri3d_conv3d_route)");
    Mri3dConvMfmaPlanInfo info;
    MRI3D_REQUIRE(conv_mfma_plan_info(*g, pass, stats != 0, ConvSplit{nullptr, split, second_ld}, info), MRI3D_ENOTSUP,
                  "conv3d_mfma_plan_query: served by the marching kernel (see mri3d_conv3d_march_plan_query)");
    *out = info;
    return MRI3D_OK;
}
