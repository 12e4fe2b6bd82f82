// conv_backends.h — what the Conv3d kernel files offer each other and the dispatcher in api.hip.  Every file that defines or
// calls one of these includes this header, so a definition is always compiled against its declaration.
// Activations (x, y, dy, dx) are in the storage type g.dtype; weights, bias and their gradients are fp32.
#pragma once
#include "common.h"

namespace mri3d {

// second tensor of a split operand (conv over cat((x, x2), channels) / its data gradient written to two tensors): channels
// >= split live in `second` (pitch second_ld); split == 0: one tensor
struct ConvSplit {
    const void* second = nullptr;
    int split = 0, second_ld = 0;
};

// conv_generic.hip
size_t conv_generic_workspace_bytes(const Mri3dConvGeom& g, int pass);
int conv_generic_fwd(const Mri3dConvGeom& g, const void* x, const float* w, const float* bias, void* y, void* ws,
                     size_t ws_bytes, hipStream_t s);
int conv_generic_dgrad(const Mri3dConvGeom& g, const void* dy, const float* w, const float* bias, void* dx, void* ws,
                       size_t ws_bytes, hipStream_t s);
int conv_generic_wgrad(const Mri3dConvGeom& g, const void* x, const void* dy, float* dw, float* dbias, void* ws,
                       size_t ws_bytes, hipStream_t s);
// name of the kernel instantiation the pass launches (mri3d_conv3d_route; the vocabulary is in include/mri3d.h), written from the
// plan the launch reads.  ax / ay: ptr_align of the x-side tensor (x, dx) / of the y-side tensor (y, dy).  false: name too long.
bool conv_generic_route_name(const Mri3dConvGeom& g, int pass, bool bias, int ax, int ay, char* name, size_t name_bytes);
// the first layer with its activation folded in (mri3d_conv_cin1_act_*): one predicate, read by the queries and by the launches.
// pass: MRI3D_PASS_FWD, or MRI3D_PASS_WGRAD for the backward; a_ld: pitch of a / of da; align: ptr_align of z, a / da and workspace
bool conv_cin1_act_supported(const Mri3dConvGeom& g, int a_ld, int act, int alpha_n, int pass, int align);
size_t conv_cin1_act_workspace_bytes(const Mri3dConvGeom& g, int pass);
bool conv_cin1_act_route_name(const Mri3dConvGeom& g, int a_ld, int act, int alpha_n, int pass, int align, char* name, size_t name_bytes);
int conv_cin1_act_fwd(const Mri3dConvGeom& g, int a_ld, int act, int alpha_n, float slope, const float* x, const float* w,
                      const float* bias, const float* alpha, float* z, float* a, void* ws, size_t ws_bytes, hipStream_t s);
int conv_cin1_act_bwd(const Mri3dConvGeom& g, int da_ld, int act, int alpha_n, float slope, const float* x, const float* z,
                      const float* da, const float* alpha, float* dw, float* dbias, float* dalpha, void* ws, size_t ws_bytes,
                      hipStream_t s);

// conv_mfma.hip
bool conv_mfma_supported(const Mri3dConvGeom& g, int pass);
size_t conv_mfma_workspace_bytes(const Mri3dConvGeom& g, int pass);
int conv_mfma_fwd(const Mri3dConvGeom& g, const void* x, const float* w, const float* bias, void* y, void* ws,
                  size_t ws_bytes, hipStream_t s);
int conv_mfma_dgrad(const Mri3dConvGeom& g, const void* dy, const float* w, const float* bias, void* dx, void* ws,
                    size_t ws_bytes, hipStream_t s);
int conv_mfma_fwd_stat_blocks(const Mri3dConvGeom& g, int split = 0, int second_ld = 0);
bool conv_mfma_cat_supported(const Mri3dConvGeom& g, int split, int second_ld, int pass);
int conv_mfma_fwd_cat(const Mri3dConvGeom& g, const void* x, const void* x2, int split, int x2_ld, const float* w, const float* bias,
                      void* y, double* stat_part, void* ws, size_t ws_bytes, hipStream_t s);
int conv_mfma_dgrad_cat(const Mri3dConvGeom& g, const void* dy, const float* w, void* dx, void* dx2, int split, int dx2_ld, void* ws,
                        size_t ws_bytes, hipStream_t s);
int conv_mfma_fwd_stats(const Mri3dConvGeom& g, const void* x, const float* w, const float* bias, void* y, double* stat_part,
                        void* ws, size_t ws_bytes, hipStream_t s);
// name of the kernel instantiation the pass launches (mri3d_conv3d_route; the vocabulary is in include/mri3d.h), written from the
// same fwd_route answer (weight gradient: the same plan, below) the launch reads.  false: the pass is not served.
bool conv_mfma_route_name(const Mri3dConvGeom& g, int pass, bool stats, bool bias, const ConvSplit& sp, char* name, size_t name_bytes);
// the numbers of that launch (mri3d_conv3d_mfma_plan_query), filled from the same fwd_route answer / weight-gradient plan.  false,
// and `out` untouched: the pass is not served, or by the marching kernel (conv_march.hip has its own query)
bool conv_mfma_plan_info(const Mri3dConvGeom& g, int pass, bool stats, const ConvSplit& sp, Mri3dConvMfmaPlanInfo& out);

// Most and fewest units one persistent workgroup takes.  A HOST restatement, for the plan queries only, of the unit -> workgroup
// map the kernels compute from gridDim / blockIdx: conv_mfma_fwd2_kernel's (rows = 1) and tile_walk's of conv_mfma_wgrad.hip
// (P = gridDim.x, rows = gridDim.y * gridDim.z; the map of a row is that of row 0 rotated by P * row mod min(P, 8)).  Workgroups
// that share an XCD group (block id mod 8) take the units of the group's contiguous range round-robin.  (One __host__ __device__
// function called from both sides was tried: hipcc then allocates the scalar registers of every weight-gradient kernel's prologue
// differently, and those kernels are kept instruction for instruction.  tests/mfma_emu.py restates the walk once more and asserts
// that its longest sequence is the query's `chain`.)
struct WalkCounts { int max_tasks, min_tasks; };
inline WalkCounts xcd_walk_counts(int P, int rows, int units) {
    const int NX = P < 8 ? P : 8;
    WalkCounts c{0, units};
    for (int row = 0; row < rows && row < 8; ++row) {
        const int off = (int)(((int64_t)P * row) % NX);
        for (int bx = 0; bx < P; ++bx) {
            const int grp = (bx + off) % NX, p0 = (grp - off + NX) % NX;
            const int slot = (bx - p0) / NX, members = (P - p0 + NX - 1) / NX;
            const int r_lo = (int)(((int64_t)units * grp) / NX), r_hi = (int)(((int64_t)units * (grp + 1)) / NX);
            const int first = r_lo + slot;
            const int count = first < r_hi ? (r_hi - first + members - 1) / members : 0;
            c.max_tasks = count > c.max_tasks ? count : c.max_tasks;
            c.min_tasks = count < c.min_tasks ? count : c.min_tasks;
        }
    }
    return c;
}

// conv_mfma_wgrad.hip: the weight gradient of the 3x3x3 MFMA path.  The three queries are what conv_mfma.hip's queries over all
// passes answer with for MRI3D_PASS_WGRAD; all read the one plan the launch reads.
bool conv_mfma_wgrad_supported(const Mri3dConvGeom& g, int split = 0, int second_ld = 0);   // split > 0: ... with that split operand
size_t conv_mfma_wgrad_workspace_bytes(const Mri3dConvGeom& g);                             // 0: not served
bool conv_mfma_wgrad_route_name(const Mri3dConvGeom& g, char* name, size_t name_bytes);     // false: not served
bool conv_mfma_wgrad_plan_info(const Mri3dConvGeom& g, Mri3dConvMfmaPlanInfo& out);         // false, `out` untouched: not served
int conv_mfma_wgrad(const Mri3dConvGeom& g, const void* x, const void* dy, float* dw, float* dbias, void* ws,
                    size_t ws_bytes, hipStream_t s);
int conv_mfma_wgrad_cat(const Mri3dConvGeom& g, const void* x, const void* x2, int split, int x2_ld, const void* dy, float* dw,
                        float* dbias, void* ws, size_t ws_bytes, hipStream_t s);

// conv_march.hip: forward / data gradient marching along d.  `force` = the explicit entry points (every geometry the kernel can
// compute); otherwise the dispatcher's own choice of the layers where it is the faster kernel.
struct MarchNeeds { int grid; size_t wp_bytes; };   // workgroups (= statistics partials) and packed-weight image; grid 0: not taken
MarchNeeds conv_march_needs(const Mri3dConvGeom& g, bool dgrad, bool stats, bool force);
// the numbers the explicit entry points launch by (force = true), for mri3d_conv3d_march_plan_query; false: the plan refuses
bool conv_march_plan_info(const Mri3dConvGeom& g, bool dgrad, bool stats, Mri3dMarchPlanInfo& out);
int conv_march_run(const Mri3dConvGeom& g, bool dgrad, bool force, const void* in_v, const float* w, const float* bias, void* out_v,
                   void* ws, size_t ws_bytes, hipStream_t s, double* stat_part, const ConvSplit& sp);

// conv_pointwise.hip
bool conv_pointwise_supported(const Mri3dConvGeom& g, int pass);
size_t conv_pointwise_workspace_bytes(const Mri3dConvGeom& g, int pass);
int conv_pointwise_fwd(const Mri3dConvGeom& g, const void* x, const float* w, const float* bias, void* y, hipStream_t s);
int conv_pointwise_dgrad(const Mri3dConvGeom& g, const void* dy, const float* w, const float* bias, void* dx,
                         hipStream_t s);
int conv_pointwise_wgrad(const Mri3dConvGeom& g, const void* x, const void* dy, float* dw, float* dbias, void* ws,
                         size_t ws_bytes, hipStream_t s);
bool conv_pointwise_route_name(const Mri3dConvGeom& g, int pass, bool bias, int ax, int ay, char* name, size_t name_bytes);   // as above

}  // namespace mri3d
