/*
 * mri3d.h — C ABI of libmri3d_hip.so: the MI355X (gfx950) volumetric operator set behind the
 * 3-D U-Net / separable-conv encoder training path of kondratevakate/mri-epilepsy-diagnosis.
 *
 * The reference has no native layer: its hot path is `model(inputs)` / `loss.backward()` on torch.nn
 * modules (segmentation/routine.py:255-278, classification/routine.py:28-34).  Each entry point below
 * replaces one torch.nn operator that those calls reach; the reference call site is cited per function.
 *
 * Conventions
 *   - All tensors are device pointers into memory owned by the caller (PyTorch's caching allocator).
 *     The library never allocates, frees or synchronises; every kernel is enqueued on `stream`.
 *   - Activations are NDHWC ("channels-last-3d"): element (n,d,h,w,c) of a tensor with pitch `ld`
 *     lives at ((((n*D + d)*H + h)*W + w) * ld + c).  ld >= C lets an operator read or write a channel
 *     slice of a wider buffer (decoder concat buffers) without a copy.
 *   - Weights keep torch's parameter layout (Cout, Cin, kd, kh, kw) so state_dicts stay compatible;
 *     kernels repack into `workspace` on the fly.
 *   - dtype: storage type of the ACTIVATION tensors (x, y, dy, dx, logits ...): MRI3D_F32, or MRI3D_BF16 (bfloat16
 *     storage, fp32 arithmetic and accumulation).  Parameters, statistics, parameter gradients, losses are always fp32.
 *   - Return value: 0 = OK, negative = error; mri3d_last_error() gives a thread-local message.
 *   - Reductions are deterministic (no floating-point atomics).
 */
#ifndef MRI3D_H
#define MRI3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mri3d_stream_t; /* hipStream_t */

enum { MRI3D_OK = 0, MRI3D_EINVAL = -1, MRI3D_ENOTSUP = -2, MRI3D_ELAUNCH = -3, MRI3D_EWORKSPACE = -4 };
enum { MRI3D_F32 = 0, MRI3D_BF16 = 1 };
enum { MRI3D_ACT_NONE = 0, MRI3D_ACT_RELU = 1, MRI3D_ACT_LEAKY = 2, MRI3D_ACT_PRELU = 3 };
enum { MRI3D_UP_NEAREST = 0, MRI3D_UP_TRILINEAR = 1 };
enum { MRI3D_PASS_FWD = 0, MRI3D_PASS_DGRAD = 1, MRI3D_PASS_WGRAD = 2 };

int mri3d_version(void);
const char* mri3d_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Conv3d — replaces torch.nn.Conv3d as used by unet.UNet (segmentation/routine.py:346-356),
 * AE_model.DownBlock/UpBlock (classification/models/AE_model.py:9-26,74-91), cnn_model (cnn_model.py:14,49-148),
 * Modified3DUNet (segmentation/models/modified_3dunet.py:17-80).
 * ---------------------------------------------------------------------------------------------- */
typedef struct Mri3dConvGeom {
    int32_t n;                 /* batch */
    int32_t di, hi, wi, ci;    /* input  D,H,W,C */
    int32_t dout, ho, wo, co;  /* output D,H,W,C */
    int32_t kd, kh, kw;        /* kernel */
    int32_t sd, sh, sw;        /* stride */
    int32_t pd, ph, pw;        /* zero padding */
    int32_t dd, dh, dw;        /* dilation */
    int32_t x_ld, y_ld;        /* voxel pitch (elements) of the input / output buffers */
    int32_t dtype;             /* MRI3D_F32 */
} Mri3dConvGeom;

size_t mri3d_conv3d_workspace_bytes(const Mri3dConvGeom* g, int pass);

/* y = conv(x, w) + bias.  bias may be NULL. */
int mri3d_conv3d_fwd(const Mri3dConvGeom* g, const void* x, const void* w, const void* bias, void* y,
                     void* workspace, size_t ws_bytes, mri3d_stream_t stream);
/* dx = conv_transpose(dy, w) (+ bias, used when this is the forward of a ConvTranspose3d). dx has pitch x_ld. */
/* Forward convolution that ALSO accumulates the BatchNorm batch statistics of its output (torch.nn.BatchNorm3d in training
 * mode right after torch.nn.Conv3d: `unet.UNet`'s ConvolutionalBlock; segmentation/routine.py:258 -> unet forward): per output
 * channel sum(a) and sum(a^2) of the result a WITHOUT its bias over all N x D x H x W voxels, as float64 partials
 * stat_partials[blocks][co][2] (caller-owned, blocks = mri3d_conv3d_fwd_stats_blocks(g); 0 = geometry not supported, use
 * mri3d_conv3d_fwd + mri3d_norm_stats).  mri3d_norm_stats_from_partials turns them into mean / invstd (shift = bias). */
int32_t mri3d_conv3d_fwd_stats_blocks(const Mri3dConvGeom* g);
int mri3d_conv3d_fwd_stats(const Mri3dConvGeom* g, const void* x, const void* w, const void* bias, void* y,
                           double* stat_partials, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_conv3d_dgrad(const Mri3dConvGeom* g, const void* dy, const void* w, const void* bias, void* dx,
                       void* workspace, size_t ws_bytes, mri3d_stream_t stream);
/* dw (torch layout) = sum_v x (*) dy ; dbias = sum_v dy (dbias may be NULL). */
int mri3d_conv3d_wgrad(const Mri3dConvGeom* g, const void* x, const void* dy, void* dw, void* dbias,
                       void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* WHICH KERNEL the entry points above (split == 0) or the *_cat entry points below (split > 0, second_ld = pitch of the second
 * tensor) launch for this geometry.  Host only: no device is needed, nothing is launched; the entry points take their backend
 * from the same decision.  pass: MRI3D_PASS_*; stats != 0: the forward with fused statistics (mri3d_conv3d_fwd_stats, or a
 * non-NULL stat_partials of mri3d_conv3d_fwd_cat); bias != 0: a bias pointer is passed; align_x / align_y: the largest power of
 * two <= 16 that divides the base address of the x-side tensor (x, or dx in the data gradient; with a split: of both input
 * tensors) / of the y-side tensor (y, or dy in the gradients).  The workspace counts as 16-byte aligned.  The 3x3x3 MFMA kernels
 * need both tensors at 16, the pointwise kernels the x-side tensor at four elements; the generic kernels test each tensor on
 * its own.  name (at least 32 bytes) receives, as a C string whose first word is the kernel file:
 *   "none"       the entry point refuses (MRI3D_ENOTSUP): only with stats or a split
 *   "generic ..."    csrc/conv_generic.hip — the kernel, then the template arguments and branches that select code; a data gradient
 *                    that adds a bias (the forward of a ConvTranspose3d) ends in " bias":
 *     "generic c1c1"                        conv_c1c1_stencil_kernel / conv_c1c1_wgrad_kernel (1 -> 1 channel, 3x3x3)
 *     "generic c1taps nt{3,8}"              conv_c1_taps_kernel / conv_c1_taps_wgrad_kernel<NT> (1 -> 1 channel, <= 8 taps, fp32)
 *     "generic cin1 co{8,16}"               conv_cin1_fwd_kernel / conv_cin1_wgrad_kernel<T, CO> (first layer, one input channel)
 *     "generic taps tl{16,8,4,2} nt{3,4,6,8} cv{4,1}"   conv_fwd_taps_kernel / conv_dgrad_taps_kernel<T, TL, NT, CV> (<= 8 taps)
 *     "generic gather tl{..} vec{0,1}"      conv_fwd_generic_kernel / conv_dgrad_generic_kernel<T, TL, VEC4>
 *     "generic staps tl{..} nt{3,4,8}"      conv_dgrad_strided_taps_kernel<T, TL, NT> (strided data gradient, <= 8 valid taps)
 *     "generic strided tl{..} vec{0,1}"     conv_dgrad_strided_kernel<T, TL, VEC4>
 *     weight gradient: "generic co1 ci{1,4,8,16}" conv_wgrad_co1_kernel<T, CI>, "generic quads nt{4,6,8} civ{4,1}"
 *     conv_wgrad_quads_kernel<T, NT, CIV>, "generic small" conv_wgrad_small_kernel, "generic lds" conv_wgrad_generic_kernel
 *   "pointwise ..."  csrc/conv_pointwise.hip (1x1x1): "pointwise co{2,4}" pw_fwd_kernel<T, CO>, "pointwise co{2,4,8}[ bias]"
 *                    pw_dgrad_kernel<T, CO>, "pointwise co{2,4,8} vx{4,8} dv{0,1}" pw_wgrad_kernel<T, CO, VX, DYV>
 *   forward / data gradient on the 3x3x3 MFMA kernels — the kernel, then the template arguments that select code in it:
 *   "march[ stats][ bias]"                conv_march_kernel<T, STATS, BIAS>
 *   "direct nt{1,2,4} mode{0,1} split{0,1}"  conv_mfma_direct_kernel<T, NT, MODE, SPLIT> (mode 1: strided data gradient; split 1: the
 *                                         taps of a unit spread over the workgroup's waves — not a split operand)
 *   "tiled nt{1,2}[ stats]"               conv_mfma_fwd2_kernel<T, NT, STATS, false>
 *   "tiled_n8"                            conv_mfma_fwd2_kernel<T, 1, false, true> (exactly eight output channels)
 *   weight gradient: "cin1", "wgrad3", "wgrad4", "bf16", "bf16t", "wgrad6[ ci8][ co8]"  (conv_mfma_wgrad*_kernel)
 * Grids, tile counts and other run-time arguments are not part of a name.  The names are stable: the test suite pins its parity
 * cases to them. */
int mri3d_conv3d_route(const Mri3dConvGeom* g, int32_t pass, int32_t stats, int32_t bias, int32_t split, int32_t second_ld,
                       int32_t align_x, int32_t align_y, char* name, size_t name_bytes);

/* The first layer with its activation folded in — `unet.UNet`'s encoder.encoding_blocks[0].conv1: Conv3d(1, 8, 3, padding=1) +
 * PReLU with no normalisation in between.  Two kernels instead of conv, activation, activation backward and weight gradient:
 *   forward:  z = conv(x, w) + bias and a = act(z), both stored (the backward needs z's sign and, for dalpha, its value);
 *   backward: dW, db and dalpha from (x, z, da); the gradient of z is formed in registers and never stored.  There is no dx.
 * z, a, dW and db have the bits of mri3d_conv3d_fwd + mri3d_norm_act_fwd (identity norm) + mri3d_norm_act_bwd (training = 0) +
 * mri3d_conv3d_wgrad: same FMA chains, same summation orders.  dalpha is the same float64 sum of exact products over another
 * partition of the voxels, rounded to fp32 per channel as there.
 * g: the convolution, g->y_ld = the pitch of z; a_ld: the pitch of a (forward) / of da (backward); act: MRI3D_ACT_RELU, _LEAKY
 * (slope) or _PRELU (alpha: alpha_n = 1 or g->co slopes); pass: MRI3D_PASS_FWD, or MRI3D_PASS_WGRAD for the backward; align: the
 * largest power of two <= 16 dividing the addresses of z and a / da (x is read one element at a time).
 * mri3d_conv_cin1_act_supported = 1 (host only) for one input channel, 8 or 16 output channels, 3x3x3, stride 1, padding 1,
 * dilation 1, fp32, pitches of z and a / da multiples of 4, align = 16, and in the backward eight output channels (with sixteen
 * the layer's plain weight gradient is an MFMA kernel with another summation order: keep mri3d_norm_act_bwd + mri3d_conv3d_wgrad).
 * bf16 is declined.  The entry points return MRI3D_ENOTSUP exactly where it answers 0.
 * mri3d_conv_cin1_act_route: "cin1 act fwd co{8,16}" conv_cin1_act_fwd_kernel<CO>, "cin1 act bwd co8" conv_cin1_act_bwd_kernel<8>
 * (+ wgrad_reduce_kernel, and cin1_act_dalpha_kernel where dalpha is wanted), "none" where the predicate declines.
 * dbias, dalpha may be NULL (dalpha is written for PReLU only).  No allocation, no synchronisation. */
int32_t mri3d_conv_cin1_act_supported(const Mri3dConvGeom* g, int32_t a_ld, int32_t act, int32_t alpha_n, int32_t pass, int32_t align);
size_t mri3d_conv_cin1_act_workspace_bytes(const Mri3dConvGeom* g, int32_t pass);
int mri3d_conv_cin1_act_route(const Mri3dConvGeom* g, int32_t a_ld, int32_t act, int32_t alpha_n, int32_t pass, int32_t align,
                              char* name, size_t name_bytes);
int mri3d_conv_cin1_act_fwd(const Mri3dConvGeom* g, int32_t a_ld, int32_t act, int32_t alpha_n, float slope, const void* x,
                            const void* w, const void* bias, const void* alpha, void* z, void* a, void* workspace, size_t ws_bytes,
                            mri3d_stream_t stream);
int mri3d_conv_cin1_act_bwd(const Mri3dConvGeom* g, int32_t da_ld, int32_t act, int32_t alpha_n, float slope, const void* x,
                            const void* z, const void* da, const void* alpha, void* dw, void* dbias, void* dalpha, void* workspace,
                            size_t ws_bytes, mri3d_stream_t stream);

/* Convolution over torch.cat((x, x2), dim=1) WITHOUT the concatenation — `unet.UNet`'s decoder, x = cat((skip, upsampled))
 * in front of its first ConvolutionalBlock (segmentation/routine.py:346-356 -> unet DecodingBlock.forward).  g describes the
 * concatenated convolution (g->ci = all input channels, g->x_ld = voxel pitch of x); channels [0, split) are read from x,
 * channels [split, ci) from x2 (voxel pitch x2_ld).  The data gradient is written as two dense tensors dx (pitch g->x_ld) and
 * dx2 (pitch dx2_ld); the weight gradient reads both.  Workspace sizes are those of the plain passes
 * (mri3d_conv3d_workspace_bytes).  stat_partials (may be NULL): as in mri3d_conv3d_fwd_stats.
 * mri3d_conv3d_cat_supported(g, split, second_ld, pass) = 1 when the pass is served (3x3x3 / stride 1 / pad 1 on the tiled MFMA
 * kernels, split a multiple of 16, every pointer 16-byte aligned); otherwise concatenate (mri3d_copy_channels) and call the plain
 * entry points.
 * mri3d_conv3d_fwd_cat_stats_blocks(g, split, second_ld) = the number of blocks of stat_partials mri3d_conv3d_fwd_cat writes for
 * exactly this geometry, split and second-tensor pitch: the required size of stat_partials is [blocks][g->co][2] doubles.  It may
 * differ from mri3d_conv3d_fwd_stats_blocks of the same geometry (the second tensor's pitch takes part in the choice of kernel);
 * 0 = no fused statistics (pass stat_partials = NULL). */
int32_t mri3d_conv3d_cat_supported(const Mri3dConvGeom* g, int32_t split, int32_t second_ld, int32_t pass);
int32_t mri3d_conv3d_fwd_cat_stats_blocks(const Mri3dConvGeom* g, int32_t split, int32_t second_ld);
int mri3d_conv3d_fwd_cat(const Mri3dConvGeom* g, const void* x, const void* x2, int32_t split, int32_t x2_ld, const void* w,
                         const void* bias, void* y, double* stat_partials, void* workspace, size_t ws_bytes,
                         mri3d_stream_t stream);
int mri3d_conv3d_dgrad_cat(const Mri3dConvGeom* g, const void* dy, const void* w, void* dx, void* dx2, int32_t split,
                           int32_t dx2_ld, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_conv3d_wgrad_cat(const Mri3dConvGeom* g, const void* x, const void* x2, int32_t split, int32_t x2_ld, const void* dy,
                           void* dw, void* dbias, void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* The d-marching forward / data-gradient kernel BY NAME (csrc/conv_march.hip; nn.Conv3d 3x3x3 / stride 1 / pad 1 of `unet.UNet`,
 * segmentation/routine.py:346-356).  mri3d_conv3d_fwd / _dgrad / _fwd_stats / _fwd_cat / _dgrad_cat choose it themselves for the
 * layers it is faster on; these entry points take every geometry it can compute (mri3d_conv3d_march_supported(g, pass) = 1), so a
 * caller — the parity tests — reaches it with any volume.  x2 / dx2 may be NULL (one tensor; split, *_ld ignored); stat_partials may
 * be NULL, else [mri3d_conv3d_march_stats_blocks(g)][co][2].  Workspace: mri3d_conv3d_workspace_bytes of the pass. */
int32_t mri3d_conv3d_march_supported(const Mri3dConvGeom* g, int32_t pass);
int32_t mri3d_conv3d_march_stats_blocks(const Mri3dConvGeom* g);
int mri3d_conv3d_fwd_march(const Mri3dConvGeom* g, const void* x, const void* x2, int32_t split, int32_t x2_ld, const void* w,
                           const void* bias, void* y, double* stat_partials, void* workspace, size_t ws_bytes,
                           mri3d_stream_t stream);
int mri3d_conv3d_dgrad_march(const Mri3dConvGeom* g, const void* dy, const void* w, void* dx, void* dx2, int32_t split,
                             int32_t dx2_ld, void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* THE NUMBERS OF THE LAUNCH PLAN of the two entry points above: the same plan function they launch by, host only (no device is
 * needed, nothing is launched).  Kc = input channels of the pass (forward ci, data gradient co), Nc = its output channels; the
 * pitches of g are those the entry point gets (a split operand is queried as ONE tensor, x_ld >= ci, as the two queries above).
 *   chunks        32-byte input-channel chunks = ceil(Kc / 8) fp32, ceil(Kc / 16) bf16 (at most 4)
 *   blocks        16-channel output blocks = ceil(Nc / 16); one workgroup computes one block of one column segment
 *   wgh, wgw      the 8 waves of a workgroup own wgh x wgw columns of 8 rows x 16 voxels (h x w)
 *   gch, gcw      workgroup-columns along h and w
 *   nseg, seglen  d segments and their length in planes (the last one may be shorter)
 *   nbuf          LDS plane buffers per wave: 3 with one chunk (the DMA runs two items ahead), else 2 (one item ahead)
 *   grid          workgroups = blocks x gcw x gch x nseg x n = the statistics blocks (mri3d_conv3d_march_stats_blocks)
 *   whole_chunks  1 where Kc fills its last chunk (a single tensor of whole chunks takes the constant-offset DMA path)
 *   dispatcher    1 where mri3d_conv3d_fwd / _dgrad / _fwd_stats would choose this kernel for the layer themselves
 *   smem_bytes    dynamic LDS of the launch;  wp_bytes  packed-weight image in the workspace
 * pass: MRI3D_PASS_FWD / _DGRAD; stats != 0: the forward with fused statistics (with the data gradient: MRI3D_EINVAL).  Returns
 * MRI3D_ENOTSUP exactly where mri3d_conv3d_march_supported(g, pass) = 0 for a valid geometry, and with stats for more than 8 output
 * blocks (mri3d_conv3d_march_stats_blocks = 0); MRI3D_EINVAL for NULL, an unknown pass or an inconsistent geometry. */
typedef struct Mri3dMarchPlanInfo {
    int32_t chunks, blocks, wgh, wgw, gch, gcw, nseg, seglen, nbuf, grid, whole_chunks, dispatcher;
    int64_t smem_bytes, wp_bytes;
} Mri3dMarchPlanInfo;
int32_t mri3d_conv3d_march_plan_query(const Mri3dConvGeom* g, int32_t pass, int32_t stats, Mri3dMarchPlanInfo* out);

/* THE NUMBERS OF THE LAUNCH PLAN of the 3x3x3 MFMA kernels of csrc/conv_mfma.hip and csrc/conv_mfma_wgrad.hip, for the call
 * mri3d_conv3d_route names with the same arguments (mri3d_conv3d_fwd / _fwd_stats / _dgrad / _wgrad, split > 0: the *_cat entry
 * points).  Host only: no device is needed, nothing is launched, nothing is allocated; the numbers are read from the plan objects
 * the launch reads.  Returns MRI3D_ENOTSUP, and leaves *out alone, exactly where mri3d_conv3d_route names a kernel of another file
 * ("generic ...", "pointwise ...", "march ...") or "none"; MRI3D_EINVAL as mri3d_conv3d_route, and for a NULL out.
 * Kc = input channels of the pass (forward ci, data gradient co), Nc = its output channels.
 *   kernel        MRI3D_MFMA_*: the first word(s) of the route name
 *   ck, chunks, partial_chunk   channels per K chunk, chunks = ceil(Kc / ck), 1 where the last chunk is not full (weight gradient:
 *                 ck = input channels per ci-tile, chunks = cit)
 *   nt, ntt, gy   tiled / direct: 16-channel N-tiles per wave, N-tiles = ceil(Nc / 16), N-blocks = ntt / nt
 *   tile_d, tile_h, tile_w      output tile in voxels (direct: 1 x 1 x 16, an M-tile of 16 voxels; bf16t: tile_d = segl)
 *   tiles_d, tiles_h, tiles_w, ntiles   tiles per axis, and in all samples (direct: ntiles = M-tiles; bf16t: tasks)
 *   units         work units the grid shares: tiled ntiles * gy, direct M-tiles * gy, weight gradient ntiles
 *   grid          workgroups of the launch (weight gradient: p * cit * cob)
 *   mode, split, wbn   direct: strided data gradient, a unit's taps spread over the workgroup's four waves, 16-voxel blocks per row
 *                 residue (mode 1)
 *   cit, cob, tg, p, ci8, co8, segl   weight gradient: ci-tiles, 16-channel output blocks, tap groups (accumulators without the
 *                 one of dbias), workgroups per (ci-tile, output block), the eight-channel forms of wgrad6, planes per bf16t task
 *   max_tasks, min_tasks   most / fewest units (tiled, weight gradient) one persistent workgroup takes (direct: 1, 1)
 *   chain         weight gradient: the longest fp32 accumulation chain of one accumulator element of one wave, in products:
 *                 max_tasks * tile_d * tile_h * tile_w / 4 (a wave owns a quarter of every tile's voxels)
 *   stats_blocks  statistics partials the forward writes (= grid with stats, else 0)
 *   workspace_bytes   what the launch requires of the workspace: packed-weight image / weight-gradient partials */
enum { MRI3D_MFMA_TILED = 1, MRI3D_MFMA_TILED_N8 = 2, MRI3D_MFMA_DIRECT = 3, MRI3D_MFMA_CIN1 = 4, MRI3D_MFMA_WGRAD3 = 5,
       MRI3D_MFMA_WGRAD4 = 6, MRI3D_MFMA_BF16 = 7, MRI3D_MFMA_BF16T = 8, MRI3D_MFMA_WGRAD6 = 9 };
typedef struct Mri3dConvMfmaPlanInfo {
    int32_t kernel, ck, chunks, partial_chunk, nt, ntt, gy, tile_d, tile_h, tile_w, tiles_d, tiles_h, tiles_w, ntiles, units, grid,
        mode, split, wbn, cit, cob, tg, p, ci8, co8, segl, max_tasks, min_tasks, chain, stats_blocks;
    int64_t workspace_bytes;
} Mri3dConvMfmaPlanInfo;
int32_t mri3d_conv3d_mfma_plan_query(const Mri3dConvGeom* g, int32_t pass, int32_t stats, int32_t bias, int32_t split, int32_t second_ld,
                                     int32_t align_x, int32_t align_y, Mri3dConvMfmaPlanInfo* out);

/* Conv3d over a nearest-neighbour upsampled input that is never formed (csrc/upconv.hip):
 *     y = conv3d(upsample_nearest(x, scale_factor = scale), w, bias, stride 1, padding g->p*)
 * replaces nn.Upsample(scale_factor=4, mode='nearest') followed by the block's first nn.Conv3d in UpBlock
 * (classification/models/AE_model.py:110-120 with up='upsample'; the last block: Conv3d(8, 1, (3,1,1)) at 160x192x160).
 * g describes the convolution on the VIRTUAL fine input: di, hi, wi = scale x the extents of the coarse tensor x
 * (n, di/scale, hi/scale, wi/scale, ci) whose voxel pitch is x_ld; y / dy have pitch y_ld.  dgrad writes the gradient of the
 * COARSE tensor (each coarse voxel = the sum over its scale^3 fine voxels, fixed summation order).  Served geometries:
 * mri3d_upconv3d_supported(g, scale) = 1 (scale 2 or 4, stride 1, dilation 1, <= 8 taps, the (ci, co, taps) instances listed in
 * upconv.hip); everything else returns MRI3D_ENOTSUP and the caller keeps the two separate operators.  wgrad workspace:
 * mri3d_upconv3d_workspace_bytes. */
int32_t mri3d_upconv3d_supported(const Mri3dConvGeom* g, int32_t scale);
size_t mri3d_upconv3d_workspace_bytes(const Mri3dConvGeom* g, int32_t scale);
int mri3d_upconv3d_fwd(const Mri3dConvGeom* g, int32_t scale, const void* x, const float* w, const float* bias, void* y,
                       mri3d_stream_t stream);
int mri3d_upconv3d_dgrad(const Mri3dConvGeom* g, int32_t scale, const void* dy, const float* w, void* dx, mri3d_stream_t stream);
int mri3d_upconv3d_wgrad(const Mri3dConvGeom* g, int32_t scale, const void* x, const void* dy, float* dw, float* dbias,
                         void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* The first two convolutions of the autoencoder's first DownBlock (classification/models/AE_model.py:45-53, shipped kwargs conv_k=6,
 * conv_s=2, conv_pad=2): first = Conv3d(1, 8, (6,1,1), stride (s,1,1), padding (p,0,0)) on the input volume, second =
 * Conv3d(8, 8, (1,k,1), stride (1,s,1), padding (0,p,0)) on its output (csrc/sepconv.hip).  mri3d_convpair_wgrad_first computes the
 * FIRST convolution's weight / bias gradient from the gradient dy2 of the SECOND convolution's output (pitch second->y_ld), the
 * second convolution's weight w2 (torch layout) and the input x (pitch first->x_ld): what mri3d_conv3d_dgrad(second) followed by
 * mri3d_conv3d_wgrad(first) compute, without the intermediate gradient tensor.  dw1: (8, 1, 6, 1, 1); dbias1: (8) or NULL.
 * Served pairs: mri3d_convpair_supported = 1 (second's input must be first's output); else MRI3D_ENOTSUP. */
int32_t mri3d_convpair_supported(const Mri3dConvGeom* first, const Mri3dConvGeom* second);
size_t mri3d_convpair_workspace_bytes(const Mri3dConvGeom* first, const Mri3dConvGeom* second);
int mri3d_convpair_wgrad_first(const Mri3dConvGeom* first, const Mri3dConvGeom* second, const void* x, const void* dy2, const float* w2,
                               float* dw1, float* dbias1, void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* THE NUMBERS OF THE LAUNCH PLAN of the two fused operators above: same geometry arguments and checks as the entry points, the
 * same plan function the entry points launch by, host only (no device is needed, nothing is launched).  Fields a pass does not
 * use are 0.
 *   hch       upconv forward / weight gradient: rows of H per slab = min(ho, 1024 / wo), at least 1 (hch < ho: a slab is a part
 *             of an (n, od) plane, the last part may be ragged)
 *   grid      workgroups launched: min(slabs, 4096) forward, min(slabs, 1024) weight gradient, min(rows, 8192) data gradient,
 *             min(ceil(rows / 4), 1024) pair; the kernels loop where there are more slabs / rows than that
 *   gtrips    trips of that loop a workgroup makes at most: ceil(slabs / grid), ceil(rows / grid), pair: ceil(rows / (4 grid))
 *   trips     upconv forward / weight gradient: trips of the 256-lane loop over the hch x wo voxels of a full slab
 *   per       upconv data gradient: coarse voxels of a row per pass = 256 / scale^3
 *   passes    upconv data gradient: passes per coarse row = ceil(wc / per); lanes past wc in the last pass are masked
 *   chunks    pair: 64-voxel chunks of W a wave walks per row
 *   slabs     upconv forward / weight gradient: n x dout x ceil(ho / hch)
 *   rows      upconv data gradient: coarse rows n x dc x hc; pair: rows (n, d1, h) of the first convolution's output
 * pass: MRI3D_PASS_FWD / _DGRAD / _WGRAD (anything else: MRI3D_EINVAL).  Both return MRI3D_OK or the error the entry point gives
 * for the geometry (MRI3D_ENOTSUP where mri3d_upconv3d_supported / mri3d_convpair_supported is 0); g / first / second and out
 * must not be NULL. */
typedef struct Mri3dFusedConvPlanInfo {
    int32_t hch, grid, gtrips, trips, per, passes, chunks;
    int64_t slabs, rows;
} Mri3dFusedConvPlanInfo;
int32_t mri3d_upconv3d_plan_query(const Mri3dConvGeom* g, int32_t scale, int32_t pass, Mri3dFusedConvPlanInfo* out);
int32_t mri3d_convpair_plan_query(const Mri3dConvGeom* first, const Mri3dConvGeom* second, Mri3dFusedConvPlanInfo* out);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm3d / InstanceNorm3d fused with the following activation — replaces
 * nn.BatchNorm3d + nn.PReLU (unet.UNet ConvolutionalBlock), nn.BatchNorm3d + LeakyReLU/ReLU
 * (AE_model.py:30-36, cnn_model.py), nn.InstanceNorm3d + LeakyReLU (modified_3dunet.py:20-94).
 * groups = 1 (batch norm: statistics over n*vox per channel) or n (instance norm: per (n,c)); GroupNorm
 * (nn.GroupNorm(4, C) of segmentation/models/unet3d.py:12) = instance mode with group_c = C/4 channels pooled.
 * ---------------------------------------------------------------------------------------------- */
typedef struct Mri3dNormGeom {
    int32_t n;        /* batch */
    int64_t vox;      /* D*H*W */
    int32_t c;        /* channels */
    int32_t x_ld;     /* voxel pitch of x / dx */
    int32_t y_ld;     /* voxel pitch of y / dy */
    int32_t instance; /* 0 = batch statistics, 1 = per-instance statistics */
    int32_t act;      /* MRI3D_ACT_* applied after the affine transform */
    int32_t alpha_n;  /* PReLU: number of alpha parameters (1 or c) */
    float slope;      /* LeakyReLU negative slope */
    float eps;
    int32_t group_c;  /* GroupNorm: channels per group (needs instance = 1; statistics per (n, group)); 0 otherwise */
    int32_t dtype;
} Mri3dNormGeom;

size_t mri3d_norm_workspace_bytes(const Mri3dNormGeom* g);

/* THE LAUNCH PLAN mri3d_norm_stats (MRI3D_NORM_PASS_STATS), mri3d_norm_act_fwd (_FWD) and mri3d_norm_act_bwd (_BWD) use for this
 * geometry.  Host only: no device is needed, nothing is launched; the entry points take their plan from the same decision.
 * align: the largest power of two <= 16 that divides the base address of every tensor the pass touches (x; x and y; x, dy and
 * dx).  A 256-thread block is VT voxel rows x CL channel lanes of vec channels each (vec 8: bf16 forward only; CL * VT <= 256,
 * the remaining threads idle); the grid is nblk blocks per group x cy channel chunks x groups, each group gvox voxels.  The
 * statistics pass ignores y_ld.  Returns MRI3D_OK or the error the entry point gives for the geometry. */
enum { MRI3D_NORM_PASS_STATS = 0, MRI3D_NORM_PASS_FWD = 1, MRI3D_NORM_PASS_BWD = 2 };
typedef struct Mri3dNormPlanInfo {
    int32_t vec, CL, VT, cy, nblk, groups;
    int64_t gvox;
} Mri3dNormPlanInfo;
int32_t mri3d_norm_plan_query(const Mri3dNormGeom* g, int32_t pass, int32_t align, Mri3dNormPlanInfo* out);

/* mean/invstd: [groups*c] floats where groups = instance ? n : 1.
 * If running_mean/running_var are non-NULL (batch mode only) they are updated in place:
 *   running = (1-momentum)*running + momentum*stat, with the unbiased variance, as torch does. */
int mri3d_norm_stats(const Mri3dNormGeom* g, const void* x, float* mean, float* invstd,
                     float* running_mean, float* running_var, float momentum,
                     void* workspace, size_t ws_bytes, mri3d_stream_t stream);
/* mean / invstd (and the running-statistics update of mri3d_norm_stats) from float64 partial sums
 * partials[nblk][c][2] = (sum(x - shift[c]), sum((x - shift[c])^2)) over disjoint parts of the N x vox voxels (batch statistics
 * only).  shift may be NULL (zero). */
int mri3d_norm_stats_from_partials(const Mri3dNormGeom* g, const double* partials, int32_t nblk, const float* shift,
                                   float* mean, float* invstd, float* running_mean, float* running_var, float momentum,
                                   mri3d_stream_t stream);
/* y = act(gamma * (x - mean) * invstd + beta).  gamma/beta may be NULL (affine=False); alpha is the
 * PReLU parameter (device pointer) when act == MRI3D_ACT_PRELU.  mean/invstd NULL => identity norm. */
int mri3d_norm_act_fwd(const Mri3dNormGeom* g, const void* x, const float* mean, const float* invstd,
                       const float* gamma, const float* beta, const float* alpha, void* y,
                       mri3d_stream_t stream);
/* Backward of norm_act_fwd.  training != 0: statistics were computed from x (batch/instance mode);
 * training == 0: mean/invstd are constants (eval-mode BatchNorm, activation-only layers): dx does not depend on the sums then, and
 * one pass over (x, dy) writes dx and the partial sums.  dgamma/dbeta/dalpha may be NULL. */
int mri3d_norm_act_bwd(const Mri3dNormGeom* g, int training, const void* x, const void* dy,
                       const float* mean, const float* invstd, const float* gamma, const float* beta,
                       const float* alpha, void* dx, float* dgamma, float* dbeta, float* dalpha,
                       void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* norm_act followed by a narrow 1x1x1 convolution, as ONE operator: out = W . act(norm(x)) + bias — `unet.UNet`'s classifier
 * (Conv3d(2*c0, out_classes, 1), segmentation/routine.py:346-356) right after the last conv -> BatchNorm3d -> PReLU block.  The
 * activation and its gradient, full-resolution tensors that exist only to cross a kernel boundary, are never stored.
 * g describes the norm_act part with batch (training != 0), running or no statistics (mean = invstd = NULL); g->x_ld = voxel pitch
 * of x / dx, g->y_ld = voxel pitch of out / dout; w is the head's weight (co, c), bias (co) or NULL.  fp32 results of _fwd are
 * bit-identical to mri3d_norm_act_fwd + mri3d_conv3d_fwd; in bf16 the activation is rounded to bf16 before the dot product, as
 * the stored tensor would be.
 * mri3d_norm_act_pw_supported(g, co) = 1 (host only): batch-type statistics (not instance / group), c % 4 == 0 with c/4 a power
 * of two <= 16, 1 <= co <= 4, x_ld % 4 == 0; x and dx must be aligned to 4 elements.  Otherwise 0: keep the two operators.
 * _bwd: dx (pitch x_ld), dgamma, dbeta, dalpha, dw (co, c), dbias (co); every one of them may be NULL.  With training == 0 and
 * a parameter gradient wanted, dx and all sums come from one pass over (x, dout).  Workspace: mri3d_norm_act_pw_workspace_bytes
 * (host only; 0 when not supported), 8-byte aligned. */
int32_t mri3d_norm_act_pw_supported(const Mri3dNormGeom* g, int32_t co);
size_t mri3d_norm_act_pw_workspace_bytes(const Mri3dNormGeom* g, int32_t co);
int mri3d_norm_act_pw_fwd(const Mri3dNormGeom* g, int32_t co, const void* x, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, const float* alpha, const float* w, const float* bias,
                          void* out, mri3d_stream_t stream);
int mri3d_norm_act_pw_bwd(const Mri3dNormGeom* g, int32_t co, int training, const void* x, const void* dout,
                          const float* mean, const float* invstd, const float* gamma, const float* beta, const float* alpha,
                          const float* w, void* dx, float* dgamma, float* dbeta, float* dalpha, float* dw, float* dbias,
                          void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MaxPool3d — nn.MaxPool3d(2) in unet.UNet / AE_model.py:27 / cnn_model.py:115-148, (4,2) in cnn_model.py:221,232.
 * idx: one byte per output element = window-local offset (kd,kh,kw raster) of the arg-max.
 * ---------------------------------------------------------------------------------------------- */
typedef struct Mri3dPoolGeom {
    int32_t n, di, hi, wi, dout, ho, wo, c;
    int32_t kd, kh, kw, sd, sh, sw, pd, ph, pw;
    int32_t x_ld, y_ld;
    int32_t dtype;
} Mri3dPoolGeom;
int mri3d_maxpool3d_fwd(const Mri3dPoolGeom* g, const void* x, void* y, uint8_t* idx, mri3d_stream_t stream);
int mri3d_maxpool3d_bwd(const Mri3dPoolGeom* g, const void* dy, const uint8_t* idx, void* dx, mri3d_stream_t stream);
/* dx = maxpool3d_bwd(dy) + addend: `addend` (same storage type, voxel pitch addend_ld >= c) is the other gradient of the pool's
 * input when that tensor also feeds a skip connection (unet.UNet encoder: `skip = x; x = pool(x)`), which autograd would
 * otherwise sum in a separate full-resolution pass. */
int mri3d_maxpool3d_bwd_add(const Mri3dPoolGeom* g, const void* dy, const uint8_t* idx, const void* addend,
                            int32_t addend_ld, void* dx, mri3d_stream_t stream);
/* WHICH KERNEL mri3d_maxpool3d_fwd (pass = MRI3D_PASS_FWD), mri3d_maxpool3d_bwd (MRI3D_PASS_DGRAD, addend_ld = 0) or
 * mri3d_maxpool3d_bwd_add (MRI3D_PASS_DGRAD, addend_ld = the addend's pitch) launches for this geometry.  Host only: no device is
 * needed, nothing is launched; it runs the entry point's checks and reads the launch plan the entry point launches by.
 * align_tensors: the largest power of two <= 16 that divides the base address of every tensor of the pass (x and y; dy, dx and the
 * addend); align_idx: the same for the index bytes.  name (at least 40 bytes) receives the kernel template of csrc/resample.hip
 * without its "_kernel" and its template arguments as the plan chose them, T = f32 | bf16:
 *   "maxpool2_fwd<T,{4,8}>"       MaxPool3d(2) on even extents, lanes along input lines; VEC = 8: bf16 only, here and below
 *   "maxpool_fwd<T,{1,4,8}>"      every other pool, and a MaxPool3d(2) whose channels, pitches or alignments allow no vector
 *   "maxpool_bwd<T,{1,4,8}>"      followed by "+add" with an addend
 * Grids and other run-time arguments are not part of a name.  The names are stable: the test suite pins its parity cases to them. */
int mri3d_maxpool3d_route(const Mri3dPoolGeom* g, int32_t pass, int32_t addend_ld, int32_t align_tensors, int32_t align_idx,
                          char* name, size_t name_bytes);

/* norm_act followed by MaxPool3d(2) with the activation kept as the skip tensor, as ONE operator — the tail of an encoder level
 * of `unet.UNet` (conv -> BatchNorm3d -> PReLU -> skip, MaxPool3d(2)).  _fwd reads x once and writes skip = act(norm(x)), pooled =
 * maxpool(skip) and the pool's index bytes; _bwd takes the two gradients that meet at the activation, da = dskip + scatter(dpool),
 * without storing da.  Results are those of mri3d_norm_act_fwd + mri3d_maxpool3d_fwd and of mri3d_maxpool3d_bwd_add +
 * mri3d_norm_act_bwd, bit for bit in fp32 (same expressions, same per-block partial sums); in bf16 the activation and da are
 * rounded to bf16 where the two operators would have stored them.
 * g describes the norm_act part: batch (training != 0), running or no statistics (mean = invstd = NULL); g->x_ld = voxel pitch of
 * x / dx, g->y_ld = voxel pitch of skip / dskip.  pg describes the pool: pg->x_ld = g->y_ld (its input is skip), pg->y_ld = voxel
 * pitch of pooled / dpool; n, c, dtype and di*hi*wi = g->vox agree with g.
 * mri3d_norm_act_pool_supported(g, pg) = 1 (host only): kernel 2, stride 2, padding 0 on even extents; batch-type statistics (not
 * instance / group); c % 4 == 0 with c/4 a power of two <= 16; every pitch a multiple of 4; n * vox and the elements of one
 * sample below 2^31; x, dx, skip, dskip, pooled, dpool and idx must be aligned to 4 elements.  Otherwise 0: keep the two
 * operators.
 * _bwd: dskip or dpool may be NULL (zeros); dx, dgamma, dbeta, dalpha may be NULL.  Workspace:
 * mri3d_norm_act_pool_workspace_bytes (host only; 0 when not supported), 8-byte aligned. */
int32_t mri3d_norm_act_pool_supported(const Mri3dNormGeom* g, const Mri3dPoolGeom* pg);
size_t mri3d_norm_act_pool_workspace_bytes(const Mri3dNormGeom* g, const Mri3dPoolGeom* pg);
int mri3d_norm_act_pool_fwd(const Mri3dNormGeom* g, const Mri3dPoolGeom* pg, const void* x, const float* mean,
                            const float* invstd, const float* gamma, const float* beta, const float* alpha, void* skip,
                            void* pooled, uint8_t* idx, mri3d_stream_t stream);
int mri3d_norm_act_pool_bwd(const Mri3dNormGeom* g, const Mri3dPoolGeom* pg, int training, const void* x, const void* dskip,
                            const void* dpool, const uint8_t* idx, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, const float* alpha, void* dx, float* dgamma, float* dbeta, float* dalpha,
                            void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Upsample — nn.Upsample(scale_factor=2, mode='trilinear', align_corners=False) (unet.UNet decoder),
 * mode='nearest' (modified_3dunet.py:13, AE_model.py:70-73), F.interpolate(size=...) (AE_model.py:119).
 * rd/rh/rw: source step per destination step (torch's "scale" = 1/scale_factor, or in/out for size=).
 * ---------------------------------------------------------------------------------------------- */
typedef struct Mri3dUpGeom {
    int32_t n, di, hi, wi, dout, ho, wo, c;
    int32_t x_ld, y_ld;
    int32_t mode;          /* MRI3D_UP_* */
    int32_t align_corners; /* trilinear only */
    float rd, rh, rw;
    int32_t dtype;
} Mri3dUpGeom;
size_t mri3d_upsample3d_workspace_bytes(const Mri3dUpGeom* g);
int mri3d_upsample3d_fwd(const Mri3dUpGeom* g, const void* x, void* y, mri3d_stream_t stream);
int mri3d_upsample3d_bwd(const Mri3dUpGeom* g, const void* dy, void* dx, void* workspace, size_t ws_bytes,
                         mri3d_stream_t stream);
/* WHICH KERNEL mri3d_upsample3d_fwd (pass = MRI3D_PASS_FWD) or mri3d_upsample3d_bwd (MRI3D_PASS_DGRAD) launches for this geometry,
 * as mri3d_maxpool3d_route answers for the pool.  align: the largest power of two <= 16 that divides the base address of both
 * tensors.  name (at least 40 bytes), T = f32 | bf16:
 *   "upsample2x_fwd_march<T,{4,8},{1,2,4,8}>"   trilinear x2 without align_corners, channels and pitches in quads: <T, VEC, NPV>
 *   "upsample_fwd<T,{1,4}>"                     every other forward
 *   "upsample2x_bwd_march<T>"                   trilinear x2 as above with c % 16 == 0
 *   "upsample2x_bwd<T>"                         trilinear x2 as above, every other channel count (the LDS-tiled kernel)
 *   "upsample_nearest_int_bwd<T,{2,4}>"         nearest with output = S x input in every axis, channels and pitches in quads
 *   "tables+upsample_bwd<T,{1,4}>"              every other backward: upsample_tables_kernel fills the workspace, then the gather
 * Segment lengths, tile counts and grids are not part of a name. */
int mri3d_upsample3d_route(const Mri3dUpGeom* g, int32_t pass, int32_t align, char* name, size_t name_bytes);

/* THE NUMBERS OF THE LAUNCH PLAN whose kernel mri3d_maxpool3d_route / mri3d_upsample3d_route name: same arguments, same checks,
 * same plan function, host only.  Fields a kernel does not use are 0.
 *   vec       channels per lane item (1, 4, 8)
 *   npv       upsample2x_fwd_march: lane items per voxel and channel pass (NPV); upsample_nearest_int_bwd: the scale S
 *   hch       slab kernels: rows of H per slab (hch < the pass's H extent: a slab is a part of a plane, the last part may be ragged)
 *   grid      workgroups launched; the kernels loop where the plan has more slabs / items than that
 *   segs      marching kernels: segments along D per column (forward: of segl coarse planes, backward: of 8); tile kernel: D tiles
 *   segl      upsample2x_fwd_march: coarse planes per segment (16, 8 or 4)
 *   tiles_h, tiles_w   tile and marching kernels: coarse tiles in H and W
 *   passes    marching kernels: channel passes per tile
 *   items     tile and marching kernels: n x segs x tiles_h x tiles_w x passes work items
 *   tables    1: upsample_tables_kernel fills the workspace before the gather
 *   lds_bytes dynamic LDS of the launch
 * Both return MRI3D_OK or the error the route query gives for the arguments; out must not be NULL. */
typedef struct Mri3dResamplePlanInfo {
    int32_t vec, npv, hch, grid, segs, segl, tiles_h, tiles_w, passes, items, tables;
    int64_t lds_bytes;
} Mri3dResamplePlanInfo;
int32_t mri3d_maxpool3d_plan_query(const Mri3dPoolGeom* g, int32_t pass, int32_t addend_ld, int32_t align_tensors,
                                   int32_t align_idx, Mri3dResamplePlanInfo* out);
int32_t mri3d_upsample3d_plan_query(const Mri3dUpGeom* g, int32_t pass, int32_t align, Mri3dResamplePlanInfo* out);

/* ------------------------------------------------------------------------------------------------
 * Fused softmax(dim=C) + soft-Dice loss — F.softmax + get_dice_loss + .mean()
 * (segmentation/routine.py:239-253,272-274).  target has ct = 1 (broadcast over classes, the
 * reference's behaviour) or ct = c channels.  stats: [n*c*3] floats (tp, sum_p, sum_g) kept for bwd.
 * ---------------------------------------------------------------------------------------------- */
typedef struct Mri3dDiceGeom {
    int32_t n;
    int64_t vox;
    int32_t c, ct;
    int32_t x_ld, t_ld;
    float eps;
    int32_t dtype;
} Mri3dDiceGeom;
size_t mri3d_softmax_dice_workspace_bytes(const Mri3dDiceGeom* g);
int mri3d_softmax_dice_fwd(const Mri3dDiceGeom* g, const void* logits, const void* target, float* loss,
                           float* stats, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
/* dlogits = dloss * d(loss)/d(logits); dloss is a device pointer to one float. */
int mri3d_softmax_dice_bwd(const Mri3dDiceGeom* g, const void* logits, const void* target, const float* stats,
                           const float* dloss, void* dlogits, mri3d_stream_t stream);

/* argmax over channels -> uint8 mask (validate_dsc_asd, segmentation/routine.py:226-227). First max wins. */
int mri3d_argmax_u8(const void* logits, uint8_t* out, int64_t nvox, int32_t c, int32_t ld, int32_t dtype,
                    mri3d_stream_t stream);

/* Overlap counts of two uint8 masks for the validation metrics of validate_dsc_asd (segmentation/routine.py:198-235;
 * compute_dice_coefficient segmentation/metrics.py:312-329; get_iou_score routine.py:198-203), exact integers:
 *   counts[0] = sum(gt)  [1] = sum(pred)  [2] = sum(gt & pred)  [3] = #(gt>0 and pred>0)  [4] = #(gt>0 or pred>0)
 *   Dice = 2*counts[2] / (counts[0] + counts[1])   (NaN when the denominator is 0);   IoU = counts[3] / counts[4]. */
size_t mri3d_mask_overlap_workspace_bytes(void);
int mri3d_mask_overlap(const uint8_t* pred, const uint8_t* gt, int64_t nvox, int64_t* counts, void* workspace,
                       size_t ws_bytes, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Label maps on the device (labels.hip): the raw label volume becomes a uint8 class map, the loss and the validation
 * scores read that class map.  Storage types of a label volume (int32 and float32 share a size, hence codes of their own):
 * ---------------------------------------------------------------------------------------------- */
enum { MRI3D_LABEL_U8 = 0, MRI3D_LABEL_I16 = 1, MRI3D_LABEL_I32 = 2, MRI3D_LABEL_F32 = 3 };

/* Id remap — prepare_batch's binarisation (segmentation/routine.py:185-196: np.isin(first, LIST_FCD) -> 1,
 * targets >= 1000 -> 1, targets != 1 -> 0) and, with another table, the class map of a FreeSurfer parcellation (the seg_parc
 * checkpoints).  in: n labels of in_dtype (any MRI3D_LABEL_*); out: MRI3D_LABEL_U8 or MRI3D_LABEL_F32.  Per element v, with
 * lut[0..lut_len) uint8 on the device (1 <= lut_len <= 65536) and above, other in 0..255:
 *     v >= lut_len (compared as a value: 1000.5 and +inf count)   -> above
 *     v an integer in [0, lut_len)                                -> lut[v]
 *     anything else (negative, fractional, NaN, -inf)             -> other
 * lut_len = 1000, lut[i] = 1 for i in LIST_FCD or i == 1, above = 1, other = 0 is prepare_batch's rule for its first sample.
 * out == in is allowed when the two have the same type (in place); any other overlap is MRI3D_EINVAL, as is a pointer that
 * is not aligned to its own element.  16 bytes per load where the addresses allow it, single elements in front and behind. */
int mri3d_label_remap(const void* in, int32_t in_dtype, void* out, int32_t out_dtype, int64_t n, const uint8_t* lut,
                      int32_t lut_len, int32_t above, int32_t other, mri3d_stream_t stream);

/* Softmax-Dice against a class map — F.softmax + get_dice_loss + .mean() (segmentation/routine.py:239-253,272-274) with the
 * target given as class indices instead of float one-hot channels: g_c(v) = [labels(v) == c].  logits (n, vox, x_ld >= c)
 * fp32 or bf16, labels dense uint8 (n, vox), 2 <= c <= 32 (else MRI3D_ENOTSUP).  A label >= c belongs to no class: the voxel
 * adds to sum_p only (the way to ignore voxels).  loss, stats ([n*c*3] floats (tp, sum_p, sum_g)) and the backward
 * expression are those of mri3d_softmax_dice_*; sums are taken in double in a fixed order: same inputs, same bits. */
typedef struct Mri3dDiceIndexGeom {
    int32_t n;
    int64_t vox;
    int32_t c;
    int32_t x_ld;
    float eps;
    int32_t dtype;
} Mri3dDiceIndexGeom;
size_t mri3d_softmax_dice_index_workspace_bytes(const Mri3dDiceIndexGeom* g);
int mri3d_softmax_dice_index_fwd(const Mri3dDiceIndexGeom* g, const void* logits, const uint8_t* labels, float* loss,
                                 float* stats, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_softmax_dice_index_bwd(const Mri3dDiceIndexGeom* g, const void* logits, const uint8_t* labels,
                                 const float* stats, const float* dloss, void* dlogits, mri3d_stream_t stream);

/* Voxel-wise cross-entropy / focal loss against a class map, alone or fused with the softmax-Dice above (ce_loss.hip).  Inputs
 * as mri3d_softmax_dice_index_*: logits (n, vox, x_ld >= c) fp32 or bf16, labels dense uint8 (n, vox), 2 <= c <= 32 (else
 * MRI3D_ENOTSUP), a label >= c marks an ignored voxel.  weight: c class weights, float32 on the device, or NULL for all ones.
 *     logp_y = z_y - max z - log sum_j exp(z_j - max z),  pt = softmax(z)_y
 *     l_v    = -w_y (1 - pt)^gamma logp_y                                (0 for an ignored voxel)
 *     CE     = sum_v l_v / sum_v w_y     over the non-ignored voxels of the whole batch; when no voxel counts (sum_v w_y == 0) CE is
 *              0 and its gradient exactly 0, where torch's cross_entropy gives NaN
 *     loss   = dice_weight * Dice_index + ce_weight * CE
 * gamma = 0 is F.cross_entropy(weight, ignore_index, reduction = "mean"); gamma in [1, 8] the focal loss; anything else, a negative
 * or non-finite loss weight, or both loss weights zero: MRI3D_EINVAL.  dice_weight == 0 runs the CE-only kernels, which carry no
 * Dice sums.  stats: 4 + n*c*3 floats = {CE, 1 / sum_w (0 when nothing counts), sum_v l_v, Dice_index}, then (with dice_weight > 0)
 * the (tp, sum_p, sum_g) triples of mri3d_softmax_dice_index_fwd.  The backward reads them and dloss on the device and writes
 * dlogits = dloss * d(loss)/d(logits) with one store per element (bf16: rounded once).  Sums are taken in double in a fixed order:
 * same inputs, same bits.  Bytes per voxel: forward c * esz + 1, backward 2 * c * esz + 1, with or without the Dice part.
 * mri3d_softmax_ce_index_plan_query (host only) reports what a pass launches by, for pass = MRI3D_PASS_FWD or MRI3D_PASS_DGRAD
 * (the backward) and the alignments of the logits (with the backward: of logits and dlogits together) and of the labels, each the
 * largest power of two <= 16 dividing the address: the class bucket (2, 4, 8, 16, 32), the read mode (0: element by element, 1: a
 * voxel's classes in 4-element vectors, 2: two dense classes, 4 voxels per lane), whether the Dice part is compiled in, blocks per
 * sample, lanes per sample (256 a block), and the work items of sample 0 (voxels; mode 2: 4-voxel groups and the single voxels
 * behind them) as whole trips of all lanes and a remainder. */
typedef struct Mri3dCeIndexGeom {
    int32_t n;
    int64_t vox;
    int32_t c;
    int32_t x_ld;
    float eps;
    int32_t dtype;
    float gamma;
    float dice_weight;
    float ce_weight;
} Mri3dCeIndexGeom;
typedef struct Mri3dCeIndexPlanInfo {
    int32_t bucket, mode, dice, blocks, lanes, whole_trips, remainder;
    int64_t items;
} Mri3dCeIndexPlanInfo;
size_t mri3d_softmax_ce_index_workspace_bytes(const Mri3dCeIndexGeom* g);
int mri3d_softmax_ce_index_plan_query(const Mri3dCeIndexGeom* g, int32_t pass, int32_t align_logits, int32_t align_labels,
                                      Mri3dCeIndexPlanInfo* out);
int mri3d_softmax_ce_index_fwd(const Mri3dCeIndexGeom* g, const void* logits, const uint8_t* labels, const float* weight,
                               float* loss, float* stats, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_softmax_ce_index_bwd(const Mri3dCeIndexGeom* g, const void* logits, const uint8_t* labels, const float* weight,
                               const float* stats, const float* dloss, void* dlogits, mri3d_stream_t stream);

/* Confusion counts of two class maps — the per-class form of validate_dsc_asd's Dice / IoU (segmentation/routine.py:198-235,
 * metrics.py:312-329), exact integers.  pred, gt: nvox uint8 each, 2 <= c <= 32 (else MRI3D_ENOTSUP).
 *   counts[g*c + p] = #(gt == g and pred == p)      counts[c*c] = #(gt >= c or pred >= c)        (int64[c*c + 1])
 * workspace: mri3d_confusion_workspace_bytes(c) bytes (0 for c outside 2..32), 8-byte aligned. */
size_t mri3d_confusion_workspace_bytes(int32_t c);
int mri3d_confusion_counts(const uint8_t* pred, const uint8_t* gt, int64_t nvox, int32_t c, int64_t* counts,
                           void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Intensity standardisation ahead of the path: the reference's collate function runs `normalize`
 * (classification/train_ENC_CLF.ipynb cell 9) on every volume — np.percentile at 13 percentiles over all voxels, then a
 * piecewise-linear map between landmarks evaluated in float64.
 *   order_stats: out[i] = the ranks[i]-th smallest element (0-based) of x[0..n); ranks is a HOST array of nranks <= 32.
 *                Exact (integer radix histograms).  np.percentile's linear interpolation between two neighbouring order
 *                statistics is left to the caller (13 float64 operations).
 *   piecewise_linear: y = (float)(slope[b] * (double)x + intercept[b]), b = #{e : edges[e] <= x} (np.digitize, right=False),
 *                multiply and add rounded separately as numpy does; edges / slope / intercept are HOST arrays,
 *                nseg <= 16 segments, nseg-1 non-decreasing edges.
 * ---------------------------------------------------------------------------------------------- */
size_t mri3d_order_stats_workspace_bytes(void);
int mri3d_order_stats_f32(const float* x, int64_t n, const int64_t* ranks, int32_t nranks, float* out, void* workspace,
                          size_t ws_bytes, mri3d_stream_t stream);
int mri3d_piecewise_linear_f32(const float* x, float* y, int64_t n, const double* edges, const double* slope,
                               const double* intercept, int32_t nseg, mri3d_stream_t stream);
/* TorchIO transforms the notebooks apply after the histogram standardisation (segmentation/pretraining_3d_unet.ipynb cell 9:
 * `ZNormalization(masking_method=ZNormalization.mean)`, `CropOrPad(...)`).  Third-party arithmetic, restated from its
 * documentation ("parity unpinned"):
 *   znorm_mean_mask: mask = x > mean(x);  y = (x - mean(x[mask])) / std(x[mask]) (unbiased);  stats (device, 4 doubles) =
 *                    {mean of all voxels, masked count, masked mean, masked std}.
 *   crop_or_pad:     centred crop / zero-pad of `outer` contiguous (di,hi,wi) volumes to (dout,ho,wo); the odd voxel of an
 *                    uneven difference goes to the far end (ini = floor(diff/2)). */
size_t mri3d_znorm_workspace_bytes(void);
int mri3d_znorm_mean_mask_f32(const float* x, float* y, int64_t n, double* stats, void* workspace, size_t ws_bytes,
                              mri3d_stream_t stream);
int mri3d_crop_or_pad_f32(const float* x, float* y, int32_t outer, int32_t di, int32_t hi, int32_t wi, int32_t dout,
                          int32_t ho, int32_t wo, float fill, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Intensity statistics of a stack of volumes (intensity.hip): what the reference looks at before and after harmonisation.
 * plot_histogram (classification/transfer/full_sample_classification.ipynb cell 9) evaluates scipy.stats.gaussian_kde over all
 * voxels of a volume at np.linspace(min, max, 100), for 140 volumes (classification/weights/data_140.csv); the landmark training
 * of HistogramStandardization.train (segmentation/.ipynb_checkpoints/baseline_3d_unet-checkpoint.ipynb, `_get_average_mapping`
 * restated in classification/train_ENC_CLF.ipynb cell 9) needs the same per-volume range and masks.
 * x: `batch` rows of n fp32 values; mask (may be NULL): `batch` rows of n bytes, a voxel counts where its byte is non-zero.
 *   moments[row][8] (float64) = {count, non-finite count, min, max, mean, unbiased variance, 0, 0}.  count is the number of counted
 *     voxels; the non-finite ones among them (NaN, +-inf) are counted apart and min, max, mean and variance describe the finite
 *     rest: +inf, -inf, NaN, NaN when there is none, variance NaN below two finite voxels and exactly 0 when min == max.  Sums of x
 *     and x^2 are taken in float64 in a fixed order (block partials in the workspace, then one block per row): same input, same
 *     bits, whatever the alignment of a row and the contents of the workspace.
 *   kde: density[row][j] = sum_i exp(-(p_j - x_i)^2 / 2h^2) / (count sqrt(2 pi h^2)) over the counted voxels of the row,
 *     h^2 = variance * factor^2, gaussian_kde's covariance.  bw_rule 0: Scott, factor = count^(-1/5) (scipy's default, the
 *     reference's); 1: Silverman, (count 3/4)^(-1/5); 2: factor = bw_scalar > 0.  `moments` is the device array the moments entry
 *     wrote; no host round trip lies between the two.  positions: m float64 on the device shared by all rows, or NULL for
 *     np.linspace(min, max, num=m) of each row, bit for bit (j * step and + min rounded separately, the last position max itself,
 *     m == 1: [min]).  positions_out[row][m] receives the positions used, density[row][m] the estimate, both float64.  The
 *     exponent is evaluated in fp32 on centred, scaled values, sums run in fp32 over 256 voxels and in float64 beyond, in a fixed
 *     order.  A row with count < 2, variance 0 or a non-finite voxel gets NaN densities.  1 <= m <= 1024, else MRI3D_EINVAL.
 *   workspace: mri3d_intensity_workspace_bytes(n, batch, m) bytes, 8-byte aligned, serves both entries (m = 0: moments alone);
 *     0 for invalid arguments.  mri3d_kde_plan: out = {blocks per row, voxels per tile, position slots per lane, trips of a
 *     block's tile loop}.  Both queries are host only.
 * ---------------------------------------------------------------------------------------------- */
size_t mri3d_intensity_workspace_bytes(int64_t n, int32_t batch, int32_t m);
int mri3d_kde_plan(int64_t n, int32_t batch, int32_t m, int32_t out[4]);
int mri3d_intensity_moments_f32(const float* x, const uint8_t* mask, int64_t n, int32_t batch, double* moments,
                                void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_kde_f32(const float* x, const uint8_t* mask, int64_t n, int32_t batch, const double* moments, const double* positions,
                  int32_t m, int32_t bw_rule, double bw_scalar, double* positions_out, double* density, void* workspace,
                  size_t ws_bytes, mri3d_stream_t stream);

/* Average surface distance inputs of validate_dsc_asd (segmentation/routine.py:205-214): for two (d,h,w) uint8 masks
 * (non-zero = inside) and the 256-entry surface-element area table of metrics.py:57-71 (HOST array, for the spacing in use)
 *   sums[0] = sum(dist_to_pred_surface * area), sums[1] = sum(area) over the surface elements of gt,
 *   sums[2], sums[3] = the same over the surface elements of pred with distances to the gt surface       (device doubles)
 * with surface elements and areas as compute_surface_distances defines them (segmentation/metrics.py:25-178) and the exact
 * Euclidean distance transform for unit spacing.  compute_average_surface_distance = (sums[0]/sums[1], sums[2]/sums[3]). */
size_t mri3d_surface_distance_workspace_bytes(int32_t d, int32_t h, int32_t w);
int mri3d_surface_distance(const uint8_t* gt, const uint8_t* pred, int32_t d, int32_t h, int32_t w,
                           const double* area_table, double* sums, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
/* The surface-element lists behind compute_surface_distances (segmentation/metrics.py:25-178), for the order-dependent metrics
 * (compute_robust_hausdorff, compute_surface_overlap_at_tolerance, compute_surface_dice_at_tolerance, metrics.py:208-310):
 * per direction, the exact squared distance of every surface element to the other surface (>= 0x3f000000: the other mask
 * has no surface) and its neighbour code, in arbitrary order; counts[0], counts[1] (device) = list lengths (entries beyond
 * `capacity` are dropped: size the lists for (d+1)(h+1)(w+1) to be safe).  Same workspace as mri3d_surface_distance. */
int mri3d_surface_elements(const uint8_t* gt, const uint8_t* pred, int32_t d, int32_t h, int32_t w, int32_t* d2_gt,
                           uint8_t* code_gt, int32_t* d2_pred, uint8_t* code_pred, int64_t capacity, uint64_t* counts,
                           void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Connected components of a mask or a class map (components.hip): what scipy.ndimage.label, np.bincount and a
 * cluster filter give on the host, for the lesion-wise scores of a detector and the usual mask clean-up.  One (d,h,w) uint8
 * volume in C order, d*h*w < 2^31 (else MRI3D_ENOTSUP); a 2-D map is a volume with d = 1.  All integer: the same bits every run.
 * No allocation, no synchronisation; no kernel waits for another workgroup.
 *
 * mri3d_components_label: connectivity 6, 18 or 26 (faces; faces and edges; faces, edges and corners; anything else
 *   MRI3D_EINVAL).  by_value == 0: foreground is mask != 0.  by_value != 0: two voxels connect only when their values are equal
 *   and non-zero (the components of every class of a class map in one call).  labels: int32 (d,h,w), 0 = background, component ids
 *   1..K in the order of each component's first voxel in C-order scan (scipy.ndimage.label's numbering); count[0] = K (device
 *   int32).  Workspace: mri3d_components_workspace_bytes (0 for a volume the entry point refuses), 4-byte aligned.
 * mri3d_components_stats: per component id 1..capacity (a row per id, row id-1; components above `capacity` are dropped)
 *   stats[capacity][8] (device int64) = voxel count, count of voxels with other != 0 (0 without `other`), dmin, dmax, hmin, hmax,
 *     wmin, wmax (inclusive; a row no voxel reaches: 0, 0, d, -1, h, -1, w, -1);
 *   peak[capacity] (device float32) = max of `score` over the component (-inf for a row no voxel reaches); score and peak are
 *     both given or both NULL; scores are finite (-0 orders below +0);
 *   hit[capacity_other] (device uint8) = 1 where component j+1 of `other_labels`, a second int32 label volume, shares a voxel
 *     with any foreground voxel (label > 0) of `labels`, else 0; other_labels, hit and capacity_other > 0 are given together or
 *     all NULL / 0.  `other` (uint8 mask) and `other_labels` are independent of each other.
 * mri3d_components_select: out[i] = keep[labels[i]] over nvox voxels; keep is a uint8 table of keep_len entries (count + 1, with
 *   keep[0] = 0 for the background); a label outside the table selects 0.
 * mri3d_components_plan_query: host only; what the launches of mri3d_components_label go by: tile extents, tiles per axis, the
 *   grid of each of its six launches (tile union-find, boundary merge, root count, scan, rank, relabel), scan_blocks = block
 *   counts the scan walks, offsets = backward neighbours per voxel (3, 9, 13), static LDS bytes of the tile kernel and the
 *   workspace.  -1 for NULL, non-positive extents or a connectivity the entry point calls invalid, -2 for a volume it refuses. */
typedef struct Mri3dComponentsPlanInfo {
    int32_t td, th, tw, tiles_d, tiles_h, tiles_w, grid_local, grid_merge, grid_roots, grid_scan, grid_rank, grid_relabel,
        scan_blocks, offsets;
    int64_t lds_bytes, ws_bytes;
} Mri3dComponentsPlanInfo;
size_t mri3d_components_workspace_bytes(int32_t d, int32_t h, int32_t w);
int32_t mri3d_components_plan_query(int32_t d, int32_t h, int32_t w, int32_t connectivity, Mri3dComponentsPlanInfo* out);
int mri3d_components_label(const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t connectivity, int32_t by_value,
                           int32_t* labels, int32_t* count, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_components_stats(const int32_t* labels, int32_t d, int32_t h, int32_t w, int32_t capacity, const uint8_t* other,
                           const float* score, int64_t* stats, float* peak, const int32_t* other_labels, int32_t capacity_other,
                           uint8_t* hit, mri3d_stream_t stream);
int mri3d_components_select(const int32_t* labels, int64_t nvox, const uint8_t* keep, int32_t keep_len, uint8_t* out,
                            mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Patch pipeline: the windows TorchIO cuts for patch training and grid inference
 * (torchio.Queue + torchio.sampler.ImageSampler, segmentation/routine.py:150-178 and pretraining_3d_unet.ipynb cell 24;
 * torchio.inference.GridSampler / GridAggregator.add_batch(labels, locations), pretraining_3d_unet.ipynb cell 26).
 * Third-party arithmetic, restated in oracle/patches.py ("parity unpinned").  Volumes are `nvol` contiguous (d,h,w) arrays
 * of `elem_bytes`-sized elements in HBM; `loc_host` is a HOST table of npatch x 4 int32 = (volume index, d0, h0, w0), checked
 * here against the volume (MRI3D_EINVAL when a window leaves it) and handed to the kernels by value.
 *   extract_patches:          out[p, z, y, x] = volumes[loc[p].vol, d0+z, h0+y, w0+x]
 *   aggregate_patches_u8:     each (pd,ph,pw) uint8 label window is cropped by `border` voxels on all six faces and written
 *                             to out[vol] at its location, in patch order: where cropped windows overlap the later patch
 *                             wins (what sequential add_batch slicing does); voxels no cropped window covers are untouched.
 *   aggregate_patches_argmax: the same, reading logits [p][z][y][x][ld] and taking argmax over c channels in flight
 *                             (labels = logits.argmax(dim=1, keepdim=True); first maximum wins).
 * ---------------------------------------------------------------------------------------------- */
int mri3d_extract_patches(const void* volumes, int32_t elem_bytes, int32_t nvol, int32_t d, int32_t h, int32_t w,
                          const int32_t* loc_host, int32_t npatch, int32_t pd, int32_t ph, int32_t pw, void* out,
                          mri3d_stream_t stream);
int mri3d_aggregate_patches_u8(const uint8_t* patches, const int32_t* loc_host, int32_t npatch, int32_t pd, int32_t ph,
                               int32_t pw, int32_t bd, int32_t bh, int32_t bw, uint8_t* out, int32_t nvol, int32_t d,
                               int32_t h, int32_t w, mri3d_stream_t stream);
int mri3d_aggregate_patches_argmax(const void* logits, int32_t c, int32_t ld, int32_t dtype, const int32_t* loc_host,
                                   int32_t npatch, int32_t pd, int32_t ph, int32_t pw, int32_t bd, int32_t bh, int32_t bw,
                                   uint8_t* out, int32_t nvol, int32_t d, int32_t h, int32_t w, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Detection (reference detection/patch_utils.py, detection/model_utils.py): mirrored left/right patch pairs cut along the
 * grey-matter template, and the patch map painted back into a voxel mask.  Volume, template and masks are dense (nx, ny, nz)
 * arrays in the reference's axis order, A[x, y, z] at (x*ny + y)*nz + z.  Slice z is B = np.rot90(A[:, :, z]), B[r, c] =
 * A[c, ny-1-r, z]; a strip is the h rows r = row0 .. row0+h-1; a patch is (z, row0, col0) with
 *   channel 0  B[row0+i, col0+t],   channel 1  B[row0+i, nx-1-col0-t],   i < h, t < w.
 *   strip_starts:        starts[z][row0], z < nz, row0 <= ny-h: the first column of the strip holding a template value > 0, -1
 *                        for an empty strip.
 *   mirror_patches:      out[p] = the (2, h, w) patch of table[p] = (z, row0, col0), a DEVICE table of npatch x 3 int32; dense
 *                        NCHW (channels_last = 0) or [p][i][t][channel] (channels_last = 1).  Bit-exact copy.  `order`: NULL, or
 *                        a device permutation of 0..npatch-1 giving the order in which the patches are worked on (it changes no
 *                        result).  The host cannot read the table: an entry that leaves the volume (or an order entry outside
 *                        0..npatch-1) is never dereferenced, that patch is written as zeros (resp. not written).
 *   mirror_patch_labels: out[p] = 1 where any mask byte under channel 0 of patch p is non-zero, else 0.
 *   patch_vote:          map, out: [4][strips][slices] uint8.  count = non-zero 4-neighbours in the (strip, slice) plane of the
 *                        same patch kind, zero outside the array; out = 1 where count == 4, 0 where count == 0, else map.  Every
 *                        cell is decided from `map`: out must not overlap it (MRI3D_EINVAL).
 *   paint_patches:       map [4][ny/h][nz] (kind 0 side, 1 middle, 2 middle mirrored, 3 side mirrored), starts [nz][ny/h] (of the
 *                        strips row0 = j*h) -> out (nx, ny, nz): a voxel takes the map value of the patch whose channel-0 footprint
 *                        covers it, the middle patch where a side and a middle patch overlap; 0 in empty strips, in rows past the
 *                        last whole strip and outside every patch.  Side patches exist where start < nx/2 - w.
 * All: MRI3D_EINVAL for a null pointer, h <= 0, h > ny, w <= 0, nx/2 - w < 1 (no room for a middle patch), npatch <= 0;
 * MRI3D_ENOTSUP for sizes that leave int32 indexing.  No allocation, no synchronisation, no workspace.
 * ---------------------------------------------------------------------------------------------- */
int mri3d_strip_starts_f32(const float* gm, int32_t nx, int32_t ny, int32_t nz, int32_t h, int32_t* starts, mri3d_stream_t stream);
int mri3d_mirror_patches_f32(const float* volume, int32_t nx, int32_t ny, int32_t nz, const int32_t* table, const int32_t* order,
                             int64_t npatch, int32_t h, int32_t w, int32_t channels_last, float* out, mri3d_stream_t stream);
int mri3d_mirror_patch_labels_u8(const uint8_t* mask, int32_t nx, int32_t ny, int32_t nz, const int32_t* table, int64_t npatch,
                                 int32_t h, int32_t w, uint8_t* out, mri3d_stream_t stream);
int mri3d_patch_vote_u8(const uint8_t* map, int32_t strips, int32_t slices, uint8_t* out, mri3d_stream_t stream);
int mri3d_paint_patches_u8(const uint8_t* map, const int32_t* starts, int32_t nx, int32_t ny, int32_t nz, int32_t h, int32_t w,
                           uint8_t* out, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Augmentation: the random stages of the reference's TorchIO `training_transform`
 * (segmentation/results_validation.ipynb, the `training_transform = Compose([...])` cell; pretraining_3d_unet.ipynb cell 24:
 * RandomBiasField, RandomFlip(axes=(0,)), OneOf({RandomAffine(): 0.8, RandomElasticDeformation(): 0.2}); applied through
 * torchio.ImagesDataset(subjects, transform=transform), segmentation/routine.py:91).  Third-party arithmetic, absent from the
 * reference tree: defined here and restated in tests/augment_ref.py ("parity unpinned").  Random parameters are drawn by the
 * caller on the host; both entries are deterministic.
 *   warp3d:  resamples `s` contiguous (d,h,w) volumes.  For output voxel o = (d,h,w) of subject n, in voxel indices,
 *              src = A[n][:, :3] o + A[n][:, 3] + u_n(o)        A: DEVICE (s,3,4) fp32, row-major
 *            u_n = 0 when `grid` is NULL, else the tensor-product uniform cubic B-spline over the DEVICE control grid
 *            (s,3,gd,gh,gw) fp32 (component, then d,h,w; every g >= 4, gw <= 64): per axis of extent N with m = g - 3,
 *            p = (o + 0.5) m / N, i = clamp(floor p, 0, m - 1), f = p - i, weights (1-f)^3/6, (3f^3-6f^2+4)/6,
 *            (-3f^3+3f^2+3f+1)/6, f^3/6 on control points i .. i+3.
 *            A sample is inside when -0.5 <= src_a <= N_a - 0.5 on all axes.  image (fp32, may be NULL with image_out):
 *            trilinear over floor(src), floor(src)+1 with indices clamped to the volume; outside: pad_values[n] when
 *            `pad_values` (DEVICE, s floats) is given, else pad_value.  label (label_bytes = 1, 2 or 4, raw bits, may be NULL
 *            with label_out): the element at clamp(floor(src + 0.5)); outside: zero bits.  Both are written in one pass.
 *            No destination may overlap a source, the other destination or a parameter buffer (MRI3D_EINVAL).
 *   bias_field: y = x * exp(P(xh,yh,zh)), (xh,yh,zh) = the voxel's (d,h,w) mapped to np.linspace(-1,1,N) per axis (0 when
 *            N == 1); P = sum c_ijk xh^i yh^j zh^k over i in 0..order, j in 0..order-i, k in 0..order-i-j, coefficients in
 *            that nesting order: coef_host is a HOST array of s x (order+1)(order+2)(order+3)/6 floats handed to the kernel by
 *            value.  order <= 3 (MRI3D_ENOTSUP above).  y == x (in place) is allowed, a partial overlap is not.
 *   kspace_mix: the k-space half of TorchIO's RandomMotion (the `RescaleIntensity((0, 1)), RandomMotion()` pair that opens the
 *            reference's transform lists, commented out).  The artefact Fourier-transforms n = K + 1 volumes (the unmoved one
 *            and K rigidly moved copies, made by warp3d), fills slabs of the shifted spectrum ALONG THE LAST AXIS ONLY, each slab
 *            from one spectrum, transforms back and keeps the real part.  The slab masks depend on the w frequency alone, so
 *            the transforms along d and h cancel against their inverses; along w, a mask times a spectrum is a circular
 *            convolution with the mask's inverse transform, whose imaginary part meets a real image and is dropped:
 *              out[i,d,h,z] = sum_{m<n} sum_{z'<w} coef[i,m,(z - z') mod w] * images[i,m,d,h,z']
 *              coef[i,m,r]  = (1/w) sum_{k in S_m} cos(2 pi k r / w)
 *            S_m = the unshifted frequencies whose shifted position falls in the slab(s) filled from image m (drawn and summed
 *            by the caller in float64: transforms.motion_coefficients).  images: DEVICE (s,n,d,h,w) fp32 contiguous; coef:
 *            DEVICE (s,n,w) fp32; out: DEVICE (s,d,h,w), must not overlap images or coef.  fp32 accumulation in one fixed order
 *            (m ascending, then z' ascending): bit-identical run to run, no atomics, no workspace.  MRI3D_EINVAL before any
 *            launch for a null pointer, a non-positive extent, n outside 1..8 or w > 256 (a lane keeps w / 64 outputs in
 *            registers and a block the input rows of its 4 waves in LDS; the reference's volumes are 160-200 wide).
 * ---------------------------------------------------------------------------------------------- */
int mri3d_warp3d(const float* image, float* image_out, const void* label, void* label_out, int32_t label_bytes, int32_t s,
                 int32_t d, int32_t h, int32_t w, const float* affine, const float* grid, int32_t gd, int32_t gh, int32_t gw,
                 float pad_value, const float* pad_values, mri3d_stream_t stream);
int mri3d_bias_field_f32(const float* x, float* y, int32_t s, int32_t d, int32_t h, int32_t w, const float* coef_host,
                         int32_t order, mri3d_stream_t stream);
int mri3d_kspace_mix_f32(const float* images, /* DEVICE (s, n, d, h, w) contiguous */
                         float* out,          /* DEVICE (s, d, h, w); must not overlap images */
                         int32_t s, int32_t n, int32_t d, int32_t h, int32_t w,
                         const float* coef,   /* DEVICE (s, n, w) */
                         mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Channel-slice plumbing: torch.cat along channels (unet.UNet decoder, modified_3dunet.py:158-178) and
 * residual adds (modified_3dunet.py:108, cnn_model.py:34).
 *   copy: dst[v, 0:c] = src[v, 0:c]      add: dst[v, 0:c] = a[v,0:c] + b[v,0:c]
 * ---------------------------------------------------------------------------------------------- */
int mri3d_copy_channels(const void* src, void* dst, int64_t nvox, int32_t c, int32_t src_ld, int32_t dst_ld,
                        int32_t dtype, mri3d_stream_t stream);
int mri3d_add_channels(const void* a, const void* b, void* dst, int64_t nvox, int32_t c, int32_t a_ld,
                       int32_t b_ld, int32_t dst_ld, int32_t dtype, mri3d_stream_t stream);
/* Storage-type cast at the edge of a bf16 region (the `.to(bfloat16)` / `.float()` an autocast region inserts;
 * BASELINE configs[3]): dst[v, 0:c] = (dst_dtype) src[v, 0:c], round-to-nearest-even towards bf16. */
int mri3d_convert_channels(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t nvox, int32_t c,
                           int32_t src_ld, int32_t dst_ld, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * BayesConv3d (variational dropout) — segmentation/models/3d_bayes_layers.py:195-232, used by 3d_bayes_unet.py::UNet3D(bayes=True).
 * The layer is a mean convolution, a variance convolution over x^2 and one Gaussian sample per output element; the two
 * convolutions and their gradients are mri3d_conv3d_* calls, the passes around them are below.  The noise `eps` is an INPUT
 * (fp32, drawn by the caller): nothing here is random, every entry is deterministic.
 *   weights (fp32 parameters, n elements, any layout):
 *     raw = logsigma - log(mu^2 + 1e-8)    log_alpha = clamp(raw, -5, 5)    v = mu^2 exp(log_alpha)
 *     eval == 0:  w_var = v                 (w_mean = mu: w_mean is not written and may be NULL)
 *     eval != 0:  m = [log_alpha < threshold]    w_mean = mu m    w_var = v m
 *     bwd: dmu, dlogsigma from the gradients of w_mean, w_var, log_alpha (each may be NULL = no gradient), with the clamp passing
 *     the gradient on the closed interval and the mask m carrying none; pass d_w_mean also in train mode (w_mean = mu there).
 *     mu = 0 gives finite values and gradients.
 *   volume passes (NDHWC, one voxel pitch per tensor, dtype = storage of every tensor except eps, which is always fp32):
 *     square:      x2 = x^2
 *     sample_fwd:  y = mu_out + eps sqrt(1e-4 + var_out)              y == mu_out (same pitch) is allowed
 *     sample_bwd:  dvar = dy eps / (2 sqrt(1e-4 + var_out))
 *     dx:          dx = dx_mean + 2 x dx_var                          dx == dx_mean (same pitch) is allowed
 *     16 bytes per lane when c and every pitch are multiples of 4 (fp32) / 8 (bf16) and every pointer is 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int mri3d_bayes_weights_fwd(const float* mu, const float* logsigma, int64_t n, int32_t eval, float threshold, float* w_mean,
                            float* w_var, float* log_alpha, mri3d_stream_t stream);
int mri3d_bayes_weights_bwd(const float* mu, const float* logsigma, int64_t n, int32_t eval, float threshold,
                            const float* d_w_mean, const float* d_w_var, const float* d_log_alpha, float* dmu,
                            float* dlogsigma, mri3d_stream_t stream);
int mri3d_bayes_square(const void* x, void* x2, int64_t nvox, int32_t c, int32_t x_ld, int32_t x2_ld, int32_t dtype,
                       mri3d_stream_t stream);
int mri3d_bayes_sample_fwd(const void* mu_out, const void* var_out, const float* eps, void* y, int64_t nvox, int32_t c,
                           int32_t mu_ld, int32_t var_ld, int32_t eps_ld, int32_t y_ld, int32_t dtype, mri3d_stream_t stream);
int mri3d_bayes_sample_bwd(const void* dy, const void* var_out, const float* eps, void* dvar, int64_t nvox, int32_t c,
                           int32_t dy_ld, int32_t var_ld, int32_t eps_ld, int32_t dvar_ld, int32_t dtype,
                           mri3d_stream_t stream);
int mri3d_bayes_dx(const void* dx_mean, const void* dx_var, const void* x, void* dx, int64_t nvox, int32_t c,
                   int32_t dx_mean_ld, int32_t dx_var_ld, int32_t x_ld, int32_t dx_ld, int32_t dtype, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Monte-Carlo predictive statistics — the read-out of the stochastic models (3d_bayes_unet.py::UNet3D(bayes=True), which samples
 * in train and eval mode; Dropout3d in modified_3dunet.py and unet.UNet(monte_carlo_dropout=p)): T sampled forward passes become
 * a mean prediction with its uncertainty maps.  nvox = N*D*H*W voxels of NDHWC logits (fp32 or bf16, widened on load) with
 * 2 <= c <= 32 classes (else MRI3D_ENOTSUP) and voxel pitch ld >= c.
 *   state: an fp32 buffer of mri3d_mc_state_bytes(nvox, c) bytes that the caller owns and only these entries read or write; it
 *     holds, per voxel, sum_t p_c and sum_t p_c^2 for each class and sum_t sum_c p_c log p_c.  The query is host only and returns
 *     0 for nvox <= 0 or c outside 2..32.
 *   accumulate: adds `reps` draws in one read-modify-write of the state.  Draw r of voxel v starts at element
 *     (r*rep_stride + v)*ld of `logits`, r = 0..reps-1 in that order, rep_stride >= nvox voxels when reps > 1 (a batch of reps*N
 *     volumes with draw r of volume n at batch index r*N + n has rep_stride = nvox).  first != 0 overwrites the state (it need
 *     not be initialised), first == 0 adds to it.  One call with reps = k leaves the very bits that k calls with reps = 1 leave.
 *     Per draw:  m = max_c z_c   S = sum_c exp(z_c - m)   log p_c = z_c - m - log S   p_c = exp(z_c - m) / S;  the entropy term is
 *     p_c * log p_c with log p_c from the logits, so a probability that underflows to 0 adds exactly 0.
 *   finalize, with T = samples; every output is dense and may be NULL, but not all five:
 *     mean_p[v][c] = sum p / T                        variance[v][c] = max(sum p^2 / T - mean^2, 0)   (population variance)
 *     entropy[v] = -sum_c (mean > 0 ? mean log mean : 0)       mutual_info[v] = max(entropy + (sum_t sum_c p log p) / T, 0)
 *     mask[v] = first maximal mean_p[v][c] (the rule of mri3d_argmax_u8, on the floats written to mean_p)
 *   Non-finite logits are outside the contract.  No workspace, no atomics: the same inputs give the same bits.  c == 2 with dense
 *   logits and 16-byte aligned pointers (and draws, when reps > 1) moves 16 bytes per lane and access; anything else one voxel
 *   per lane.
 * ---------------------------------------------------------------------------------------------- */
size_t mri3d_mc_state_bytes(int64_t nvox, int32_t c);
int mri3d_mc_accumulate(const void* logits, int64_t nvox, int32_t c, int32_t ld, int32_t dtype, int32_t reps,
                        int64_t rep_stride, int32_t first, void* state, size_t state_bytes, mri3d_stream_t stream);
int mri3d_mc_finalize(const void* state, size_t state_bytes, int64_t nvox, int32_t c, int32_t samples, float* mean_p,
                      float* variance, float* entropy, float* mutual_info, uint8_t* mask, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * AdamW / Adam on one flat fp32 buffer — torch.optim.AdamW (segmentation/routine.py:358) and
 * torch.optim.Adam with L2 weight_decay (classification/routine.py:271,275).
 * grad_scale multiplies the gradient first (1/world_size after the RCCL sum all-reduce).
 * decoupled != 0: AdamW (p *= 1 - lr*wd); decoupled == 0: Adam (g += wd*p).
 * ---------------------------------------------------------------------------------------------- */
int mri3d_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int32_t step, float grad_scale, int32_t decoupled,
                    mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Affine registration to a template (register.hip): the device pieces of an intensity-based registration, the counterpart of
 * the FLIRT call in the reference's detection/preprocessing_utils.py:11-73.  Volumes are dense (d, h, w); the "fixed" volume is
 * the template's grid, the "moving" one the subject's.  An affine is 12 fp32 numbers, a row-major (3, 4) matrix that maps a
 * fixed voxel index o = (d, h, w) to a moving voxel index, warp3d's convention.  The file is compiled without contraction and
 * writes no fused multiply-add: every * and + below is one fp32 rounding, in the order written (tests/register_ref.py restates it).
 *
 *   coordinates   r_a = (A[a][0]*d + A[a][1]*h) + A[a][3]          s_a = A[a][2]*w + r_a                  a = 0, 1, 2
 *   inside        -0.5 <= s_a <= N_a - 0.5 on all three axes (N the moving extents); a NaN coordinate is outside
 *   trilinear     q_a = min(max(s_a, -1), N_a)   e_a = floor(q_a)   f_a = q_a - e_a (exact)   indices e_a, e_a + 1 clamped to
 *                 [0, N_a - 1];  along w: x = v0 + f_2*(v1 - v0) for the four (d, h) corner pairs, then along h:
 *                 y = x0 + f_1*(x1 - x0), then along d: v = y0 + f_0*(y1 - y0)
 *   nearest       index clamp(floor(q_a + 0.5), 0, N_a - 1)
 *
 * mri3d_quantize_u8: out[i] = clamp(floor((x[i] - lo) * scale), 0, bins - 1) as a byte; 255 ("skip") where the mask byte is 0
 *   (mask may be NULL) or x[i] is not finite.  2 <= bins <= 64, scale finite.
 * mri3d_joint_hist: for candidate c of k (1..64), every fixed voxel o whose byte bf = fixed_bins[o] is not 255 and whose sample
 *   under affines[c] is inside adds 1 to hist[c][bf][bm], bm = clamp(floor((v - m_lo) * m_scale), 0, bins - 1) (a NaN v goes to
 *   bin 0).  A fixed byte in bins..254 is treated as skip.  hist: DEVICE int64 (k, bins, bins), fully written.  affines: DEVICE
 *   (k, 3, 4) fp32.  Counts are integers summed with integer atomics: the same inputs give the same bits whatever the workspace
 *   held.  workspace: mri3d_joint_hist_workspace_bytes(df, hf, wf, k, bins) bytes (0 for invalid arguments), 4-byte aligned.
 *   Every volume has fewer than 2^31 voxels (else MRI3D_ENOTSUP).
 * mri3d_joint_hist_plan (host only): out = {blocks per candidate group, candidate groups, candidates that share one block's
 *   fixed loads, fixed rows per block and trip (one per wave), trips of a block's row loop, LDS bytes, reduction stages, fixed
 *   voxels per wave step}.
 * mri3d_hist_costs: out[c] = {cost, n}, DEVICE float64 (k, 2), n the counted samples of hist[c], one block per candidate, float64
 *   in a fixed order.  With p = hist / n, p_i its row sums (fixed), p_j its column sums (moving), y_j = j + 0.5:
 *     kind 0  correlation ratio   sum_i p_i Var_i(y) / Var(y),  Var_i(y) = sum_j p_ij (y_j - mean_i)^2 / p_i
 *     kind 1  -MI = -(H_f + H_m - H_fm),  H = -sum p log p (natural logarithm)
 *     kind 2  -(H_f + H_m) / H_fm
 *   +inf when n < min_count, n == 0 or the denominator (Var(y), H_fm) is 0.
 * mri3d_resample_affine: image_out[o] = trilinear sample of `image`, pad_value outside; label_out[o] = the raw bits of the
 *   nearest element of `label` (label_bytes 1, 2 or 4), zero bits outside.  One pass writes both; either pair may be NULL, not
 *   both.  `affine`: DEVICE, 12 floats.  No destination may overlap a source or the affine.
 * mri3d_downsample2_mean_f32: y (ceil(d/2), ceil(h/2), ceil(w/2)); y[o] = (sum of the voxels of x in the cell 2o .. 2o + 1 that
 *   exist, added in (d, h, w) order to a sum that starts at the first) * (1 / their number); the number is 1, 2, 4 or 8.
 * No entry allocates or synchronises; arguments are validated on the host before any launch.
 * ---------------------------------------------------------------------------------------------- */
int mri3d_quantize_u8(const float* x, const uint8_t* mask, int64_t n, float lo, float scale, int32_t bins, uint8_t* out,
                      mri3d_stream_t stream);
size_t mri3d_joint_hist_workspace_bytes(int32_t df, int32_t hf, int32_t wf, int32_t k, int32_t bins);
int mri3d_joint_hist_plan(int32_t df, int32_t hf, int32_t wf, int32_t k, int32_t bins, int32_t out[8]);
int mri3d_joint_hist(const uint8_t* fixed_bins, int32_t df, int32_t hf, int32_t wf, const float* moving, int32_t dm, int32_t hm,
                     int32_t wm, const float* affines, int32_t k, float m_lo, float m_scale, int32_t bins, int64_t* hist,
                     void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_hist_costs(const int64_t* hist, int32_t k, int32_t bins, int32_t kind, double min_count, double* out,
                     mri3d_stream_t stream);
int mri3d_resample_affine(const float* image, float* image_out, const void* label, void* label_out, int32_t label_bytes,
                          int32_t dm, int32_t hm, int32_t wm, int32_t df, int32_t hf, int32_t wf, const float* affine,
                          float pad_value, mri3d_stream_t stream);
int mri3d_downsample2_mean_f32(const float* x, int32_t d, int32_t h, int32_t w, float* y, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Bias-field estimation over tissue classes (tissue.hip): the device passes of an EM for a K-class Gaussian mixture on
 * log-intensity with a smooth multiplicative field, the model behind the `_restore` image that the reference takes from FSL FAST
 * (detection/preprocessing_utils.py:11-53), with an optional Potts prior on the labels (mri3d_tissue_mrf_pass).  No 26-neighbourhood,
 * no anisotropic beta, no mean-field (soft) neighbours, no partial volumes, no spline field.  x: DEVICE fp32 (d, h, w), fewer
 * than 2^31 voxels (else MRI3D_ENOTSUP); mask: DEVICE uint8 of the same shape or NULL.  All arithmetic is float64.
 *
 *   selected      mask byte != 0 (no mask: always), x finite and > 0;   y = log(x)
 *   coordinates   (xh, yh, zh) = the voxel's (d, h, w) mapped to np.linspace(-1, 1, N) per axis (0 when N == 1), as bias_field
 *   field         b = sum_n c_n xh^i yh^j zh^k, the terms in bias_field's nesting (i, then j, then k, i + j + k <= order),
 *                 M = (order + 1)(order + 2)(order + 3) / 6 of them;  r = y - b
 *   posteriors    p_k proportional to pi_k v_k^-1/2 exp(-(r - mu_k)^2 / (2 v_k)), normalised through the largest log term
 *
 * params_host: HOST array of 3K + M doubles (pi[K], mu[K], v[K], c[M]), read before the call returns.  2 <= classes <= 4,
 * 0 <= order <= 3 (MRI3D_ENOTSUP above 3); pi finite and >= 0 with one > 0, mu and c finite, v finite and > 0 (else MRI3D_EINVAL).
 *
 * mri3d_tissue_em_pass: one pass with the parameters fixed.  sums: DEVICE float64, 2 + 3K + N2 + M numbers, fully written:
 *     [0] n, the selected voxels           [1] LL = sum log sum_k pi_k N(r; mu_k, v_k), the -1/2 log 2 pi included
 *     [2 + k] S0_k = sum p_k               [2 + K + k] S1_k = sum p_k r            [2 + 2K + k] S2_k = sum p_k r^2
 *     [2 + 3K + m]      Mw[a][b][c] = sum w xh^a yh^b zh^c,  w = sum_k p_k / v_k,  the N2 = (2 order + 1)(2 order + 2)(2 order + 3) / 6
 *                       exponent triples with a + b + c <= 2 order enumerated a, then b, then c (c fastest), m their running number
 *     [2 + 3K + N2 + m] Mt[a][b][c] = sum t xh^a yh^b zh^c,  t = sum_k p_k (y - mu_k) / v_k,  a + b + c <= order, same enumeration
 *   Two stages without float atomics: a wave sums one (d, h) row into 2 + 3K + (2 order + 1) + (order + 1) numbers in the
 *   workspace, then one block per table entry adds the rows, times xh^a yh^b, in a fixed order.  The same inputs give the same
 *   bits whatever the workspace held.  workspace: mri3d_tissue_em_workspace_bytes(d, h, w, classes, order) bytes (0 for invalid
 *   arguments), 8-byte aligned; neither it nor sums may overlap x or the mask.
 * mri3d_tissue_em_plan (host only): out = {stage-1 blocks, rows per block and trip (one per wave), trips of a block's row loop,
 *   wave steps of 64 voxels per row, sums per row, table entries (= stage-2 blocks), stage-2 threads per entry, rows d * h}.
 *   The workspace is out[4] * out[7] doubles.
 * mri3d_tissue_apply: the final pass over EVERY voxel: restored = x exp(-b) and, unless NULL, field = exp(b), each rounded once
 *   to fp32; labels (uint8) = 0 where the voxel is not selected, else 1 + the rank, by ascending mu (equal means in the caller's
 *   order), of the class with the largest log pi_k - 1/2 log v_k - (r - mu_k)^2 / (2 v_k), the first of equal maxima in that
 *   rank order.  restored == x (in place) is allowed; any other overlap among the buffers is MRI3D_EINVAL.
 * mri3d_tissue_mrf_pass: mri3d_tissue_em_pass with a Markov random field (Potts) prior on a label volume, one half-sweep of
 *   red-black ICM: hidden-MRF EM.  Labels are uint8 (d, h, w): 0 where a voxel is not selected, else 1 + its class in the order
 *   of params_host (not by ascending mu).  n_k = how many of the voxel's up to six face neighbours inside the volume hold k + 1
 *   in labels_in; any other byte (0, or one above K) counts for no class.  Per selected voxel
 *       logt_k = log pi_k - 1/2 log v_k - 1/2 log 2 pi - (r - mu_k)^2 / (2 v_k) + beta n_k,   p_k = softmax_k logt_k,
 *       new = 1 + argmax_k logt_k, the first of equal maxima;
 *   sums has mri3d_tissue_em_pass's layout and definitions with these p_k, [1] the pseudo-log-likelihood
 *   sum [logsumexp_k logt_k - log sum_k pi_k exp(beta n_k)]; with beta = 0 the table is the plain pass's whatever the labels.
 *   mode 0 or 1: labels_out = new where the voxel is selected and (d + h + w) & 1 == mode, labels_in where it is selected and of
 *   the other colour, 0 where it is not selected.  mode 2, the start: no neighbour term, labels_in is not read and may be NULL,
 *   every selected voxel gets new.  labels_out is fully written.  labels_in and labels_out are two buffers: a resting voxel still
 *   contributes its posterior, read from active neighbours, so a pass in place would depend on the launch order; with two buffers
 *   every voxel reads labels_in only, there are no atomics and the same inputs give the same bits.  0 <= beta <= 8 and finite,
 *   mode 0..2, labels_in NULL only in mode 2, no overlap among labels_in, labels_out, x, mask, sums and the workspace (else
 *   MRI3D_EINVAL).  The plan and the workspace are mri3d_tissue_em_pass's (mri3d_tissue_em_plan, mri3d_tissue_em_workspace_bytes).
 * No entry allocates or synchronises; arguments are validated on the host before any launch.
 * ---------------------------------------------------------------------------------------------- */
size_t mri3d_tissue_em_workspace_bytes(int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order);
int mri3d_tissue_em_plan(int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order, int32_t out[8]);
int mri3d_tissue_em_pass(const float* x, const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order,
                         const double* params_host, double* sums, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_tissue_apply(const float* x, const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order,
                       const double* params_host, float* restored, uint8_t* labels, float* field, mri3d_stream_t stream);
int mri3d_tissue_mrf_pass(const float* x, const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t classes, int32_t order,
                          const double* params_host, double beta, int32_t mode, const uint8_t* labels_in, uint8_t* labels_out,
                          double* sums, void* workspace, size_t ws_bytes, mri3d_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Distance maps (distance.hip): the exact squared Euclidean distance transform of a batch of n dense (d,h,w) uint8
 * volumes in C order, ball morphology as a threshold of it, the signed map of a class map, and the boundary loss that reads it.
 *   sq[v] = squared distance in voxels from v to the nearest zero voxel of the same volume (int32; 0 at a zero voxel).
 *   value == -1: a voxel is zero when its byte is 0; 0 <= value <= 255: when its byte differs from `value` (a class of a class map;
 *     value = 0 measures the distance to the non-zero voxels).  Anything else: MRI3D_EINVAL.
 *   outside_zero == 0: only real voxels count (scipy.ndimage.distance_transform_edt); a volume without a zero voxel saturates to
 *     MRI3D_EDT_INF everywhere.  outside_zero != 0: the volume is surrounded by zero voxels (scipy's border_value = 0 erosion).
 *   d^2 + h^2 + w^2 >= MRI3D_EDT_INF or d*h*w >= 2^31: MRI3D_ENOTSUP.  A 2-D map is d = 1.  Integers only, no atomics: the same bits
 *   every run.  No allocation, no synchronisation.
 * mri3d_edt_sq_u8: out = sq (int32).
 * mri3d_edt_threshold_u8: out (uint8) = sq <= r2 (greater == 0) or sq > r2 (greater != 0), 0 <= r2 < MRI3D_EDT_INF (else
 *   MRI3D_EINVAL); the int32 map is never written.  With the ball of radius r and r2 = floor(r^2): value = 0, outside_zero = 0,
 *   greater = 0 is binary_dilation; value = -1, greater = 1 is binary_erosion with border_value = !outside_zero.
 * mri3d_signed_sqdist_u8: labels is a class map, `classes` in [2, 32] (else MRI3D_ENOTSUP), ids a HOST array of k class ids, 1 <= k
 *   <= 32 and every id < classes (else MRI3D_EINVAL).  out: int32 (n, k, d, h, w).  For plane i (class c = ids[i]) and a voxel of label y:
 *     y >= classes: INT32_MIN (the voxel is ignored);  class c absent from the volume, or no counted voxel of it of another class: 0;
 *     y != c: +(squared distance to the nearest voxel of class c);  y == c: -(squared distance to the nearest voxel not of class c,
 *     ignored voxels included).
 *   Absence and fullness are decided on the device (a class mask per volume): nothing comes to the host.
 * Workspace of all three: mri3d_edt_workspace_bytes(n, d, h, w) bytes (0 for a shape they refuse), 8-byte aligned.
 * mri3d_edt_plan (host only): what the three passes launch by.  The w pass stages rows_w consecutive rows per workgroup (partial_w:
 *   rows of the last workgroup when it is not whole, else 0); the h and d passes stage tiles of all len values of tx_h / tx_d
 *   neighbouring lines (partial_*: lines of the last tile of a slice when it is not whole).  staged_* = 0: the line is longer than
 *   the tile, lanes read global memory (rows_w = 1, tx = 64).  batch = n; grid_*: workgroups; lds_bytes: static LDS of a pass.
 *
 * Boundary loss (Kervadec et al., MIDL 2019) of logits NDHWC with voxel pitch x_ld >= c, fp32 or bf16, 2 <= c <= 32 (else
 * MRI3D_ENOTSUP), against map = the (n, k, vox) int32 signed map of the k distinct class ids (k outside [1, 32], an id >= c or given
 * twice: MRI3D_EINVAL):
 *   loss = (1 / cnt) sum over (n, i, v) with s != INT32_MIN of softmax(z)[n, ids[i], v] * phi(s[n, i, v]),  cnt = number of terms,
 *   phi(s) = sqrt(s) for s > 0, -(sqrt(-s) - 1) for s < 0, 0 for s = 0;  cnt == 0: loss 0 and a zero gradient.
 *   dlogits_j = dloss / cnt * p_j (phi_j [j among ids] - sum_i p_ids[i] phi_i), the softmax recomputed; dlogits has the logits'
 *   layout with its own voxel pitch dx_ld >= c (else MRI3D_EINVAL).
 * stats: 4 floats the forward leaves for the backward {loss, 1 / cnt, cnt, sum}.  Sums are double block partials folded in a fixed
 * order: the same bits every run.  Workspace of the forward: mri3d_softmax_boundary_workspace_bytes(), 8-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
#define MRI3D_EDT_INF 0x3f000000
typedef struct Mri3dEdtPlanInfo {
    int32_t rows_w, staged_w, partial_w, tx_h, staged_h, partial_h, tx_d, staged_d, partial_d, batch;
    int64_t grid_w, grid_h, grid_d, lds_bytes, ws_bytes;
} Mri3dEdtPlanInfo;
typedef struct Mri3dBoundaryGeom {
    int32_t n;
    int64_t vox;
    int32_t c;
    int32_t x_ld;
    int32_t dtype;
    int32_t k;
    int32_t ids[32];
} Mri3dBoundaryGeom;
size_t mri3d_edt_workspace_bytes(int32_t n, int32_t d, int32_t h, int32_t w);
int mri3d_edt_plan(int32_t n, int32_t d, int32_t h, int32_t w, Mri3dEdtPlanInfo* out);
int mri3d_edt_sq_u8(const uint8_t* in, int32_t n, int32_t d, int32_t h, int32_t w, int32_t value, int32_t outside_zero, int32_t* out,
                    void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_edt_threshold_u8(const uint8_t* in, int32_t n, int32_t d, int32_t h, int32_t w, int32_t value, int32_t outside_zero,
                           int32_t r2, int32_t greater, uint8_t* out, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_signed_sqdist_u8(const uint8_t* labels, int32_t n, int32_t d, int32_t h, int32_t w, int32_t classes, const int32_t* ids,
                           int32_t k, int32_t* out, void* workspace, size_t ws_bytes, mri3d_stream_t stream);
size_t mri3d_softmax_boundary_workspace_bytes(void);
int mri3d_softmax_boundary_fwd(const Mri3dBoundaryGeom* g, const void* logits, const int32_t* map, float* loss, float* stats,
                               void* workspace, size_t ws_bytes, mri3d_stream_t stream);
int mri3d_softmax_boundary_bwd(const Mri3dBoundaryGeom* g, const void* logits, const int32_t* map, const float* stats,
                               const float* dloss, void* dlogits, int32_t dx_ld, mri3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MRI3D_H */
