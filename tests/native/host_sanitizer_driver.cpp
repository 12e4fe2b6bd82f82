// Host-side sanitizer driver: the C-ABI library's HOST code — argument validation, plan /
// dispatch selection, workspace sizing, error-string formatting — compiled for the host only with
// -fsanitize=address,undefined together with this file, and driven WITHOUT a GPU: every call below must return before any
// kernel launch (invalid arguments, or a pure workspace query).  GPU AddressSanitizer is not available on this pool; the
// device code is covered by the parity suite instead.  Exit code 0 and no sanitizer report = pass.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "mri3d.h"

static int g_fail = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                       \
        }                                                                   \
    } while (0)

static Mri3dConvGeom conv(int n, int d, int h, int w, int ci, int co, int k, int s, int p, int dil, int dtype, int xpad,
                          int ypad) {
    Mri3dConvGeom g;
    memset(&g, 0, sizeof(g));
    g.n = n; g.di = d; g.hi = h; g.wi = w; g.ci = ci; g.co = co;
    g.kd = g.kh = g.kw = k; g.sd = g.sh = g.sw = s; g.pd = g.ph = g.pw = p; g.dd = g.dh = g.dw = dil;
    g.dout = (d + 2 * p - dil * (k - 1) - 1) / s + 1;
    g.ho = (h + 2 * p - dil * (k - 1) - 1) / s + 1;
    g.wo = (w + 2 * p - dil * (k - 1) - 1) / s + 1;
    g.x_ld = ci + xpad; g.y_ld = co + ypad; g.dtype = dtype;
    return g;
}

int main() {
    EXPECT(mri3d_version() >= 100);
    char fake[64];                       // a non-null pointer that is never dereferenced on the host
    void* P = fake;
    alignas(16) static char A[64];       // the same, 16-byte aligned: passes the MFMA paths' alignment checks

    // ---- conv: workspace queries over a sweep of geometries (plan functions of every kernel family), incl. degenerate ones
    const int chans[] = {1, 2, 3, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192};
    const int sizes[][3] = {{1, 1, 1}, {2, 3, 5}, {8, 8, 8}, {10, 12, 10}, {32, 32, 32}, {80, 96, 80}, {160, 192, 160}, {192, 192, 192}};
    size_t checked = 0, stats_routes = 0, routes = 0;
    char name[32];
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int ci : chans)
            for (int co : chans)
                for (auto& sz : sizes)
                    for (int cfg = 0; cfg < 5; ++cfg) {
                        const int k = cfg == 3 ? 1 : (cfg == 4 ? 4 : 3), s = cfg == 1 ? 2 : (cfg == 4 ? 2 : 1);
                        const int p = cfg == 3 ? 0 : 1, dil = cfg == 2 ? 3 : 1;
                        if (sz[0] + 2 * p - dil * (k - 1) - 1 < 0 || sz[1] + 2 * p - dil * (k - 1) - 1 < 0 || sz[2] + 2 * p - dil * (k - 1) - 1 < 0) continue;
                        for (int n : {1, 2, 512}) {
                            if ((int64_t)n * sz[0] * sz[1] * sz[2] * (ci > co ? ci : co) > (int64_t)1 << 34) continue;
                            Mri3dConvGeom g = conv(n, sz[0], sz[1], sz[2], ci, co, k, s, p, dil, dtype, (ci % 3) * 2, (co % 2) * 4);
                            for (int pass = 0; pass < 3; ++pass) {
                                const size_t ws = mri3d_conv3d_workspace_bytes(&g, pass);
                                EXPECT(ws % 256 == 0 && ws < ((size_t)1 << 40));
                                ++checked;
                                // the route query names a kernel for every pass, alignment and bias; only a request for fused
                                // statistics can be refused ("none"), and a misaligned tensor never reaches the 16-byte MFMA kernels
                                // (every name fits the 32-byte minimum buffer; the two tensors' alignments are independent)
                                for (int align : {16, 8, 4})
                                    for (int align_y : {16, 4})
                                        for (int bias = 0; bias < 2; ++bias) {
                                            memset(name, 0x7f, sizeof(name));
                                            EXPECT(mri3d_conv3d_route(&g, pass, 0, bias, 0, 0, align, align_y, name, sizeof(name)) == MRI3D_OK);
                                            EXPECT(memchr(name, 0, sizeof(name)) != nullptr && name[0] != 0 && strcmp(name, "none") != 0);
                                            if (align < 16 || align_y < 16) EXPECT(strncmp(name, "generic ", 8) == 0 || strncmp(name, "pointwise ", 10) == 0);
                                            ++routes;
                                        }
                            }
                            // statistics: served exactly where the block query promises them
                            EXPECT(mri3d_conv3d_route(&g, MRI3D_PASS_FWD, 1, 1, 0, 0, 16, 16, name, sizeof(name)) == MRI3D_OK);
                            EXPECT((strcmp(name, "none") != 0) == (mri3d_conv3d_fwd_stats_blocks(&g) > 0));
                            EXPECT(mri3d_conv3d_route(&g, MRI3D_PASS_FWD, 1, 1, 0, 0, 8, 8, name, sizeof(name)) == MRI3D_OK && strcmp(name, "none") == 0);
                            // where the query promises fused statistics, the launch path reaches the same route: with a 16-byte
                            // workspace it stops at the packed-weight image (always larger), neither "not served" nor a launch
                            if (mri3d_conv3d_fwd_stats_blocks(&g) > 0) {
                                EXPECT(mri3d_conv3d_fwd_stats(&g, A, A, A, A, (double*)A, A, 16, nullptr) == MRI3D_EWORKSPACE);
                                ++stats_routes;
                            }
                        }
                    }
    EXPECT(checked > 10000 && stats_routes > 1000 && routes > 60000);
    EXPECT(mri3d_conv3d_workspace_bytes(nullptr, 0) == 0);

    // ---- conv: argument validation (every branch returns before a launch)
    Mri3dConvGeom g = conv(2, 16, 16, 16, 16, 16, 3, 1, 1, 1, MRI3D_F32, 0, 0);
    EXPECT(mri3d_conv3d_fwd(nullptr, P, P, P, P, P, 0, nullptr) == MRI3D_EINVAL);
    EXPECT(strlen(mri3d_last_error()) > 0);
    EXPECT(mri3d_conv3d_fwd(&g, nullptr, P, P, P, P, 0, nullptr) == MRI3D_EINVAL);
    EXPECT(mri3d_conv3d_dgrad(&g, P, nullptr, P, P, P, 0, nullptr) == MRI3D_EINVAL);
    EXPECT(mri3d_conv3d_wgrad(&g, P, P, nullptr, P, P, 0, nullptr) == MRI3D_EINVAL);
    {   // workspace too small for the MFMA path (16-byte aligned fake pointers)
        alignas(16) static char buf[64];
        EXPECT(mri3d_conv3d_fwd(&g, buf, buf, buf, buf, buf, 16, nullptr) == MRI3D_EWORKSPACE);
        EXPECT(mri3d_conv3d_wgrad(&g, buf, buf, buf, buf, buf, 16, nullptr) == MRI3D_EWORKSPACE);
        EXPECT(mri3d_conv3d_dgrad(&g, buf, buf, buf, buf, nullptr, 0, nullptr) == MRI3D_EWORKSPACE);
    }
    Mri3dConvGeom bad = g;
    bad.dtype = 7;
    EXPECT(mri3d_conv3d_fwd(&bad, P, P, P, P, P, 0, nullptr) == MRI3D_ENOTSUP);
    bad = g; bad.dout = 15;
    EXPECT(mri3d_conv3d_fwd(&bad, P, P, P, P, P, 0, nullptr) == MRI3D_EINVAL);
    EXPECT(strstr(mri3d_last_error(), "do not match") != nullptr);
    bad = g; bad.x_ld = 8;
    EXPECT(mri3d_conv3d_wgrad(&bad, P, P, P, P, P, 0, nullptr) == MRI3D_EINVAL);
    bad = g; bad.n = 0;
    EXPECT(mri3d_conv3d_dgrad(&bad, P, P, P, P, P, 0, nullptr) == MRI3D_EINVAL);
    bad = g; bad.kd = 0;
    EXPECT(mri3d_conv3d_fwd(&bad, P, P, P, P, P, 0, nullptr) == MRI3D_EINVAL);
    bad = g; bad.pd = -1;
    EXPECT(mri3d_conv3d_fwd(&bad, P, P, P, P, P, 0, nullptr) == MRI3D_EINVAL);

    // ---- route query: argument validation
    EXPECT(mri3d_conv3d_route(nullptr, 0, 0, 0, 0, 0, 16, 16, name, sizeof(name)) == MRI3D_EINVAL);
    EXPECT(mri3d_conv3d_route(&g, 0, 0, 0, 0, 0, 16, 16, nullptr, sizeof(name)) == MRI3D_EINVAL);
    EXPECT(mri3d_conv3d_route(&g, 0, 0, 0, 0, 0, 16, 16, name, 8) == MRI3D_EINVAL);                  // name buffer too small
    EXPECT(mri3d_conv3d_route(&g, 3, 0, 0, 0, 0, 16, 16, name, sizeof(name)) == MRI3D_EINVAL);       // no such pass
    EXPECT(mri3d_conv3d_route(&g, MRI3D_PASS_WGRAD, 1, 0, 0, 0, 16, 16, name, sizeof(name)) == MRI3D_EINVAL);   // statistics outside the forward
    EXPECT(mri3d_conv3d_route(&g, 0, 0, 0, -16, 0, 16, 16, name, sizeof(name)) == MRI3D_EINVAL);
    EXPECT(mri3d_conv3d_route(&bad, 0, 0, 0, 0, 0, 16, 16, name, sizeof(name)) == MRI3D_EINVAL);     // (bad.pd = -1)

    // ---- split operands (conv over cat((x, x2))): the support query over a sweep, refusals without a launch
    {
        // the *_cat entry point of a pass with a 16-byte workspace: MRI3D_EWORKSPACE exactly where the support query says 1 (the
        // launch path found a kernel and stopped at its workspace), MRI3D_ENOTSUP where it says 0; never a launch
        auto cat_agrees = [&](const Mri3dConvGeom& c, int split, int ld, int pass) {
            const int rc = pass == 0   ? mri3d_conv3d_fwd_cat(&c, A, A, split, ld, A, A, A, nullptr, A, 16, nullptr)
                           : pass == 1 ? mri3d_conv3d_dgrad_cat(&c, A, A, A, A, split, ld, A, 16, nullptr)
                                       : mri3d_conv3d_wgrad_cat(&c, A, A, split, ld, A, A, A, A, 16, nullptr);
            return rc == (mri3d_conv3d_cat_supported(&c, split, ld, pass) == 1 ? MRI3D_EWORKSPACE : MRI3D_ENOTSUP);
        };
        int served = 0;
        for (int dtype = 0; dtype < 2; ++dtype)
            for (int ca : {8, 16, 32, 48})
                for (int cb : {8, 16, 24, 32, 64})
                    for (int sz : {6, 40, 160}) {
                        Mri3dConvGeom c = conv(2, sz, sz + 8, sz, ca + cb, 16, 3, 1, 1, 1, dtype, 0, 0);
                        c.x_ld = ca;
                        for (int pass = 0; pass < 3; ++pass) {
                            served += mri3d_conv3d_cat_supported(&c, ca, cb, pass);
                            for (int extra : {0, 4, 8, 12}) {
                                EXPECT(cat_agrees(c, ca, cb + extra, pass));
                                // the route query names a kernel exactly where the split entry point is served
                                EXPECT(mri3d_conv3d_route(&c, pass, 0, 1, ca, cb + extra, 16, 16, name, sizeof(name)) == MRI3D_OK);
                                EXPECT((strcmp(name, "none") != 0) == (mri3d_conv3d_cat_supported(&c, ca, cb + extra, pass) == 1));
                            }
                        }
                        EXPECT(mri3d_conv3d_cat_supported(&c, 0, cb, 0) == 0);          // no first part
                        EXPECT(mri3d_conv3d_cat_supported(&c, ca + cb, cb, 0) == 0);    // no second part
                        EXPECT(mri3d_conv3d_fwd_cat_stats_blocks(&c, 0, cb) == 0);
                        EXPECT(mri3d_conv3d_fwd_cat_stats_blocks(&c, ca + cb, cb) == 0);
                        const int blocks = mri3d_conv3d_fwd_cat_stats_blocks(&c, ca, cb);
                        EXPECT(blocks >= 0 && (blocks == 0 || mri3d_conv3d_cat_supported(&c, ca, cb, 0) == 1));
                        // a dense second tensor (pitch = its channel count, a multiple of 8) takes the same kernel as the
                        // concatenation in one tensor
                        Mri3dConvGeom whole = c;
                        whole.x_ld = ca + cb;
                        if (blocks > 0 && cb % 8 == 0) EXPECT(blocks == mri3d_conv3d_fwd_stats_blocks(&whole));
                    }
        EXPECT(served > 0);
        // statistics partials of the split forward: the block count must be that of the kernel which runs.  fp32 volumes of >= 4 M
        // voxels with 16 output channels go to the marching kernel, but only with a second-tensor pitch of a multiple of 8; the
        // other pitches (20, 28: served, multiples of 4) run the tiled kernel, whose grid is larger (512 against 240 at 160x192x160)
        int swept = 0;
        for (int dtype = 0; dtype < 2; ++dtype)
            for (int n : {1, 2})
                for (auto& sz : {std::vector<int>{160, 192, 160}, std::vector<int>{128, 128, 256}, std::vector<int>{40, 48, 40}})
                    for (int cb : {16, 32})
                        for (int extra : {0, 4, 8, 12}) {
                            const int ld = cb + extra;
                            Mri3dConvGeom c = conv(n, sz[0], sz[1], sz[2], 16 + cb, 16, 3, 1, 1, 1, dtype, 0, 0);
                            c.x_ld = 16;
                            const int blocks = mri3d_conv3d_fwd_cat_stats_blocks(&c, 16, ld);
                            const int supported = mri3d_conv3d_cat_supported(&c, 16, ld, 0);
                            EXPECT((blocks > 0) == (supported == 1));
                            for (int pass = 0; pass < 3; ++pass) EXPECT(cat_agrees(c, 16, ld, pass));
                            if (!supported) continue;
                            ++swept;
                            Mri3dConvGeom whole = c;
                            whole.x_ld = 16 + cb;
                            EXPECT(blocks > 0 && blocks <= 512 + mri3d_conv3d_march_stats_blocks(&whole));
                            if (ld % 8 == 0) EXPECT(blocks == mri3d_conv3d_fwd_stats_blocks(&whole));
                        }
        EXPECT(swept > 20);
        {   // the case of the overrun: fp32, 1 x (16 + 16) -> 16 at 160x192x160, the second tensor a slice of a 20-channel buffer
            Mri3dConvGeom c = conv(1, 160, 192, 160, 32, 16, 3, 1, 1, 1, MRI3D_F32, 0, 0);
            Mri3dConvGeom whole = c;
            c.x_ld = 16;
            const int one = mri3d_conv3d_fwd_stats_blocks(&whole);
            EXPECT(one > 0 && one < 512);                                             // the marching kernel's grid
            for (int ld : {20, 28}) {
                EXPECT(mri3d_conv3d_cat_supported(&c, 16, ld, 0) == 1);
                EXPECT(mri3d_conv3d_fwd_cat_stats_blocks(&c, 16, ld) == 512);         // the tiled kernel's grid
            }
            EXPECT(mri3d_conv3d_fwd_cat_stats_blocks(&c, 16, 16) == one && mri3d_conv3d_fwd_cat_stats_blocks(&c, 16, 24) == one);
            EXPECT(mri3d_conv3d_fwd_cat_stats_blocks(nullptr, 16, 16) == 0);
        }
        EXPECT(mri3d_conv3d_cat_supported(nullptr, 16, 32, 0) == 0);
        Mri3dConvGeom c = conv(2, 160, 192, 160, 48, 16, 3, 1, 1, 1, 0, 0, 0);
        c.x_ld = 16;
        EXPECT(mri3d_conv3d_cat_supported(&c, 16, 32, 0) == 1 && mri3d_conv3d_cat_supported(&c, 16, 32, 1) == 1 &&
               mri3d_conv3d_cat_supported(&c, 16, 32, 2) == 1);
        EXPECT(mri3d_conv3d_cat_supported(&c, 8, 40, 0) == 0);                         // split not a multiple of 16
        EXPECT(mri3d_conv3d_fwd_cat(&c, nullptr, P, 16, 32, P, P, P, nullptr, P, 0, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_conv3d_fwd_cat(&c, P, nullptr, 16, 32, P, P, P, nullptr, P, 0, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_conv3d_dgrad_cat(&c, P, P, P, nullptr, 16, 32, P, 0, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_conv3d_wgrad_cat(&c, P, nullptr, 16, 32, P, P, P, P, 0, nullptr) == MRI3D_EINVAL);
        alignas(16) static char buf2[64];
        EXPECT(mri3d_conv3d_fwd_cat(&c, buf2, buf2, 8, 40, buf2, buf2, buf2, nullptr, buf2, 0, nullptr) == MRI3D_ENOTSUP);   // bad split
        EXPECT(mri3d_conv3d_fwd_cat(&c, buf2, buf2 + 4, 16, 32, buf2, buf2, buf2, nullptr, buf2, 0, nullptr) == MRI3D_ENOTSUP);   // misaligned x2
        EXPECT(mri3d_conv3d_fwd_cat(&c, buf2, buf2, 16, 32, buf2, buf2, buf2, nullptr, buf2, 16, nullptr) == MRI3D_EWORKSPACE);
        c.x_ld = 8;   // pitch of the first tensor smaller than its channel count
        EXPECT(mri3d_conv3d_fwd_cat(&c, buf2, buf2, 16, 32, buf2, buf2, buf2, nullptr, buf2, 0, nullptr) == MRI3D_EINVAL);
    }

    // ---- the marching kernel's plan query over the sweep: it answers exactly where the support query says 1, its grid is the
    // statistics block count, its weight image fits the workspace; refusals and bad arguments without a launch
    {
        Mri3dMarchPlanInfo mi;
        size_t served = 0, refused = 0, dispatched = 0;
        for (int dtype = 0; dtype < 2; ++dtype)
            for (int ci : chans)
                for (int co : chans)
                    for (auto& sz : sizes)
                        for (int pad : {0, 4, 8})
                            for (int pass = 0; pass < 2; ++pass) {
                                Mri3dConvGeom c = conv(2, sz[0], sz[1], sz[2], ci, co, 3, 1, 1, 1, dtype, pad, pad);
                                const int rc = mri3d_conv3d_march_plan_query(&c, pass, 0, &mi);
                                EXPECT(rc == (mri3d_conv3d_march_supported(&c, pass) == 1 ? MRI3D_OK : MRI3D_ENOTSUP));
                                if (rc == MRI3D_OK) {
                                    ++served;
                                    dispatched += mi.dispatcher;
                                    EXPECT(mi.chunks >= 1 && mi.chunks <= 4 && mi.blocks >= 1 && mi.wgh * mi.wgw == 8);
                                    EXPECT(mi.nbuf == (mi.chunks == 1 ? 3 : 2) && mi.smem_bytes > 0 && mi.smem_bytes <= 160 * 1024);
                                    EXPECT((int64_t)mi.grid == (int64_t)mi.blocks * mi.gch * mi.gcw * mi.nseg * c.n);
                                    EXPECT((mi.nseg - 1) * mi.seglen < sz[0] && sz[0] <= mi.nseg * mi.seglen);
                                    EXPECT(mi.wp_bytes > 0 && (size_t)mi.wp_bytes <= mri3d_conv3d_workspace_bytes(&c, pass));
                                } else {
                                    ++refused;
                                }
                                if (pass == 0) {
                                    const int rs = mri3d_conv3d_march_plan_query(&c, 0, 1, &mi);
                                    const int blocks = mri3d_conv3d_march_stats_blocks(&c);
                                    EXPECT(rs == MRI3D_OK ? (blocks > 0 && blocks == mi.grid && mi.blocks <= 8) : (rs == MRI3D_ENOTSUP && blocks == 0));
                                } else {
                                    EXPECT(mri3d_conv3d_march_plan_query(&c, 1, 1, &mi) == MRI3D_EINVAL);   // no statistics in the data gradient
                                }
                            }
        EXPECT(served > 1000 && refused > 1000 && dispatched > 0);
        Mri3dConvGeom c = conv(1, 160, 192, 160, 16, 16, 3, 1, 1, 1, MRI3D_BF16, 0, 0);
        EXPECT(mri3d_conv3d_march_plan_query(&c, 0, 1, &mi) == MRI3D_OK && mi.dispatcher == 1 && mi.chunks == 1 && mi.nbuf == 3);
        EXPECT(mri3d_conv3d_march_plan_query(&c, 2, 0, &mi) == MRI3D_EINVAL);                              // no weight gradient here
        EXPECT(mri3d_conv3d_march_plan_query(nullptr, 0, 0, &mi) == MRI3D_EINVAL && mri3d_conv3d_march_plan_query(&c, 0, 0, nullptr) == MRI3D_EINVAL);
        for (int k : {1, 5}) {
            Mri3dConvGeom o = conv(1, 16, 16, 16, 16, 16, k, 1, k / 2, 1, MRI3D_F32, 0, 0);
            EXPECT(mri3d_conv3d_march_plan_query(&o, 0, 0, &mi) == MRI3D_ENOTSUP);
        }
        Mri3dConvGeom st = conv(1, 16, 16, 16, 16, 16, 3, 2, 1, 1, MRI3D_F32, 0, 0), di = conv(1, 16, 16, 16, 16, 16, 3, 1, 2, 2, MRI3D_F32, 0, 0);
        EXPECT(mri3d_conv3d_march_plan_query(&st, 0, 0, &mi) == MRI3D_ENOTSUP && mri3d_conv3d_march_plan_query(&di, 1, 0, &mi) == MRI3D_ENOTSUP);
        Mri3dConvGeom wide = conv(1, 2, 8, 16, 8, 136, 3, 1, 1, 1, MRI3D_F32, 0, 0);                       // nine output blocks
        EXPECT(mri3d_conv3d_march_plan_query(&wide, 0, 0, &mi) == MRI3D_OK && mi.blocks == 9 && mri3d_conv3d_march_plan_query(&wide, 0, 1, &mi) == MRI3D_ENOTSUP);
        wide.dout += 1;
        EXPECT(mri3d_conv3d_march_plan_query(&wide, 0, 0, &mi) == MRI3D_EINVAL);
    }

    // ---- other families: null geometry / null pointers / zero sizes must be refused, workspace queries must not crash
    EXPECT(mri3d_norm_stats(nullptr, P, nullptr, nullptr, nullptr, nullptr, 0.1f, P, 0, nullptr) != MRI3D_OK);
    EXPECT(mri3d_norm_act_fwd(nullptr, P, nullptr, nullptr, nullptr, nullptr, nullptr, P, nullptr) != MRI3D_OK);
    EXPECT(mri3d_maxpool3d_fwd(nullptr, P, P, nullptr, nullptr) != MRI3D_OK);
    EXPECT(mri3d_maxpool3d_bwd(nullptr, P, nullptr, P, nullptr) != MRI3D_OK);
    EXPECT(mri3d_upsample3d_fwd(nullptr, P, P, nullptr) != MRI3D_OK);
    EXPECT(mri3d_softmax_dice_fwd(nullptr, P, P, nullptr, nullptr, P, 0, nullptr) != MRI3D_OK);
    for (int c : {1, 8, 16, 48, 96, 128}) {
        Mri3dNormGeom ng;
        memset(&ng, 0, sizeof(ng));
        ng.n = 2; ng.vox = (int64_t)160 * 192 * 160; ng.c = c; ng.x_ld = c; ng.y_ld = c; ng.eps = 1e-5f; ng.group_c = 0;
        for (int inst = 0; inst < 2; ++inst)
            for (int dt = 0; dt < 2; ++dt) {
                ng.instance = inst; ng.dtype = dt;
                EXPECT(mri3d_norm_workspace_bytes(&ng) > 0);
            }
        Mri3dUpGeom ug;
        memset(&ug, 0, sizeof(ug));
        ug.n = 2; ug.di = 40; ug.hi = 48; ug.wi = 40; ug.dout = 80; ug.ho = 96; ug.wo = 80; ug.c = c; ug.x_ld = c; ug.y_ld = c;
        ug.mode = MRI3D_UP_TRILINEAR; ug.rd = ug.rh = ug.rw = 0.5f;
        (void)mri3d_upsample3d_workspace_bytes(&ug);
        Mri3dDiceGeom dg;
        memset(&dg, 0, sizeof(dg));
        dg.n = 2; dg.vox = (int64_t)160 * 192 * 160; dg.c = 2; dg.ct = 1; dg.x_ld = 2; dg.t_ld = 1; dg.eps = 1e-9f;
        EXPECT(mri3d_softmax_dice_workspace_bytes(&dg) > 0);
    }
    {   // pool / upsample route and plan queries: the four launch plans over channels, dtypes and alignments name a kernel and
        // give its numbers, launch nothing
        char rname[40];
        long routes = 0, plans = 0;
        for (int c : {1, 3, 4, 8, 12, 16, 24, 40, 64})
            for (int dt = 0; dt < 2; ++dt)
                for (int align : {4, 8, 16}) {
                    Mri3dPoolGeom pg;
                    memset(&pg, 0, sizeof(pg));
                    pg.n = 2; pg.di = 8; pg.hi = 6; pg.wi = 10; pg.dout = 4; pg.ho = 3; pg.wo = 5; pg.c = c; pg.x_ld = c; pg.y_ld = c;
                    pg.kd = pg.kh = pg.kw = 2; pg.sd = pg.sh = pg.sw = 2; pg.dtype = dt;
                    for (int addend_ld : {-1, 0, c, c + 4}) {
                        memset(rname, 0x7f, sizeof(rname));
                        const int pass = addend_ld < 0 ? MRI3D_PASS_FWD : MRI3D_PASS_DGRAD;
                        EXPECT(mri3d_maxpool3d_route(&pg, pass, addend_ld < 0 ? 0 : addend_ld, align, align, rname, sizeof(rname)) == MRI3D_OK);
                        EXPECT(memchr(rname, 0, sizeof(rname)) != nullptr && rname[0] != 0);
                        ++routes;
                        Mri3dResamplePlanInfo info;
                        memset(&info, 0x7f, sizeof(info));
                        EXPECT(mri3d_maxpool3d_plan_query(&pg, pass, addend_ld < 0 ? 0 : addend_ld, align, align, &info) == MRI3D_OK);
                        EXPECT((info.vec == 1 || info.vec == 4 || info.vec == 8) && c % info.vec == 0 && info.hch >= 1 && info.grid >= 1 &&
                               info.items == 0 && info.tables == 0 && info.lds_bytes == 0);
                        ++plans;
                    }
                    Mri3dUpGeom ug;
                    memset(&ug, 0, sizeof(ug));
                    ug.n = 2; ug.di = 4; ug.hi = 5; ug.wi = 6; ug.c = c; ug.x_ld = c; ug.y_ld = c; ug.dtype = dt;
                    for (int kind = 0; kind < 3; ++kind) {      // trilinear x2, nearest x4, trilinear to a size
                        const int sc = kind == 0 ? 2 : 4;
                        ug.dout = kind == 2 ? 7 : sc * ug.di; ug.ho = kind == 2 ? 9 : sc * ug.hi; ug.wo = kind == 2 ? 11 : sc * ug.wi;
                        ug.mode = kind == 1 ? MRI3D_UP_NEAREST : MRI3D_UP_TRILINEAR;
                        ug.rd = (float)ug.di / ug.dout; ug.rh = (float)ug.hi / ug.ho; ug.rw = (float)ug.wi / ug.wo;
                        for (int pass : {MRI3D_PASS_FWD, MRI3D_PASS_DGRAD}) {
                            memset(rname, 0x7f, sizeof(rname));
                            EXPECT(mri3d_upsample3d_route(&ug, pass, align, rname, sizeof(rname)) == MRI3D_OK);
                            EXPECT(memchr(rname, 0, sizeof(rname)) != nullptr && rname[0] != 0);
                            ++routes;
                            Mri3dResamplePlanInfo info;
                            memset(&info, 0x7f, sizeof(info));
                            EXPECT(mri3d_upsample3d_plan_query(&ug, pass, align, &info) == MRI3D_OK);
                            EXPECT((info.vec == 1 || info.vec == 4 || info.vec == 8) && c % info.vec == 0 && info.grid >= 1 &&
                                   (info.tables == 0 || info.tables == 1) && info.lds_bytes >= 0);
                            if (info.items != 0)      // the tile and marching kernels: their items are the product of their counts
                                EXPECT((int64_t)info.items == (int64_t)ug.n * info.segs * info.tiles_h * info.tiles_w * (info.passes ? info.passes : 1) &&
                                       info.grid <= (info.items + 7) / 8 * 8);
                            else
                                EXPECT(info.hch >= 1 && info.segl == 0);
                            ++plans;
                        }
                    }
                    if (c == 1 && dt == 0 && align == 4) {       // argument validation
                        EXPECT(mri3d_maxpool3d_route(nullptr, MRI3D_PASS_FWD, 0, 16, 16, rname, sizeof(rname)) == MRI3D_EINVAL);
                        EXPECT(mri3d_maxpool3d_route(&pg, MRI3D_PASS_WGRAD, 0, 16, 16, rname, sizeof(rname)) == MRI3D_EINVAL);
                        EXPECT(mri3d_maxpool3d_route(&pg, MRI3D_PASS_FWD, c, 16, 16, rname, sizeof(rname)) == MRI3D_EINVAL);      // an addend in the forward
                        EXPECT(mri3d_maxpool3d_route(&pg, MRI3D_PASS_DGRAD, 0, 16, 16, rname, 8) == MRI3D_EINVAL);
                        EXPECT(mri3d_upsample3d_route(nullptr, MRI3D_PASS_FWD, 16, rname, sizeof(rname)) == MRI3D_EINVAL);
                        EXPECT(mri3d_upsample3d_route(&ug, MRI3D_PASS_WGRAD, 16, rname, sizeof(rname)) == MRI3D_EINVAL);
                        EXPECT(mri3d_upsample3d_route(&ug, MRI3D_PASS_FWD, 16, nullptr, sizeof(rname)) == MRI3D_EINVAL);
                        Mri3dResamplePlanInfo info;
                        EXPECT(mri3d_maxpool3d_plan_query(nullptr, MRI3D_PASS_FWD, 0, 16, 16, &info) == MRI3D_EINVAL);
                        EXPECT(mri3d_maxpool3d_plan_query(&pg, MRI3D_PASS_FWD, 0, 16, 16, nullptr) == MRI3D_EINVAL);
                        EXPECT(mri3d_maxpool3d_plan_query(&pg, MRI3D_PASS_WGRAD, 0, 16, 16, &info) == MRI3D_EINVAL);
                        EXPECT(mri3d_maxpool3d_plan_query(&pg, MRI3D_PASS_FWD, c, 16, 16, &info) == MRI3D_EINVAL);
                        EXPECT(mri3d_upsample3d_plan_query(nullptr, MRI3D_PASS_FWD, 16, &info) == MRI3D_EINVAL);
                        EXPECT(mri3d_upsample3d_plan_query(&ug, MRI3D_PASS_FWD, 16, nullptr) == MRI3D_EINVAL);
                        EXPECT(mri3d_upsample3d_plan_query(&ug, MRI3D_PASS_WGRAD, 16, &info) == MRI3D_EINVAL);
                    }
                }
        EXPECT(routes == 9 * 2 * 3 * (4 + 6) && plans == routes);
    }
    EXPECT(mri3d_norm_workspace_bytes(nullptr) == 0);
    EXPECT(mri3d_mask_overlap_workspace_bytes() > 0 && mri3d_order_stats_workspace_bytes() > 0 && mri3d_znorm_workspace_bytes() > 0);
    EXPECT(mri3d_surface_distance_workspace_bytes(160, 192, 160) > 0);
    EXPECT(mri3d_argmax_u8(nullptr, nullptr, 10, 2, 2, 0, nullptr) != MRI3D_OK);
    EXPECT(mri3d_mask_overlap(nullptr, nullptr, 10, nullptr, nullptr, 0, nullptr) != MRI3D_OK);
    EXPECT(mri3d_copy_channels(nullptr, nullptr, 10, 4, 4, 4, 0, nullptr) != MRI3D_OK);
    EXPECT(mri3d_adam_step(nullptr, nullptr, nullptr, nullptr, 10, 1e-3f, 0.9f, 0.999f, 1e-8f, 0.01f, 1, 1.0f, 1, nullptr) != MRI3D_OK);
    {   // patch windows are validated on the host: out-of-volume origins must be refused, long lists must not overrun anything
        std::vector<int32_t> loc(3 * 200, 0);
        loc[3 * 150 + 1] = 1000;   // h origin outside the volume
        EXPECT(mri3d_extract_patches(P, 4, 1, 64, 64, 64, loc.data(), 200, 32, 32, 32, P, nullptr) != MRI3D_OK);
    }
    {   // fused autoencoder operators (round 3): predicates, workspace sizes and every refusal are host-side
        Mri3dConvGeom up;
        memset(&up, 0, sizeof(up));
        up.n = 4; up.di = 160; up.hi = 192; up.wi = 160; up.ci = 8; up.dout = 160; up.ho = 192; up.wo = 160; up.co = 1;
        up.kd = 3; up.kh = 1; up.kw = 1; up.sd = up.sh = up.sw = 1; up.pd = 1; up.dd = up.dh = up.dw = 1; up.x_ld = 8; up.y_ld = 1;
        EXPECT(mri3d_upconv3d_supported(&up, 4) == 1 && mri3d_upconv3d_supported(&up, 2) == 1 && mri3d_upconv3d_supported(&up, 3) == 0);
        EXPECT(mri3d_upconv3d_supported(nullptr, 4) == 0 && mri3d_upconv3d_workspace_bytes(nullptr, 4) == 0);
        EXPECT(mri3d_upconv3d_workspace_bytes(&up, 4) > 0);
        EXPECT(mri3d_upconv3d_fwd(&up, 4, nullptr, (const float*)P, nullptr, P, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_upconv3d_fwd(&up, 3, P, (const float*)P, nullptr, P, nullptr) == MRI3D_ENOTSUP);
        EXPECT(mri3d_upconv3d_dgrad(&up, 4, P, nullptr, P, nullptr) == MRI3D_EINVAL);
        std::vector<float> b3(64);
        float* q = b3.data();
        EXPECT(mri3d_upconv3d_fwd(&up, 4, q + 1, q, nullptr, q, nullptr) == MRI3D_EINVAL);                 // x off four channels
        EXPECT(mri3d_upconv3d_wgrad(&up, 4, q, q, q, q, q, 16, nullptr) == MRI3D_EINVAL);                   // workspace too small
        Mri3dConvGeom bad2 = up;
        bad2.sd = 2;
        EXPECT(mri3d_upconv3d_supported(&bad2, 4) == 0);                                                    // strided convolution
        bad2 = up; bad2.ci = 16; bad2.co = 8; bad2.x_ld = 16; bad2.y_ld = 8;
        EXPECT(mri3d_upconv3d_supported(&bad2, 4) == 0);                                                    // no (16, 8, 3) instance
        Mri3dConvGeom first, second;
        memset(&first, 0, sizeof(first));
        first.n = 4; first.di = 160; first.hi = 192; first.wi = 160; first.ci = 1; first.dout = 80; first.ho = 192; first.wo = 160; first.co = 8;
        first.kd = 6; first.kh = 1; first.kw = 1; first.sd = 2; first.sh = first.sw = 1; first.pd = 2; first.dd = first.dh = first.dw = 1;
        first.x_ld = 1; first.y_ld = 8;
        second = first;
        second.di = 80; second.ci = 8; second.dout = 80; second.ho = 96; second.kd = 1; second.kh = 6; second.sd = 1; second.sh = 2;
        second.pd = 0; second.ph = 2; second.x_ld = 8; second.y_ld = 8;
        EXPECT(mri3d_convpair_supported(&first, &second) == 1 && mri3d_convpair_supported(&second, &first) == 0);
        EXPECT(mri3d_convpair_supported(nullptr, &second) == 0 && mri3d_convpair_workspace_bytes(&first, nullptr) == 0);
        EXPECT(mri3d_convpair_workspace_bytes(&first, &second) > 0);
        EXPECT(mri3d_convpair_wgrad_first(&first, &second, nullptr, P, (const float*)P, (float*)P, nullptr, P, 0, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_convpair_wgrad_first(&second, &first, P, P, (const float*)P, (float*)P, nullptr, P, 0, nullptr) == MRI3D_ENOTSUP);
        EXPECT(mri3d_convpair_wgrad_first(&first, &second, q, q, q, q, nullptr, q, 16, nullptr) == MRI3D_EINVAL);   // workspace too small
        Mri3dConvGeom s3 = second;
        s3.sh = 1; s3.ho = 191;   // six taps at stride 1 reach a row through six taps: more than the kernel's three slots
        EXPECT(mri3d_convpair_supported(&first, &s3) == 0);
        // the plan queries: the entry points' checks, then the plan functions they launch by
        Mri3dFusedConvPlanInfo fi;
        for (int pass = 0; pass < 3; ++pass)
            for (int scale : {2, 4}) {
                EXPECT(mri3d_upconv3d_plan_query(&up, scale, pass, &fi) == MRI3D_OK && fi.grid > 0 && fi.gtrips > 0);
                Mri3dConvGeom thin = up;
                thin.hi = thin.ho = 4; thin.wi = thin.wo = 1028;
                EXPECT(mri3d_upconv3d_plan_query(&thin, scale, pass, &fi) == MRI3D_OK && (pass == MRI3D_PASS_DGRAD || (fi.hch == 1 && fi.trips == 5)));
            }
        EXPECT(mri3d_upconv3d_plan_query(&up, 3, 0, &fi) == MRI3D_ENOTSUP && mri3d_upconv3d_plan_query(&bad2, 4, 0, &fi) == MRI3D_ENOTSUP);
        EXPECT(mri3d_upconv3d_plan_query(&up, 4, 3, &fi) == MRI3D_EINVAL && mri3d_upconv3d_plan_query(nullptr, 4, 0, &fi) == MRI3D_EINVAL);
        EXPECT(mri3d_upconv3d_plan_query(&up, 4, 0, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_convpair_plan_query(&first, &second, &fi) == MRI3D_OK && fi.rows == 4 * 80 * 192 && fi.grid == 1024 && fi.chunks == 3);
        EXPECT(mri3d_convpair_plan_query(&first, &s3, &fi) == MRI3D_ENOTSUP && mri3d_convpair_plan_query(nullptr, &second, &fi) == MRI3D_EINVAL);
        EXPECT(mri3d_convpair_plan_query(&first, &second, nullptr) == MRI3D_EINVAL);
    }
    {   // norm + activation and its two folds (pointwise head, max pool): every refusal below comes before a launch
        Mri3dNormGeom ng;
        memset(&ng, 0, sizeof(ng));
        ng.n = 2; ng.vox = (int64_t)16 * 16 * 16; ng.c = 16; ng.x_ld = 16; ng.y_ld = 16; ng.act = MRI3D_ACT_PRELU; ng.alpha_n = 1;
        ng.eps = 1e-5f; ng.dtype = MRI3D_F32;
        Mri3dNormGeom nbad = ng;
        nbad.alpha_n = 3;                                   // neither 1 nor c: refused by every predicate and entry point
        float* F = (float*)A;                               // aligned to 4 elements, never dereferenced
        void* odd = A + 4;                                  // off a 4-element boundary
        const size_t big = (size_t)1 << 30;

        // plain backward
        EXPECT(mri3d_norm_act_bwd(nullptr, 0, A, A, nullptr, nullptr, nullptr, nullptr, F, A, nullptr, nullptr, nullptr, A, big, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_norm_act_bwd(&nbad, 0, A, A, nullptr, nullptr, nullptr, nullptr, F, A, nullptr, nullptr, nullptr, A, big, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_norm_act_bwd(&ng, 0, A, A, nullptr, nullptr, nullptr, nullptr, F, nullptr, nullptr, nullptr, nullptr, A, big, nullptr) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_bwd: null pointer") != nullptr);
        EXPECT(mri3d_norm_act_bwd(&ng, 0, A, A, F, nullptr, nullptr, nullptr, F, A, nullptr, nullptr, nullptr, A, big, nullptr) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_bwd: mean/invstd must both be set") != nullptr);
        EXPECT(mri3d_norm_act_bwd(&ng, 1, A, A, nullptr, nullptr, nullptr, nullptr, F, A, nullptr, nullptr, nullptr, A, big, nullptr) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_bwd: training mode needs statistics") != nullptr);
        EXPECT(mri3d_norm_act_bwd(&ng, 0, A, A, nullptr, nullptr, nullptr, nullptr, nullptr, A, nullptr, nullptr, nullptr, A, big, nullptr) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_bwd: PReLU needs alpha") != nullptr);
        EXPECT(mri3d_norm_act_bwd(&ng, 0, A, A, nullptr, nullptr, nullptr, nullptr, F, A, nullptr, nullptr, nullptr, A, 16, nullptr) == MRI3D_EWORKSPACE);
        EXPECT(mri3d_norm_act_bwd(&ng, 0, A, A, nullptr, nullptr, nullptr, nullptr, F, A, nullptr, nullptr, nullptr, nullptr, big, nullptr) == MRI3D_EWORKSPACE);

        // plan query: refusals, then the sweep that contains every geometry of tests/norm_cases.py (channel counts, pitches,
        // alignments, statistics groups and the voxel counts at which the block count changes class), with the plan's invariants
        {
            Mri3dNormPlanInfo info;
            EXPECT(mri3d_norm_plan_query(nullptr, MRI3D_NORM_PASS_FWD, 16, &info) == MRI3D_EINVAL);
            EXPECT(mri3d_norm_plan_query(&nbad, MRI3D_NORM_PASS_FWD, 16, &info) == MRI3D_EINVAL);
            EXPECT(mri3d_norm_plan_query(&ng, MRI3D_NORM_PASS_FWD, 16, nullptr) == MRI3D_EINVAL);
            EXPECT(mri3d_norm_plan_query(&ng, 3, 16, &info) == MRI3D_EINVAL);
            EXPECT(mri3d_norm_plan_query(&ng, MRI3D_NORM_PASS_BWD, 12, &info) == MRI3D_EINVAL);
            EXPECT(mri3d_norm_plan_query(&ng, MRI3D_NORM_PASS_BWD, 0, &info) == MRI3D_EINVAL);
            long plans = 0;
            const int extra_c[] = {128, 256, 260, 1024, 1028};
            for (int ci = 1; ci <= 75; ++ci) {
                const int c = ci <= 70 ? ci : extra_c[ci - 71];
                for (int pad = 0; pad < 10; ++pad)
                    for (int groups : {1, 3, 40, 1030})
                        for (int dt = 0; dt < 2; ++dt)
                            for (int al : {2, 4, 8, 16})
                                for (int pass = 0; pass < 3; ++pass) {
                                    Mri3dNormGeom q;
                                    memset(&q, 0, sizeof(q));
                                    q.n = groups; q.instance = groups > 1; q.c = c; q.x_ld = c + pad; q.y_ld = c + pad; q.alpha_n = 1;
                                    q.eps = 1e-5f; q.dtype = dt; q.vox = 1;
                                    EXPECT(mri3d_norm_plan_query(&q, pass, al, &info) == MRI3D_OK);
                                    const int64_t row = (int64_t)8 * info.VT;
                                    int64_t cap = 1024 / ((int64_t)info.groups * info.cy);
                                    if (cap < 1) cap = 1;
                                    for (int64_t gv : {(int64_t)1, row, row + 1, row * cap - 1, row * cap, row * cap + 1}) {
                                        if (gv < 1) continue;
                                        q.vox = gv;
                                        EXPECT(mri3d_norm_plan_query(&q, pass, al, &info) == MRI3D_OK);
                                        EXPECT(info.CL * info.VT <= 256 && info.CL >= 1 && info.VT >= 1 && info.nblk >= 1);
                                        EXPECT((int64_t)info.cy * info.CL * info.vec >= c && c % info.vec == 0);
                                        EXPECT(info.groups == groups && info.gvox == gv);
                                        const size_t need = (size_t)info.groups * info.nblk * c * 3 * 8 + (size_t)info.groups * c * 3 * 4;
                                        EXPECT(need <= mri3d_norm_workspace_bytes(&q));
                                        ++plans;
                                    }
                                }
            }
            EXPECT(plans > 100000);
        }

        // pointwise head: co = 2
        ng.y_ld = 2; nbad.y_ld = 2;
        EXPECT(mri3d_norm_act_pw_supported(&ng, 2) == 1 && mri3d_norm_act_pw_supported(&nbad, 2) == 0 && mri3d_norm_act_pw_supported(&ng, 5) == 0);
        EXPECT(mri3d_norm_act_pw_supported(nullptr, 2) == 0 && mri3d_norm_act_pw_workspace_bytes(nullptr, 2) == 0);
        const size_t pw_need = mri3d_norm_act_pw_workspace_bytes(&ng, 2);
        EXPECT(pw_need > 0 && pw_need % 8 == 0 && mri3d_norm_act_pw_workspace_bytes(&nbad, 2) == 0);
        EXPECT(mri3d_norm_act_pw_fwd(nullptr, 2, A, nullptr, nullptr, nullptr, nullptr, F, F, nullptr, A, nullptr) == MRI3D_EINVAL);
        EXPECT(mri3d_norm_act_pw_fwd(&nbad, 2, A, nullptr, nullptr, nullptr, nullptr, F, F, nullptr, A, nullptr) == MRI3D_ENOTSUP);
        EXPECT(mri3d_norm_act_pw_fwd(&ng, 2, nullptr, nullptr, nullptr, nullptr, nullptr, F, F, nullptr, A, nullptr) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_pw_fwd: null pointer") != nullptr);
        EXPECT(mri3d_norm_act_pw_fwd(&ng, 2, A, F, nullptr, nullptr, nullptr, F, F, nullptr, A, nullptr) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_pw_fwd: mean/invstd must both be set") != nullptr);
        EXPECT(mri3d_norm_act_pw_fwd(&ng, 2, A, nullptr, nullptr, nullptr, nullptr, nullptr, F, nullptr, A, nullptr) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_pw_fwd: PReLU needs alpha") != nullptr);
        EXPECT(mri3d_norm_act_pw_fwd(&ng, 2, odd, nullptr, nullptr, nullptr, nullptr, F, F, nullptr, A, nullptr) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "aligned") != nullptr);
        auto pw_bwd = [&](const Mri3dNormGeom* gp, int training, const void* x, const float* mean, const float* alpha, void* dx, void* ws,
                          size_t ws_bytes) {
            return mri3d_norm_act_pw_bwd(gp, 2, training, x, A, mean, nullptr, nullptr, nullptr, alpha, F, dx, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, ws, ws_bytes, nullptr);
        };
        EXPECT(pw_bwd(nullptr, 0, A, nullptr, F, A, A, big) == MRI3D_EINVAL);
        EXPECT(pw_bwd(&nbad, 0, A, nullptr, F, A, A, big) == MRI3D_ENOTSUP);
        EXPECT(pw_bwd(&ng, 0, nullptr, nullptr, F, A, A, big) == MRI3D_EINVAL);
        EXPECT(pw_bwd(&ng, 0, A, F, F, A, A, big) == MRI3D_EINVAL);                 // mean without invstd
        EXPECT(pw_bwd(&ng, 1, A, nullptr, F, A, A, big) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_pw_bwd: training mode needs statistics") != nullptr);
        EXPECT(pw_bwd(&ng, 0, A, nullptr, nullptr, A, A, big) == MRI3D_EINVAL);     // PReLU without alpha
        EXPECT(pw_bwd(&ng, 0, A, nullptr, F, odd, A, big) == MRI3D_EINVAL);         // dx off four elements
        EXPECT(pw_bwd(&ng, 0, A, nullptr, F, A, A, pw_need - 1) == MRI3D_EWORKSPACE);
        EXPECT(pw_bwd(&ng, 0, A, nullptr, F, A, A + 4, big) == MRI3D_EWORKSPACE);   // workspace off eight bytes
        EXPECT(pw_bwd(&ng, 0, A, nullptr, F, A, nullptr, big) == MRI3D_EWORKSPACE);

        // max-pool tail: 16^3 -> 8^3
        ng.y_ld = 16; nbad.y_ld = 16;
        Mri3dPoolGeom pl;
        memset(&pl, 0, sizeof(pl));
        pl.n = 2; pl.di = pl.hi = pl.wi = 16; pl.dout = pl.ho = pl.wo = 8; pl.c = 16; pl.kd = pl.kh = pl.kw = 2; pl.sd = pl.sh = pl.sw = 2;
        pl.x_ld = 16; pl.y_ld = 16; pl.dtype = MRI3D_F32;
        Mri3dPoolGeom pbad = pl;
        pbad.kd = 3;
        uint8_t* I = (uint8_t*)A;
        EXPECT(mri3d_norm_act_pool_supported(&ng, &pl) == 1 && mri3d_norm_act_pool_supported(&nbad, &pl) == 0 &&
               mri3d_norm_act_pool_supported(&ng, &pbad) == 0);
        EXPECT(mri3d_norm_act_pool_supported(nullptr, &pl) == 0 && mri3d_norm_act_pool_supported(&ng, nullptr) == 0);
        EXPECT(mri3d_norm_act_pool_workspace_bytes(nullptr, &pl) == 0 && mri3d_norm_act_pool_workspace_bytes(&ng, nullptr) == 0 &&
               mri3d_norm_act_pool_workspace_bytes(&ng, &pbad) == 0);
        const size_t pool_need = mri3d_norm_act_pool_workspace_bytes(&ng, &pl);
        EXPECT(pool_need > 0 && pool_need % 8 == 0 && pool_need < pw_need);         // no side partials
        auto pool_fwd = [&](const Mri3dNormGeom* gp, const Mri3dPoolGeom* pp, const void* x, const float* mean, const float* alpha,
                            uint8_t* idx) {
            return mri3d_norm_act_pool_fwd(gp, pp, x, mean, nullptr, nullptr, nullptr, alpha, A, A, idx, nullptr);
        };
        EXPECT(pool_fwd(nullptr, &pl, A, nullptr, F, I) == MRI3D_EINVAL && pool_fwd(&ng, nullptr, A, nullptr, F, I) == MRI3D_EINVAL);
        EXPECT(pool_fwd(&nbad, &pl, A, nullptr, F, I) == MRI3D_ENOTSUP && pool_fwd(&ng, &pbad, A, nullptr, F, I) == MRI3D_ENOTSUP);
        EXPECT(pool_fwd(&ng, &pl, nullptr, nullptr, F, I) == MRI3D_EINVAL && pool_fwd(&ng, &pl, A, nullptr, F, nullptr) == MRI3D_EINVAL);
        EXPECT(pool_fwd(&ng, &pl, A, F, F, I) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_pool_fwd: mean/invstd must both be set") != nullptr);
        EXPECT(pool_fwd(&ng, &pl, A, nullptr, nullptr, I) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_pool_fwd: PReLU needs alpha") != nullptr);
        EXPECT(pool_fwd(&ng, &pl, odd, nullptr, F, I) == MRI3D_EINVAL && pool_fwd(&ng, &pl, A, nullptr, F, I + 1) == MRI3D_EINVAL);
        auto pool_bwd = [&](const Mri3dNormGeom* gp, const Mri3dPoolGeom* pp, int training, const void* x, const void* dskip,
                            const uint8_t* idx, const float* mean, const float* alpha, void* ws, size_t ws_bytes) {
            return mri3d_norm_act_pool_bwd(gp, pp, training, x, dskip, A, idx, mean, nullptr, nullptr, nullptr, alpha, A, nullptr, nullptr,
                                           nullptr, ws, ws_bytes, nullptr);
        };
        EXPECT(pool_bwd(nullptr, &pl, 0, A, A, I, nullptr, F, A, big) == MRI3D_EINVAL && pool_bwd(&ng, nullptr, 0, A, A, I, nullptr, F, A, big) == MRI3D_EINVAL);
        EXPECT(pool_bwd(&nbad, &pl, 0, A, A, I, nullptr, F, A, big) == MRI3D_ENOTSUP && pool_bwd(&ng, &pbad, 0, A, A, I, nullptr, F, A, big) == MRI3D_ENOTSUP);
        EXPECT(pool_bwd(&ng, &pl, 0, nullptr, A, I, nullptr, F, A, big) == MRI3D_EINVAL);
        EXPECT(pool_bwd(&ng, &pl, 0, A, A, nullptr, nullptr, F, A, big) == MRI3D_EINVAL);       // dpool without the index bytes
        EXPECT(pool_bwd(&ng, &pl, 0, A, A, I, F, F, A, big) == MRI3D_EINVAL);                   // mean without invstd
        EXPECT(pool_bwd(&ng, &pl, 1, A, A, I, nullptr, F, A, big) == MRI3D_EINVAL);
        EXPECT(strstr(mri3d_last_error(), "norm_act_pool_bwd: training mode needs statistics") != nullptr);
        EXPECT(pool_bwd(&ng, &pl, 0, A, A, I, nullptr, nullptr, A, big) == MRI3D_EINVAL);       // PReLU without alpha
        EXPECT(pool_bwd(&ng, &pl, 0, A, odd, I, nullptr, F, A, big) == MRI3D_EINVAL);           // dskip off four elements
        EXPECT(pool_bwd(&ng, &pl, 0, A, A, I, nullptr, F, A, pool_need - 1) == MRI3D_EWORKSPACE);
        EXPECT(pool_bwd(&ng, &pl, 1, A, A, I, nullptr, F, A, pool_need - 1) == MRI3D_EINVAL);   // the arguments are checked first
        EXPECT(pool_bwd(&ng, &pl, 0, A, A, I, nullptr, F, A + 4, big) == MRI3D_EWORKSPACE);     // workspace off eight bytes
        EXPECT(pool_bwd(&ng, &pl, 0, A, A, I, nullptr, F, nullptr, big) == MRI3D_EWORKSPACE);
    }
    if (g_fail) {
        fprintf(stderr, "%d host checks failed\n", g_fail);
        return 1;
    }
    printf("host sanitizer driver: %zu workspace queries and the validation branches ran clean\n", checked);
    return 0;
}
