// detection.hip — the device half of the patch-based FCD detector (reference detection/patch_utils.py, detection/model_utils.py).
// The volume, the grey-matter template and the masks are dense (X, Y, Z) arrays in the reference's axis order, z fastest:
//   A[x, y, z] at (x * Y + y) * Z + z.
// The reference works on slices B = np.rot90(A[:, :, z]), B[r, c] = A[c, Y-1-r, z] (patch_utils.py:21-23), on strips of h rows
// r = row0 .. row0+h-1 (patch_utils.py:25-28, 85-88) and on patches (z, row0, col0) of two channels (patch_utils.py:40-70):
//   channel 0   B[row0+i, col0+t]       = A[col0+t,     Y-1-row0-i, z]
//   channel 1   B[row0+i, X-1-col0-t]   = A[X-1-col0-t, Y-1-row0-i, z]        i < h, t < w
// with col0 = start, X-start-w (the side patches) or mid, X-mid-w (the middle patches), mid = X/2 - w, and start the first column
// of the strip that holds a template value > 0.
//   strip_starts    start of every strip (every z, every row0): lanes walk z, so every load is one contiguous run of the template
//   mirror_patches  the two-channel gather, a pure copy.  A patch row runs along x (stride Y*Z elements), so no load of one patch
//                   coalesces; the patches of one (row0, col0) and neighbouring z read neighbouring elements.  `order` (a
//                   permutation that sorts the table by (row0, col0, z)) makes those patches neighbours in launch order, and the
//                   blocks with the same blockIdx % 8, which share an XCD and its L2, take one contiguous run of it.
//   patch_labels    any mask voxel under channel 0 of a patch, one wave per patch
//   patch_vote      the 4-neighbour vote over the (strip, slice) plane of the patch map (model_utils.py:183-194), integer counts
//   paint_patches   patch map -> voxel mask as a gather: one lane per output voxel, no atomics and no write races
// The patch table lives on the device, so the host cannot check it: an entry that leaves the volume is never dereferenced, its
// patch is written as zeros (the Python builder raises for such an entry before anything is launched).
#include "common.h"

namespace mri3d {

struct VolDims { int X, Y, Z; };

__device__ __forceinline__ bool patch_inside(VolDims d, int z, int row0, int col0, int h, int w) {
    return (unsigned)z < (unsigned)d.Z && row0 >= 0 && row0 <= d.Y - h && col0 >= 0 && col0 <= d.X - w;
}

__global__ void __launch_bounds__(256)
strip_starts_kernel(const float* __restrict__ gm, int* __restrict__ starts, VolDims d, int h, int nrow) {
    const int total = nrow * d.Z;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int z = i % d.Z, row0 = i / d.Z;
        const int ytop = d.Y - 1 - row0;   // row r = row0 + k is y = ytop - k
        int found = -1;
        for (int x = 0; x < d.X && found < 0; ++x) {
            const float* col = gm + ((long long)x * d.Y + (ytop - h + 1)) * d.Z + z;
            bool any = false;
            for (int k = 0; k < h; ++k) any |= col[(long long)k * d.Z] > 0.f;
            if (any) found = x;
        }
        starts[(long long)z * nrow + row0] = found;
    }
}

template <bool CL>
__global__ void __launch_bounds__(256)
mirror_patches_kernel(const float* __restrict__ vol, const int* __restrict__ table, const int* __restrict__ order,
                      float* __restrict__ out, VolDims d, long long P, int h, int w) {
    long long p = blockIdx.x;
    if (order) {
        const long long chunk = (P + 7) / 8;
        const long long q = (long long)(blockIdx.x % 8) * chunk + blockIdx.x / 8;
        if (q >= P) return;
        p = order[q];
        if (p < 0 || p >= P) return;
    }
    const int z = table[3 * p], row0 = table[3 * p + 1], col0 = table[3 * p + 2];
    const bool inside = patch_inside(d, z, row0, col0, h, w);
    const int per = 2 * h * w;
    float* dst = out + p * per;
    for (int e = threadIdx.x; e < per; e += blockDim.x) {
        int c, i, t;
        if (CL) { c = e & 1; t = (e >> 1) % w; i = (e >> 1) / w; }
        else { t = e % w; i = (e / w) % h; c = e / (w * h); }
        float v = 0.f;
        if (inside) {
            const int x = c ? d.X - 1 - col0 - t : col0 + t;
            v = vol[((long long)x * d.Y + (d.Y - 1 - row0 - i)) * d.Z + z];
        }
        dst[e] = v;
    }
}

__global__ void __launch_bounds__(256)
patch_labels_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ table, uint8_t* __restrict__ out, VolDims d,
                    long long P, int h, int w) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per patch
    if (p >= P) return;
    const int z = table[3 * p], row0 = table[3 * p + 1], col0 = table[3 * p + 2];
    int any = 0;
    if (patch_inside(d, z, row0, col0, h, w)) {
        for (int e = lane; e < h * w; e += 64) {
            const int t = e % w, i = e / w;
            any |= mask[((long long)(col0 + t) * d.Y + (d.Y - 1 - row0 - i)) * d.Z + z] != 0;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) any |= __shfl_xor(any, off, 64);
    if (lane == 0) out[p] = (uint8_t)(any != 0);
}

__global__ void __launch_bounds__(256)
patch_vote_kernel(const uint8_t* __restrict__ map, uint8_t* __restrict__ out, int R, int S) {
    const int total = 4 * R * S;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int s = i % S, r = (i / S) % R;
        int count = 0;
        if (r > 0) count += map[i - S] != 0;
        if (r + 1 < R) count += map[i + S] != 0;
        if (s > 0) count += map[i - 1] != 0;
        if (s + 1 < S) count += map[i + 1] != 0;
        out[i] = count == 4 ? (uint8_t)1 : count == 0 ? (uint8_t)0 : map[i];
    }
}

__global__ void __launch_bounds__(256)
paint_patches_kernel(const uint8_t* __restrict__ map, const int* __restrict__ starts, uint8_t* __restrict__ out, VolDims d, int h,
                     int w, int R) {
    const int total = d.X * d.Y * d.Z;   // below 2^31 (checked on the host)
    const int mid = d.X / 2 - w;
    const int plane = R * d.Z;
    for (long long li = blockIdx.x * blockDim.x + threadIdx.x; li < total; li += gridDim.x * blockDim.x) {
        const int i = (int)li;
        const int z = i % d.Z, y = (i / d.Z) % d.Y, x = i / (d.Z * d.Y);
        const int j = (d.Y - 1 - y) / h;
        uint8_t v = 0;
        const int start = j < R ? starts[z * R + j] : -1;
        if (start >= 0) {
            // the reference paints kind 0, 3, 1, 2 in that order (model_utils.py:211-215): the last one that covers the voxel stays
            const int cell = j * d.Z + z;
            int kind = -1;
            if (start < mid) {
                if ((unsigned)(x - start) < (unsigned)w) kind = 0;
                if ((unsigned)(x - (d.X - start - w)) < (unsigned)w) kind = 3;
            }
            if ((unsigned)(x - mid) < (unsigned)w) kind = 1;
            if ((unsigned)(x - (d.X - mid - w)) < (unsigned)w) kind = 2;
            if (kind >= 0) v = map[kind * plane + cell];
        }
        out[i] = v;
    }
}

static int check_volume(const char* who, int X, int Y, int Z, int h, int w, bool need_w) {
    MRI3D_REQUIRE(X > 0 && Y > 0 && Z > 0, MRI3D_EINVAL, "%s: volume %d x %d x %d", who, X, Y, Z);
    MRI3D_REQUIRE(h > 0 && h <= Y, MRI3D_EINVAL, "%s: strip height %d in a slice of %d rows", who, h, Y);
    if (need_w) {
        MRI3D_REQUIRE(w > 0, MRI3D_EINVAL, "%s: patch width %d", who, w);
        MRI3D_REQUIRE(X / 2 - w >= 1, MRI3D_EINVAL, "%s: a patch width of %d leaves no middle patch in %d columns (X/2 - w < 1)", who, w, X);
    }
    MRI3D_REQUIRE((int64_t)X * Y * Z < 0x7fffffffLL, MRI3D_ENOTSUP, "%s: a volume of %lld voxels (int32 indexing)", who,
                  (long long)X * Y * Z);
    return MRI3D_OK;
}

static int check_patches(const char* who, int64_t P, int h, int w) {
    MRI3D_REQUIRE(P > 0, MRI3D_EINVAL, "%s: %lld patches", who, (long long)P);
    MRI3D_REQUIRE((int64_t)2 * h * w < 0x7fffffffLL && P <= 0x7fffffffLL / 4, MRI3D_ENOTSUP, "%s: %lld patches of 2 x %d x %d (int32 indexing)",
                  who, (long long)P, h, w);
    return MRI3D_OK;
}

}  // namespace mri3d

using namespace mri3d;

extern "C" int mri3d_strip_starts_f32(const float* gm, int32_t nx, int32_t ny, int32_t nz, int32_t h, int32_t* starts,
                                      mri3d_stream_t stream) {
    MRI3D_REQUIRE(gm && starts, MRI3D_EINVAL, "strip_starts: null pointer");
    if (int rc = check_volume("strip_starts", nx, ny, nz, h, 0, false)) return rc;
    const int nrow = ny - h + 1;
    hipLaunchKernelGGL(strip_starts_kernel, dim3(stream_grid((int64_t)nrow * nz, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       gm, starts, VolDims{nx, ny, nz}, h, nrow);
    return check_launch("strip_starts");
}

extern "C" int mri3d_mirror_patches_f32(const float* volume, int32_t nx, int32_t ny, int32_t nz, const int32_t* table,
                                        const int32_t* order, int64_t npatch, int32_t h, int32_t w, int32_t channels_last,
                                        float* out, mri3d_stream_t stream) {
    MRI3D_REQUIRE(volume && table && out, MRI3D_EINVAL, "mirror_patches: null pointer");
    MRI3D_REQUIRE(channels_last == 0 || channels_last == 1, MRI3D_EINVAL, "mirror_patches: layout %d (0 NCHW, 1 channels last)", channels_last);
    if (int rc = check_volume("mirror_patches", nx, ny, nz, h, w, true)) return rc;
    if (int rc = check_patches("mirror_patches", npatch, h, w)) return rc;
    const unsigned grid = order ? (unsigned)(8 * cdiv64(npatch, 8)) : (unsigned)npatch;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (channels_last)
        hipLaunchKernelGGL(mirror_patches_kernel<true>, dim3(grid), dim3(256), 0, s, volume, table, order, out, VolDims{nx, ny, nz},
                           (long long)npatch, h, w);
    else
        hipLaunchKernelGGL(mirror_patches_kernel<false>, dim3(grid), dim3(256), 0, s, volume, table, order, out, VolDims{nx, ny, nz},
                           (long long)npatch, h, w);
    return check_launch("mirror_patches");
}

extern "C" int mri3d_mirror_patch_labels_u8(const uint8_t* mask, int32_t nx, int32_t ny, int32_t nz, const int32_t* table,
                                            int64_t npatch, int32_t h, int32_t w, uint8_t* out, mri3d_stream_t stream) {
    MRI3D_REQUIRE(mask && table && out, MRI3D_EINVAL, "mirror_patch_labels: null pointer");
    if (int rc = check_volume("mirror_patch_labels", nx, ny, nz, h, w, true)) return rc;
    if (int rc = check_patches("mirror_patch_labels", npatch, h, w)) return rc;
    hipLaunchKernelGGL(patch_labels_kernel, dim3((unsigned)cdiv64(npatch, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), mask,
                       table, out, VolDims{nx, ny, nz}, (long long)npatch, h, w);
    return check_launch("mirror_patch_labels");
}

extern "C" int mri3d_patch_vote_u8(const uint8_t* map, int32_t strips, int32_t slices, uint8_t* out, mri3d_stream_t stream) {
    MRI3D_REQUIRE(map && out, MRI3D_EINVAL, "patch_vote: null pointer");
    MRI3D_REQUIRE(strips > 0 && slices > 0, MRI3D_EINVAL, "patch_vote: a map of %d strips x %d slices", strips, slices);
    MRI3D_REQUIRE((int64_t)4 * strips * slices < 0x7fffffffLL, MRI3D_ENOTSUP, "patch_vote: a map of 4 x %d x %d cells (int32 indexing)", strips,
                  slices);
    const size_t bytes = (size_t)4 * strips * slices;
    MRI3D_REQUIRE(!overlaps(map, bytes, out, bytes), MRI3D_EINVAL, "patch_vote: every cell is decided from the input map, so the output must not overlap it");
    hipLaunchKernelGGL(patch_vote_kernel, dim3(stream_grid((int64_t)bytes, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), map, out,
                       strips, slices);
    return check_launch("patch_vote");
}

extern "C" int mri3d_paint_patches_u8(const uint8_t* map, const int32_t* starts, int32_t nx, int32_t ny, int32_t nz, int32_t h,
                                      int32_t w, uint8_t* out, mri3d_stream_t stream) {
    MRI3D_REQUIRE(map && starts && out, MRI3D_EINVAL, "paint_patches: null pointer");
    if (int rc = check_volume("paint_patches", nx, ny, nz, h, w, true)) return rc;
    hipLaunchKernelGGL(paint_patches_kernel, dim3(stream_grid((int64_t)nx * ny * nz, 256 * 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), map, starts, out, VolDims{nx, ny, nz}, h, w, ny / h);
    return check_launch("paint_patches");
}
