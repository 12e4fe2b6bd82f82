// components.hip — connected components of a uint8 volume on the device: labels numbered as scipy.ndimage.label numbers them,
// per-component statistics, and mask selection by component.  Everything is integer, so every result is the same
// bits on every run.
//
// Labelling, six launches over one int32 `parent` array of the volume's size (background voxels hold -1):
//   1. cc_local_kernel     one workgroup per 8x8x32 tile: union-find in LDS over the tile's own voxels; every foreground voxel gets
//                          the GLOBAL linear index of its tile-local root, the smallest index of its set.
//   2. cc_merge_kernel     every voxel looks at its backward neighbours (the 3 / 9 / 13 offsets that precede it in C order) that
//                          lie in ANOTHER tile and unions across the boundary on `parent` with atomicMin.
//   3. cc_roots_kernel     every voxel finds its root and writes it to `labels`; each block of kCcChunk voxels counts its roots
//                          (parent[i] == i).
//   4. cc_scan_kernel      one workgroup: exclusive scan of the block counts; the total is the component count.
//   5. cc_rank_kernel      a root's number is 1 + the count of roots at smaller indices: the roots are the minima of their
//                          components, so index order IS first-voxel order, scipy's numbering.  Written over `parent`.
//   6. cc_relabel_kernel   labels[i] = rank[root of i].
//
// Why no loop here can spin (no kernel waits for another workgroup: no flag, no ticket, no barrier across workgroups):
//   * parent[i] <= i at all times: it starts at a set's minimum and only atomicMin lowers it.  find() therefore walks a strictly
//     decreasing chain and ends at an index whose parent is itself.
//   * unite(): after find() of both sides, the larger root a is pointed at the smaller b with old = atomicMin(&parent[a], b).
//     old == a: the link is made.  Otherwise old < a, and the loop goes on with (old, b): max(a, b) strictly decreases every turn.
//   * launch 2 reads `parent` while other workgroups change it.  Every value parent[i] ever holds is an ancestor of i in i's set,
//     so a stale value (another XCD's L2 or this CU's L1) still names a member of the right set that is <= i; what decides is the
//     atomicMin, which acts on memory and returns the true old value, so a stale read costs a turn and never a wrong link.  The
//     reads are agent-scope relaxed atomic loads all the same, so that the chain walked is as fresh as the hardware gives.
//   * launches 3-6 only read what an earlier launch wrote, or write what no other thread of the launch reads.
#include "common.h"

namespace mri3d {

constexpr int kCcTd = 8, kCcTh = 8, kCcTw = 32;              // tile extents (powers of two: the merge kernel shifts)
constexpr int kCcTdLog = 3, kCcThLog = 3, kCcTwLog = 5;
constexpr int kCcTile = kCcTd * kCcTh * kCcTw;               // 2048 voxels
constexpr int kCcThreads = 256;
constexpr int kCcPer = kCcTile / kCcThreads;                 // voxels per thread in the tile kernel
constexpr int kCcChunk = 2048;                               // voxels per block in the root count / rank launches
constexpr int kCcChunkPer = kCcChunk / kCcThreads;
constexpr int kCcScanThreads = 1024;
constexpr int kCcLdsBytes = kCcTile * (int)sizeof(int) + kCcTile;

// backward neighbour k of 13: (dz, dy, dx) lexicographically before (0, 0, 0), ordered by the number of non-zero coordinates, so
// that the 6-, 18- and 26-neighbourhoods are the first 3, 9 and 13
__device__ __constant__ signed char kCcOff[13][3] = {
    {-1, 0, 0}, {0, -1, 0}, {0, 0, -1},
    {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1}, {-1, 0, 1}, {0, -1, -1}, {0, -1, 1},
    {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

__device__ __forceinline__ int cc_lds_find(int* lp, int i) {
    for (;;) {
        const int p = __hip_atomic_load(&lp[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == i) return i;
        i = p;   // p < i
    }
}

__device__ __forceinline__ void cc_lds_unite(int* lp, int a, int b) {
    for (;;) {
        a = cc_lds_find(lp, a);
        b = cc_lds_find(lp, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lp[a], b);
        if (old == a) return;
        a = old;   // old < a
    }
}

__device__ __forceinline__ int cc_find(const int* parent, int i) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == i) return i;
        i = p;   // p < i (foreground voxels only: the caller never starts at a background voxel, and no chain reaches one)
    }
}

__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;   // old < a
    }
}

// what two voxels compare: the value itself with by_value, else "non-zero"
__device__ __forceinline__ unsigned cc_key(uint8_t v, int by_value) { return by_value ? (unsigned)v : (v ? 1u : 0u); }

__global__ void __launch_bounds__(kCcThreads)
cc_local_kernel(const uint8_t* __restrict__ mask, int* __restrict__ parent, int D, int H, int W, int tiles_h, int tiles_w,
                int noff, int by_value) {
    __shared__ int lp[kCcTile];
    __shared__ uint8_t lv[kCcTile];
    const int tile = blockIdx.x;
    const int tx = tile % tiles_w, ty = (tile / tiles_w) % tiles_h, tz = tile / (tiles_w * tiles_h);
    const int z0 = tz * kCcTd, y0 = ty * kCcTh, x0 = tx * kCcTw;
#pragma unroll
    for (int k = 0; k < kCcPer; ++k) {
        const int l = k * kCcThreads + threadIdx.x;
        const int lx = l & (kCcTw - 1), ly = (l >> kCcTwLog) & (kCcTh - 1), lz = l >> (kCcTwLog + kCcThLog);
        const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
        const bool in = z < D && y < H && x < W;
        lv[l] = in ? (uint8_t)cc_key(mask[((size_t)z * H + y) * W + x], by_value) : (uint8_t)0;
        lp[l] = l;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcPer; ++k) {
        const int l = k * kCcThreads + threadIdx.x;
        const uint8_t v = lv[l];
        if (v == 0) continue;
        const int lx = l & (kCcTw - 1), ly = (l >> kCcTwLog) & (kCcTh - 1), lz = l >> (kCcTwLog + kCcThLog);
        for (int o = 0; o < noff; ++o) {
            const int nz = lz + kCcOff[o][0], ny = ly + kCcOff[o][1], nx = lx + kCcOff[o][2];
            if ((unsigned)nz >= (unsigned)kCcTd || (unsigned)ny >= (unsigned)kCcTh || (unsigned)nx >= (unsigned)kCcTw) continue;
            const int nl = (nz * kCcTh + ny) * kCcTw + nx;   // a voxel outside the volume holds 0 and matches nothing
            if (lv[nl] == v) cc_lds_unite(lp, l, nl);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcPer; ++k) {
        const int l = k * kCcThreads + threadIdx.x;
        const int lx = l & (kCcTw - 1), ly = (l >> kCcTwLog) & (kCcTh - 1), lz = l >> (kCcTwLog + kCcThLog);
        const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
        if (z >= D || y >= H || x >= W) continue;
        int g = -1;
        if (lv[l]) {
            const int r = cc_lds_find(lp, l);   // local order is C order inside a tile: the local minimum is the global one
            const int rx = r & (kCcTw - 1), ry = (r >> kCcTwLog) & (kCcTh - 1), rz = r >> (kCcTwLog + kCcThLog);
            g = ((z0 + rz) * H + (y0 + ry)) * W + (x0 + rx);
        }
        parent[((size_t)z * H + y) * W + x] = g;
    }
}

__global__ void __launch_bounds__(kCcThreads)
cc_merge_kernel(const uint8_t* __restrict__ mask, int* parent, int D, int H, int W, int nvox, int noff, int by_value) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < nvox; p += (long long)gridDim.x * blockDim.x) {
        const int i = (int)p;
        const int x = i % W, t = i / W;
        const int y = t % H, z = t / H;
        unsigned v = 0;   // read only once a neighbour in another tile turns up
        bool have = false;
        for (int o = 0; o < noff; ++o) {
            const int nz = z + kCcOff[o][0], ny = y + kCcOff[o][1], nx = x + kCcOff[o][2];
            if ((unsigned)nz >= (unsigned)D || (unsigned)ny >= (unsigned)H || (unsigned)nx >= (unsigned)W) continue;
            if ((((nz ^ z) >> kCcTdLog) | ((ny ^ y) >> kCcThLog) | ((nx ^ x) >> kCcTwLog)) == 0) continue;   // same tile: launch 1
            if (!have) { v = cc_key(mask[i], by_value); have = true; }
            if (v == 0) break;
            const int ni = (nz * H + ny) * W + nx;
            if (cc_key(mask[ni], by_value) == v) cc_unite(parent, i, ni);
        }
    }
}

// block-wide sum of one int per thread (256 threads); every thread gets the total
__device__ __forceinline__ int cc_block_sum(int v, int* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();   // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(kCcThreads)
cc_roots_kernel(const int* __restrict__ parent, int* __restrict__ labels, int* __restrict__ block_count, int nvox) {
    __shared__ int red[4];
    const int base = blockIdx.x * kCcChunk;   // nvox < 2^31 and base < nvox
    int roots = 0;
#pragma unroll
    for (int k = 0; k < kCcChunkPer; ++k) {
        const long long p = (long long)base + k * kCcThreads + threadIdx.x;
        if (p >= nvox) continue;
        const int i = (int)p;
        const int first = parent[i];
        int r = first;
        if (first >= 0 && first != i) r = cc_find(parent, first);
        labels[i] = r;          // the root's index, -1 for background
        roots += first == i;
    }
    roots = cc_block_sum(roots, red);
    if (threadIdx.x == 0) block_count[blockIdx.x] = roots;
}

// in place: block_count[b] becomes the number of roots in the blocks before b; count[0] = all roots
__global__ void __launch_bounds__(kCcScanThreads)
cc_scan_kernel(int* __restrict__ block_count, int nblk, int* __restrict__ count) {
    __shared__ int wave_tot[kCcScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nblk; base += kCcScanThreads) {
        const int i = base + threadIdx.x;
        const int v = i < nblk ? block_count[i] : 0;
        int inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int u = __shfl_up(inc, off, 64);
            if (lane >= off) inc += u;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < kCcScanThreads / 64; ++q) {
            const int s = wave_tot[q];
            before += q < wave ? s : 0;
            total += s;
        }
        if (i < nblk) block_count[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = carry;
}

// rank[i] = the component number of root i (other entries are not written and never read)
__global__ void __launch_bounds__(kCcThreads)
cc_rank_kernel(const int* __restrict__ labels, const int* __restrict__ block_offset, int* __restrict__ rank, int nvox) {
    __shared__ int wave_tot[4];
    const long long base = (long long)blockIdx.x * kCcChunk + threadIdx.x * kCcChunkPer;   // a thread owns kCcChunkPer consecutive voxels
    bool is_root[kCcChunkPer];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kCcChunkPer; ++k) {
        const long long p = base + k;
        is_root[k] = p < nvox && labels[p < nvox ? p : 0] == (int)p;
        mine += is_root[k];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(inc, off, 64);
        if (lane >= off) inc += u;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int before = block_offset[blockIdx.x] + inc - mine;
    for (int q = 0; q < wave; ++q) before += wave_tot[q];
#pragma unroll
    for (int k = 0; k < kCcChunkPer; ++k)
        if (is_root[k]) rank[base + k] = ++before;
}

__global__ void __launch_bounds__(kCcThreads)
cc_relabel_kernel(int* __restrict__ labels, const int* __restrict__ rank, int nvox) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < nvox; p += (long long)gridDim.x * blockDim.x) {
        const int r = labels[p];
        labels[p] = r < 0 ? 0 : rank[r];
    }
}

// ---------------------------------------------------------------- statistics
// peak is accumulated as a signed integer that orders as the float does (finite scores; -0 orders below +0), so that the maximum is an
// integer atomicMax; cc_stats_finish_kernel turns the keys back into floats
__device__ __forceinline__ int cc_float_key(float f) {
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float cc_key_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__global__ void __launch_bounds__(256)
cc_stats_init_kernel(long long* __restrict__ stats, int* __restrict__ peak_key, int capacity, uint8_t* __restrict__ hit,
                     int capacity_other, int D, int H, int W) {
    const int n = max(capacity, capacity_other);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        if (j < capacity) {
            long long* row = stats + (size_t)j * 8;
            row[0] = 0, row[1] = 0;
            row[2] = D, row[3] = -1, row[4] = H, row[5] = -1, row[6] = W, row[7] = -1;
            if (peak_key) peak_key[j] = cc_float_key(-INFINITY);
        }
        if (hit && j < capacity_other) hit[j] = 0;
    }
}

__device__ __forceinline__ int cc_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int cc_wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int cc_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void cc_stats_add(long long* row, int* peak_key, int id, int cnt, int ov, int zmin, int zmax, int ymin,
                                             int ymax, int xmin, int xmax, int key) {
    atomicAdd(reinterpret_cast<unsigned long long*>(row), (unsigned long long)cnt);
    if (ov) atomicAdd(reinterpret_cast<unsigned long long*>(row + 1), (unsigned long long)ov);
    atomicMin(row + 2, (long long)zmin);
    atomicMax(row + 3, (long long)zmax);
    atomicMin(row + 4, (long long)ymin);
    atomicMax(row + 5, (long long)ymax);
    atomicMin(row + 6, (long long)xmin);
    atomicMax(row + 7, (long long)xmax);
    if (peak_key) atomicMax(peak_key + (id - 1), key);
}

// Reduce before the global atomics (a large component would otherwise send every voxel to one row): a workgroup owns kCcStatChunk
// consecutive voxels and keeps a table of kCcSlots components in LDS (open addressing, kCcProbes probes); a voxel whose id finds a
// slot goes to LDS atomics, one that finds none (a chunk of dust with more ids than slots) straight to the global row, and the
// table is flushed once at the end.  A wave whose 64 voxels all carry one id (the inside of a large component) reduces in
// registers first.  Sums and min / max of integers: neither the order of arrival nor the path taken changes a bit of the result.
constexpr int kCcStatChunk = 4096, kCcSlots = 64, kCcProbes = 4;

struct CcSlots {
    int key[kCcSlots], cnt[kCcSlots], ov[kCcSlots], lo[3][kCcSlots], hi[3][kCcSlots], peak[kCcSlots];
};

__device__ __forceinline__ void cc_stats_put(CcSlots& t, long long* stats, int* peak_key, int id, int cnt, int ov, int zmin, int zmax,
                                             int ymin, int ymax, int xmin, int xmax, int key) {
    int slot = id & (kCcSlots - 1);
    bool found = false;
    for (int probe = 0; probe < kCcProbes && !found; ++probe) {
        const int k = atomicCAS(&t.key[slot], 0, id);   // ids are > 0: 0 marks a free slot
        found = k == 0 || k == id;
        if (!found) slot = (slot + 1) & (kCcSlots - 1);
    }
    if (!found) {
        cc_stats_add(stats + (size_t)(id - 1) * 8, peak_key, id, cnt, ov, zmin, zmax, ymin, ymax, xmin, xmax, key);
        return;
    }
    atomicAdd(&t.cnt[slot], cnt);
    if (ov) atomicAdd(&t.ov[slot], ov);
    atomicMin(&t.lo[0][slot], zmin), atomicMax(&t.hi[0][slot], zmax);
    atomicMin(&t.lo[1][slot], ymin), atomicMax(&t.hi[1][slot], ymax);
    atomicMin(&t.lo[2][slot], xmin), atomicMax(&t.hi[2][slot], xmax);
    atomicMax(&t.peak[slot], key);
}

__global__ void __launch_bounds__(256)
cc_stats_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ other, const float* __restrict__ score,
                const int* __restrict__ other_labels, long long* stats, int* peak_key, uint8_t* hit, int capacity,
                int capacity_other, int H, int W, int nvox) {
    __shared__ CcSlots t;
    if (threadIdx.x < kCcSlots) {
        const int q = threadIdx.x;
        t.key[q] = 0, t.cnt[q] = 0, t.ov[q] = 0, t.peak[q] = (int)0x80000000;
        t.lo[0][q] = t.lo[1][q] = t.lo[2][q] = 0x7fffffff;
        t.hi[0][q] = t.hi[1][q] = t.hi[2][q] = -1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long base = (long long)blockIdx.x * kCcStatChunk;
    for (int k = 0; k < kCcStatChunk / 256; ++k) {
        const long long p = base + k * 256 + threadIdx.x;
        const bool in = p < nvox;
        const int id = in ? labels[p] : 0;
        const bool fg = id > 0;
        if (fg && other_labels) {
            const int j = other_labels[p];
            if (j > 0 && j <= capacity_other) hit[j - 1] = 1;   // every writer stores the same byte
        }
        const bool use = fg && id <= capacity;
        const int i = (int)p;
        const int x = in ? i % W : 0, r = in ? i / W : 0;
        const int y = r % H, z = r / H;
        const int ov = use && other && other[p] ? 1 : 0;
        const int key = use && score ? cc_float_key(score[p]) : (int)0x80000000;
        const int id0 = __shfl(id, 0, 64);
        if (__all(id == id0)) {        // wave-uniform
            if (id0 <= 0 || id0 > capacity) continue;
            const int ovs = cc_wave_sum(ov), zmin = cc_wave_min(z), zmax = cc_wave_max(z), ymin = cc_wave_min(y),
                      ymax = cc_wave_max(y), xmin = cc_wave_min(x), xmax = cc_wave_max(x), kmax = cc_wave_max(key);
            if (lane == 0) cc_stats_put(t, stats, peak_key, id0, 64, ovs, zmin, zmax, ymin, ymax, xmin, xmax, kmax);
        } else if (use) {
            cc_stats_put(t, stats, peak_key, id, 1, ov, z, z, y, y, x, x, key);
        }
    }
    __syncthreads();
    if (threadIdx.x < kCcSlots && t.key[threadIdx.x] != 0) {
        const int q = threadIdx.x, id = t.key[q];
        cc_stats_add(stats + (size_t)(id - 1) * 8, peak_key, id, t.cnt[q], t.ov[q], t.lo[0][q], t.hi[0][q], t.lo[1][q], t.hi[1][q],
                     t.lo[2][q], t.hi[2][q], t.peak[q]);
    }
}

__global__ void __launch_bounds__(256) cc_stats_finish_kernel(int* __restrict__ peak_key, int capacity) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < capacity; j += gridDim.x * blockDim.x)
        reinterpret_cast<float*>(peak_key)[j] = cc_key_float(peak_key[j]);
}

__global__ void __launch_bounds__(256)
cc_select_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ keep, int keep_len, uint8_t* __restrict__ out,
                 long long nvox) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < nvox; p += (long long)gridDim.x * blockDim.x) {
        const int id = labels[p];
        out[p] = (unsigned)id < (unsigned)keep_len ? keep[id] : (uint8_t)0;
    }
}

// connectivity -> number of backward offsets; 0 for anything but 6, 18, 26
static inline int cc_noff(int connectivity) { return connectivity == 6 ? 3 : connectivity == 18 ? 9 : connectivity == 26 ? 13 : 0; }

static inline bool cc_size_ok(int d, int h, int w) { return (int64_t)d * h * w < ((int64_t)1 << 31); }

struct CcPlan {
    int tiles_d, tiles_h, tiles_w, grid_local, grid_stream, scan_blocks;
    size_t ws_bytes;
};

// the one place the launches and the query take their numbers from; the volume is valid and below 2^31 voxels
static inline CcPlan cc_plan(int d, int h, int w) {
    CcPlan p;
    const int64_t n = (int64_t)d * h * w;
    p.tiles_d = cdiv(d, kCcTd), p.tiles_h = cdiv(h, kCcTh), p.tiles_w = cdiv(w, kCcTw);
    p.grid_local = p.tiles_d * p.tiles_h * p.tiles_w;   // at most one tile per voxel
    p.grid_stream = stream_grid(n, kCcThreads);
    p.scan_blocks = (int)cdiv64(n, kCcChunk);
    p.ws_bytes = align_up((size_t)n * sizeof(int), 256) + align_up((size_t)p.scan_blocks * sizeof(int), 256);
    return p;
}

}  // namespace mri3d

using namespace mri3d;

extern "C" size_t mri3d_components_workspace_bytes(int32_t d, int32_t h, int32_t w) {
    if (d <= 0 || h <= 0 || w <= 0 || !cc_size_ok(d, h, w)) return 0;
    return cc_plan(d, h, w).ws_bytes;
}

extern "C" int32_t mri3d_components_plan_query(int32_t d, int32_t h, int32_t w, int32_t connectivity, Mri3dComponentsPlanInfo* out) {
    if (!out || d <= 0 || h <= 0 || w <= 0 || cc_noff(connectivity) == 0) return -1;
    if (!cc_size_ok(d, h, w)) return -2;
    const CcPlan p = cc_plan(d, h, w);
    out->td = kCcTd, out->th = kCcTh, out->tw = kCcTw;
    out->tiles_d = p.tiles_d, out->tiles_h = p.tiles_h, out->tiles_w = p.tiles_w;
    out->grid_local = p.grid_local;
    out->grid_merge = p.grid_stream;
    out->grid_roots = p.scan_blocks;
    out->grid_scan = 1;
    out->grid_rank = p.scan_blocks;
    out->grid_relabel = p.grid_stream;
    out->scan_blocks = p.scan_blocks;
    out->offsets = cc_noff(connectivity);
    out->lds_bytes = kCcLdsBytes;
    out->ws_bytes = (int64_t)p.ws_bytes;
    return 0;
}

extern "C" int mri3d_components_label(const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t connectivity, int32_t by_value,
                                      int32_t* labels, int32_t* count, void* workspace, size_t ws_bytes, mri3d_stream_t stream) {
    MRI3D_REQUIRE(mask && labels && count && d > 0 && h > 0 && w > 0, MRI3D_EINVAL, "components_label: bad arguments");
    const int noff = cc_noff(connectivity);
    MRI3D_REQUIRE(noff != 0, MRI3D_EINVAL, "components_label: connectivity %d is not 6, 18 or 26", (int)connectivity);
    MRI3D_REQUIRE(cc_size_ok(d, h, w), MRI3D_ENOTSUP, "components_label: volume too large");
    const CcPlan p = cc_plan(d, h, w);
    MRI3D_REQUIRE(workspace && ws_bytes >= p.ws_bytes && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0, MRI3D_EWORKSPACE,
                  "components_label: workspace %zu < %zu, or not 4-byte aligned", ws_bytes, p.ws_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nvox = d * h * w;
    int* parent = static_cast<int*>(workspace);
    int* block_count = reinterpret_cast<int*>(static_cast<char*>(workspace) + align_up((size_t)nvox * sizeof(int), 256));
    const int bv = by_value ? 1 : 0;
    hipLaunchKernelGGL(cc_local_kernel, dim3(p.grid_local), dim3(kCcThreads), 0, s, mask, parent, d, h, w, p.tiles_h, p.tiles_w, noff, bv);
    hipLaunchKernelGGL(cc_merge_kernel, dim3(p.grid_stream), dim3(kCcThreads), 0, s, mask, parent, d, h, w, nvox, noff, bv);
    hipLaunchKernelGGL(cc_roots_kernel, dim3(p.scan_blocks), dim3(kCcThreads), 0, s, parent, labels, block_count, nvox);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(kCcScanThreads), 0, s, block_count, p.scan_blocks, count);
    hipLaunchKernelGGL(cc_rank_kernel, dim3(p.scan_blocks), dim3(kCcThreads), 0, s, labels, block_count, parent, nvox);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(p.grid_stream), dim3(kCcThreads), 0, s, labels, parent, nvox);
    return check_launch("components_label");
}

extern "C" int mri3d_components_stats(const int32_t* labels, int32_t d, int32_t h, int32_t w, int32_t capacity, const uint8_t* other,
                                      const float* score, int64_t* stats, float* peak, const int32_t* other_labels,
                                      int32_t capacity_other, uint8_t* hit, mri3d_stream_t stream) {
    MRI3D_REQUIRE(labels && stats && capacity > 0 && d > 0 && h > 0 && w > 0, MRI3D_EINVAL, "components_stats: bad arguments");
    MRI3D_REQUIRE((score != nullptr) == (peak != nullptr), MRI3D_EINVAL, "components_stats: score and peak go together");
    MRI3D_REQUIRE(other_labels ? (hit && capacity_other > 0) : (!hit && capacity_other == 0), MRI3D_EINVAL,
                  "components_stats: other_labels, hit and capacity_other go together");
    MRI3D_REQUIRE(cc_size_ok(d, h, w), MRI3D_ENOTSUP, "components_stats: volume too large");
    MRI3D_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0, MRI3D_EINVAL, "components_stats: stats is not 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nvox = d * h * w;
    int* peak_key = reinterpret_cast<int*>(peak);
    const int rows = std::max(capacity, capacity_other);
    hipLaunchKernelGGL(cc_stats_init_kernel, dim3(stream_grid(rows, 256)), dim3(256), 0, s, reinterpret_cast<long long*>(stats), peak_key,
                       capacity, hit, capacity_other, d, h, w);
    hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)cdiv64(nvox, kCcStatChunk)), dim3(256), 0, s, labels, other, score, other_labels,
                       reinterpret_cast<long long*>(stats), peak_key, hit, capacity, capacity_other, h, w, nvox);
    if (peak_key)
        hipLaunchKernelGGL(cc_stats_finish_kernel, dim3(stream_grid(capacity, 256)), dim3(256), 0, s, peak_key, capacity);
    return check_launch("components_stats");
}

extern "C" int mri3d_components_select(const int32_t* labels, int64_t nvox, const uint8_t* keep, int32_t keep_len, uint8_t* out,
                                       mri3d_stream_t stream) {
    MRI3D_REQUIRE(labels && keep && out && nvox > 0 && keep_len > 0, MRI3D_EINVAL, "components_select: bad arguments");
    hipLaunchKernelGGL(cc_select_kernel, dim3(stream_grid(nvox, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), labels, keep,
                       keep_len, out, (long long)nvox);
    return check_launch("components_select");
}
