// Exact connected-component labelling of label volumes on the device, for all frames and classes in one launch sequence, and what stands
// on it: the per-component table (voxel count, bounding box, first voxel), the overlap runs of two labelled volumes and a table gather
// (the reference labels on the host, scipy.ndimage.label in kwatsch/medpy_metrics.py).  include/aesr_hip_components.h states the
// definitions.
//
//   aesr_components_label
//     tile      one workgroup labels a 16 x 64 tile of one slice in LDS: union-find over the in-tile pairs of adjacent voxels of equal
//               class (workgroup-scope atomics only), then parent[p] = global linear index of the tile-local root, the minimum index of
//               p's component within the tile; -1 for a voxel without class.
//     merge     the pairs of adjacent voxels of equal class that lie in different tiles or, with ndim = 3, in consecutive slices:
//               union by atomicMin at device scope (termination and stale reads: the comment at cc_union).
//     flatten   a launch of its own, so plain loads: every voxel follows its chain to the root (parent[r] == r), the root goes to
//               `labels` for now; roots are counted per (unit, class, workgroup).
//     scan      per (unit, class): the exclusive prefix of the root counts in workgroup order and n_components.
//     number    every root gets its raster rank + 1 (workgroup base + waves before it + ballot / mbcnt prefix inside the wave), written
//               over its own parent entry, which nothing reads as a parent any more.
//     assign    labels[p] = number of p's root.
//   aesr_components_tables / apply_table: offsets (exclusive scan of n_components, one workgroup), then integer atomics on rows, or a gather.
//   aesr_components_overlap_count / runs: flag the start of every x-run of equal (unit, class, label A, label B), count per workgroup,
//     scan, pack by raster rank.
// Everything is integer and roots are minimum indices: no result depends on the order in which atomics arrive.
#include "aesr_kernels.h"
#include "aesr_hostcheck.h"
#include "../../include/aesr_hip_components.h"

#define CC_THREADS 256
#define CC_TW 64                                    // tile: 16 rows of 64 voxels, four consecutive voxels of a row per thread
#define CC_TH 16
#define CC_TILE (CC_TW * CC_TH)
#define CC_MAXC AESR_COMPONENTS_MAX_CLASSES
#define CC_COLS AESR_COMPONENTS_COLUMNS
#define CC_SCAN_THREADS 1024
#define CC_WAVES (CC_THREADS / 64)

typedef int i32x4 __attribute__((ext_vector_type(4)));

// byte offsets of the workspace sections, all multiples of 16
struct CcLayout {
    size_t parent, partial, block_off, offs, ov_partial, ov_off, total;
    long long T;
    int nb2, nbT;          // workgroups of 256 voxels: per slice (the larger of the two unit kinds, times N * Z), over the whole array
};

static CcLayout cc_layout(int N, int Z, int H, int W, int C) {
    CcLayout L;
    L.T = (long long)N * Z * H * W;
    L.nb2 = (int)(((long long)H * W + CC_THREADS - 1) / CC_THREADS);
    L.nbT = (int)((L.T + CC_THREADS - 1) / CC_THREADS);
    const size_t per_class = (size_t)N * Z * (size_t)L.nb2;          // >= N * ceil(Z H W / 256), the count with ndim = 3
    size_t o = 0;
    L.parent = o;       o += aesr_up16((size_t)L.T * 4);
    L.partial = o;      o += aesr_up16(per_class * C * 4);
    L.block_off = o;    o += aesr_up16(per_class * C * 4);
    L.offs = o;         o += aesr_up16(((size_t)N * Z * C + 1) * 4);
    L.ov_partial = o;   o += aesr_up16((size_t)L.nbT * 4);
    L.ov_off = o;       o += aesr_up16((size_t)L.nbT * 4);
    L.total = o;
    return L;
}

// ---- union-find ------------------------------------------------------------------------------------------------------------------------
// The same algorithm twice: on a tile's LDS array at workgroup scope, and on parent[] in global memory at agent scope.
//
// Invariant: an entry only ever decreases, and parent[x] <= x (it starts as x or as a smaller index of the same tile, and atomicMin only
// lowers it).  A voxel x is a root while parent[x] == x.
//
// Termination.  find walks x -> parent[x] while they differ: every value ever stored in parent[x] is < x once it differs from x, so the
// chain is strictly decreasing whatever mixture of old and new values the loads return, and it ends at the latest at index 0.  union takes
// the two roots a > b it found and does old = atomicMin(&parent[a], b).  old == a: a was a root and now hangs under b, done.  Otherwise
// somebody lowered parent[a] to old < a in the meantime; the entry now holds min(old, b), so one of the two links a -> old, a -> b is in
// place and the other is restored by continuing with the pair (old, b), which is strictly smaller than (a, b) in its larger member.  The
// sum of the pair decreases with every retry: no waiting on another thread, no spin, the loop ends by itself.
//
// Stale reads.  Per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so a load of parent[x] may return
// a value that another workgroup has since lowered.  Every read in the merge kernel is a relaxed agent-scope atomic load (it bypasses
// L1), every write is the device-scope atomicMin, whose RETURN value is always the true one.  An old value of parent[x] is still a member
// of x's component -- links are only ever replaced together with a union that reconnects the old target -- so a find that ends at a
// former root merely makes the atomicMin report old != a and the loop goes on from the true value; a find that ends at the same index for
// both voxels means they are connected.  No thread reads the RESULT inside this kernel: the flatten pass is a launch of its own, behind
// the kernel boundary, where all of parent[] is visible.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* parent, int a) {
    int pa;
    while ((pa = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, SCOPE)) != a) a = pa;
    return a;
}

template <int SCOPE>
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find<SCOPE>(parent, a);
        b = cc_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

// workgroup (slice s = n * Z + z, tile row ty, tile column tx); thread t the voxels (ty * 16 + t / 16, tx * 64 + 4 (t % 16) ... + 3)
template <bool VEC>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const float* __restrict__ vol, int* __restrict__ parent, AesrClasses cls, int C, int H,
                                                             int W, int txn, int tyn, int diag) {
    __shared__ int lab[CC_TILE];
    __shared__ int kc[CC_TILE];
    unsigned int bid = blockIdx.x;
    const int tx = (int)(bid % (unsigned int)txn);
    bid /= (unsigned int)txn;
    const int ty = (int)(bid % (unsigned int)tyn), s = (int)(bid / (unsigned int)tyn);
    const int ly = (int)threadIdx.x / (CC_TW / 4), lx0 = ((int)threadIdx.x % (CC_TW / 4)) * 4;
    const int y = ty * CC_TH + ly, x0 = tx * CC_TW + lx0;
    const int base = s * H * W;                                   // < N Z H W < 2^31
    const bool row_in = y < H && x0 < W;
    const int g0 = row_in ? base + y * W + x0 : 0;                // only formed inside the array: no overflow past 2^31
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int k[4];
    if (row_in) {
        if (VEC) {          // W % 4 == 0 and x0 % 4 == 0: all four are inside, and g0 % 4 == 0
            const f32x4 q = *reinterpret_cast<const f32x4*>(vol + g0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < W) v[j] = vol[g0 + j];
        }
    }
    const int li0 = ly * CC_TW + lx0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        k[j] = (row_in && x0 + j < W) ? aesr_class_of(v[j], cls, C) : -1;
        kc[li0 + j] = k[j];
        lab[li0 + j] = li0 + j;
    }
    __syncthreads();
    // the backward neighbours inside the tile.  A pair is left out only where the two voxels are connected through pairs that ARE taken:
    // up, when left and up-left have the class too (left - p and up-left - up are row pairs, left - up-left is the same case one voxel
    // earlier); up-left, when up or left has the class; up-right, when up has it.
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (k[j] < 0) continue;
        const int li = li0 + j, lx = lx0 + j;
        const bool left = lx > 0 && kc[li - 1] == k[j];
        if (left) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, li, li - 1);
        if (ly > 0) {
            const bool up = kc[li - CC_TW] == k[j];
            const bool upleft = lx > 0 && kc[li - CC_TW - 1] == k[j];
            if (up && !(left && upleft)) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, li, li - CC_TW);
            if (diag) {
                if (upleft && !up && !left) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, li, li - CC_TW - 1);
                if (!up && lx < CC_TW - 1 && kc[li - CC_TW + 1] == k[j]) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, li, li - CC_TW + 1);
            }
        }
    }
    __syncthreads();
    int out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        out[j] = -1;
        if (k[j] >= 0) {
            const int r = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, li0 + j);          // a voxel with a class: inside the array, so is its root
            out[j] = base + (ty * CC_TH + r / CC_TW) * W + tx * CC_TW + r % CC_TW;
        }
    }
    if (row_in) {
        if (VEC) {
            *reinterpret_cast<i32x4*>(parent + g0) = (i32x4){out[0], out[1], out[2], out[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < W) parent[g0 + j] = out[j];
        }
    }
}

// one thread per voxel p: the backward neighbours q < p of equal class in another tile of the slice, and (zr) in the slice above
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const float* __restrict__ vol, int* parent, AesrClasses cls, int C, int T, int Z, int H,
                                                              int W, int zr, int conn) {
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (gp >= T) return;
    const int p = (int)gp;
    const float v = vol[p];
    if (aesr_class_of(v, cls, C) < 0) return;
    const int x = p % W, y = (p / W) % H, z = (p / (W * H)) % Z;
    const bool xe = x % CC_TW == 0, ye = y % CC_TH == 0;          // p is the first voxel of its tile in x / in y
    const bool diag = conn >= 2;
    if (x > 0 && xe && vol[p - 1] == v) cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, p, p - 1);
    if (y > 0) {
        if (ye && vol[p - W] == v) cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, p, p - W);
        if (diag) {
            if (x > 0 && (xe || ye) && vol[p - W - 1] == v) cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, p, p - W - 1);
            if (x < W - 1 && (ye || (x + 1) % CC_TW == 0) && vol[p - W + 1] == v) cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, p, p - W + 1);
        }
    }
    if (zr && z > 0) {
        const int HW = H * W, a = p - HW;
        const bool above = vol[a] == v;
        // left out where left and above-left have the class too: left - p and above-left - above are pairs of their slices, and
        // left - above-left is this case one voxel earlier
        if (above && !(x > 0 && vol[p - 1] == v && vol[a - 1] == v)) cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, p, a);
        if (diag && !above) {          // with `above` in the class every other neighbour in its slice is adjacent to it there
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int l1 = 1 + (dy != 0) + (dx != 0);
                    if (l1 == 1 || l1 > conn) continue;
                    const int yy = y + dy, xx = x + dx;
                    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                    const int q = a + dy * W + dx;
                    if (vol[q] == v) cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, p, q);
                }
        }
    }
}

// workgroup b of unit u takes the voxels [b * 256, (b + 1) * 256) of that unit, one per thread
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const float* __restrict__ vol, const int* __restrict__ parent, int* __restrict__ labels,
                                                                unsigned int* __restrict__ partial, AesrClasses cls, int C, int Vu, int nb) {
    __shared__ unsigned int red[CC_WAVES][CC_MAXC];
    const int u = blockIdx.x / nb, b = blockIdx.x - u * nb;
    const int idx = b * CC_THREADS + (int)threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int k = -1;
    bool root = false;
    if (idx < Vu) {
        const int p = u * Vu + idx;
        int r = parent[p];
        if (r >= 0) {
            for (int q = parent[r]; q != r; q = parent[r]) r = q;          // strictly decreasing: ends at the root
            root = r == p;
            if (root) k = aesr_class_of(vol[p], cls, C);
        }
        labels[p] = r;
    }
#pragma unroll
    for (int c = 0; c < CC_MAXC; ++c)
        if (c < C) {
            const unsigned int s = (unsigned int)__popcll(__ballot(root && k == c));
            if (lane == 0) red[wave][c] = s;
        }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        unsigned int s = 0;
#pragma unroll
        for (int w = 0; w < CC_WAVES; ++w) s += red[w][threadIdx.x];
        partial[((size_t)u * C + threadIdx.x) * nb + b] = s;
    }
}

// workgroup (u, c): block_off[(u, c)][b] = roots of that class in the workgroups before b, n_components[u][c] = their total
__global__ __launch_bounds__(CC_THREADS) void cc_scan_kernel(const unsigned int* __restrict__ partial, unsigned int* __restrict__ block_off,
                                                             int* __restrict__ n_components, int nb) {
    __shared__ unsigned int sh[CC_THREADS];
    const int per = (nb + CC_THREADS - 1) / CC_THREADS;
    const int b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    const unsigned int* p = partial + (size_t)blockIdx.x * nb;
    unsigned int* o = block_off + (size_t)blockIdx.x * nb;
    unsigned int s = 0;
    for (int b = b0; b < b1; ++b) s += p[b];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int run = 0;
        for (int t = 0; t < CC_THREADS; ++t) {
            const unsigned int v = sh[t];
            sh[t] = run;
            run += v;
        }
        n_components[blockIdx.x] = (int)run;          // at most one root per voxel: < 2^31
    }
    __syncthreads();
    unsigned int run = sh[threadIdx.x];
    for (int b = b0; b < b1; ++b) {
        o[b] = run;
        run += p[b];
    }
}

// same voxel assignment as cc_flatten_kernel; a root (labels[p] == p) writes its number over its parent entry
__global__ __launch_bounds__(CC_THREADS) void cc_number_kernel(const float* __restrict__ vol, const int* __restrict__ labels, int* __restrict__ parent,
                                                               const unsigned int* __restrict__ block_off, AesrClasses cls, int C, int Vu, int nb) {
    __shared__ unsigned int wtot[CC_MAXC][CC_WAVES];
    const int u = blockIdx.x / nb, b = blockIdx.x - u * nb;
    const int idx = b * CC_THREADS + (int)threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = u * Vu + min(idx, Vu - 1);
    int k = -1;
    if (idx < Vu && labels[p] == p) k = aesr_class_of(vol[p], cls, C);
    unsigned int below = 0;
#pragma unroll
    for (int c = 0; c < CC_MAXC; ++c)
        if (c < C) {
            const unsigned long long m = __ballot(k == c);
            if (k == c) below = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
            if (lane == 0) wtot[c][wave] = (unsigned int)__popcll(m);
        }
    __syncthreads();
    if (k >= 0) {
        unsigned int rank = block_off[((size_t)u * C + k) * nb + b] + below;
        for (int w = 0; w < wave; ++w) rank += wtot[k][w];
        parent[p] = (int)rank + 1;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_assign_kernel(int* __restrict__ labels, const int* __restrict__ parent, int T) {
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (gp >= T) return;
    const int r = labels[gp];
    labels[gp] = r < 0 ? 0 : parent[r];
}

// one workgroup: offs[i] = n_components[0] + ... + n_components[i - 1], i = u * C + c; offs[UC] = the total (saturating at 2^31 - 1)
__global__ __launch_bounds__(CC_SCAN_THREADS) void cc_offsets_kernel(const int* __restrict__ n_components, int* __restrict__ offs, int UC) {
    __shared__ long long sh[CC_SCAN_THREADS];
    const int per = (UC + CC_SCAN_THREADS - 1) / CC_SCAN_THREADS;
    const int i0 = min((int)threadIdx.x * per, UC), i1 = min(i0 + per, UC);
    long long s = 0;
    for (int i = i0; i < i1; ++i) s += max(n_components[i], 0);
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int t = 0; t < CC_SCAN_THREADS; ++t) {
            const long long v = sh[t];
            sh[t] = run;
            run += v;
        }
        offs[UC] = (int)min(run, 2147483647LL);
    }
    __syncthreads();
    long long run = sh[threadIdx.x];
    for (int i = i0; i < i1; ++i) {
        offs[i] = (int)min(run, 2147483647LL);
        run += max(n_components[i], 0);
    }
}

// the initial values of the rows: count 0, box minima at the largest value, box maxima 0, first voxel at the largest value
__global__ __launch_bounds__(CC_THREADS) void cc_table_init_kernel(unsigned long long* __restrict__ table, unsigned long long cells) {
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= cells) return;
    const int col = (int)(i % CC_COLS);
    table[i] = (col == 1 || col == 3 || col == 5 || col == 7) ? 0x7fffffffffffffffull : 0ull;
}

// what one thread, then one wave, has gathered for one table row; everything fits an int (indices are below 2^31)
struct CcAcc {
    int row, cnt, z0, z1, y0, y1, x0, x1, first;
};

__device__ __forceinline__ void cc_table_flush(unsigned long long* table, const CcAcc& a) {
    unsigned long long* r = table + (size_t)a.row * CC_COLS;
    atomicAdd(r + 0, (unsigned long long)a.cnt);
    atomicMin(r + 1, (unsigned long long)a.z0);
    atomicMax(r + 2, (unsigned long long)a.z1);
    atomicMin(r + 3, (unsigned long long)a.y0);
    atomicMax(r + 4, (unsigned long long)a.y1);
    atomicMin(r + 5, (unsigned long long)a.x0);
    atomicMax(r + 6, (unsigned long long)a.x1);
    atomicMin(r + 7, (unsigned long long)a.first);
}

// Four consecutive voxels per thread.  Neighbouring voxels mostly belong to one component, and every voxel of a large component would
// otherwise send eight atomics to the same row: a thread merges its voxels of equal row, then a wave merges the lanes that share the
// row of its first active lane (twice at the most: a wave rarely spans more than two large components) by a shuffle reduction, and only
// what is left goes out lane by lane.  Sums, minima and maxima of integers: the order changes nothing.
__global__ __launch_bounds__(CC_THREADS) void cc_table_kernel(const float* __restrict__ vol, const int* __restrict__ labels,
                                                              const int* __restrict__ n_components, const int* __restrict__ offs,
                                                              unsigned long long* table, unsigned long long rows, AesrClasses cls, int C, int T,
                                                              int Z, int H, int W, int Vu) {
    const long long g0 = ((long long)blockIdx.x * CC_THREADS + threadIdx.x) * 4;
    const int lane = threadIdx.x & 63;
    CcAcc acc;
    acc.row = -1;
    acc.cnt = acc.z1 = acc.y1 = acc.x1 = 0;
    acc.z0 = acc.y0 = acc.x0 = acc.first = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long gp = g0 + j;
        int row = -1;
        int p = 0;
        if (gp < T) {
            p = (int)gp;
            const int lab = labels[p];
            const int k = lab > 0 ? aesr_class_of(vol[p], cls, C) : -1;
            if (k >= 0) {
                const int uc = (p / Vu) * C + k;
                const unsigned long long r = (unsigned long long)offs[uc] + (unsigned int)(lab - 1);
                if (lab <= n_components[uc] && r < rows) row = (int)r;          // always true for the counts of this labelling; rows < 2^31
            }
        }
        if (row < 0) continue;
        if (row != acc.row) {
            if (acc.row >= 0) cc_table_flush(table, acc);
            acc.row = row;
            acc.cnt = acc.z1 = acc.y1 = acc.x1 = 0;
            acc.z0 = acc.y0 = acc.x0 = acc.first = 0x7fffffff;
        }
        const int x = p % W, y = (p / W) % H, z = (p / (W * H)) % Z;
        acc.cnt += 1;
        acc.z0 = min(acc.z0, z); acc.z1 = max(acc.z1, z + 1);
        acc.y0 = min(acc.y0, y); acc.y1 = max(acc.y1, y + 1);
        acc.x0 = min(acc.x0, x); acc.x1 = max(acc.x1, x + 1);
        acc.first = min(acc.first, p % (Z * H * W));
    }
    for (int round = 0; round < 2; ++round) {          // every condition below is the same for all lanes of the wave
        const unsigned long long active = __ballot(acc.row >= 0);
        if (active == 0) break;
        const int leader = __ffsll((long long)active) - 1;
        const int lrow = __shfl(acc.row, leader);
        const bool member = acc.row == lrow;
        if (__popcll(__ballot(member)) < 4) break;
        CcAcc w;
        w.row = lrow;
        w.cnt = member ? acc.cnt : 0;
        w.z0 = member ? acc.z0 : 0x7fffffff; w.y0 = member ? acc.y0 : 0x7fffffff; w.x0 = member ? acc.x0 : 0x7fffffff;
        w.first = member ? acc.first : 0x7fffffff;
        w.z1 = member ? acc.z1 : 0; w.y1 = member ? acc.y1 : 0; w.x1 = member ? acc.x1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            w.cnt += __shfl_xor(w.cnt, off);
            w.z0 = min(w.z0, __shfl_xor(w.z0, off)); w.z1 = max(w.z1, __shfl_xor(w.z1, off));
            w.y0 = min(w.y0, __shfl_xor(w.y0, off)); w.y1 = max(w.y1, __shfl_xor(w.y1, off));
            w.x0 = min(w.x0, __shfl_xor(w.x0, off)); w.x1 = max(w.x1, __shfl_xor(w.x1, off));
            w.first = min(w.first, __shfl_xor(w.first, off));
        }
        if (lane == leader) cc_table_flush(table, w);
        if (member) acc.row = -1;
    }
    if (acc.row >= 0) cc_table_flush(table, acc);
}

__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(const float* __restrict__ vol, const int* __restrict__ labels,
                                                              const int* __restrict__ n_components, const int* __restrict__ offs,
                                                              const float* __restrict__ table, unsigned long long table_len, float* __restrict__ out,
                                                              AesrClasses cls, int C, int T, int Vu) {
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (gp >= T) return;
    const int p = (int)gp;
    const int lab = labels[p];
    float o = 0.f;
    if (lab > 0) {
        const int k = aesr_class_of(vol[p], cls, C);
        if (k >= 0) {
            const int uc = (p / Vu) * C + k;
            const unsigned long long row = (unsigned long long)offs[uc] + (unsigned int)(lab - 1);
            if (lab <= n_components[uc] && row < table_len) o = table[row];
        }
    }
    out[p] = o;
}

// true when voxel p starts an x-run of equal (unit, class, label A, label B); k, la, lb are its class index and labels
__device__ __forceinline__ bool cc_run_start(const float* __restrict__ va, const int* __restrict__ la, const float* __restrict__ vb,
                                             const int* __restrict__ lb, int p, int W, const AesrClasses& cls, int C, int& k, int& a, int& b) {
    k = aesr_class_of(va[p], cls, C);
    if (k < 0 || aesr_class_of(vb[p], cls, C) != k) return false;
    a = la[p];
    b = lb[p];
    if (a <= 0 || b <= 0) return false;
    if (p % W == 0) return true;
    const int q = p - 1;          // the same row, so the same unit
    return !(aesr_class_of(va[q], cls, C) == k && aesr_class_of(vb[q], cls, C) == k && la[q] == a && lb[q] == b);
}

__global__ __launch_bounds__(CC_THREADS) void cc_overlap_count_kernel(const float* __restrict__ va, const int* __restrict__ la,
                                                                      const float* __restrict__ vb, const int* __restrict__ lb,
                                                                      unsigned int* __restrict__ partial, AesrClasses cls, int C, int T, int W) {
    __shared__ unsigned int red[CC_WAVES];
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    int k, a, b;
    const bool hit = gp < T && cc_run_start(va, la, vb, lb, (int)gp, W, cls, C, k, a, b);
    const unsigned int s = (unsigned int)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
#pragma unroll
        for (int w = 0; w < CC_WAVES; ++w) t += red[w];
        partial[blockIdx.x] = t;
    }
}

// one workgroup: off[b] = run starts in the workgroups before b, count[0] = their total
__global__ __launch_bounds__(CC_SCAN_THREADS) void cc_overlap_scan_kernel(const unsigned int* __restrict__ partial, unsigned int* __restrict__ off,
                                                                          long long* __restrict__ count, int nb) {
    __shared__ long long sh[CC_SCAN_THREADS];
    const int per = (nb + CC_SCAN_THREADS - 1) / CC_SCAN_THREADS;
    const int b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    long long s = 0;
    for (int b = b0; b < b1; ++b) s += partial[b];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int t = 0; t < CC_SCAN_THREADS; ++t) {
            const long long v = sh[t];
            sh[t] = run;
            run += v;
        }
        count[0] = run;          // at most one per voxel: < 2^31
    }
    __syncthreads();
    unsigned int run = (unsigned int)sh[threadIdx.x];
    for (int b = b0; b < b1; ++b) {
        off[b] = run;
        run += partial[b];
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_overlap_runs_kernel(const float* __restrict__ va, const int* __restrict__ la,
                                                                     const float* __restrict__ vb, const int* __restrict__ lb,
                                                                     const unsigned int* __restrict__ off, int* __restrict__ runs,
                                                                     unsigned long long limit, AesrClasses cls, int C, int T, int W, int Vu) {
    __shared__ unsigned int wtot[CC_WAVES];
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int k = -1, a = 0, b = 0;
    const bool hit = gp < T && cc_run_start(va, la, vb, lb, (int)gp, W, cls, C, k, a, b);
    const unsigned long long m = __ballot(hit);
    const unsigned int below = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (lane == 0) wtot[wave] = (unsigned int)__popcll(m);
    __syncthreads();
    if (hit) {
        unsigned long long at = (unsigned long long)off[blockIdx.x] + below;
        for (int w = 0; w < wave; ++w) at += wtot[w];
        if (at < limit) {          // always true for the count of this workspace
            int* o = runs + at * 4;
            o[0] = (int)(gp / Vu);
            o[1] = k;
            o[2] = a;
            o[3] = b;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
// sizes every entry point and the query share; 0 = fine, else the code with the message set (fn == NULL: silent, for the query)
static int cc_check_sizes(const char* fn, int N, int Z, int H, int W, int C) {
    if (N <= 0 || Z <= 0 || H <= 0 || W <= 0) {
        if (fn) aesr_set_error("%s: N, Z, H, W = %d, %d, %d, %d must all be positive", fn, N, Z, H, W);
        return AESR_ERR_ARG;
    }
    if (C < 1 || C > CC_MAXC) {
        if (fn) aesr_set_error("%s: C=%d classes, 1 to %d are supported", fn, C, CC_MAXC);
        return AESR_ERR_ARG;
    }
    if ((double)N * Z * H * W >= 2147483648.0) {
        if (fn) aesr_set_error("%s: N * Z * H * W = %d x %d x %d x %d has 2^31 voxels or more", fn, N, Z, H, W);
        return AESR_ERR_ARG;
    }
    if ((double)N * Z * C >= 2147483648.0) {          // U * C (unit, class) pairs are counted in an int
        if (fn) aesr_set_error("%s: N * Z * C = %d x %d x %d gives 2^31 (unit, class) pairs or more", fn, N, Z, C);
        return AESR_ERR_ARG;
    }
    return AESR_OK;
}

// ndim and the class ids; fills cls
static int cc_check_classes(const char* fn, const int* classes, int C, int ndim, AesrClasses* cls) {
    AESR_CHECK_ARG(classes, "%s: a null pointer", fn);
    AESR_CHECK_ARG(ndim == 2 || ndim == 3, "%s: ndim=%d, 2 or 3 are supported", fn, ndim);
    return aesr_fill_classes(fn, classes, C, cls);
}

// the host copy of n_components: 0 = fine with *rows = their sum
static int cc_check_counts(const char* fn, const int* host, long long UC, long long Vu, unsigned long long* rows) {
    unsigned long long sum = 0;
    bool many = false;
    for (long long i = 0; i < UC; ++i) {
        AESR_CHECK_ARG(host[i] >= 0 && host[i] <= Vu, "%s: n_components_host[%lld] = %d is not what aesr_components_label wrote for this size", fn,
                       i, host[i]);
        many = many || host[i] > AESR_COMPONENTS_MAX_PER_CLASS;
        sum += (unsigned long long)host[i];
    }
    if (many) {
        aesr_set_error("%s: more than 2^24 components in one (unit, class): their numbers are not exact in fp32", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    *rows = sum;
    return AESR_OK;
}

static inline unsigned int cc_blocks(long long items) { return (unsigned int)((items + CC_THREADS - 1) / CC_THREADS); }

extern "C" {

size_t aesr_components_workspace_bytes(int N, int Z, int H, int W, int C) {
    if (cc_check_sizes(NULL, N, Z, H, W, C) != AESR_OK) return 0;
    return cc_layout(N, Z, H, W, C).total;
}

int aesr_components_label(const float* vol, int* labels, int* n_components, void* workspace, int N, int Z, int H, int W, const int* classes,
                          int C, int ndim, int connectivity, void* stream) {
    const char* fn = "aesr_components_label";
    int rc = cc_check_sizes(fn, N, Z, H, W, C);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(vol && labels && n_components && workspace, "%s: a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)vol % 4 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)n_components % 4 == 0,
                   "%s: vol, labels or n_components is not 4-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace is not 16-byte aligned", fn);
    AesrClasses cls;
    rc = cc_check_classes(fn, classes, C, ndim, &cls);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(connectivity >= 1 && connectivity <= ndim, "%s: connectivity=%d must be in 1 ... ndim = %d", fn, connectivity, ndim);
    const CcLayout L = cc_layout(N, Z, H, W, C);
    const int U = ndim == 2 ? N * Z : N;
    const int Vu = ndim == 2 ? H * W : Z * H * W;
    const AesrBuf bufs[4] = {{vol, (size_t)L.T * 4, false}, {labels, (size_t)L.T * 4, true}, {n_components, (size_t)U * C * 4, true},
                           {workspace, L.total, true}};
    if (aesr_any_overlap(bufs, 4)) {
        aesr_set_error("%s: an output or the workspace overlaps an input or another output", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* parent = (int*)(ws + L.parent);
    unsigned int* partial = (unsigned int*)(ws + L.partial);
    unsigned int* block_off = (unsigned int*)(ws + L.block_off);
    const int T = (int)L.T;
    const int nb = (int)(((long long)Vu + CC_THREADS - 1) / CC_THREADS);          // U * nb <= N * Z * nb2: the sections hold it
    const int txn = ceil_div(W, CC_TW), tyn = ceil_div(H, CC_TH);
    const dim3 tiles((unsigned int)((long long)N * Z * txn * tyn));          // every tile holds a voxel: <= T
    const int diag = connectivity >= 2 ? 1 : 0;
    const bool vec = (uintptr_t)vol % 16 == 0 && W % 4 == 0;          // parent is the workspace's first section: 16-byte aligned
    if (vec)
        hipLaunchKernelGGL((cc_tile_kernel<true>), tiles, dim3(CC_THREADS), 0, st, vol, parent, cls, C, H, W, txn, tyn, diag);
    else
        hipLaunchKernelGGL((cc_tile_kernel<false>), tiles, dim3(CC_THREADS), 0, st, vol, parent, cls, C, H, W, txn, tyn, diag);
    AESR_LAUNCH_CHECK("components_tile");
    hipLaunchKernelGGL(cc_merge_kernel, dim3(cc_blocks(T)), dim3(CC_THREADS), 0, st, vol, parent, cls, C, T, Z, H, W, ndim == 3 ? 1 : 0,
                       connectivity);
    AESR_LAUNCH_CHECK("components_merge");
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned int)(U * nb)), dim3(CC_THREADS), 0, st, vol, (const int*)parent, labels, partial, cls, C,
                       Vu, nb);
    AESR_LAUNCH_CHECK("components_flatten");
    hipLaunchKernelGGL(cc_scan_kernel, dim3((unsigned int)(U * C)), dim3(CC_THREADS), 0, st, (const unsigned int*)partial, block_off, n_components,
                       nb);
    AESR_LAUNCH_CHECK("components_scan");
    hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned int)(U * nb)), dim3(CC_THREADS), 0, st, vol, (const int*)labels, parent,
                       (const unsigned int*)block_off, cls, C, Vu, nb);
    AESR_LAUNCH_CHECK("components_number");
    hipLaunchKernelGGL(cc_assign_kernel, dim3(cc_blocks(T)), dim3(CC_THREADS), 0, st, labels, (const int*)parent, T);
    AESR_LAUNCH_CHECK("components_assign");
    return AESR_OK;
}

int aesr_components_tables(const float* vol, const int* labels, const int* n_components, const int* n_components_host, void* workspace,
                           long long* table, size_t capacity, int N, int Z, int H, int W, const int* classes, int C, int ndim, void* stream) {
    const char* fn = "aesr_components_tables";
    int rc = cc_check_sizes(fn, N, Z, H, W, C);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(vol && labels && n_components && n_components_host && workspace, "%s: a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)vol % 4 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)n_components % 4 == 0,
                   "%s: vol, labels or n_components is not 4-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace is not 16-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)table % 8 == 0, "%s: table is not 8-byte aligned", fn);
    AesrClasses cls;
    rc = cc_check_classes(fn, classes, C, ndim, &cls);
    if (rc != AESR_OK) return rc;
    const CcLayout L = cc_layout(N, Z, H, W, C);
    const int U = ndim == 2 ? N * Z : N;
    const int Vu = ndim == 2 ? H * W : Z * H * W;
    unsigned long long rows = 0;
    rc = cc_check_counts(fn, n_components_host, (long long)U * C, Vu, &rows);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(rows <= capacity, "%s: the table has %llu rows, the buffer only %zu", fn, rows, capacity);
    AESR_CHECK_ARG(table || rows == 0, "%s: table is a null pointer", fn);
    const AesrBuf bufs[5] = {{vol, (size_t)L.T * 4, false}, {labels, (size_t)L.T * 4, false}, {n_components, (size_t)U * C * 4, false},
                           {workspace, L.total, true}, {table, capacity * CC_COLS * 8, true}};
    if (aesr_any_overlap(bufs, 5)) {
        aesr_set_error("%s: an output or the workspace overlaps an input or another output", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    int* offs = (int*)((char*)workspace + L.offs);
    const int T = (int)L.T;
    hipLaunchKernelGGL(cc_offsets_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, n_components, offs, U * C);
    AESR_LAUNCH_CHECK("components_offsets");
    if (rows == 0) return AESR_OK;
    hipLaunchKernelGGL(cc_table_init_kernel, dim3(cc_blocks((long long)(rows * CC_COLS))), dim3(CC_THREADS), 0, st, (unsigned long long*)table,
                       rows * CC_COLS);
    AESR_LAUNCH_CHECK("components_table_init");
    hipLaunchKernelGGL(cc_table_kernel, dim3(cc_blocks(((long long)T + 3) / 4)), dim3(CC_THREADS), 0, st, vol, labels, n_components, (const int*)offs,
                       (unsigned long long*)table, rows, cls, C, T, Z, H, W, Vu);
    AESR_LAUNCH_CHECK("components_table");
    return AESR_OK;
}

int aesr_components_apply_table(const float* vol, const int* labels, const int* n_components, const int* n_components_host, void* workspace,
                                const float* table, size_t table_len, float* out, int N, int Z, int H, int W, const int* classes, int C,
                                int ndim, void* stream) {
    const char* fn = "aesr_components_apply_table";
    int rc = cc_check_sizes(fn, N, Z, H, W, C);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(vol && labels && n_components && n_components_host && workspace && out, "%s: a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)vol % 4 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)n_components % 4 == 0 && (uintptr_t)table % 4 == 0 &&
                       (uintptr_t)out % 4 == 0,
                   "%s: vol, labels, n_components, table or out is not 4-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace is not 16-byte aligned", fn);
    AesrClasses cls;
    rc = cc_check_classes(fn, classes, C, ndim, &cls);
    if (rc != AESR_OK) return rc;
    const CcLayout L = cc_layout(N, Z, H, W, C);
    const int U = ndim == 2 ? N * Z : N;
    const int Vu = ndim == 2 ? H * W : Z * H * W;
    unsigned long long rows = 0;
    rc = cc_check_counts(fn, n_components_host, (long long)U * C, Vu, &rows);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(rows <= table_len, "%s: the components need %llu table entries, the table has only %zu", fn, rows, table_len);
    AESR_CHECK_ARG(table || rows == 0, "%s: table is a null pointer", fn);
    const AesrBuf bufs[6] = {{vol, (size_t)L.T * 4, false}, {labels, (size_t)L.T * 4, false}, {n_components, (size_t)U * C * 4, false},
                           {table, table_len * 4, false}, {workspace, L.total, true}, {out, (size_t)L.T * 4, true}};
    if (aesr_any_overlap(bufs, 6)) {
        aesr_set_error("%s: an output or the workspace overlaps an input or another output", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    int* offs = (int*)((char*)workspace + L.offs);
    const int T = (int)L.T;
    hipLaunchKernelGGL(cc_offsets_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, n_components, offs, U * C);
    AESR_LAUNCH_CHECK("components_offsets");
    hipLaunchKernelGGL(cc_apply_kernel, dim3(cc_blocks(T)), dim3(CC_THREADS), 0, st, vol, labels, n_components, (const int*)offs, table,
                       (unsigned long long)rows, out, cls, C, T, Vu);
    AESR_LAUNCH_CHECK("components_apply");
    return AESR_OK;
}

// the checks the two overlap entry points share
static int cc_check_overlap_args(const char* fn, const float* vol_a, const int* labels_a, const float* vol_b, const int* labels_b,
                                 void* workspace, int N, int Z, int H, int W, const int* classes, int C, int ndim, AesrClasses* cls) {
    int rc = cc_check_sizes(fn, N, Z, H, W, C);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(vol_a && labels_a && vol_b && labels_b && workspace, "%s: a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)vol_a % 4 == 0 && (uintptr_t)labels_a % 4 == 0 && (uintptr_t)vol_b % 4 == 0 && (uintptr_t)labels_b % 4 == 0,
                   "%s: a volume or a label map is not 4-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace is not 16-byte aligned", fn);
    return cc_check_classes(fn, classes, C, ndim, cls);
}

int aesr_components_overlap_count(const float* vol_a, const int* labels_a, const float* vol_b, const int* labels_b, void* workspace,
                                  long long* count, int N, int Z, int H, int W, const int* classes, int C, int ndim, void* stream) {
    const char* fn = "aesr_components_overlap_count";
    AesrClasses cls;
    const int rc = cc_check_overlap_args(fn, vol_a, labels_a, vol_b, labels_b, workspace, N, Z, H, W, classes, C, ndim, &cls);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(count, "%s: a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)count % 8 == 0, "%s: count is not 8-byte aligned", fn);
    const CcLayout L = cc_layout(N, Z, H, W, C);
    const size_t vb = (size_t)L.T * 4;
    const AesrBuf bufs[6] = {{vol_a, vb, false}, {labels_a, vb, false}, {vol_b, vb, false}, {labels_b, vb, false}, {workspace, L.total, true},
                           {count, 8, true}};
    if (aesr_any_overlap(bufs, 6)) {
        aesr_set_error("%s: an output or the workspace overlaps an input or another output", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned int* partial = (unsigned int*)((char*)workspace + L.ov_partial);
    unsigned int* off = (unsigned int*)((char*)workspace + L.ov_off);
    const int T = (int)L.T;
    hipLaunchKernelGGL(cc_overlap_count_kernel, dim3((unsigned int)L.nbT), dim3(CC_THREADS), 0, st, vol_a, labels_a, vol_b, labels_b, partial, cls,
                       C, T, W);
    AESR_LAUNCH_CHECK("components_overlap_count");
    hipLaunchKernelGGL(cc_overlap_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, (const unsigned int*)partial, off, count, L.nbT);
    AESR_LAUNCH_CHECK("components_overlap_scan");
    return AESR_OK;
}

int aesr_components_overlap_runs(const float* vol_a, const int* labels_a, const float* vol_b, const int* labels_b, void* workspace,
                                 long long count_host, int* runs, size_t capacity, int N, int Z, int H, int W, const int* classes, int C,
                                 int ndim, void* stream) {
    const char* fn = "aesr_components_overlap_runs";
    AesrClasses cls;
    const int rc = cc_check_overlap_args(fn, vol_a, labels_a, vol_b, labels_b, workspace, N, Z, H, W, classes, C, ndim, &cls);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG((uintptr_t)runs % 4 == 0, "%s: runs is not 4-byte aligned", fn);
    const CcLayout L = cc_layout(N, Z, H, W, C);
    AESR_CHECK_ARG(count_host >= 0 && count_host <= L.T, "%s: count_host = %lld is not what aesr_components_overlap_count wrote for this size", fn,
                   count_host);
    AESR_CHECK_ARG((unsigned long long)count_host <= capacity, "%s: there are %lld runs, the buffer holds only %zu", fn, count_host, capacity);
    AESR_CHECK_ARG(runs || count_host == 0, "%s: runs is a null pointer", fn);
    const size_t vb = (size_t)L.T * 4;
    const AesrBuf bufs[6] = {{vol_a, vb, false}, {labels_a, vb, false}, {vol_b, vb, false}, {labels_b, vb, false}, {workspace, L.total, false},
                           {runs, capacity * 16, true}};
    if (aesr_any_overlap(bufs, 6)) {
        aesr_set_error("%s: the output overlaps an input or the workspace", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    if (count_host == 0) return AESR_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned int* off = (const unsigned int*)((char*)workspace + L.ov_off);
    const int T = (int)L.T;
    const int Vu = ndim == 2 ? H * W : Z * H * W;
    hipLaunchKernelGGL(cc_overlap_runs_kernel, dim3((unsigned int)L.nbT), dim3(CC_THREADS), 0, st, vol_a, labels_a, vol_b, labels_b, off, runs,
                       (unsigned long long)count_host, cls, C, T, W, Vu);
    AESR_LAUNCH_CHECK("components_overlap_runs");
    return AESR_OK;
}

}  // extern "C"
