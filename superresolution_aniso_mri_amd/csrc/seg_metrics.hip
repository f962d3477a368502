// Overlap counts and surface distances of label volumes on the device: what Dice, Jaccard, Hausdorff distance, HD95 and the average
// symmetric surface distance are made of (the reference computes them on the host with a binary erosion and an exact Euclidean distance
// transform per class and direction, kwatsch/medpy_metrics.py).  include/aesr_hip_surface.h states the definitions.
//
//   phase one (aesr_surface_borders)
//     classify   one pass over result and reference: a voxel's class, whether it is a border voxel of that class (stencil over the
//                neighbours of the requested connectivity), one flag byte per (n, side, voxel) = 0 or class index + 1 -- a voxel belongs to
//                at most one class, so one byte serves all classes -- and per workgroup the integer partials |A|, |B|, |A n B|, border A,
//                border B of every class.
//     finish     per (n, class): the partials added in block order (integers: exact), and for both sides the exclusive prefix of the
//                border counts over the workgroups, which is every workgroup's base rank in phase two.
//   phase two (aesr_surface_distances)
//     offsets    list lengths and offsets from the counts (exclusive scan over the lists, one workgroup).
//     x pass     one wave per line: the line's border voxels as 64-bit ballot masks in LDS, every lane finds the nearest set bit with
//                clz / ctz.  Index distance as int, SURF_NONE for a line without border voxel.
//     y pass     per voxel min_y' ((dy sy)^2 + (gx sx)^2) in fp64 by brute force over the column, staged in LDS SURF_YCHUNK rows at a time.
//     gather     only at the border voxels of the other side: min_z' ((dz sz)^2 + m_y), sqrt, written to the packed list at its raster
//                rank = workgroup base + waves before it + 64-bit ballot / mbcnt prefix inside the wave.
//     reduce     per list its sum and maximum: per-thread partials over a fixed stride, then a fixed-order tree.
// No floating-point atomics, no buffer that needs initialisation; which thread takes which voxel and the order of every sum depend on the
// sizes alone, so two runs give the same bits.  -ffp-contract=off (Makefile) keeps a*a + b from becoming an fma.
#include "aesr_kernels.h"
#include "aesr_hostcheck.h"
#include "../../include/aesr_hip_surface.h"

#include <cmath>

#define SURF_THREADS 256
#define SURF_VPT 4                                  // consecutive voxels per thread: one 16-byte label load per side, one flag word
#define SURF_VPB (SURF_THREADS * SURF_VPT)          // voxels per workgroup, the unit of the compaction
#define SURF_MAXC AESR_SURFACE_MAX_CLASSES
#define SURF_NQ 5                                   // partial counters per class: |A|, |B|, |A n B|, border A, border B
#define SURF_NONE 0x7fffffff                        // x pass: no border voxel in this line
#define SURF_XWORDS (AESR_SURFACE_MAX_W / 64)
#define SURF_YCOLS 16
#define SURF_YROWS 4                                // output rows per thread of the y pass
#define SURF_YCHUNK 256                             // column rows staged at a time: 256 * 16 * 8 B = 32 KB
#define SURF_SCAN_THREADS 1024

// byte offsets of the workspace sections, all multiples of 16
struct SurfLayout {
    size_t my, list_tab, gx, partial, block_off, flags, total;
    long long V, Vp;
    int nb;
};

static SurfLayout surf_layout(int N, int Z, int H, int W, int C) {
    SurfLayout L;
    L.V = (long long)Z * H * W;
    L.Vp = (L.V + 3) / 4 * 4;
    L.nb = (int)((L.V + SURF_VPB - 1) / SURF_VPB);
    const size_t lists = (size_t)N * C * 2;
    size_t o = 0;
    L.my = o;          o += aesr_up16(lists * (size_t)L.V * 8);
    L.list_tab = o;    o += aesr_up16(lists * 2 * 8);
    L.gx = o;          o += aesr_up16(lists * (size_t)L.V * 4);
    L.partial = o;     o += aesr_up16((size_t)N * L.nb * C * SURF_NQ * 4);
    L.block_off = o;   o += aesr_up16(lists * (size_t)L.nb * 4);
    L.flags = o;       o += aesr_up16((size_t)N * 2 * (size_t)L.Vp);
    L.total = o;
    return L;
}

// true when voxel (z, y, x) of mask (vol == v) has a neighbour that is not in the mask; outside the array counts as not in it
__device__ __forceinline__ bool surf_is_border(const float* __restrict__ vol, float v, int z, int y, int x, int Z, int H, int W, int zr,
                                               int conn) {
    for (int dz = -zr; dz <= zr; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int l1 = (dz != 0) + (dy != 0) + (dx != 0);
                if (l1 == 0 || l1 > conn) continue;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz < 0 || zz >= Z || yy < 0 || yy >= H || xx < 0 || xx >= W) return true;
                if (!(vol[((size_t)zz * H + yy) * W + xx] == v)) return true;
            }
    return false;
}

// workgroup b of volume n takes the voxels [b * SURF_VPB, (b + 1) * SURF_VPB) of that volume, thread t the four at b * SURF_VPB + 4 t
template <bool VEC>
__global__ __launch_bounds__(SURF_THREADS) void surf_classify_kernel(const float* __restrict__ result, const float* __restrict__ reference,
                                                                     unsigned int* __restrict__ flags, unsigned int* __restrict__ partial,
                                                                     AesrClasses cls, int C, int V, int Vp, int Z, int H, int W, int nb,
                                                                     int zr, int conn) {
    __shared__ unsigned int red[SURF_THREADS / 64][SURF_MAXC * SURF_NQ];
    const int n = blockIdx.x / nb, b = blockIdx.x - n * nb;
    const int idx0 = b * SURF_VPB + (int)threadIdx.x * SURF_VPT;
    const float* __restrict__ rv = result + (size_t)n * V;
    const float* __restrict__ gv = reference + (size_t)n * V;
    float a[SURF_VPT] = {0.f, 0.f, 0.f, 0.f}, g[SURF_VPT] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (idx0 < V) {          // V % 4 == 0 here: all four are inside
            const f32x4 va = *reinterpret_cast<const f32x4*>(rv + idx0), vg = *reinterpret_cast<const f32x4*>(gv + idx0);
            a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
            g[0] = vg.x; g[1] = vg.y; g[2] = vg.z; g[3] = vg.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < SURF_VPT; ++j)
            if (idx0 + j < V) {
                a[j] = rv[idx0 + j];
                g[j] = gv[idx0 + j];
            }
    }
    int kA[SURF_VPT], kB[SURF_VPT];
    bool bA[SURF_VPT], bB[SURF_VPT];
    unsigned int wordA = 0, wordB = 0;
    const int HW = H * W;
#pragma unroll
    for (int j = 0; j < SURF_VPT; ++j) {
        const int idx = idx0 + j;
        kA[j] = kB[j] = -1;
        bA[j] = bB[j] = false;
        if (idx < V) {
            const int z = idx / HW, rem = idx - z * HW, y = rem / W, x = rem - y * W;
            kA[j] = aesr_class_of(a[j], cls, C);
            kB[j] = aesr_class_of(g[j], cls, C);
            if (kA[j] >= 0) bA[j] = surf_is_border(rv, a[j], z, y, x, Z, H, W, zr, conn);
            if (kB[j] >= 0) bB[j] = surf_is_border(gv, g[j], z, y, x, Z, H, W, zr, conn);
            if (bA[j]) wordA |= (unsigned int)(kA[j] + 1) << (8 * j);
            if (bB[j]) wordB |= (unsigned int)(kB[j] + 1) << (8 * j);
        }
    }
    if (idx0 < V) {          // idx0 is a multiple of 4 below V, so the whole word lies below Vp; bytes past V are written as 0
        flags[((size_t)n * 2 + 0) * (Vp / 4) + idx0 / 4] = wordA;
        flags[((size_t)n * 2 + 1) * (Vp / 4) + idx0 / 4] = wordB;
    }
    // counts: ballots are wave-uniform, lane 0 keeps the sums
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < SURF_MAXC; ++c) {
        if (c < C) {
            unsigned int s[SURF_NQ] = {0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < SURF_VPT; ++j) {
                s[0] += (unsigned int)__popcll(__ballot(kA[j] == c));
                s[1] += (unsigned int)__popcll(__ballot(kB[j] == c));
                s[2] += (unsigned int)__popcll(__ballot(kA[j] == c && kB[j] == c));
                s[3] += (unsigned int)__popcll(__ballot(kA[j] == c && bA[j]));
                s[4] += (unsigned int)__popcll(__ballot(kB[j] == c && bB[j]));
            }
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < SURF_NQ; ++q) red[wave][c * SURF_NQ + q] = s[q];
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < C * SURF_NQ) {
        unsigned int s = 0;
#pragma unroll
        for (int w = 0; w < SURF_THREADS / 64; ++w) s += red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * (C * SURF_NQ) + threadIdx.x] = s;
    }
}

// workgroup (n, c): counts[n][c][0 .. 6], and block_off[(n, c, side)][b] = border voxels of that list in the workgroups before b
__global__ __launch_bounds__(SURF_THREADS) void surf_finish_kernel(const unsigned int* __restrict__ partial, unsigned int* __restrict__ block_off,
                                                                   long long* __restrict__ counts, int C, int V, int nb) {
    __shared__ unsigned long long sh[SURF_THREADS];
    __shared__ unsigned long long tot[SURF_NQ];
    const int n = blockIdx.x / C, c = blockIdx.x - n * C;
    const int per = (nb + SURF_THREADS - 1) / SURF_THREADS;
    const int b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    const unsigned int* p = partial + (size_t)n * nb * (C * SURF_NQ) + c * SURF_NQ;
    for (int q = 0; q < SURF_NQ; ++q) {
        unsigned long long s = 0;
        for (int b = b0; b < b1; ++b) s += p[(size_t)b * (C * SURF_NQ) + q];
        sh[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long run = 0;
            for (int t = 0; t < SURF_THREADS; ++t) {
                const unsigned long long v = sh[t];
                sh[t] = run;
                run += v;
            }
            tot[q] = run;
        }
        __syncthreads();
        if (q >= 3) {
            unsigned int run = (unsigned int)sh[threadIdx.x];          // < 2^31: at most one per voxel
            unsigned int* o = block_off + ((size_t)blockIdx.x * 2 + (q - 3)) * nb;
            for (int b = b0; b < b1; ++b) {
                o[b] = run;
                run += p[(size_t)b * (C * SURF_NQ) + q];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        long long* o = counts + (size_t)blockIdx.x * AESR_SURFACE_COUNTS;
        o[0] = (long long)tot[0];
        o[1] = (long long)tot[1];
        o[2] = (long long)tot[2];
        o[3] = (long long)(tot[0] + tot[1] - tot[2]);
        o[4] = (long long)V;
        o[5] = (long long)tot[3];
        o[6] = (long long)tot[4];
    }
}

// one workgroup: list_tab[l] = (offset, length), l = (n * C + c) * 2 + d; length = border count of the source side, 0 if a mask is empty
__global__ __launch_bounds__(SURF_SCAN_THREADS) void surf_offsets_kernel(const long long* __restrict__ counts, long long* __restrict__ list_tab,
                                                                         int lists) {
    __shared__ long long sh[SURF_SCAN_THREADS];
    const int per = (lists + SURF_SCAN_THREADS - 1) / SURF_SCAN_THREADS;
    const int l0 = min((int)threadIdx.x * per, lists), l1 = min(l0 + per, lists);
    long long s = 0;
    for (int l = l0; l < l1; ++l) {
        const long long* c = counts + (size_t)(l >> 1) * AESR_SURFACE_COUNTS;
        s += (c[0] > 0 && c[1] > 0) ? c[5 + (l & 1)] : 0;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int t = 0; t < SURF_SCAN_THREADS; ++t) {
            const long long v = sh[t];
            sh[t] = run;
            run += v;
        }
    }
    __syncthreads();
    long long run = sh[threadIdx.x];
    for (int l = l0; l < l1; ++l) {
        const long long* c = counts + (size_t)(l >> 1) * AESR_SURFACE_COUNTS;
        const long long len = (c[0] > 0 && c[1] > 0) ? c[5 + (l & 1)] : 0;
        list_tab[2 * (size_t)l] = run;
        list_tab[2 * (size_t)l + 1] = len;
        run += len;
    }
}

// one wave per line (field f = (n * C + c) * 2 + side, z, y): gx[f][z][y][x] = min |x - x'| over the border voxels x' of the line
__global__ __launch_bounds__(SURF_THREADS) void surf_xpass_kernel(const unsigned char* __restrict__ flags, int* __restrict__ gx, int C, int V,
                                                                  int Vp, int W, long long lines, int lines_per_field) {
    __shared__ unsigned long long mask[SURF_THREADS / 64][SURF_XWORDS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long line = (long long)blockIdx.x * (SURF_THREADS / 64) + wave;
    const bool active = line < lines;          // whole waves; an idle wave still takes part in the barrier
    const int f = active ? (int)(line / lines_per_field) : 0, zy = active ? (int)(line - (long long)f * lines_per_field) : 0;
    const int side = f & 1, nc = f >> 1, n = nc / C, c = nc - n * C;
    const unsigned char* fl = flags + ((size_t)n * 2 + side) * Vp + (size_t)zy * W;
    const int nw = active ? (W + 63) / 64 : 0;
    for (int k = 0; k < nw; ++k) {
        const int x = k * 64 + lane;
        const unsigned long long m = __ballot(x < W && fl[x] == (unsigned char)(c + 1));
        if (lane == 0) mask[wave][k] = m;
    }
    __syncthreads();
    int* o = gx + (size_t)f * V + (size_t)zy * W;
    for (int k0 = 0; k0 < nw; ++k0) {
        const int x = k0 * 64 + lane;
        int best = SURF_NONE;
        for (int k = 0; k < nw; ++k) {
            const unsigned long long m = mask[wave][k];
            if (m == 0) continue;          // uniform
            if (k < k0) best = min(best, x - (k * 64 + 63 - __clzll((long long)m)));
            else if (k > k0) best = min(best, k * 64 + (__ffsll((long long)m) - 1) - x);
            else {
                const unsigned long long le = m & (~0ull >> (63 - lane)), ge = m & (~0ull << lane);
                if (le) best = min(best, lane - (63 - __clzll((long long)le)));
                if (ge) best = min(best, (__ffsll((long long)ge) - 1) - lane);
            }
        }
        if (x < W) o[x] = best;
    }
}

// workgroup (field, z, x tile of 16 columns, y tile of 64 rows); thread (tx, ty) the rows y0 + ty + 16 r of column x0 + tx
__global__ __launch_bounds__(SURF_THREADS) void surf_ypass_kernel(const int* __restrict__ gx, double* __restrict__ my, int H, int W, int xt,
                                                                  int yt, double sy, double sx) {
    __shared__ double col[SURF_YCHUNK][SURF_YCOLS];
    const int tx = threadIdx.x & (SURF_YCOLS - 1), ty = threadIdx.x / SURF_YCOLS;
    unsigned int bid = blockIdx.x;
    const int bx = bid % xt; bid /= xt;
    const int by = bid % yt; bid /= yt;          // bid: field * Z + z
    const size_t slice = (size_t)bid * H * W;
    const int x = bx * SURF_YCOLS + tx, y0 = by * (SURF_YCOLS * SURF_YROWS) + ty;
    double m[SURF_YROWS];
#pragma unroll
    for (int r = 0; r < SURF_YROWS; ++r) m[r] = INFINITY;
    for (int c0 = 0; c0 < H; c0 += SURF_YCHUNK) {
        const int rows = min(SURF_YCHUNK, H - c0);
        __syncthreads();
        for (int i = ty; i < rows; i += SURF_THREADS / SURF_YCOLS) {
            double t = INFINITY;
            if (x < W) {
                const int g = gx[slice + (size_t)(c0 + i) * W + x];
                if (g != SURF_NONE) {
                    const double d = (double)g * sx;
                    t = d * d;
                }
            }
            col[i][tx] = t;
        }
        __syncthreads();
        for (int i = 0; i < rows; ++i) {
            const double t = col[i][tx];
#pragma unroll
            for (int r = 0; r < SURF_YROWS; ++r) {
                const double d = (double)(y0 + SURF_YCOLS * r - (c0 + i)) * sy;
                m[r] = fmin(m[r], d * d + t);          // inf + finite = inf: no NaN can arise
            }
        }
    }
    if (x < W) {
#pragma unroll
        for (int r = 0; r < SURF_YROWS; ++r) {
            const int y = y0 + SURF_YCOLS * r;
            if (y < H) my[slice + (size_t)y * W + x] = m[r];
        }
    }
}

// same voxel assignment as surf_classify_kernel; every border voxel of either side writes its distance at its raster rank
__global__ __launch_bounds__(SURF_THREADS) void surf_gather_kernel(const unsigned int* __restrict__ flags, const unsigned int* __restrict__ block_off,
                                                                   const long long* __restrict__ list_tab, const double* __restrict__ my,
                                                                   double* __restrict__ dist, unsigned long long capacity, int C, int V, int Vp,
                                                                   int Z, int H, int W, int nb, int zloop, double sz) {
    __shared__ unsigned int wtot[2][SURF_MAXC][SURF_THREADS / 64];
    const int n = blockIdx.x / nb, b = blockIdx.x - n * nb;
    const int idx0 = b * SURF_VPB + (int)threadIdx.x * SURF_VPT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned int word[2] = {0, 0};
    if (idx0 < V) {
        word[0] = flags[((size_t)n * 2 + 0) * (Vp / 4) + idx0 / 4];
        word[1] = flags[((size_t)n * 2 + 1) * (Vp / 4) + idx0 / 4];
    }
    int in_wave[2][SURF_VPT];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int j = 0; j < SURF_VPT; ++j) in_wave[s][j] = 0;
#pragma unroll
        for (int c = 0; c < SURF_MAXC; ++c) {
            if (c < C) {
                unsigned int below = 0, total = 0, own = 0;
#pragma unroll
                for (int j = 0; j < SURF_VPT; ++j) {
                    const bool hit = ((word[s] >> (8 * j)) & 0xffu) == (unsigned int)(c + 1);
                    const unsigned long long m = __ballot(hit);
                    below += __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
                    total += (unsigned int)__popcll(m);
                    if (hit) in_wave[s][j] = -1 - (int)own;          // marks a hit; the lanes below are added once all four are counted
                    own += hit ? 1u : 0u;
                }
#pragma unroll
                for (int j = 0; j < SURF_VPT; ++j) {
                    const bool hit = ((word[s] >> (8 * j)) & 0xffu) == (unsigned int)(c + 1);
                    if (hit) in_wave[s][j] = (int)below + (-1 - in_wave[s][j]);
                }
                if (lane == 0) wtot[s][c][wave] = total;
            }
        }
    }
    __syncthreads();
    const int HW = H * W;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int j = 0; j < SURF_VPT; ++j) {
            const int code = (int)((word[s] >> (8 * j)) & 0xffu);
            if (code == 0 || code > C) continue;
            const int c = code - 1, idx = idx0 + j;
            const size_t l = ((size_t)n * C + c) * 2 + s;          // this list; its distances come from the field of the OTHER side
            const long long off = list_tab[2 * l], len = list_tab[2 * l + 1];
            if (len == 0) continue;          // one of the two masks is empty: no list
            unsigned int rank = block_off[l * nb + b] + (unsigned int)in_wave[s][j];
            for (int w = 0; w < wave; ++w) rank += wtot[s][c][w];
            const double* f = my + (l ^ 1) * (size_t)V;
            double d2;
            if (zloop) {
                const int z = idx / HW, rem = idx - z * HW;
                d2 = INFINITY;
                for (int zz = 0; zz < Z; ++zz) {
                    const double dz = (double)(z - zz) * sz;
                    d2 = fmin(d2, dz * dz + f[(size_t)zz * HW + rem]);
                }
            } else {
                d2 = f[idx];
            }
            const unsigned long long at = (unsigned long long)off + rank;
            if ((long long)rank < len && at < capacity) dist[at] = sqrt(d2);          // always true for the counts of this workspace
        }
    }
}

// workgroup l: stats[l] = (sum, max) of list l; thread t adds the elements t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(SURF_THREADS) void surf_reduce_kernel(const double* __restrict__ dist, const long long* __restrict__ list_tab,
                                                                   double* __restrict__ stats, unsigned long long capacity) {
    __shared__ double ssum[SURF_THREADS], smax[SURF_THREADS];
    const size_t l = blockIdx.x;
    const long long off = list_tab[2 * l];
    long long len = list_tab[2 * l + 1];
    if ((unsigned long long)(off + len) > capacity) len = 0;
    double s = 0.0, m = 0.0;
    for (long long i = threadIdx.x; i < len; i += SURF_THREADS) {
        const double v = dist[off + i];
        s += v;
        m = fmax(m, v);
    }
    ssum[threadIdx.x] = s;
    smax[threadIdx.x] = m;
    __syncthreads();
    for (int h = SURF_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            ssum[threadIdx.x] += ssum[threadIdx.x + h];
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[2 * l] = ssum[0];
        stats[2 * l + 1] = smax[0];
    }
}

// sizes both launch entry points and the query share; 0 = fine, else the code with the message set (fn == NULL: silent, for the query)
static int surf_check_sizes(const char* fn, int N, int Z, int H, int W, int C) {
    if (N <= 0 || Z <= 0 || H <= 0 || W <= 0) {
        if (fn) aesr_set_error("%s: N, Z, H, W = %d, %d, %d, %d must all be positive", fn, N, Z, H, W);
        return AESR_ERR_ARG;
    }
    if (C < 1 || C > SURF_MAXC) {
        if (fn) aesr_set_error("%s: C=%d classes, 1 to %d are supported", fn, C, SURF_MAXC);
        return AESR_ERR_ARG;
    }
    if ((double)N * Z * H * W >= 2147483648.0) {
        if (fn) aesr_set_error("%s: N * Z * H * W = %d x %d x %d x %d has 2^31 voxels or more", fn, N, Z, H, W);
        return AESR_ERR_ARG;
    }
    if ((double)N * C >= 1073741824.0) {          // 2 N C lists are counted in an int
        if (fn) aesr_set_error("%s: N * C = %d x %d gives 2^31 lists or more", fn, N, C);
        return AESR_ERR_ARG;
    }
    if (W > AESR_SURFACE_MAX_W) {
        if (fn) aesr_set_error("%s: W=%d, lines of up to %d voxels are supported", fn, W, AESR_SURFACE_MAX_W);
        return AESR_ERR_UNSUPPORTED;
    }
    return AESR_OK;
}

extern "C" {

size_t aesr_surface_workspace_bytes(int N, int Z, int H, int W, int C) {
    if (surf_check_sizes(NULL, N, Z, H, W, C) != AESR_OK) return 0;
    return surf_layout(N, Z, H, W, C).total;
}

int aesr_surface_borders(const float* result, const float* reference, void* workspace, long long* counts, int N, int Z, int H, int W,
                         const int* classes, int C, int ndim, int connectivity, void* stream) {
    const char* fn = "aesr_surface_borders";
    const int rc = surf_check_sizes(fn, N, Z, H, W, C);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(result && reference && workspace && counts && classes, "%s: a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)result % 4 == 0 && (uintptr_t)reference % 4 == 0, "%s: a label pointer is not 4-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace is not 16-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)counts % 8 == 0, "%s: counts is not 8-byte aligned", fn);
    AESR_CHECK_ARG(ndim == 2 || ndim == 3, "%s: ndim=%d, 2 or 3 are supported", fn, ndim);
    AESR_CHECK_ARG(connectivity >= 1 && connectivity <= ndim, "%s: connectivity=%d must be in 1 ... ndim = %d", fn, connectivity, ndim);
    AesrClasses cls;
    const int rc_cls = aesr_fill_classes(fn, classes, C, &cls);
    if (rc_cls != AESR_OK) return rc_cls;
    const SurfLayout L = surf_layout(N, Z, H, W, C);
    const size_t vol_bytes = (size_t)N * (size_t)L.V * 4, cnt_bytes = (size_t)N * C * AESR_SURFACE_COUNTS * 8;
    const AesrBuf bufs[4] = {{result, vol_bytes, false}, {reference, vol_bytes, false}, {workspace, L.total, true}, {counts, cnt_bytes, true}};
    if (aesr_any_overlap(bufs, 4)) {
        aesr_set_error("%s: an output or the workspace overlaps an input or another output", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned int* flags = (unsigned int*)(ws + L.flags);
    unsigned int* partial = (unsigned int*)(ws + L.partial);
    unsigned int* block_off = (unsigned int*)(ws + L.block_off);
    const int V = (int)L.V, Vp = (int)L.Vp, zr = ndim == 3 ? 1 : 0;
    const dim3 grid((unsigned int)(N * L.nb));          // <= N * V < 2^31
    const bool vec = (uintptr_t)result % 16 == 0 && (uintptr_t)reference % 16 == 0 && V % 4 == 0;
    if (vec)
        hipLaunchKernelGGL((surf_classify_kernel<true>), grid, dim3(SURF_THREADS), 0, st, result, reference, flags, partial, cls, C, V, Vp, Z, H,
                           W, L.nb, zr, connectivity);
    else
        hipLaunchKernelGGL((surf_classify_kernel<false>), grid, dim3(SURF_THREADS), 0, st, result, reference, flags, partial, cls, C, V, Vp, Z,
                           H, W, L.nb, zr, connectivity);
    AESR_LAUNCH_CHECK("surface_classify");
    hipLaunchKernelGGL(surf_finish_kernel, dim3((unsigned int)(N * C)), dim3(SURF_THREADS), 0, st, (const unsigned int*)partial, block_off,
                       counts, C, V, L.nb);
    AESR_LAUNCH_CHECK("surface_finish");
    return AESR_OK;
}

int aesr_surface_distances(void* workspace, const long long* counts, const long long* counts_host, double* distances, size_t capacity,
                           double* stats, int N, int Z, int H, int W, int C, int ndim, const double* spacing, void* stream) {
    const char* fn = "aesr_surface_distances";
    const int rc = surf_check_sizes(fn, N, Z, H, W, C);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(workspace && counts && counts_host && stats && spacing, "%s: a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace is not 16-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)counts % 8 == 0 && (uintptr_t)distances % 8 == 0 && (uintptr_t)stats % 8 == 0,
                   "%s: counts, distances or stats is not 8-byte aligned", fn);
    AESR_CHECK_ARG(ndim == 2 || ndim == 3, "%s: ndim=%d, 2 or 3 are supported", fn, ndim);
    for (int a = 0; a < 3; ++a)
        AESR_CHECK_ARG(spacing[a] > 0.0 && std::isfinite(spacing[a]), "%s: spacing[%d]=%g must be positive and finite", fn, a, spacing[a]);
    const SurfLayout L = surf_layout(N, Z, H, W, C);
    unsigned long long need = 0;
    for (int i = 0; i < N * C; ++i) {
        const long long* c = counts_host + (size_t)i * AESR_SURFACE_COUNTS;
        bool ok = c[4] == L.V;
        for (int q = 0; q < AESR_SURFACE_COUNTS; ++q) ok = ok && c[q] >= 0 && c[q] <= L.V;
        ok = ok && c[5] <= c[0] && c[6] <= c[1];
        AESR_CHECK_ARG(ok, "%s: counts_host[%d] is not what aesr_surface_borders wrote for this size", fn, i);
        if (c[0] > 0 && c[1] > 0) need += (unsigned long long)(c[5] + c[6]);
    }
    AESR_CHECK_ARG(need <= capacity, "%s: the lists hold %llu distances, the buffer only %zu", fn, need, capacity);
    AESR_CHECK_ARG(distances || need == 0, "%s: distances is a null pointer", fn);
    const size_t cnt_bytes = (size_t)N * C * AESR_SURFACE_COUNTS * 8, st_bytes = (size_t)N * C * 4 * 8, d_bytes = capacity * 8;
    // counts is only read: it is checked against the three buffers that are written, which is every pair of the four
    const AesrBuf bufs[4] = {{counts, cnt_bytes, false}, {workspace, L.total, true}, {distances, d_bytes, true}, {stats, st_bytes, true}};
    if (aesr_any_overlap(bufs, 4)) {
        aesr_set_error("%s: an output overlaps an input, the workspace or another output", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* my = (double*)(ws + L.my);
    long long* list_tab = (long long*)(ws + L.list_tab);
    int* gx = (int*)(ws + L.gx);
    const unsigned int* block_off = (const unsigned int*)(ws + L.block_off);
    const unsigned char* flags = (const unsigned char*)(ws + L.flags);
    const int V = (int)L.V, Vp = (int)L.Vp, lists = N * C * 2;
    const long long lines = (long long)lists * Z * H;          // <= 16 * N * V / W < 2^35
    const long long xblocks = (lines + SURF_THREADS / 64 - 1) / (SURF_THREADS / 64);
    const int xt = ceil_div(W, SURF_YCOLS), yt = ceil_div(H, SURF_YCOLS * SURF_YROWS);
    const long long yblocks = (long long)lists * Z * xt * yt;
    AESR_CHECK_ARG(xblocks < 2147483648LL && yblocks < 2147483648LL, "%s: %d lists of %d x %d x %d voxels need more workgroups than a launch has",
                   fn, lists, Z, H, W);
    hipLaunchKernelGGL(surf_offsets_kernel, dim3(1), dim3(SURF_SCAN_THREADS), 0, st, counts, list_tab, lists);
    AESR_LAUNCH_CHECK("surface_offsets");
    hipLaunchKernelGGL(surf_xpass_kernel, dim3((unsigned int)xblocks), dim3(SURF_THREADS), 0, st, flags, gx, C, V, Vp, W, lines, Z * H);
    AESR_LAUNCH_CHECK("surface_xpass");
    hipLaunchKernelGGL(surf_ypass_kernel, dim3((unsigned int)yblocks), dim3(SURF_THREADS), 0, st, (const int*)gx, my, H, W, xt, yt, spacing[1],
                       spacing[2]);
    AESR_LAUNCH_CHECK("surface_ypass");
    hipLaunchKernelGGL(surf_gather_kernel, dim3((unsigned int)(N * L.nb)), dim3(SURF_THREADS), 0, st, (const unsigned int*)flags, block_off,
                       (const long long*)list_tab, (const double*)my, distances, (unsigned long long)capacity, C, V, Vp, Z, H, W, L.nb,
                       ndim == 3 ? 1 : 0, spacing[0]);
    AESR_LAUNCH_CHECK("surface_gather");
    hipLaunchKernelGGL(surf_reduce_kernel, dim3((unsigned int)lists), dim3(SURF_THREADS), 0, st, (const double*)distances,
                       (const long long*)list_tab, stats, (unsigned long long)capacity);
    AESR_LAUNCH_CHECK("surface_reduce");
    return AESR_OK;
}

}  // extern "C"
