// Shape-based interpolation of label maps on the device (Raya & Udupa 1990, Herman et al. 1992): signed Euclidean distance maps of every
// class in every slice, then per output slice a linear blend of the maps of the two neighbouring input slices and an arg-max over the
// classes.  include/aesr_hip_shape.h states the definitions.
//
//   signed distances (aesr_shape_signed_distances), the structure of seg_metrics.hip's distance transform, 2-D per slice:
//     x pass   one wave per line (n, class, z, y): the line's pixels of the class as 64-bit ballot masks in LDS, and the complement of the
//              mask inside the line; every lane finds the nearest set bit of both with clz / ctz.  Two int fields in the workspace,
//              gx[(n, class)][side][z][y][x]: side 0 the index distance to the nearest pixel OF the class (0 on the class itself), side 1
//              to the nearest pixel NOT of it; SHP_NONE where the line holds none.
//     y pass   per pixel min_y' ((dy sy) (dy sy) + (gx sx) (gx sx)) in fp64 by brute force over the column, both sides staged in LDS
//              SHP_YCHUNK rows at a time; a pixel of the class (side 0 is 0 there) minimises over side 1 and gets +sqrt, any other pixel
//              minimises over side 0 and gets -sqrt; a minimum over nothing stays +inf and becomes BIG, which the host computed.
//   blend and arg-max (aesr_shape_interpolate): a lane owns 4 consecutive pixels of an output slice (one 32-bit store) or one (a byte);
//     the output slice, hence gap and alpha, is the same in every lane of a workgroup; gap is clamped in the kernel.
// No atomics, no buffer that needs initialisation, no workgroup waits on another; which thread takes which pixel depends on the sizes
// alone, and every loop is bounded by a size argument.
#include "aesr_kernels.h"
#include "aesr_hostcheck.h"
#include "../../include/aesr_hip_shape.h"

#include <cmath>

#pragma clang fp contract(off)

#define SHP_THREADS 256
#define SHP_MAXC AESR_SHAPE_MAX_CLASSES
#define SHP_MAX_W AESR_SHAPE_MAX_W                // longest line the x pass supports
#define SHP_XWORDS (SHP_MAX_W / 64)
#define SHP_NONE 0x7fffffff                       // x pass: the line holds no pixel of this side
#define SHP_YCOLS 16
#define SHP_YROWS 4                               // output rows per thread of the y pass
#define SHP_YCHUNK 128                            // column rows staged at a time: 2 sides * 128 * 16 * 8 B = 32 KB

static_assert(SHP_MAXC == AESR_MAX_CLASSES, "the class table of the label-volume files holds AESR_MAX_CLASSES classes");

struct ShpClasses {
    int v[SHP_MAXC];          // the class values, ascending; entries from C on are unused
};

// the value of class c without indexing the kernel arguments by a register
__device__ __forceinline__ int shp_class_value(const ShpClasses& cls, int c) {
    int v = 0;
#pragma unroll
    for (int i = 0; i < SHP_MAXC; ++i)
        if (i == c) v = cls.v[i];
    return v;
}

// index distance from pixel k0 * 64 + lane to the nearest set bit of the nw words at mk, SHP_NONE if no bit is set
__device__ __forceinline__ int shp_nearest(const unsigned long long* mk, int nw, int k0, int lane) {
    const int x = k0 * 64 + lane;
    int best = SHP_NONE;
    for (int k = 0; k < nw; ++k) {
        const unsigned long long m = mk[k];
        if (m == 0) continue;          // uniform
        if (k < k0) best = min(best, x - (k * 64 + 63 - __clzll((long long)m)));
        else if (k > k0) best = min(best, k * 64 + (__ffsll((long long)m) - 1) - x);
        else {
            const unsigned long long le = m & (~0ull >> (63 - lane)), ge = m & (~0ull << lane);
            if (le) best = min(best, lane - (63 - __clzll((long long)le)));
            if (ge) best = min(best, (__ffsll((long long)ge) - 1) - lane);
        }
    }
    return best;
}

// one wave per line: line = ((n * C + c) * Z + z) * H + y; ZH = Z * H
__global__ __launch_bounds__(SHP_THREADS) void shp_xpass_kernel(const unsigned char* __restrict__ labels, int* __restrict__ gx, ShpClasses cls,
                                                                int C, int ZH, int W, long long lines) {
    __shared__ unsigned long long mask[SHP_THREADS / 64][2][SHP_XWORDS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long line = (long long)blockIdx.x * (SHP_THREADS / 64) + wave;
    const bool active = line < lines;          // whole waves; an idle wave still takes part in the barrier
    const int nc = active ? (int)(line / ZH) : 0, zy = active ? (int)(line - (long long)nc * ZH) : 0;
    const int n = nc / C, c = nc - n * C;
    const unsigned char value = (unsigned char)shp_class_value(cls, c);
    const unsigned char* __restrict__ lab = labels + ((size_t)n * ZH + zy) * W;
    const int nw = active ? (W + 63) / 64 : 0;
    for (int k = 0; k < nw; ++k) {
        const int x = k * 64 + lane;
        const bool inside = x < W;
        const unsigned long long m = __ballot(inside && lab[x] == value), all = __ballot(inside);
        if (lane == 0) {
            mask[wave][0][k] = m;
            mask[wave][1][k] = all & ~m;
        }
    }
    __syncthreads();
    int* __restrict__ o0 = gx + ((size_t)nc * 2 * ZH + zy) * W;
    int* __restrict__ o1 = o0 + (size_t)ZH * W;
    for (int k0 = 0; k0 < nw; ++k0) {
        const int x = k0 * 64 + lane;
        const int d0 = shp_nearest(mask[wave][0], nw, k0, lane), d1 = shp_nearest(mask[wave][1], nw, k0, lane);
        if (x < W) {
            o0[x] = d0;
            o1[x] = d1;
        }
    }
}

// workgroup ((n, c), z, y tile of 64 rows, x tile of 16 columns); thread (tx, ty) the rows y0 + ty + 16 r of column x0 + tx
__global__ __launch_bounds__(SHP_THREADS) void shp_ypass_kernel(const int* __restrict__ gx, double* __restrict__ sdm, int Z, int H, int W, int xt,
                                                                int yt, double sy, double sx, double big) {
    __shared__ double col[2][SHP_YCHUNK][SHP_YCOLS];
    const int tx = threadIdx.x & (SHP_YCOLS - 1), ty = threadIdx.x / SHP_YCOLS;
    unsigned int bid = blockIdx.x;
    const int bx = bid % xt; bid /= xt;
    const int by = bid % yt; bid /= yt;          // bid: (n * C + c) * Z + z
    const unsigned int nc = bid / Z, z = bid - nc * Z;
    const size_t HW = (size_t)H * W;
    const int* __restrict__ g0 = gx + ((size_t)nc * 2 * Z + z) * HW;          // side 0: to the nearest pixel of the class
    const int* __restrict__ g1 = g0 + (size_t)Z * HW;                         // side 1: to the nearest pixel outside it
    const int x = bx * SHP_YCOLS + tx, y0 = by * (SHP_YCOLS * SHP_YROWS) + ty;
    double m[SHP_YROWS];
    bool member[SHP_YROWS];
#pragma unroll
    for (int r = 0; r < SHP_YROWS; ++r) {
        const int y = y0 + SHP_YCOLS * r;
        m[r] = INFINITY;
        member[r] = x < W && y < H && g0[(size_t)y * W + x] == 0;
    }
    for (int c0 = 0; c0 < H; c0 += SHP_YCHUNK) {
        const int rows = min(SHP_YCHUNK, H - c0);
        __syncthreads();
        for (int i = ty; i < rows; i += SHP_THREADS / SHP_YCOLS) {
            double t0 = INFINITY, t1 = INFINITY;
            if (x < W) {
                const int a = g0[(size_t)(c0 + i) * W + x], b = g1[(size_t)(c0 + i) * W + x];
                if (a != SHP_NONE) {
                    const double d = (double)a * sx;
                    t0 = d * d;
                }
                if (b != SHP_NONE) {
                    const double d = (double)b * sx;
                    t1 = d * d;
                }
            }
            col[0][i][tx] = t0;
            col[1][i][tx] = t1;
        }
        __syncthreads();
        for (int i = 0; i < rows; ++i) {
            const double t0 = col[0][i][tx], t1 = col[1][i][tx];
#pragma unroll
            for (int r = 0; r < SHP_YROWS; ++r) {
                const double d = (double)(y0 + SHP_YCOLS * r - (c0 + i)) * sy;
                m[r] = fmin(m[r], d * d + (member[r] ? t1 : t0));          // inf + finite = inf: no NaN can arise
            }
        }
    }
    if (x < W) {
        double* __restrict__ o = sdm + (size_t)bid * HW;
#pragma unroll
        for (int r = 0; r < SHP_YROWS; ++r) {
            const int y = y0 + SHP_YCOLS * r;
            if (y < H) {
                const double mag = m[r] == INFINITY ? big : sqrt(m[r]);
                o[(size_t)y * W + x] = member[r] ? mag : -mag;
            }
        }
    }
}

// workgroup (n, j, strip of 256 units); V = 4: a unit is 4 consecutive pixels and one 32-bit store, V = 1: one pixel, one byte
template <int V>
__global__ __launch_bounds__(SHP_THREADS) void shp_blend_kernel(const double* __restrict__ sdm, const int* __restrict__ gap,
                                                                const double* __restrict__ alpha, unsigned char* __restrict__ out, ShpClasses cls,
                                                                int C, int Z, unsigned int HW, unsigned int units, unsigned int strips, int J) {
    unsigned int bid = blockIdx.x;
    const unsigned int strip = bid % strips; bid /= strips;
    const unsigned int j = bid % (unsigned int)J, n = bid / (unsigned int)J;
    const unsigned int u = strip * SHP_THREADS + threadIdx.x;
    if (u >= units) return;
    // whatever the table holds, g and g1 are slices of the volume
    const int top = Z >= 2 ? Z - 2 : 0, gj = gap[j];
    const int g = gj < 0 ? 0 : (gj > top ? top : gj), g1 = g + 1 < Z ? g + 1 : Z - 1;
    const double a = alpha[j], om = 1.0 - a;
    const size_t p = (size_t)u * V;
    double best[V];
    int which[V];
#pragma unroll
    for (int c = 0; c < SHP_MAXC; ++c) {
        if (c < C) {
            const double* __restrict__ s0 = sdm + (((size_t)n * C + c) * Z + g) * HW + p;
            const double* __restrict__ s1 = sdm + (((size_t)n * C + c) * Z + g1) * HW + p;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double val = om * s0[v] + a * s1[v];
                if (c == 0 || val > best[v]) {          // strictly greater: ties stay with the smaller class value
                    best[v] = val;
                    which[v] = cls.v[c];
                }
            }
        }
    }
    unsigned char* __restrict__ o = out + ((size_t)n * J + j) * HW + p;
    if (V == 4) {
        *reinterpret_cast<unsigned int*>(o) = (unsigned int)which[0] | (unsigned int)which[V > 1 ? 1 : 0] << 8 |
                                              (unsigned int)which[V > 2 ? 2 : 0] << 16 | (unsigned int)which[V > 3 ? 3 : 0] << 24;
    } else {
        o[0] = (unsigned char)which[0];
    }
}

// sizes the entry points share; 0 = fine, else the code with the message set (fn == NULL: silent, for the query)
static int shp_check_sizes(const char* fn, int N, int Z, int H, int W, int C) {
    if (N <= 0 || Z <= 0 || H <= 0 || W <= 0) {
        if (fn) aesr_set_error("%s: N, Z, H, W = %d, %d, %d, %d must all be positive", fn, N, Z, H, W);
        return AESR_ERR_ARG;
    }
    if (C < 1 || C > SHP_MAXC) {
        if (fn) aesr_set_error("%s: C=%d classes, 1 to %d are supported", fn, C, SHP_MAXC);
        return AESR_ERR_ARG;
    }
    if ((double)N * C * Z * H * W >= 2147483648.0) {
        if (fn) aesr_set_error("%s: N * C * Z * H * W = %d x %d x %d x %d x %d has 2^31 elements or more", fn, N, C, Z, H, W);
        return AESR_ERR_ARG;
    }
    return AESR_OK;
}

static int shp_fill_classes(const char* fn, const int* classes_host, int C, ShpClasses* cls) {
    for (int c = 0; c < SHP_MAXC; ++c) cls->v[c] = 0;
    for (int c = 0; c < C; ++c) {
        AESR_CHECK_ARG(classes_host[c] >= 0 && classes_host[c] <= 255, "%s: classes_host[%d]=%d is not a label value in 0..255", fn, c,
                       classes_host[c]);
        AESR_CHECK_ARG(c == 0 || classes_host[c] > classes_host[c - 1], "%s: classes_host is not ascending (%d follows %d)", fn, classes_host[c],
                       c ? classes_host[c - 1] : 0);
        cls->v[c] = classes_host[c];
    }
    return AESR_OK;
}

extern "C" {

size_t aesr_shape_workspace_bytes(int N, int Z, int H, int W, int C) {
    if (shp_check_sizes(NULL, N, Z, H, W, C) != AESR_OK || W > SHP_MAX_W) return 0;
    return aesr_up16((size_t)N * C * 2 * Z * H * W * sizeof(int));          // the two fields of the x pass
}

int aesr_shape_signed_distances(const uint8_t* labels, double* sdm, void* workspace, size_t workspace_bytes, int N, int Z, int H, int W,
                                const int* classes_host, int C, double sy, double sx, void* stream) {
    const char* fn = "aesr_shape_signed_distances";
    AESR_CHECK_ARG(labels, "%s: labels is a null pointer", fn);
    AESR_CHECK_ARG(sdm, "%s: sdm is a null pointer", fn);
    AESR_CHECK_ARG(workspace, "%s: workspace is a null pointer", fn);
    AESR_CHECK_ARG(classes_host, "%s: classes_host is a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)sdm % 8 == 0, "%s: sdm is not 8-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace is not 16-byte aligned", fn);
    const int rc = shp_check_sizes(fn, N, Z, H, W, C);
    if (rc != AESR_OK) return rc;
    ShpClasses cls;
    const int rc_cls = shp_fill_classes(fn, classes_host, C, &cls);
    if (rc_cls != AESR_OK) return rc_cls;
    AESR_CHECK_ARG(sy > 0.0 && std::isfinite(sy), "%s: sy=%g must be positive and finite", fn, sy);
    AESR_CHECK_ARG(sx > 0.0 && std::isfinite(sx), "%s: sx=%g must be positive and finite", fn, sx);
    if (W > SHP_MAX_W) {
        aesr_set_error("%s: W=%d, lines of up to %d pixels are supported", fn, W, SHP_MAX_W);
        return AESR_ERR_UNSUPPORTED;
    }
    const size_t need = aesr_shape_workspace_bytes(N, Z, H, W, C);
    AESR_CHECK_ARG(workspace_bytes >= need, "%s: workspace_bytes=%zu, %zu are needed", fn, workspace_bytes, need);
    const size_t vox = (size_t)N * Z * H * W;
    const AesrBuf bufs[3] = {{labels, vox, false}, {sdm, vox * C * 8, true}, {workspace, need, true}};
    if (aesr_any_overlap(bufs, 3)) {
        aesr_set_error("%s: sdm or workspace overlaps labels or the other", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    const double hy = (double)H * sy, wx = (double)W * sx;
    const double big = std::sqrt(hy * hy + wx * wx);
    AESR_CHECK_ARG(std::isfinite(big), "%s: sy=%g, sx=%g: the extent of a slice is not finite in fp64", fn, sy, sx);
    hipStream_t st = (hipStream_t)stream;
    int* gx = (int*)workspace;
    const long long lines = (long long)N * C * Z * H;          // < 2^31
    const long long xblocks = (lines + SHP_THREADS / 64 - 1) / (SHP_THREADS / 64);
    const int xt = ceil_div(W, SHP_YCOLS), yt = ceil_div(H, SHP_YCOLS * SHP_YROWS);
    const long long yblocks = (long long)N * C * Z * xt * yt;          // <= N * C * Z * H * W < 2^31
    hipLaunchKernelGGL(shp_xpass_kernel, dim3((unsigned int)xblocks), dim3(SHP_THREADS), 0, st, (const unsigned char*)labels, gx, cls, C, Z * H, W,
                       lines);
    AESR_LAUNCH_CHECK("shape_xpass");
    hipLaunchKernelGGL(shp_ypass_kernel, dim3((unsigned int)yblocks), dim3(SHP_THREADS), 0, st, (const int*)gx, sdm, Z, H, W, xt, yt, sy, sx, big);
    AESR_LAUNCH_CHECK("shape_ypass");
    return AESR_OK;
}

int aesr_shape_interpolate(const double* sdm, const int* gap, const double* alpha, uint8_t* out, int N, int C, int Z, int H, int W, int J,
                           const int* classes_host, void* stream) {
    const char* fn = "aesr_shape_interpolate";
    AESR_CHECK_ARG(sdm, "%s: sdm is a null pointer", fn);
    AESR_CHECK_ARG(gap, "%s: gap is a null pointer", fn);
    AESR_CHECK_ARG(alpha, "%s: alpha is a null pointer", fn);
    AESR_CHECK_ARG(out, "%s: out is a null pointer", fn);
    AESR_CHECK_ARG(classes_host, "%s: classes_host is a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)sdm % 8 == 0, "%s: sdm is not 8-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)alpha % 8 == 0, "%s: alpha is not 8-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)gap % 4 == 0, "%s: gap is not 4-byte aligned", fn);
    const int rc = shp_check_sizes(fn, N, Z, H, W, C);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(J > 0, "%s: J=%d must be positive", fn, J);
    AESR_CHECK_ARG((double)N * J * H * W < 2147483648.0, "%s: N * J * H * W = %d x %d x %d x %d has 2^31 elements or more", fn, N, J, H, W);
    ShpClasses cls;
    const int rc_cls = shp_fill_classes(fn, classes_host, C, &cls);
    if (rc_cls != AESR_OK) return rc_cls;
    const size_t HW = (size_t)H * W;
    const AesrBuf bufs[4] = {{sdm, (size_t)N * C * Z * HW * 8, false}, {gap, (size_t)J * 4, false}, {alpha, (size_t)J * 8, false},
                             {out, (size_t)N * J * HW, true}};
    if (aesr_any_overlap(bufs, 4)) {
        aesr_set_error("%s: out overlaps sdm, gap or alpha", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    const bool vec = HW % 4 == 0 && (uintptr_t)out % 4 == 0;
    const unsigned int units = (unsigned int)(vec ? HW / 4 : HW);
    const unsigned int strips = (units + SHP_THREADS - 1) / SHP_THREADS;
    const long long blocks = (long long)N * J * strips;          // <= N * J * H * W < 2^31
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL((shp_blend_kernel<4>), dim3((unsigned int)blocks), dim3(SHP_THREADS), 0, st, sdm, gap, alpha, (unsigned char*)out, cls, C,
                           Z, (unsigned int)HW, units, strips, J);
    else
        hipLaunchKernelGGL((shp_blend_kernel<1>), dim3((unsigned int)blocks), dim3(SHP_THREADS), 0, st, sdm, gap, alpha, (unsigned char*)out, cls, C,
                           Z, (unsigned int)HW, units, strips, J);
    AESR_LAUNCH_CHECK("shape_blend");
    return AESR_OK;
}

}  // extern "C"
