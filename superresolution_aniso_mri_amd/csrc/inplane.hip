// In-plane resampling of N slices [N][H][W] -> [N][Ho][Wo] (the reference's datasets/common.py:157-206 apply_2d_zoom_3d / _4d: per slice
// scipy.ndimage.gaussian_filter(slice, 0.25 / zoom), then scipy.ndimage.zoom(volume, (1, zy, zx), order=1)) as ONE launch.
// The caller makes every coordinate decision on the host in float64 (include/aesr_hip_preproc.h): per output row / column the first
// input index, the linear weight and whether the line is dead (exactly 0).  The kernel only looks them up.
//   - a workgroup (256 threads) owns an output tile of TH x TW (the launcher picks them: TW <= 64 so that a staged row is one wave wide
//     where the zoom allows, TH <= 32 so that the tile's LDS stays within IP_LDS_BYTES);
//   - it stages the tile's input footprint in LDS: the rows / columns its taps reach plus `radius` on each side for the blur, the
//     reflect boundary (d c b a | a b c d) resolved while staging -- a wave takes a row, its lanes run along w (256 contiguous bytes);
//   - H blur A -> B, W blur B -> A, each tap sum in double in scipy's order (centre, then the pairs from the outermost inwards) and
//     rounded to fp32 where scipy rounds (it filters fp32 input in double and stores fp32 after each pass); skipped for do_blur = 0;
//   - the four bilinear taps are gathered from LDS, summed in double, rounded once and stored along w: 16 bytes per lane when Wo % 4 == 0
//     and `out` is 16-byte aligned (a tile row starts at a multiple of 4), 4 bytes per lane (256 contiguous bytes per wave) otherwise.
// The input is read once (plus halos, which neighbouring workgroups find in L2), the output written once; no HBM scratch, no atomics.
// LDS rows have an odd pitch: the vector-store gather reads four rows per wave instruction, and an odd pitch spreads them over the banks.
#include <math.h>

#include <vector>

#include "../../include/aesr_hip_preproc.h"
#include "aesr_kernels.h"

#define IP_MAXR 8
#define IP_THREADS 256
#define IP_LDS_BYTES (32 * 1024)

__device__ __forceinline__ int ip_reflect(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// device copies of the host tables, all inside the caller's workspace: [ty | tx | wy (IP_MAXR + 1) | wx (IP_MAXR + 1)] doubles, then
// [iy | ix] ints.  wy[k], k = 0..ry: the centre weight and the right half of the symmetric kernel.
struct IpTables {
    const double *ty, *tx, *wy, *wx;
    const int *iy, *ix;
};

__device__ __forceinline__ float ip_tap(const float* __restrict__ C, int P, int r0, int r1, int c0, int c1, double ty, double tx) {
    const double wy0 = 1.0 - ty, wx0 = 1.0 - tx;
    double v = (double)C[r0 * P + c0] * wy0 * wx0;
    v += (double)C[r0 * P + c1] * wy0 * tx;
    v += (double)C[r1 * P + c0] * ty * wx0;
    v += (double)C[r1 * P + c1] * ty * tx;
    return (float)v;
}

// 1-D grid: block = (n * nty + tile_y) * ntx + tile_x, x tiles fastest.  LDS: A = rowsA x P floats, then B (blur only).
template <bool VEC4>
__global__ __launch_bounds__(IP_THREADS) void inplane_kernel(const float* __restrict__ in, float* __restrict__ out, IpTables tb, int H, int W,
                                                             int Ho, int Wo, int TH, int TW, int ntx, int tps, int P, int rowsA, int ry, int rx,
                                                             int do_blur) {
    extern __shared__ float ip_lds[];
    float* __restrict__ A = ip_lds;
    float* __restrict__ B = ip_lds + rowsA * P;
    const unsigned int b = blockIdx.x;
    const int n = b / tps, t = b - n * tps, tyi = t / ntx, txi = t - tyi * ntx;
    const int oy0 = tyi * TH, oy1 = min(oy0 + TH, Ho), ox0 = txi * TW, ox1 = min(ox0 + TW, Wo);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the tile's source span, from the tables (only the last line of an axis can be dead; a tile that starts with it has nothing to stage)
    const int ya = tb.iy[oy0], xa = tb.ix[ox0];
    if (ya >= 0 && xa >= 0) {                       // uniform over the workgroup
        int yl = tb.iy[oy1 - 1], xl = tb.ix[ox1 - 1];
        if (yl < 0) yl = tb.iy[oy1 - 2];
        if (xl < 0) xl = tb.ix[ox1 - 2];
        const int FH = min(yl + 1, H - 1) - ya + 1, FW = min(xl + 1, W - 1) - xa + 1;
        const int hy = do_blur ? ry : 0, hx = do_blur ? rx : 0;
        const int RA = FH + 2 * hy, CA = FW + 2 * hx;          // <= rowsA, <= P (the launcher sized them for the largest tile)
        const float* __restrict__ src = in + (size_t)n * H * W;
        for (int r = wave; r < RA; r += 4) {
            const float* __restrict__ row = src + (size_t)ip_reflect(ya - hy + r, H) * W;
            for (int c = lane; c < CA; c += 64) A[r * P + c] = row[ip_reflect(xa - hx + c, W)];
        }
        __syncthreads();
        if (do_blur) {
            // along H: B[r][c] = blurred row ya + r, for every staged column
            const double w0 = tb.wy[0];
            for (int r = wave; r < FH; r += 4)
                for (int c = lane; c < CA; c += 64) {
                    const float* __restrict__ p = A + (r + ry) * P + c;
                    double acc = (double)p[0] * w0;
                    for (int k = ry; k >= 1; --k) acc += ((double)p[-k * P] + (double)p[k * P]) * tb.wy[k];
                    B[r * P + c] = (float)acc;
                }
            __syncthreads();
            // along W: A[r][c] = blurred (ya + r, xa + c)
            const double v0 = tb.wx[0];
            for (int r = wave; r < FH; r += 4)
                for (int c = lane; c < FW; c += 64) {
                    const float* __restrict__ p = B + r * P + c + rx;
                    double acc = (double)p[0] * v0;
                    for (int k = rx; k >= 1; --k) acc += ((double)p[-k] + (double)p[k]) * tb.wx[k];
                    A[r * P + c] = (float)acc;
                }
            __syncthreads();
        }
    }
    float* __restrict__ dst = out + (size_t)n * Ho * Wo;
    if (VEC4) {
        // TW <= 64 and TW, Wo multiples of 4: 16 lanes cover a tile row, a wave covers 4 rows
        const int ox = ox0 + 4 * (lane & 15);
        if (ox >= ox1) return;
        int c0[4], c1[4];
        double tx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = tb.ix[ox + j];
            tx[j] = tb.tx[ox + j];
            c0[j] = i < 0 ? -1 : i - xa;
            c1[j] = min(i + 1, W - 1) - xa;
        }
        for (int oy = oy0 + wave * 4 + (lane >> 4); oy < oy1; oy += 16) {
            const int i = tb.iy[oy];
            const double ty = tb.ty[oy];
            const int r0 = i - ya, r1 = min(i + 1, H - 1) - ya;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (i < 0 || c0[j] < 0) ? 0.f : ip_tap(A, P, r0, r1, c0[j], c1[j], ty, tx[j]);
            *(f32x4*)(dst + (size_t)oy * Wo + ox) = v;
        }
    } else {
        for (int ox = ox0 + lane; ox < ox1; ox += 64) {
            const int ixv = tb.ix[ox];
            const double tx = tb.tx[ox];
            const int c0 = ixv - xa, c1 = min(ixv + 1, W - 1) - xa;
            for (int oy = oy0 + wave; oy < oy1; oy += 4) {
                const int i = tb.iy[oy];
                float v = 0.f;
                if (i >= 0 && ixv >= 0) v = ip_tap(A, P, i - ya, min(i + 1, H - 1) - ya, c0, c1, tb.ty[oy], tx);
                dst[(size_t)oy * Wo + ox] = v;
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static bool ip_table_ok(const int* i0, const double* t, int n_out, int n) {
    int prev = 0;
    for (int o = 0; o < n_out; ++o) {
        if (i0[o] == -1 && o == n_out - 1) continue;
        if (i0[o] < prev || i0[o] > n - 1 || !(t[o] >= 0.0 && t[o] <= 1.0)) return false;
        prev = i0[o];
    }
    return true;
}

// the longest source span (first index .. last index + 1, clamped) of any tile of `tile` outputs
static int ip_max_span(const int* i0, int n_out, int n, int tile) {
    int best = 0;
    for (int o0 = 0; o0 < n_out; o0 += tile) {
        if (i0[o0] < 0) continue;
        int o1 = (n_out - o0 < tile ? n_out : o0 + tile) - 1;
        if (i0[o1] < 0) --o1;
        const int hi = i0[o1] + 1 < n - 1 ? i0[o1] + 1 : n - 1;
        if (hi - i0[o0] + 1 > best) best = hi - i0[o0] + 1;
    }
    return best;
}

static bool ip_symmetric(const double* w, int r) {
    for (int k = 1; k <= r; ++k)
        if (w[r - k] != w[r + k]) return false;
    return true;
}

static size_t ip_workspace_bytes(int Ho, int Wo) {
    return ((size_t)Ho + Wo + 2 * (IP_MAXR + 1)) * sizeof(double) + ((size_t)Ho + Wo + 1) / 2 * 2 * sizeof(int);
}

extern "C" {

int aesr_inplane_out_size(int n, double zoom) {
    if (n <= 0 || !(zoom > 0.0) || !isfinite(zoom)) return 0;
    const double r = nearbyint((double)n * zoom);          // the default rounding mode: halves to even, like Python's round
    return r >= 1.0 && r < 2147483647.0 ? (int)r : 0;
}

size_t aesr_inplane_workspace_bytes(int Ho, int Wo) { return Ho > 0 && Wo > 0 ? ip_workspace_bytes(Ho, Wo) : 0; }

int aesr_inplane_resample(const float* in, float* out, void* workspace, int N, int H, int W, int Ho, int Wo, const double* wy_host, int ry,
                          const double* wx_host, int rx, const int* iy_host, const double* ty_host, const int* ix_host,
                          const double* tx_host, int do_blur, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AESR_CHECK_ARG(in && out && workspace && iy_host && ty_host && ix_host && tx_host, "aesr_inplane_resample: null pointer");
    AESR_CHECK_ARG(!do_blur || (wy_host && wx_host), "aesr_inplane_resample: do_blur needs both weight arrays");
    AESR_CHECK_ARG(N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "aesr_inplane_resample: empty shape %d x %d x %d -> %d x %d", N, H, W, Ho, Wo);
    AESR_CHECK_ARG((size_t)H * W < ((size_t)1 << 30) && (size_t)Ho * Wo < ((size_t)1 << 30),
                   "aesr_inplane_resample: a slice of %d x %d -> %d x %d has 2^30 elements or more", H, W, Ho, Wo);
    AESR_CHECK_ARG((uintptr_t)workspace % 8 == 0, "aesr_inplane_resample: the workspace must be 8-byte aligned");
    if (do_blur) {
        AESR_CHECK_ARG(ry >= 0 && rx >= 0, "aesr_inplane_resample: negative radius (%d, %d)", ry, rx);
        if (ry > IP_MAXR || rx > IP_MAXR) {
            aesr_set_error("aesr_inplane_resample: blur radius (%d, %d) exceeds the supported %d per axis (zoom below ~0.12)", ry, rx, IP_MAXR);
            return AESR_ERR_UNSUPPORTED;
        }
        AESR_CHECK_ARG(ip_symmetric(wy_host, ry) && ip_symmetric(wx_host, rx), "aesr_inplane_resample: the blur weights must be symmetric");
    } else {
        ry = rx = 0;
    }
    AESR_CHECK_ARG(ip_table_ok(iy_host, ty_host, Ho, H), "aesr_inplane_resample: the row table is not a valid (index, weight, dead) table for H=%d", H);
    AESR_CHECK_ARG(ip_table_ok(ix_host, tx_host, Wo, W), "aesr_inplane_resample: the column table is not a valid (index, weight, dead) table for W=%d", W);
    // tile: the widest TW (multiple of 4, <= 64) whose staged rows are one wave wide, then the tallest TH whose footprint fits the LDS
    int TW = 4, spanW = 0;
    for (int tw = 64; tw >= 4; tw -= 4) {
        spanW = ip_max_span(ix_host, Wo, W, tw);
        if (spanW + 2 * rx <= 64 || tw == 4) {
            TW = tw;
            break;
        }
    }
    int TH = 0, spanH = 0, P = 0;
    size_t lds = 0;
    for (int th = 32; th >= 1; th /= 2) {
        spanH = ip_max_span(iy_host, Ho, H, th);
        P = (spanW + 2 * rx) | 1;
        lds = ((size_t)spanH + 2 * ry + (do_blur ? spanH : 0)) * P * sizeof(float);
        if (lds <= IP_LDS_BYTES) {
            TH = th;
            break;
        }
    }
    if (TH == 0) {
        aesr_set_error("aesr_inplane_resample: a one-row tile needs %zu bytes of LDS, more than the supported %d (source span %d x %d)", lds,
                       IP_LDS_BYTES, spanH, spanW);
        return AESR_ERR_UNSUPPORTED;
    }
    const int ntx = ceil_div(Wo, TW), nty = ceil_div(Ho, TH);
    const size_t tiles = (size_t)N * ntx * nty;
    AESR_CHECK_ARG(tiles < ((size_t)1 << 31), "aesr_inplane_resample: %d slices of %d x %d need %zu tiles", N, Ho, Wo, tiles);
    // pack the tables and copy them into the workspace; the host arrays are the caller's: wait until the copy has read them
    const size_t nd = (size_t)Ho + Wo + 2 * (IP_MAXR + 1), bytes = ip_workspace_bytes(Ho, Wo);
    std::vector<double> pack(bytes / sizeof(double), 0.0);
    double* d = pack.data();
    for (int o = 0; o < Ho; ++o) d[o] = ty_host[o];
    for (int o = 0; o < Wo; ++o) d[Ho + o] = tx_host[o];
    double* wy = d + Ho + Wo;
    double* wx = wy + IP_MAXR + 1;
    wy[0] = wx[0] = 1.0;
    if (do_blur) {
        for (int k = 0; k <= ry; ++k) wy[k] = wy_host[ry + k];
        for (int k = 0; k <= rx; ++k) wx[k] = wx_host[rx + k];
    }
    int* ii = (int*)(d + nd);
    for (int o = 0; o < Ho; ++o) ii[o] = iy_host[o];
    for (int o = 0; o < Wo; ++o) ii[Ho + o] = ix_host[o];
    hipError_t e = hipMemcpyAsync(workspace, pack.data(), bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        aesr_set_error("aesr_inplane_resample: copying the tables failed: %s", hipGetErrorString(e));
        return AESR_ERR_HIP;
    }
    const double* dd = (const double*)workspace;
    IpTables tb;
    tb.ty = dd;
    tb.tx = dd + Ho;
    tb.wy = dd + Ho + Wo;
    tb.wx = tb.wy + IP_MAXR + 1;
    tb.iy = (const int*)(dd + nd);
    tb.ix = tb.iy + Ho;
    const int rowsA = spanH + 2 * ry;
    if (Wo % 4 == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(inplane_kernel<true>, dim3((unsigned int)tiles), dim3(IP_THREADS), lds, st, in, out, tb, H, W, Ho, Wo, TH, TW, ntx,
                           ntx * nty, P, rowsA, ry, rx, do_blur ? 1 : 0);
    else
        hipLaunchKernelGGL(inplane_kernel<false>, dim3((unsigned int)tiles), dim3(IP_THREADS), lds, st, in, out, tb, H, W, Ho, Wo, TH, TW, ntx,
                           ntx * nty, P, rowsA, ry, rx, do_blur ? 1 : 0);
    AESR_LAUNCH_CHECK("inplane_resample");
    return AESR_OK;
}

}  // extern "C"
