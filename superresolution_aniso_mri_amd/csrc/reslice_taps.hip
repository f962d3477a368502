// Affine reslicing with a higher-order kernel at a free 3-D position: cubic B-spline over a separable 3-D pre-filter, Lanczos- and
// cosine-windowed sinc (ITK's WindowedSincInterpolateImageFunction, the reference's kwatsch/create_nifti_from_dicom.py:202-253).
// csrc/reslice_taps.h has the contract.
// The tap gather:
//   - one lane per output voxel, lanes along the output x, a workgroup (256 threads) on a 64 x 4 tile of one output slice, as in reslice.hip:
//     an output row is a straight line through the source, so neighbouring lanes read neighbouring addresses;
//   - the position comes from reslice.hip's own device function (reslice_position.h).  Per axis the T = 2 R weights and element offsets are
//     made ONCE per voxel and reused for the N frames.  Of sin(pi (t - k)) = +-sin(pi t) one sinpi per axis remains for the sinc factor; the
//     window's sine or cosine at t - k comes from one sincospi per axis (two for Lanczos: rtp_axis) and the angle-sum rule: cos and sin
//     of k pi / R (k pi / (2 R)) have constant arguments once the tap loop is unrolled and are folded at compile time;
//   - the x and y arrays stay in registers: the ky and kx loops are unrolled on the template's tap count, every index a compile-time
//     constant.  The z arrays go to LDS, one column per lane ([T][256]: a wave reads 64 consecutive doubles, no bank conflict, no barrier --
//     a lane reads only what it wrote), and kz is a rolled loop: the body is T x T taps, not T^3 (22 KiB of code at R = 5; 1000 taps
//     unrolled would be several times the 64 KiB instruction cache).  The T loads of a row are issued together, ahead of their sum;
//   - per frame and voxel T^3 loads, T^2 (T + 1) multiplies and T^3 adds in fp64, summed kz, ky, kx ascending, one rounding to fp32.
// The pre-filter: z by aesr_bspline_prefilter_z (fp32 -> fp64), then in place on the fp64 buffer
//   - y: one thread per (frame, z, x) line, lanes along x: every load and store of a wave is one contiguous row segment;
//   - x: the line is the contiguous axis.  A workgroup owns 64 rows and moves them through LDS in blocks of 64 rows x 32 columns (rows
//     padded to 33 doubles: the 32 lanes of a half-wave fall on 32 different bank pairs), loaded and stored with all 256 threads along the
//     rows, so global traffic is in 256-byte row segments; one lane per row then runs the recursion over the block in LDS and carries its
//     state to the next block.  Three sweeps: the exact causal start (two running sums over the whole line), causal ascending, anti-causal
//     descending; a line that fits one block is loaded and stored once.  A line is read and written by one workgroup only.
// No workspace beyond the caller's `coef`, no copy, no synchronisation, no atomics, no scratch.
#include <math.h>

#include "reslice_taps.h"
#include "../../include/aesr_hip_baselines.h"
#include "aesr_kernels.h"
#include "aesr_hostcheck.h"
#include "reslice_position.h"

#pragma clang fp contract(off)

#define RTP_THREADS 256
#define RTP_LX 64              // lanes along the output x
#define RTP_PI 3.14159265358979323846

#define PFX_ROWS 64            // rows of a workgroup of the x pass
#define PFX_CW 32              // columns of a staged block
#define PFX_LD (PFX_CW + 1)    // padded row of the staged block, in doubles

// whole-sample mirror of period 2 n - 2: c b | a b c d | c b
__device__ __forceinline__ int rtp_mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// one axis: position p inside [-0.5, n - 0.5) -> the T = 2 R weights and (bounded) indices of taps k = -R + 1 ... R around floor(p)
template <int KERNEL, int R>
__device__ __forceinline__ void rtp_axis(double p, int n, double w[2 * R], int idx[2 * R]) {
    constexpr int T = 2 * R;
    const double b = floor(p), t = p - b;
    const int ib = (int)b;          // -1 ... n - 1
    if (KERNEL == AESR_TAPS_BSPLINE3) {
        const double u = 1.0 - t;
        w[0] = u * u * u / 6.0;
        w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
        w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
        w[3] = 1.0 - w[0] - w[1] - w[2];
#pragma unroll
        for (int j = 0; j < T; ++j) idx[j] = rtp_mirror(ib - 1 + j, n);
    } else {
        // The window's angle at tap k comes from an anchor by the angle-sum rule; cos and sin of the constant part fold at compile time.
        // COSINE: anchor pi t / (2 R).  LANCZOS: sinc(d / R) is 0 / 0 at d -> 0, which k = 0 reaches at t -> 0 and k = 1 at t -> 1, so its
        // sine must be accurate RELATIVE to d there: anchor pi t / R for k <= 0 and pi (t - 1) / R for k >= 1 (t - 1 is exact where it is
        // small); at k = 0 and k = 1 the constant part is 0 and the anchor's sine is used as it is, everywhere else |d| >= 1.
        const double sp = sinpi(t);
        double sa, ca, sb = 0.0, cb = 0.0;
        sincospi(KERNEL == AESR_TAPS_LANCZOS ? t / (double)R : t / (double)(2 * R), &sa, &ca);
        if (KERNEL == AESR_TAPS_LANCZOS) sincospi((t - 1.0) / (double)R, &sb, &cb);
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int k = j - R + 1;
            const double d = t - (double)k;
            const double sincd = ((k & 1) ? -sp : sp) / (RTP_PI * d);          // sin(pi (t - k)) = +-sin(pi t)
            double win;
            if (KERNEL == AESR_TAPS_LANCZOS) {
                const double ak = RTP_PI * (double)(k <= 0 ? k : k - 1) / (double)R;
                const double sine = k == 0 ? sa : (k == 1 ? sb : (k < 0 ? sa * cos(ak) - ca * sin(ak) : sb * cos(ak) - cb * sin(ak)));
                win = sine / (RTP_PI * d / (double)R);          // sinc(d / R)
            } else {
                const double ak = RTP_PI * (double)k / (double)(2 * R);
                win = ca * cos(ak) + sa * sin(ak);          // cos(pi d / (2 R))
            }
            // on a sample: exactly that sample.  t == 1.0 is the sample b + 1: p - floor(p) rounds to it for p in (-2^-54, 0), the -1e-17
            // that a composed affine leaves where the exact position is 0, and sinc(d) there is 0 / 0 at k = 1
            w[j] = t == 0.0 ? (k == 0 ? 1.0 : 0.0) : (t == 1.0 ? (k == 1 ? 1.0 : 0.0) : sincd * win);
            idx[j] = min(max(ib + k, 0), n - 1);
        }
    }
}

// S: float (samples, the sincs) or double (coefficients, BSPLINE3).  A tile is RTP_LX lanes x 4 rows; grid.x: tiles_x * tiles_y * Zo.
template <typename S, int KERNEL, int R>
__global__ __launch_bounds__(RTP_THREADS) void reslice_taps_kernel(const S* __restrict__ src, float* __restrict__ out, RslAffine A, int N,
                                                                   int Zs, int Hs, int Ws, int Zo, int Ho, int Wo, unsigned int tiles_x,
                                                                   unsigned int tiles_y, int clamp01) {
    constexpr int T = 2 * R, LX = RTP_LX;
    __shared__ double s_wz[T][RTP_THREADS];
    __shared__ int s_oz[T][RTP_THREADS];
    const unsigned int tx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
    const unsigned int ty = rest % tiles_y, zo = rest / tiles_y;          // zo < Zo: the launcher sized the grid for it
    const int xo = (int)(tx * LX + (threadIdx.x & (LX - 1)));
    const int yo = (int)(ty * (RTP_THREADS / LX) + threadIdx.x / LX);
    if (xo >= Wo || yo >= Ho) return;
    const size_t frame_src = (size_t)Zs * Hs * Ws, frame_out = (size_t)Zo * Ho * Wo;
    float* __restrict__ o = out + ((size_t)zo * Ho + yo) * Wo + xo;
    double p[3];
    rsl_affine_position(A, xo, yo, (int)zo, p);
    // ITK's buffer rule; every comparison is false for a NaN
    const bool inside = p[0] >= -0.5 && p[0] < (double)Ws - 0.5 && p[1] >= -0.5 && p[1] < (double)Hs - 0.5 && p[2] >= -0.5 && p[2] < (double)Zs - 0.5;
    if (!inside) {
        for (int n = 0; n < N; ++n) {
            *o = 0.f;
            o += frame_out;
        }
        return;
    }
    double wx[T], wy[T];
    int ix[T], iy[T];
    {
        double wz[T];
        int iz[T];
        rtp_axis<KERNEL, R>(p[0], Ws, wx, ix);
        rtp_axis<KERNEL, R>(p[1], Hs, wy, iy);
        rtp_axis<KERNEL, R>(p[2], Zs, wz, iz);
#pragma unroll
        for (int j = 0; j < T; ++j) {
            iy[j] *= Ws;
            s_wz[j][threadIdx.x] = wz[j];
            s_oz[j][threadIdx.x] = iz[j] * Hs * Ws;          // < Zs * Hs * Ws < 2^31
        }
    }
    for (int n = 0; n < N; ++n) {
        double acc = 0.0;
#pragma unroll 1
        for (int kz = 0; kz < T; ++kz) {
            const double wzv = s_wz[kz][threadIdx.x];
            const int oz = s_oz[kz][threadIdx.x];
#pragma unroll
            for (int ky = 0; ky < T; ++ky) {
                const double wzy = wzv * wy[ky];
                const S* __restrict__ line = src + (oz + iy[ky]);
                S v[T];          // the row's T loads are issued together, ahead of the sum that needs them one by one
#pragma unroll
                for (int kx = 0; kx < T; ++kx) v[kx] = line[ix[kx]];
#pragma unroll
                for (int kx = 0; kx < T; ++kx) acc += (wzy * wx[kx]) * (double)v[kx];
            }
        }
        float r = (float)acc;
        if (clamp01) r = r < 0.f ? 0.f : (r > 1.f ? 1.f : r);
        *o = r;
        src += frame_src;
        o += frame_out;
    }
}

// ---- the pre-filter ------------------------------------------------------------------------------------------------------------------
// y: one thread per (frame, z, x) line of H coefficients with stride W, in place: the recursion of z_expand.hip's bspline_prefilter_kernel
__global__ __launch_bounds__(RTP_THREADS) void bspline_prefilter_y_kernel(double* __restrict__ coef, unsigned int cols, unsigned int W, int H) {
    const unsigned int col = blockIdx.x * RTP_THREADS + threadIdx.x;
    if (col >= cols) return;
    double* __restrict__ c = coef + (size_t)(col / W) * H * W + col % W;
    const double z1 = sqrt(3.0) - 2.0, gain = 6.0;
    double zn1 = 1.0;
    for (int i = 0; i < H - 1; ++i) zn1 *= z1;          // z1^(H-1) as a running product
    double c0 = c[0] * gain + zn1 * (c[(size_t)(H - 1) * W] * gain), zi = z1;
    for (int i = 1; i < H - 1; ++i) {
        c0 += zi * (c[(size_t)i * W] * gain + zn1 * (c[(size_t)(H - 1 - i) * W] * gain));
        zi *= z1;
    }
    c0 /= 1.0 - zn1 * zn1;
    c[0] = c0;
    double prev = c0, prev2 = c0;
    for (int i = 1; i < H; ++i) {          // causal
        prev2 = prev;
        prev = c[(size_t)i * W] * gain + z1 * prev;
        c[(size_t)i * W] = prev;
    }
    double next = z1 / (z1 * z1 - 1.0) * (z1 * prev2 + prev);          // anti-causal
    c[(size_t)(H - 1) * W] = next;
    for (int i = H - 2; i >= 0; --i) {
        next = z1 * (next - c[(size_t)i * W]);
        c[(size_t)i * W] = next;
    }
}

// x: PFX_ROWS rows per workgroup through LDS in blocks of PFX_CW columns.  rows = N * Z * H lines of W >= 2 coefficients, in place.
// With z = the pole, L = W: the causal start is c0 = 6 (S1 + z^(L-1) S2) / (1 - z^(2L-2)), S1 = sum_{i=0}^{L-1} z^i x[i] and
// S2 = sum_{j=1}^{L-2} z^(L-1-j) x[j] (the mirrored half of the period), S2 by Horner's rule so that both run in ascending order.
__global__ __launch_bounds__(RTP_THREADS) void bspline_prefilter_x_kernel(double* __restrict__ coef, unsigned int rows, int W) {
    __shared__ double tile[PFX_ROWS * PFX_LD];
    const unsigned int row0 = blockIdx.x * PFX_ROWS;
    const int nrows = (int)min((unsigned int)PFX_ROWS, rows - row0);          // > 0: the launcher sized the grid for it
    double* __restrict__ base = coef + (size_t)row0 * W;
    const int nch = (W + PFX_CW - 1) / PFX_CW;
    const int r = (int)threadIdx.x;
    const bool owner = r < nrows;          // this lane runs the recursion of row r
    double* __restrict__ mine = tile + (owner ? r : 0) * PFX_LD;
    const double z1 = sqrt(3.0) - 2.0, gain = 6.0;

    // all threads: block `ch` of the rows <-> LDS; the barriers keep a block's recursion apart from its load and store
    auto load = [&](int ch) {
        __syncthreads();
        for (int idx = (int)threadIdx.x; idx < PFX_ROWS * PFX_CW; idx += RTP_THREADS) {
            const int rr = idx / PFX_CW, x = ch * PFX_CW + idx % PFX_CW;
            if (rr < nrows && x < W) tile[rr * PFX_LD + idx % PFX_CW] = base[(size_t)rr * W + x];
        }
        __syncthreads();
    };
    auto store = [&](int ch) {
        __syncthreads();
        for (int idx = (int)threadIdx.x; idx < PFX_ROWS * PFX_CW; idx += RTP_THREADS) {
            const int rr = idx / PFX_CW, x = ch * PFX_CW + idx % PFX_CW;
            if (rr < nrows && x < W) base[(size_t)rr * W + x] = tile[rr * PFX_LD + idx % PFX_CW];
        }
    };

    // sweep 1: the causal start
    double s1 = 0.0, s2 = 0.0, zi = 1.0;          // zi = z1^i
    for (int ch = 0; ch < nch; ++ch) {
        load(ch);
        if (owner) {
            const int x0 = ch * PFX_CW, n = min(PFX_CW, W - x0);
            for (int j = 0; j < n; ++j) {
                const int i = x0 + j;
                const double v = mine[j];
                s1 += zi * v;
                if (i >= 1 && i <= W - 2) s2 = s2 * z1 + v;
                if (i < W - 1) zi *= z1;          // ends as z1^(W-1)
            }
        }
    }
    const double zn1 = zi;
    double prev = gain * (s1 + zn1 * (s2 * z1)) / (1.0 - zn1 * zn1), prev2 = prev;
    // sweep 2: causal, ascending.  A line of one block is still in LDS.
    for (int ch = 0; ch < nch; ++ch) {
        if (nch > 1) load(ch);
        if (owner) {
            const int x0 = ch * PFX_CW, n = min(PFX_CW, W - x0);
            for (int j = 0; j < n; ++j) {
                if (x0 + j > 0) {
                    prev2 = prev;
                    prev = mine[j] * gain + z1 * prev;
                }
                mine[j] = prev;
            }
        }
        if (nch > 1) store(ch);
    }
    // sweep 3: anti-causal, descending; prev2, prev are the last two causal values
    double next = z1 / (z1 * z1 - 1.0) * (z1 * prev2 + prev);
    for (int ch = nch - 1; ch >= 0; --ch) {
        if (nch > 1) load(ch);
        if (owner) {
            const int x0 = ch * PFX_CW, n = min(PFX_CW, W - x0);
            for (int j = n - 1; j >= 0; --j) {
                if (x0 + j < W - 1) next = z1 * (next - mine[j]);
                mine[j] = next;
            }
        }
        store(ch);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static void rtp_launch(const float* src, const double* coef, float* out, const RslAffine& A, int N, int Zs, int Hs, int Ws, int Zo,
                       int Ho, int Wo, int kernel, int radius, int clamp01, hipStream_t st) {
    const unsigned int tiles_x = (unsigned int)ceil_div(Wo, RTP_LX), tiles_y = (unsigned int)ceil_div(Ho, RTP_THREADS / RTP_LX);
    const dim3 blocks(tiles_x * tiles_y * (unsigned int)Zo);          // <= Zo * Ho * Wo < 2^31: every tile holds a voxel
#define RTP_LAUNCH(S, ptr, K, R) \
    hipLaunchKernelGGL((reslice_taps_kernel<S, K, R>), blocks, dim3(RTP_THREADS), 0, st, ptr, out, A, N, Zs, Hs, Ws, Zo, Ho, Wo, tiles_x, tiles_y, clamp01)
    if (kernel == AESR_TAPS_BSPLINE3) RTP_LAUNCH(double, coef, AESR_TAPS_BSPLINE3, 2);
    else if (kernel == AESR_TAPS_LANCZOS && radius == 3) RTP_LAUNCH(float, src, AESR_TAPS_LANCZOS, 3);
    else if (kernel == AESR_TAPS_LANCZOS && radius == 4) RTP_LAUNCH(float, src, AESR_TAPS_LANCZOS, 4);
    else if (kernel == AESR_TAPS_LANCZOS) RTP_LAUNCH(float, src, AESR_TAPS_LANCZOS, 5);
    else if (radius == 3) RTP_LAUNCH(float, src, AESR_TAPS_COSINE, 3);
    else if (radius == 4) RTP_LAUNCH(float, src, AESR_TAPS_COSINE, 4);
    else RTP_LAUNCH(float, src, AESR_TAPS_COSINE, 5);
#undef RTP_LAUNCH
}

extern "C" {

int aesr_bspline_prefilter_3d(const float* in, double* coef, int N, int Z, int H, int W, void* stream) {
    AESR_CHECK_ARG(in, "aesr_bspline_prefilter_3d: in is a null pointer");
    AESR_CHECK_ARG(coef, "aesr_bspline_prefilter_3d: coef is a null pointer");
    AESR_CHECK_ARG((uintptr_t)in % 4 == 0, "aesr_bspline_prefilter_3d: in is not 4-byte aligned");
    AESR_CHECK_ARG((uintptr_t)coef % 8 == 0, "aesr_bspline_prefilter_3d: coef is not 8-byte aligned");
    AESR_CHECK_ARG(N > 0 && Z > 0 && H > 0 && W > 0, "aesr_bspline_prefilter_3d: N, Z, H, W = %d, %d, %d, %d must all be positive", N, Z, H, W);
    AESR_CHECK_ARG((double)N * Z * H * W < 2147483648.0, "aesr_bspline_prefilter_3d: N * Z * H * W = %d x %d x %d x %d has 2^31 elements or more", N, Z, H,
                   W);
    const size_t count = (size_t)N * Z * H * W;
    if (aesr_overlap(coef, 8 * count, in, 4 * count)) {
        aesr_set_error("aesr_bspline_prefilter_3d: coef overlaps in");
        return AESR_ERR_UNSUPPORTED;
    }
    const int rc = aesr_bspline_prefilter_z(in, coef, N, Z, H, W, stream);          // fp32 -> fp64; Z == 1 copies
    if (rc != AESR_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (H > 1) {
        const unsigned int cols = (unsigned int)N * Z * W;
        hipLaunchKernelGGL(bspline_prefilter_y_kernel, dim3((cols + RTP_THREADS - 1) / RTP_THREADS), dim3(RTP_THREADS), 0, st, coef, cols, (unsigned int)W, H);
        AESR_LAUNCH_CHECK("bspline_prefilter_3d (y)");
    }
    if (W > 1) {
        const unsigned int rows = (unsigned int)N * Z * H;
        hipLaunchKernelGGL(bspline_prefilter_x_kernel, dim3((rows + PFX_ROWS - 1) / PFX_ROWS), dim3(RTP_THREADS), 0, st, coef, rows, W);
        AESR_LAUNCH_CHECK("bspline_prefilter_3d (x)");
    }
    return AESR_OK;
}

int aesr_reslice_taps_affine(const float* src, const double* coef, float* out, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo,
                             const double* m_host, int kernel, int radius, int clamp01, void* stream) {
    const char* fn = "aesr_reslice_taps_affine";
    AESR_CHECK_ARG(out, "%s: out is a null pointer", fn);
    AESR_CHECK_ARG(m_host, "%s: m_host is a null pointer", fn);
    AESR_CHECK_ARG((src != nullptr) != (coef != nullptr), "%s: exactly one of src and coef must be given (%s are)", fn, src ? "both" : "neither");
    AESR_CHECK_ARG(kernel == AESR_TAPS_BSPLINE3 || kernel == AESR_TAPS_LANCZOS || kernel == AESR_TAPS_COSINE,
                   "%s: kernel=%d is none of 0 (bspline), 1 (lanczos), 2 (cosine)", fn, kernel);
    AESR_CHECK_ARG((kernel == AESR_TAPS_BSPLINE3) == (coef != nullptr), "%s: kernel=%d reads %s", fn, kernel,
                   kernel == AESR_TAPS_BSPLINE3 ? "coef, not src" : "src, not coef");
    AESR_CHECK_ARG((uintptr_t)src % 4 == 0, "%s: src is not 4-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)coef % 8 == 0, "%s: coef is not 8-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)out % 4 == 0, "%s: out is not 4-byte aligned", fn);
    AESR_CHECK_ARG(N > 0, "%s: N=%d must be positive", fn, N);
    AESR_CHECK_ARG(Zs > 0 && Hs > 0 && Ws > 0, "%s: Zs, Hs, Ws = %d, %d, %d must all be positive", fn, Zs, Hs, Ws);
    AESR_CHECK_ARG(Zo > 0 && Ho > 0 && Wo > 0, "%s: Zo, Ho, Wo = %d, %d, %d must all be positive", fn, Zo, Ho, Wo);
    AESR_CHECK_ARG(radius >= AESR_TAPS_MIN_RADIUS && radius <= AESR_TAPS_MAX_RADIUS, "%s: radius=%d is none of 3, 4, 5", fn, radius);
    AESR_CHECK_ARG(clamp01 == 0 || clamp01 == 1, "%s: clamp01=%d is neither 0 nor 1", fn, clamp01);
    AESR_CHECK_ARG((double)N * Zs * Hs * Ws < 2147483648.0, "%s: N * Zs * Hs * Ws = %d x %d x %d x %d has 2^31 elements or more", fn, N, Zs, Hs, Ws);
    AESR_CHECK_ARG((double)N * Zo * Ho * Wo < 2147483648.0, "%s: N * Zo * Ho * Wo = %d x %d x %d x %d has 2^31 elements or more", fn, N, Zo, Ho, Wo);
    RslAffine A;
    for (int i = 0; i < 12; ++i) {
        AESR_CHECK_ARG(isfinite(m_host[i]), "%s: m_host[%d] is not finite", fn, i);
        A.m[i] = m_host[i];
    }
    const size_t n_src = (size_t)N * Zs * Hs * Ws;
    if (aesr_overlap(out, (size_t)4 * N * Zo * Ho * Wo, src ? (const void*)src : (const void*)coef, (src ? 4 : 8) * n_src)) {
        aesr_set_error("%s: out overlaps %s", fn, src ? "src" : "coef");
        return AESR_ERR_UNSUPPORTED;
    }
    rtp_launch(src, coef, out, A, N, Zs, Hs, Ws, Zo, Ho, Wo, kernel, radius, clamp01, (hipStream_t)stream);
    AESR_LAUNCH_CHECK("reslice_taps_affine");
    return AESR_OK;
}

}  // extern "C"
