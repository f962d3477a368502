// Affine reslicing with a higher-order kernel at a free 3-D position: cubic B-spline over a separable 3-D pre-filter, Lanczos- and
// cosine-windowed sinc (ITK's WindowedSincInterpolateImageFunction, the reference's kwatsch/create_nifti_from_dicom.py:202-253).
// include/aesr_hip_reslice_taps.h has the contract; the B-spline's pre-filter is bspline_prefilter.hip.
//   - one lane per output voxel, lanes along the output x, a workgroup (256 threads) on a 64 x 4 tile of one output slice, as in reslice.hip:
//     an output row is a straight line through the source, so neighbouring lanes read neighbouring addresses;
//   - the position comes from reslice.hip's own device function (reslice_common.h).  Per axis the T = 2 R weights and element offsets are
//     made ONCE per voxel and reused for the N frames.  Of sin(pi (t - k)) = +-sin(pi t) one sinpi per axis remains for the sinc factor; the
//     window's sine or cosine at t - k comes from one sincospi per axis (two for Lanczos: rtp_axis) and the angle-sum rule: cos and sin
//     of k pi / R (k pi / (2 R)) have constant arguments once the tap loop is unrolled and are folded at compile time;
//   - the x and y arrays stay in registers: the ky and kx loops are unrolled on the template's tap count, every index a compile-time
//     constant.  The z arrays go to LDS, one column per lane ([T][256]: a wave reads 64 consecutive doubles, no bank conflict, no barrier --
//     a lane reads only what it wrote), and kz is a rolled loop: the body is T x T taps, not T^3 (22 KiB of code at R = 5; 1000 taps
//     unrolled would be several times the 64 KiB instruction cache).  The T loads of a row are issued together, ahead of their sum;
//   - per frame and voxel T^3 loads, T^2 (T + 1) multiplies and T^3 adds in fp64, summed kz, ky, kx ascending, one rounding to fp32.
// No workspace, no copy, no synchronisation, no atomics, no scratch.
#include <math.h>

#include "../../include/aesr_hip_reslice_taps.h"
#include "aesr_kernels.h"
#include "aesr_hostcheck.h"
#include "bspline_prefilter.h"
#include "reslice_common.h"

#pragma clang fp contract(off)

#define RTP_PI 3.14159265358979323846

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
        for (int j = 0; j < T; ++j) idx[j] = aesr_mirror_index(ib - 1 + j, n);
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

// S: float (samples, the sincs) or double (coefficients, BSPLINE3).  Tiles as in reslice.hip (rsl_tile_voxel).
template <typename S, int KERNEL, int R>
__global__ __launch_bounds__(RSL_THREADS) void reslice_taps_kernel(const S* __restrict__ src, float* __restrict__ out, RslAffine A, int N,
                                                                   int Zs, int Hs, int Ws, int Zo, int Ho, int Wo, unsigned int tiles_x,
                                                                   unsigned int tiles_y, int clamp01) {
    constexpr int T = 2 * R;
    __shared__ double s_wz[T][RSL_THREADS];
    __shared__ int s_oz[T][RSL_THREADS];
    int xo, yo;
    unsigned int zo;
    if (!rsl_tile_voxel(tiles_x, tiles_y, Ho, Wo, xo, yo, zo)) return;
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

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static void rtp_launch(const float* src, const double* coef, float* out, const RslAffine& A, int N, int Zs, int Hs, int Ws, int Zo,
                       int Ho, int Wo, int kernel, int radius, int clamp01, hipStream_t st) {
    const unsigned int tiles_x = (unsigned int)ceil_div(Wo, RSL_LX), tiles_y = (unsigned int)ceil_div(Ho, RSL_THREADS / RSL_LX);
    const dim3 blocks(tiles_x * tiles_y * (unsigned int)Zo);          // <= Zo * Ho * Wo < 2^31: every tile holds a voxel
#define RTP_LAUNCH(S, ptr, K, R) \
    hipLaunchKernelGGL((reslice_taps_kernel<S, K, R>), blocks, dim3(RSL_THREADS), 0, st, ptr, out, A, N, Zs, Hs, Ws, Zo, Ho, Wo, tiles_x, tiles_y, clamp01)
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
    if (const int rc = rsl_check_sizes(fn, N, Zs, Hs, Ws, Zo, Ho, Wo)) return rc;
    AESR_CHECK_ARG(radius >= AESR_TAPS_MIN_RADIUS && radius <= AESR_TAPS_MAX_RADIUS, "%s: radius=%d is none of 3, 4, 5", fn, radius);
    AESR_CHECK_ARG(clamp01 == 0 || clamp01 == 1, "%s: clamp01=%d is neither 0 nor 1", fn, clamp01);
    if (const int rc = rsl_check_counts(fn, N, Zs, Hs, Ws, Zo, Ho, Wo)) return rc;
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
