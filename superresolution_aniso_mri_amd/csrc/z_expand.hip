// Conventional through-plane interpolation of a [N][Z][H][W] volume by an integer factor (the reference's evaluate/common.py:74-118
// create_simple_interpolation, SimpleITK's ExpandImageFilter with a linear, cubic B-spline or Lanczos-windowed-sinc interpolator).
// include/aesr_hip_baselines.h; the B-spline's pre-filter is bspline_prefilter.hip.
//   - in-plane coordinates are integers, so every method is a 1-D filter along z of every (y, x) column whose taps depend on the output
//     PHASE p = o % factor only: out[q * factor + p] = sum_k w[p][k] * src[bound(q + base[p] + k)].  The host makes base and w in float64
//     (evaluate/z_interp.py: the rule of inplane.hip) and they travel by value in the kernel ARGUMENTS; the kernel only looks up;
//   - a slice is a flat row of H * W pixels; lanes run along it: 16 bytes of output per lane (VEC) when W % 4 == 0 and both pointers are
//     16-byte aligned, 4 bytes per lane otherwise.  The source is fp32 samples or the fp64 coefficients of the pre-filter;
//   - a workgroup (256 threads) owns a strip of pixels and a run of QB source positions q, i.e. QB * factor output slices.  It stages the
//     QB + span source slices the run needs in LDS (48 KiB: 48 slices of fp32, 24 of fp64), the boundary (clamp, or whole-sample mirror of
//     period 2 Z - 2, repeated while the index is outside) resolved while staging: every source element comes from HBM / L2 once per
//     workgroup (plus the z halo of the neighbouring run), not once per tap and phase, and every output slice is written once;
//   - each output is sum_k in ascending k, accumulated in double without contraction, rounded to fp32 once, then clamped to [0, 1] if asked.
//     An output slice index is the same in every lane of a wave, so the weights are read with scalar loads.
// No workspace, no copy, no synchronisation, no atomics, no scratch.
#include <math.h>

#include "../../include/aesr_hip_baselines.h"
#include "aesr_kernels.h"
#include "bspline_prefilter.h"

#pragma clang fp contract(off)

#define ZX_THREADS 256
#define ZX_LDS_BYTES (48 * 1024)
#define ZX_MIN_QB 4               // source positions per run at least (while the window allows): the halo re-read stays bounded
#define ZX_FULL_GRID 768          // workgroups that are resident at once: 256 CUs x 3 (48 KiB of LDS each)
#define ZX_MAX_BASE 4096          // |base_host[p]|: far beyond any interpolator, small enough that q + base + k cannot overflow

struct ZxTables {
    double w[AESR_ZX_MAX_FACTOR * AESR_ZX_MAX_TAPS];          // w[p * taps + k]
    int base[AESR_ZX_MAX_FACTOR];
};

// V consecutive pixels of a slice of S: the unit a lane loads, stages and (as float) stores
template <typename S, int V>
struct alignas(V == 4 ? 16 : sizeof(S)) ZxPack { S v[V]; };

__device__ __forceinline__ int zx_bound(int i, int n, int boundary) {
    return boundary == 0 ? (i < 0 ? 0 : (i >= n ? n - 1 : i)) : aesr_mirror_index(i, n);
}

// S: float (samples) or double (coefficients); V = 4 with SU = 64 units per staged slice, or V = 1 with SU = 256.  units: units per slice
// (H * W / V).  grid.x: strips, grid.y: runs of QB source positions, grid.z: frames.  span: staged slices beyond the run's QB
// (max base - min base + taps - 1); lo: min base.
template <typename S, int V, int SU>
__global__ __launch_bounds__(ZX_THREADS) void z_expand_kernel(const ZxPack<S, V>* __restrict__ src, ZxPack<float, V>* __restrict__ out, ZxTables tb,
                                                              int Z, int Zo, unsigned int units, int f, int taps, int lo, int span, int QB,
                                                              int boundary, int clamp01) {
    typedef ZxPack<S, V> P;
    __shared__ P win[ZX_LDS_BYTES / sizeof(P)];
    src += (size_t)blockIdx.z * Z * units;
    out += (size_t)blockIdx.z * Zo * units;
    const unsigned int u0 = blockIdx.x * SU;
    const int q0 = blockIdx.y * QB;
    const int no = min(QB * f, Zo - q0 * f);          // output slices of this run (> 0: the launcher sized grid.y for it)
    const int n_in = (no - 1) / f + 1 + span;         // <= ZX_LDS_BYTES / sizeof(P) / SU: the launcher chose QB for it
    for (int idx = threadIdx.x; idx < n_in * SU; idx += ZX_THREADS) {
        const unsigned int u = u0 + (idx & (SU - 1));
        if (u >= units) continue;
        win[idx] = src[(size_t)zx_bound(q0 + lo + idx / SU, Z, boundary) * units + u];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < no * SU; idx += ZX_THREADS) {
        // the output slice of the run is the same in every lane of a wave (SU is a multiple of 64): say so, and base and weights become scalar loads
        const int j = __builtin_amdgcn_readfirstlane(idx / SU), ul = idx & (SU - 1);
        const unsigned int u = u0 + ul;
        if (u >= units) continue;
        const int ql = j / f, p = j - ql * f;
        const P* __restrict__ c = win + (ql + tb.base[p] - lo) * SU + ul;
        const double* __restrict__ w = tb.w + p * taps;
        double acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = w[0] * (double)c->v[v];
        for (int k = 1; k < taps; ++k) {
            const P* __restrict__ ck = c + k * SU;
            const double wk = w[k];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] += wk * (double)ck->v[v];
        }
        ZxPack<float, V> res;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float r = (float)acc[v];
            if (clamp01) r = r < 0.f ? 0.f : (r > 1.f ? 1.f : r);
            res.v[v] = r;
        }
        out[(size_t)(q0 * f + j) * units + u] = res;
    }
}

extern "C" {

int aesr_z_expand_out_slices(int Z, int factor, int align) {
    if (Z < 1 || factor < 1 || (align != AESR_ZX_ALIGN_ITK && align != AESR_ZX_ALIGN_GRID)) return 0;
    const long long n = align == AESR_ZX_ALIGN_ITK ? (long long)Z * factor : (long long)(Z - 1) * factor + 1;
    return n < ((long long)1 << 31) ? (int)n : 0;
}

int aesr_z_expand_store_bytes(int W, const void* src, const float* out) {
    return W > 0 && W % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0 ? 16 : 4;
}

size_t aesr_bspline_coef_bytes(int N, int Z, int H, int W) {
    return N > 0 && Z > 0 && H > 0 && W > 0 ? (size_t)8 * N * Z * H * W : 0;
}

int aesr_z_expand(const float* in, const double* coef, float* out, int N, int Z, int H, int W, int factor, int Zo, int taps, const int* base_host,
                  const double* weights_host, int boundary, int clamp01, void* stream) {
    AESR_CHECK_ARG((in != nullptr) != (coef != nullptr), "aesr_z_expand: exactly one of in and coef must be given (%s are)", in ? "both" : "neither");
    AESR_CHECK_ARG(out, "aesr_z_expand: out is a null pointer");
    AESR_CHECK_ARG(base_host, "aesr_z_expand: base_host is a null pointer");
    AESR_CHECK_ARG(weights_host, "aesr_z_expand: weights_host is a null pointer");
    AESR_CHECK_ARG((uintptr_t)in % 4 == 0, "aesr_z_expand: in is not 4-byte aligned");
    AESR_CHECK_ARG((uintptr_t)coef % 8 == 0, "aesr_z_expand: coef is not 8-byte aligned");
    AESR_CHECK_ARG((uintptr_t)out % 4 == 0, "aesr_z_expand: out is not 4-byte aligned");
    AESR_CHECK_ARG(N > 0 && Z > 0 && H > 0 && W > 0, "aesr_z_expand: N, Z, H, W = %d, %d, %d, %d must all be positive", N, Z, H, W);
    AESR_CHECK_ARG(Z <= (1 << 30), "aesr_z_expand: Z=%d exceeds 2^30", Z);
    AESR_CHECK_ARG(factor >= 1, "aesr_z_expand: factor=%d must be at least 1", factor);
    AESR_CHECK_ARG(taps >= 1, "aesr_z_expand: taps=%d must be at least 1", taps);
    if (factor > AESR_ZX_MAX_FACTOR) {
        aesr_set_error("aesr_z_expand: factor=%d exceeds the supported %d", factor, AESR_ZX_MAX_FACTOR);
        return AESR_ERR_UNSUPPORTED;
    }
    if (taps > AESR_ZX_MAX_TAPS) {
        aesr_set_error("aesr_z_expand: taps=%d exceeds the supported %d (Lanczos radius above 5)", taps, AESR_ZX_MAX_TAPS);
        return AESR_ERR_UNSUPPORTED;
    }
    AESR_CHECK_ARG(boundary == AESR_ZX_CLAMP || boundary == AESR_ZX_MIRROR, "aesr_z_expand: boundary=%d is neither 0 (clamp) nor 1 (mirror)", boundary);
    AESR_CHECK_ARG(clamp01 == 0 || clamp01 == 1, "aesr_z_expand: clamp01=%d is neither 0 nor 1", clamp01);
    AESR_CHECK_ARG(Zo > 0 && (Zo == aesr_z_expand_out_slices(Z, factor, AESR_ZX_ALIGN_ITK) || Zo == aesr_z_expand_out_slices(Z, factor, AESR_ZX_ALIGN_GRID)),
                   "aesr_z_expand: Zo=%d is not what aesr_z_expand_out_slices returns for Z=%d, factor=%d (%d or %d)", Zo, Z, factor,
                   aesr_z_expand_out_slices(Z, factor, AESR_ZX_ALIGN_ITK), aesr_z_expand_out_slices(Z, factor, AESR_ZX_ALIGN_GRID));
    AESR_CHECK_ARG((size_t)N * Zo * H * W < ((size_t)1 << 31), "aesr_z_expand: N * Zo * H * W = %d x %d x %d x %d has 2^31 elements or more", N, Zo, H, W);
    ZxTables tb;
    for (int i = 0; i < AESR_ZX_MAX_FACTOR * AESR_ZX_MAX_TAPS; ++i) tb.w[i] = 0.0;
    for (int p = 0; p < AESR_ZX_MAX_FACTOR; ++p) tb.base[p] = 0;
    int lo = base_host[0], hi = base_host[0];
    for (int p = 0; p < factor; ++p) {
        AESR_CHECK_ARG(base_host[p] >= -ZX_MAX_BASE && base_host[p] <= ZX_MAX_BASE, "aesr_z_expand: base_host[%d]=%d is outside [-%d, %d]", p,
                       base_host[p], ZX_MAX_BASE, ZX_MAX_BASE);
        tb.base[p] = base_host[p];
        lo = base_host[p] < lo ? base_host[p] : lo;
        hi = base_host[p] > hi ? base_host[p] : hi;
        for (int k = 0; k < taps; ++k) {
            AESR_CHECK_ARG(isfinite(weights_host[p * taps + k]), "aesr_z_expand: weights_host[%d][%d] is not finite", p, k);
            tb.w[p * taps + k] = weights_host[p * taps + k];
        }
    }
    const bool vec = aesr_z_expand_store_bytes(W, in ? (const void*)in : (const void*)coef, out) == 16;
    const int window = ZX_LDS_BYTES / 1024 / (in ? 1 : 2);          // staged slices: a slice of a strip is 1 KiB of fp32, 2 KiB of fp64
    const int span = hi - lo + taps - 1;
    if (span >= window) {
        aesr_set_error("aesr_z_expand: base_host spreads over %d source slices with taps=%d; at most %d fit the staged window", hi - lo + 1, taps, window);
        return AESR_ERR_UNSUPPORTED;
    }
    const int NQ = ceil_div(Zo, factor);
    const size_t HW = (size_t)H * W;
    const unsigned int units = (unsigned int)(vec ? HW / 4 : HW);
    const int SU = vec ? 64 : 256;
    const unsigned int strips = (units + SU - 1) / SU;
    // the longest run the staged window holds reads the least halo, but a frame is few strips (196 for 224 x 224): shorter runs until the
    // grid fills the device once (256 CUs x 3 workgroups of 48 KiB), not below ZX_MIN_QB positions per run.  The values do not depend on it.
    int QB = window - span;
    if (QB > NQ) QB = NQ;
    while (QB > ZX_MIN_QB && (size_t)strips * ceil_div(NQ, QB) * N < ZX_FULL_GRID) QB = (QB + 1) / 2 < ZX_MIN_QB ? ZX_MIN_QB : (QB + 1) / 2;
    const dim3 grid(strips, (unsigned int)ceil_div(NQ, QB), (unsigned int)N);
    AESR_CHECK_ARG(grid.y <= 65535, "aesr_z_expand: Z=%d needs %u runs of source slices (at most 65535)", Z, grid.y);
    AESR_CHECK_ARG(grid.z <= 65535, "aesr_z_expand: N=%d frames (at most 65535)", N);
    hipStream_t st = (hipStream_t)stream;
#define ZX_LAUNCH(S, V, SUV, ptr)                                                                                                              \
    hipLaunchKernelGGL((z_expand_kernel<S, V, SUV>), grid, dim3(ZX_THREADS), 0, st, (const ZxPack<S, V>*)(ptr), (ZxPack<float, V>*)out, tb, Z, Zo, \
                       units, factor, taps, lo, span, QB, boundary, clamp01)
    if (in && vec) ZX_LAUNCH(float, 4, 64, in);
    else if (in) ZX_LAUNCH(float, 1, 256, in);
    else if (vec) ZX_LAUNCH(double, 4, 64, coef);
    else ZX_LAUNCH(double, 1, 256, coef);
#undef ZX_LAUNCH
    AESR_LAUNCH_CHECK("z_expand");
    return AESR_OK;
}

}  // extern "C"
