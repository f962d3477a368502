// Oblique reslicing: a 3-D interpolating gather of a [N][Zs][Hs][Ws] volume onto an output grid [Zo][Ho][Wo] whose voxels are given a
// continuous source position by a 3x4 affine or by a normalised sampling grid (the reference's evaluate/cardiac/resample_sax_to_lax.py:
// world-coordinate affines and a 5-D grid_sample with zero padding and align_corners=True).  include/aesr_hip_reslice.h.
//   - the position is the same for every frame: a thread computes the (clamped) offsets of its corners, their validity and their weights
//     ONCE per output voxel, in fp64, and then loops over the N frames: 8 loads, 8 multiplies and 8 adds per frame (1 load for nearest)
//     and no index arithmetic;
//   - lanes run along the output x: an output row is a straight line through the source, so neighbouring lanes read neighbouring
//     addresses (the same or the next cache line) whatever the orientation, and a wave stores one 256-byte row segment.  One voxel per
//     lane: a form with four voxels and a 16-byte store per lane was built and measured 1.4 to 2.6 times SLOWER (profiles/reslice.txt) --
//     its lanes sit four voxels apart on four rows, so each gather instruction touches more cache lines -- and was removed;
//   - a workgroup (256 threads) covers a compact tile of one output slice (64 x 4 voxels), not a long row: the source footprint of its
//     8 corners is a thin slab that the tile's rows share, and it is re-read from L2, not HBM;
//   - a corner outside the source contributes nothing (padding zeros): its offset is clamped into the volume, so every load is in bounds
//     whatever the position (not finite, 1e300), and its sample is replaced by the select, never multiplied;
//   - the eight products are added to 0.0 in double in the order dz, dy, dx ascending, without contraction, and rounded to fp32 once.
// No workspace, no copy, no synchronisation, no atomics, no scratch, no LDS.
#include <math.h>

#include "../../include/aesr_hip_reslice.h"
#include "aesr_kernels.h"
#include "aesr_hostcheck.h"
#include "reslice_common.h"

#pragma clang fp contract(off)

// one axis of the trilinear rule: position c on an axis of n samples -> clamped indices of the two neighbours, their weights and validity
__device__ __forceinline__ void rsl_axis_linear(double c, int n, int idx[2], double w[2], bool ok[2]) {
    const bool near = c >= -1.0 && c < (double)n;          // false for NaN: only then can a neighbour be inside
    const double cc = near ? c : -2.0;
    const double f = floor(cc);
    const int i0 = (int)f;
    w[0] = (f + 1.0) - cc;
    w[1] = cc - f;
    ok[0] = near && i0 >= 0;
    ok[1] = near && i0 + 1 <= n - 1;
    idx[0] = min(max(i0, 0), n - 1);
    idx[1] = min(max(i0 + 1, 0), n - 1);
}

// one axis of the nearest rule: rint rounds halves to even
__device__ __forceinline__ int rsl_axis_nearest(double c, int n, bool& ok) {
    const double r = rint(c);
    ok = r >= 0.0 && r <= (double)(n - 1);          // false for NaN
    return ok ? (int)r : 0;
}

// LINEAR: 1 = trilinear, 0 = nearest.  GRID: positions from `grid` ([Zo][Ho][Wo][3] normalised), else from the affine A.
template <int LINEAR, bool GRID>
__global__ __launch_bounds__(RSL_THREADS) void reslice_kernel(const float* __restrict__ src, const float* __restrict__ grid, float* __restrict__ out,
                                                              RslAffine A, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo,
                                                              unsigned int tiles_x, unsigned int tiles_y) {
    constexpr int K = LINEAR ? 8 : 1;
    int xo, yo;
    unsigned int zo;
    if (!rsl_tile_voxel(tiles_x, tiles_y, Ho, Wo, xo, yo, zo)) return;
    const size_t row = ((size_t)zo * Ho + yo) * Wo;
    int off[K];
    double w[K];
    unsigned int valid;
    {
        double p[3];
        if (GRID) {
            const float* __restrict__ g = grid + (row + xo) * 3;
            p[0] = ((double)g[0] + 1.0) / 2.0 * (double)(Ws - 1);
            p[1] = ((double)g[1] + 1.0) / 2.0 * (double)(Hs - 1);
            p[2] = ((double)g[2] + 1.0) / 2.0 * (double)(Zs - 1);
        } else {
            rsl_affine_position(A, xo, yo, (int)zo, p);
        }
        if (LINEAR) {
            int ix[2], iy[2], iz[2];
            double wx[2], wy[2], wz[2];
            bool okx[2], oky[2], okz[2];
            rsl_axis_linear(p[0], Ws, ix, wx, okx);
            rsl_axis_linear(p[1], Hs, iy, wy, oky);
            rsl_axis_linear(p[2], Zs, iz, wz, okz);
            unsigned int m = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
                off[k] = (iz[dz] * Hs + iy[dy]) * Ws + ix[dx];
                w[k] = (wz[dz] * wy[dy]) * wx[dx];
                m |= (okz[dz] && oky[dy] && okx[dx] ? 1u : 0u) << k;
            }
            valid = m;
        } else {
            bool okx, oky, okz;
            const int ix = rsl_axis_nearest(p[0], Ws, okx), iy = rsl_axis_nearest(p[1], Hs, oky), iz = rsl_axis_nearest(p[2], Zs, okz);
            off[0] = (iz * Hs + iy) * Ws + ix;
            w[0] = 1.0;
            valid = okx && oky && okz ? 1u : 0u;
        }
    }
    const size_t frame_src = (size_t)Zs * Hs * Ws, frame_out = (size_t)Zo * Ho * Wo;
    float* __restrict__ o = out + row + xo;
    for (int n = 0; n < N; ++n) {
        if (LINEAR) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double s = (double)src[off[k]];
                acc += (valid >> k) & 1u ? w[k] * s : 0.0;
            }
            *o = (float)acc;
        } else {
            const float s = src[off[0]];
            *o = valid ? s : 0.f;
        }
        src += frame_src;
        o += frame_out;
    }
}

// the checks the two entry points share; `fn` is the entry point's name in the message
static int rsl_check(const char* fn, const float* src, const float* out, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo, int interp) {
    AESR_CHECK_ARG(src, "%s: src is a null pointer", fn);
    AESR_CHECK_ARG(out, "%s: out is a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)src % 4 == 0, "%s: src is not 4-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)out % 4 == 0, "%s: out is not 4-byte aligned", fn);
    if (const int rc = rsl_check_sizes(fn, N, Zs, Hs, Ws, Zo, Ho, Wo)) return rc;
    AESR_CHECK_ARG(interp == AESR_RESLICE_NEAREST || interp == AESR_RESLICE_LINEAR, "%s: interp=%d is neither 0 (nearest) nor 1 (linear)", fn, interp);
    if (const int rc = rsl_check_counts(fn, N, Zs, Hs, Ws, Zo, Ho, Wo)) return rc;
    if (aesr_overlap(out, (size_t)4 * N * Zo * Ho * Wo, src, (size_t)4 * N * Zs * Hs * Ws)) {
        aesr_set_error("%s: out overlaps src", fn);
        return AESR_ERR_UNSUPPORTED;
    }
    return AESR_OK;
}

static int rsl_launch(const char* name, const float* src, const float* grid, float* out, const RslAffine& A, int N, int Zs, int Hs, int Ws, int Zo,
                      int Ho, int Wo, int interp, void* stream) {
    const unsigned int tiles_x = (unsigned int)ceil_div(Wo, RSL_LX), tiles_y = (unsigned int)ceil_div(Ho, RSL_THREADS / RSL_LX);
    const dim3 blocks(tiles_x * tiles_y * (unsigned int)Zo);          // <= Zo * Ho * Wo < 2^31: every tile holds a voxel
    hipStream_t st = (hipStream_t)stream;
#define RSL_LAUNCH(L, G) \
    hipLaunchKernelGGL((reslice_kernel<L, G>), blocks, dim3(RSL_THREADS), 0, st, src, grid, out, A, N, Zs, Hs, Ws, Zo, Ho, Wo, tiles_x, tiles_y)
    if (grid && interp) RSL_LAUNCH(1, true);
    else if (grid) RSL_LAUNCH(0, true);
    else if (interp) RSL_LAUNCH(1, false);
    else RSL_LAUNCH(0, false);
#undef RSL_LAUNCH
    AESR_LAUNCH_CHECK(name);
    return AESR_OK;
}

extern "C" {

int aesr_reslice_affine(const float* src, float* out, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo, const double* m_host, int interp,
                        void* stream) {
    AESR_CHECK_ARG(m_host, "aesr_reslice_affine: m_host is a null pointer");
    const int rc = rsl_check("aesr_reslice_affine", src, out, N, Zs, Hs, Ws, Zo, Ho, Wo, interp);
    if (rc != AESR_OK) return rc;
    RslAffine A;
    for (int i = 0; i < 12; ++i) {
        AESR_CHECK_ARG(isfinite(m_host[i]), "aesr_reslice_affine: m_host[%d] is not finite", i);
        A.m[i] = m_host[i];
    }
    return rsl_launch("reslice_affine", src, nullptr, out, A, N, Zs, Hs, Ws, Zo, Ho, Wo, interp, stream);
}

int aesr_reslice_grid(const float* src, const float* grid, float* out, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo, int interp,
                      void* stream) {
    AESR_CHECK_ARG(grid, "aesr_reslice_grid: grid is a null pointer");
    AESR_CHECK_ARG((uintptr_t)grid % 4 == 0, "aesr_reslice_grid: grid is not 4-byte aligned");
    const int rc = rsl_check("aesr_reslice_grid", src, out, N, Zs, Hs, Ws, Zo, Ho, Wo, interp);
    if (rc != AESR_OK) return rc;
    if (aesr_overlap(out, (size_t)4 * N * Zo * Ho * Wo, grid, (size_t)12 * Zo * Ho * Wo)) {
        aesr_set_error("aesr_reslice_grid: out overlaps grid");
        return AESR_ERR_UNSUPPORTED;
    }
    RslAffine A;
    for (int i = 0; i < 12; ++i) A.m[i] = 0.0;
    return rsl_launch("reslice_grid", src, grid, out, A, N, Zs, Hs, Ws, Zo, Ho, Wo, interp, stream);
}

}  // extern "C"
