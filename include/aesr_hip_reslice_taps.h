/* libaesr_hip.so -- higher-order reslicing ABI (thirteenth header of the same library; include/aesr_hip.h holds the training and
 * evaluation kernels, and its conventions apply here unchanged: pointers are DEVICE pointers unless named *_host, `stream` is a hipStream_t
 * passed as void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP / AESR_ERR_UNSUPPORTED and
 * leaves its message in aesr_last_error_string()).  m_host is read during the call and travels in the kernel arguments; no copy, no
 * allocation, no synchronisation, capturable.  A refusal comes before anything touches the device, writes nothing and names the argument.
 *
 * Affine reslicing with a higher-order kernel evaluated at a free 3-D position: the cubic B-spline over a separable 3-D pre-filter, and the
 * Lanczos- and cosine-windowed sincs (ITK's WindowedSincInterpolateImageFunction; sitkCosineWindowedSinc is what the reference's
 * kwatsch/create_nifti_from_dicom.py generate_resampled_image reslices with).  csrc/reslice_taps.hip, csrc/bspline_prefilter.hip.
 *
 * src   fp32 [N][Zs][Hs][Ws] samples (the sincs), 4-byte aligned
 * coef  fp64 [N][Zs][Hs][Ws] coefficients of aesr_bspline_prefilter_3d (BSPLINE3), 8-byte aligned, aesr_bspline_coef_bytes(N, Z, H, W) bytes
 * out   fp32 [N][Zo][Ho][Wo], 4-byte aligned
 *
 * All arithmetic is fp64 and never contracted.  Position: (x, y, z) = M (xo, yo, zo, 1) with M = m_host as 3 rows of 4, evaluated as
 * aesr_reslice_affine evaluates it (the same device function: bit-identical positions).  Inside rule (ITK's buffer rule, default pixel 0): a
 * voxel is computed only if -0.5 <= p < size - 0.5 on all three axes, anything else (a position that is not finite included) is 0.0f.
 * Per axis b = floor(p), t = p - b, taps k = -R + 1 ... R around b:
 *   BSPLINE3  R = 2; w = (u u u / 6, (t t (t - 2) 3 + 4) / 6, (u u (u - 2) 3 + 4) / 6, 1 - w0 - w1 - w2) with u = 1 - t; indices mirrored about
 *             the first and last sample (whole-sample, period 2 size - 2; size 1: index 0); source coef
 *   LANCZOS   R in {3, 4, 5}; d = t - k, w = sinc(d) sinc(d / R), sinc(u) = sin(pi u) / (pi u); t == 0: exactly the sample (1 at k = 0, else 0);
 *             t == 1 (p - floor(p) rounds to 1.0 for p in (-2^-54, 0)): exactly the sample b + 1 (1 at k = 1, else 0);
 *             not normalised (ITK does not either); indices clamped (ZeroFluxNeumann); source src
 *   COSINE    as LANCZOS with w = sinc(d) cos(pi d / (2 R))
 * Sum: acc = 0.0; for kz, ky, kx ascending, kx fastest: acc += ((wz wy) wx) (double)v; one rounding to fp32; clamp01 = 1 then clamps the fp32
 * value to [0, 1].  Indices, validity and weights are computed once per output voxel and reused for the N frames: a frame's result is
 * bit-identical whether it is computed alone or as one of N. */
#ifndef AESR_HIP_RESLICE_TAPS_H
#define AESR_HIP_RESLICE_TAPS_H

#include <stddef.h>
#include <stdint.h>

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESR_TAPS_BSPLINE3 0
#define AESR_TAPS_LANCZOS 1
#define AESR_TAPS_COSINE 2
#define AESR_TAPS_MIN_RADIUS 3
#define AESR_TAPS_MAX_RADIUS 5

/* scipy.ndimage.spline_filter(in, order=3, mode='mirror', output=float64) per frame: the 1-D filter of aesr_bspline_prefilter_z (gain 6, pole
 * sqrt(3) - 2, causal start summed exactly over the whole line, the same anti-causal start, a line of one sample is its own coefficient)
 * along z, then y, then x; y and x run in place on coef.  Three launches (fewer where H or W is 1).
 * AESR_ERR_ARG: a null pointer, in not 4-byte or coef not 8-byte aligned, a non-positive size, N Z H W >= 2^31.
 * AESR_ERR_UNSUPPORTED: coef overlapping in. */
int aesr_bspline_prefilter_3d(const float* in, double* coef, int N, int Z, int H, int W, void* stream);

/* Exactly one of src and coef is non-null: coef with kernel == AESR_TAPS_BSPLINE3 (radius is then only validated), src with the sincs.
 * AESR_ERR_ARG: a null out or m_host, both or neither of src and coef or the wrong one for the kernel, a misaligned pointer, a non-positive
 * size, a kernel outside 0..2, a radius outside 3..5, clamp01 not 0 or 1, a matrix entry that is not finite, 2^31 elements or more on either
 * side.  AESR_ERR_UNSUPPORTED: out overlapping the source. */
int aesr_reslice_taps_affine(const float* src, const double* coef, float* out, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo,
                             const double* m_host, int kernel, int radius, int clamp01, void* stream);

#ifdef __cplusplus
}
#endif
#endif
