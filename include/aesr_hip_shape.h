/* libaesr_hip.so -- shape-based label interpolation ABI (twelfth header of the same library; include/aesr_hip.h holds the training and
 * evaluation kernels, and its conventions apply here unchanged: pointers are DEVICE pointers unless named *_host, `stream` is a hipStream_t
 * passed as void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP / AESR_ERR_UNSUPPORTED and
 * leaves its message in aesr_last_error_string()).  Host arrays are read during the call and travel in the kernel arguments; no copy, no
 * synchronisation, capturable.  A refusal writes nothing and names the argument.
 *
 * Shape-based interpolation of label maps (Raya & Udupa 1990, Herman et al. 1992): per class and slice the signed Euclidean distance to
 * the class boundary, a linear blend of the maps of the two neighbouring slices, the class by arg-max.  csrc/shape_interp.hip.
 *
 * labels   uint8  [N][Z][H][W]
 * classes  C class values, 1 <= C <= 8, ascending in 0..255; the background is a class like any other
 * sdm      fp64   [N][C][Z][H][W], 8-byte aligned.  For class c, slice z, pixel p = (y, x), M = the pixels of the slice with label c:
 *            p in M:      +sqrt(min over q not in M of (dy sy) (dy sy) + (dx sx) (dx sx))
 *            p not in M:  -sqrt(min over q in M of the same)
 *          dy, dx integer index differences inside the slice; products, sum and minimum in fp64 in that form, never contracted, then one
 *          correctly rounded sqrt.  An empty set to minimise over (the class is absent from the slice or fills it) gives the magnitude
 *          BIG = sqrt((H sy) (H sy) + (W sx) (W sx)), larger than any distance inside a slice.  Nothing looks across slices.
 * gap      int32  [J] on the DEVICE, 4-byte aligned; alpha fp64 [J] on the DEVICE, 8-byte aligned
 * out      uint8  [N][J][H][W]: with g = clamp(gap[j], 0, max(Z - 2, 0)), g1 = min(g + 1, Z - 1), a = alpha[j], for every class in
 *          ascending order v_c = (1 - a) sdm[c][g] + a sdm[c][g1] in fp64, in that order, no fma; the class value of the FIRST maximum.
 *          The kernel clamps gap itself: no table content makes a load leave sdm.  a == 0 gives slice g and a == 1 slice g1 bit for bit.
 *          Four labels per lane as one 32-bit store where H W % 4 == 0 and out is 4-byte aligned, single bytes otherwise; same values. */
#ifndef AESR_HIP_SHAPE_H
#define AESR_HIP_SHAPE_H

#include <stddef.h>
#include <stdint.h>

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESR_SHAPE_MAX_CLASSES 8
/* longest line of the x pass (64 ballot words in LDS per wave) */
#define AESR_SHAPE_MAX_W 4096

/* bytes of workspace aesr_shape_signed_distances needs (16-byte aligned); 0 for sizes the library refuses */
size_t aesr_shape_workspace_bytes(int N, int Z, int H, int W, int C);

/* AESR_ERR_ARG: a null pointer, sdm not 8-byte or workspace not 16-byte aligned, a non-positive size, C outside 1..8, class values not
 * ascending in 0..255, a spacing that is not positive and finite, workspace_bytes below the query, N C Z H W >= 2^31.
 * AESR_ERR_UNSUPPORTED: W > AESR_SHAPE_MAX_W, an output or the workspace overlapping another buffer. */
int aesr_shape_signed_distances(const uint8_t* labels, double* sdm, void* workspace, size_t workspace_bytes, int N, int Z, int H, int W,
                                const int* classes_host, int C, double sy, double sx, void* stream);

/* AESR_ERR_ARG: a null pointer, sdm or alpha not 8-byte or gap not 4-byte aligned, a non-positive size, C outside 1..8, class values not
 * ascending in 0..255, N C Z H W or N J H W >= 2^31.  AESR_ERR_UNSUPPORTED: out overlapping sdm (or a table). */
int aesr_shape_interpolate(const double* sdm, const int* gap, const double* alpha, uint8_t* out, int N, int C, int Z, int H, int W, int J,
                           const int* classes_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
