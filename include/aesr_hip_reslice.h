/* libaesr_hip.so -- oblique reslicing ABI (sixth header of the same library; include/aesr_hip.h holds the training and evaluation
 * kernels, and its conventions apply here unchanged: pointers are DEVICE pointers unless named *_host, `stream` is a hipStream_t passed as
 * void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP / AESR_ERR_UNSUPPORTED and leaves
 * its message in aesr_last_error_string()).
 *
 * A 3-D interpolating gather: every voxel of an output grid [Zo][Ho][Wo] is given a continuous position (x, y, z) in the voxel grid of a
 * source volume [Zs][Hs][Ws] and takes the trilinear (or nearest) value there -- csrc/reslice.hip.  This is what puts a short-axis stack
 * into the geometry of a long-axis scan (the reference's evaluate/cardiac/resample_sax_to_lax.py: world-coordinate affines and a 5-D
 * torch.nn.functional.grid_sample(mode='bilinear' | 'nearest', padding_mode='zeros', align_corners=True)).  The position is the same for
 * all N frames; it comes from
 *   aesr_reslice_affine   (x, y, z) = M * (xo, yo, zo, 1): m_host[12] holds the rows of the 3x4 matrix M, HOST memory, read during the call
 *                         and copied into the kernel's ARGUMENTS.  Each coordinate is ((m[0] * xo + m[1] * yo) + m[2] * zo) + m[3] in fp64,
 *                         never contracted to a fused multiply-add: an M of exact integers gives exact integer positions.
 *   aesr_reslice_grid     grid[zo][yo][xo][0..2] = (x, y, z) normalised to [-1, 1] as grid_sample takes it with align_corners=True; one grid
 *                         for all N frames.  The fp32 value g is converted to fp64 FIRST and unnormalised as (g + 1) / 2 * (size - 1) with
 *                         size = Ws, Hs, Zs (in that operation order, in fp64).
 * Both calls need no workspace, copy nothing, do not synchronise and are capturable into a graph; m_host may be freed when the call returns.
 *
 * Arithmetic (all in fp64; #pragma fp contract off):
 *   AESR_RESLICE_LINEAR   x0 = floor(x), the weight pair of the axis is w[0] = (x0 + 1) - x, w[1] = x - x0; likewise y and z.  The corner
 *                         (dz, dy, dx) has the weight (wz[dz] * wy[dy]) * wx[dx] and contributes only if (x0 + dx, y0 + dy, z0 + dz) lies
 *                         inside the source: padding is zeros, a corner outside adds 0.0 and no sample is used for it (no load leaves the
 *                         volume).  The eight products weight * (double) sample are added to 0.0 in the fixed order dz, dy, dx ascending
 *                         (dx fastest) and the sum is rounded to fp32 once.
 *   AESR_RESLICE_NEAREST  (rint(x), rint(y), rint(z)), halves to even as nearbyint does; the sample there if it is inside, else 0.
 * A position that is not finite, or so far outside that no corner can be inside, gives 0.  Indices, validity and weights are computed once
 * per output voxel and reused for the N frames: a frame's result is bit-identical whether it is computed alone or as one of N.
 *
 * src: [N][Zs][Hs][Ws] fp32, out: [N][Zo][Ho][Wo] fp32; src and grid are not modified.  A lane computes one voxel and stores 4 bytes, a
 * wave one 256-byte row segment, whatever the alignment of out (a form with 16-byte stores per lane was measured slower and is not kept:
 * profiles/reslice.txt); the values do not depend on the alignment of any pointer.  No atomics, no scratch, no LDS; no other device memory
 * is touched.
 *
 * Refusals: a null pointer (src, out, grid, m_host), a device pointer that is not 4-byte aligned, a non-positive size, interp that is
 * neither 0 nor 1, an m_host entry that is not finite, 2^31 elements or more on either side (N * Zs * Hs * Ws, N * Zo * Ho * Wo):
 * AESR_ERR_ARG.  out overlapping src or grid: AESR_ERR_UNSUPPORTED.  In every refusal the message names the offending argument and nothing
 * is written. */
#ifndef AESR_HIP_RESLICE_H
#define AESR_HIP_RESLICE_H

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* AESR_RS_* of include/aesr_hip.h are the modes of aesr_resample2_*; these are the interpolators of the two calls below */
#define AESR_RESLICE_NEAREST 0
#define AESR_RESLICE_LINEAR 1

int aesr_reslice_affine(const float* src, float* out, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo, const double* m_host, int interp,
                        void* stream);

int aesr_reslice_grid(const float* src, const float* grid, float* out, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo, int interp,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
