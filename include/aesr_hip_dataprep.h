/* libaesr_hip.so -- brain data preparation ABI (third header of the same library; include/aesr_hip.h holds the training and evaluation
 * kernels, and its conventions apply here unchanged: pointers are DEVICE pointers unless named *_host, `stream` is a hipStream_t passed
 * as void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP / AESR_ERR_UNSUPPORTED and
 * leaves its message in aesr_last_error_string()).
 *
 * Thick-slice simulation: the reference's datasets/common_brains.py:37-44 simulate_thick_slices, i.e. for every (y, x) column of a
 * [Z][H][W] volume scipy.ndimage.gaussian_filter1d(column, sigma = thickness / 2.355) -- csrc/thick_slices.hip:
 *   out[o][y][x] = gaussian_filter1d(in[:, y, x], sigma)[o * z_step],   o = 0 .. aesr_thick_slices_out_slices(Z, z_step) - 1.
 * z_step = 1 writes the whole blurred volume (dataset creation); z_step = k computes only the slices that [::k] keeps (training and
 * evaluation: 1/k of the work and of the bytes written).
 *   weights_host[2 radius + 1]  the 1-D Gaussian kernel as scipy computes it (float64, normalised, symmetric; radius = int(4 sigma + 0.5)).
 *                               HOST memory, read during the call and copied into the kernel's ARGUMENTS: no workspace, no copy, no
 *                               synchronisation -- the call is capturable into a graph, the array may be freed when it returns.
 * Arithmetic, as scipy's for fp32 input: boundary `reflect` (d c b a | a b c d, repeated when the radius exceeds Z; Z = 1 works); the
 * sum is accumulated in double -- the centre tap, then the pairs (in[z - l] + in[z + l]) * w[l] from the outermost inwards --, never
 * contracted to a fused multiply-add, and rounded to fp32 once.
 * in: [Z][H][W] fp32, out: [Zo][H][W] fp32 (must not overlap); `in` is not modified.  Input is read once per workgroup (plus the z halo of
 * the neighbouring workgroup), output written once; no other device memory is touched, no atomics.  Stores are 16 bytes per lane when
 * W % 4 == 0 and both pointers are 16-byte aligned, 4 bytes per lane otherwise; the values do not depend on the path.
 *
 * Limits: radius <= 16 (thickness <= 9.7): otherwise AESR_ERR_UNSUPPORTED.  A null pointer, a non-positive size, z_step < 1, a negative
 * radius, Z * H * W >= 2^31, asymmetric weights or weights that do not sum to 1 within 1e-12: AESR_ERR_ARG.  In every refusal the message
 * names the offending argument and nothing is written. */
#ifndef AESR_HIP_DATAPREP_H
#define AESR_HIP_DATAPREP_H

#include <stddef.h>

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ceil(Z / z_step): the slices [::z_step] keeps of Z.  0 when Z <= 0 or z_step < 1.  Host only. */
int aesr_thick_slices_out_slices(int Z, int z_step);

/* 16 or 4: the bytes per lane aesr_thick_slices loads and stores for these arguments (16 when W % 4 == 0 and both pointers are 16-byte
 * aligned).  The launcher decides with this very function; the values written do not depend on it.  Host only, nothing is dereferenced. */
int aesr_thick_slices_store_bytes(int W, const float* in, const float* out);

int aesr_thick_slices(const float* in, float* out, int Z, int H, int W, int z_step, const double* weights_host, int radius, void* stream);

/* aesr_triplet_assemble (include/aesr_hip.h) without the intensity curve: the same descriptors, gather, zero padding, rot90 and
 * [from... | to...] / between layout, but `gain` and `cutoff` are ignored and the values are copied unchanged (the padding is 0).  The
 * reference's brain TEST transform (datasets/common_brains.py:58,71,85: AdjustToPatchSize + ToTensor only). */
int aesr_triplet_assemble_raw(const float* volumes, const aesr_triplet_desc* desc_host, int B, int width, float* image, float* between,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
