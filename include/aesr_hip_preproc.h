/* libaesr_hip.so -- volume pre/post-processing ABI (second header of the same library; include/aesr_hip.h holds the training and
 * evaluation kernels and its conventions on pointers, streams, status codes and aesr_last_error_string() apply here too).
 *
 * In-plane resampling to and from the training spacing: the reference's datasets/common.py:157-206 apply_2d_zoom_3d / _4d, i.e. per
 * slice scipy.ndimage.gaussian_filter(slice, 0.25 / zoom) followed by scipy.ndimage.zoom(volume, (1, zoom_y, zoom_x), order=1) --
 * csrc/inplane.hip.  Every coordinate decision is made by the CALLER on the host in float64 and crosses this boundary as tables, so
 * the kernel decides nothing about coordinates:
 *   iy_host[Ho], ty_host[Ho]   output row o reads input rows iy[o] and min(iy[o] + 1, H - 1) with weights 1 - ty[o] and ty[o];
 *                              iy[o] = -1 marks a DEAD line (scipy's mode='constant', cval=0 when rounding puts the last coordinate
 *                              past H - 1): that output row is exactly 0.  Only the last entry may be dead; the others are
 *                              non-decreasing, 0 <= iy[o] <= H - 1, 0 <= ty[o] <= 1.
 *   ix_host[Wo], tx_host[Wo]   the same along W.
 *   wy_host[2 ry + 1], wx_host[2 rx + 1]   the 1-D Gaussian kernels as scipy computes them (normalised, symmetric, doubles); read only
 *                              when do_blur != 0.  The H pass comes first, then the W pass; the boundary is scipy's 'reflect'
 *                              (d c b a | a b c d); each pass is accumulated in double in scipy's order (centre tap, then the pairs from
 *                              the outermost inwards) and rounded to fp32, as scipy does for fp32 input.  The four bilinear taps are
 *                              summed in double and rounded once.
 * All *_host arrays are HOST memory and are read during the call: the launcher packs them, copies them into `workspace` on `stream`
 * and WAITS for that copy (one hipStreamSynchronize; the arrays may be freed as soon as the call returns), then enqueues one kernel.
 * This entry point is therefore not capturable into a graph.
 *
 * in: [N][H][W] fp32, out: [N][Ho][Wo] fp32 (device; must not overlap), N = slices (T * Z for a 4-D volume: one launch).  `in` is not
 * modified (the reference blurs into its caller's array; this does not).  workspace: aesr_inplane_workspace_bytes(Ho, Wo) bytes of
 * device memory, 8-byte aligned, contents arbitrary.  Input is read once (plus the tile halos), output written once; no other device
 * memory is touched, no atomics.
 *
 * Limits: radii <= 8 per axis (zoom >= ~0.12) and a tile footprint that fits 32 KiB of LDS (always true for tables of a zoom within
 * that radius limit): otherwise AESR_ERR_UNSUPPORTED, the message names the limit, nothing is written.  A null pointer, a non-positive
 * size, H * W or Ho * Wo >= 2^30, 2^31 tiles or more, tables that break the rules above or asymmetric weights: AESR_ERR_ARG, nothing
 * is written. */
#ifndef AESR_HIP_PREPROC_H
#define AESR_HIP_PREPROC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* int(round(n * zoom)) with Python's round (halves to even): the output size scipy.ndimage.zoom gives an axis of n samples.
 * 0 when n <= 0, zoom is not a positive finite number or the result does not fit an int.  Host only. */
int aesr_inplane_out_size(int n, double zoom);

/* Bytes of device workspace aesr_inplane_resample needs for an output of Ho x Wo (the tables and the weights); 0 for a
 * non-positive size.  Host only. */
size_t aesr_inplane_workspace_bytes(int Ho, int Wo);

int aesr_inplane_resample(const float* in, float* out, void* workspace, int N, int H, int W, int Ho, int Wo, const double* wy_host, int ry,
                          const double* wx_host, int rx, const int* iy_host, const double* ty_host, const int* ix_host,
                          const double* tx_host, int do_blur, void* stream);

#ifdef __cplusplus
}
#endif
#endif
