/* libaesr_hip.so -- labelled training batches ABI (tenth header of the same library; include/aesr_hip.h holds the training and evaluation
 * kernels, and its conventions apply here unchanged: pointers are DEVICE pointers unless named *_host, `stream` is a hipStream_t passed as
 * void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP and leaves its message in
 * aesr_last_error_string()).
 *
 * aesr_triplet_assemble (include/aesr_hip.h) for volumes that come with a label map -- csrc/augment_labelled.hip.  What the reference's
 * ACDCDatasetEDESPairs (datasets/ACDC/data_with_labels.py) hands train_cardiac_aesr.py:83-105 and prepare_batch_pairs re-lays
 * (datasets/ACDC/data4d_simple.py:349-353), from two device-resident caches in ONE launch:
 *   images   float32; the volumes [Z][H][W], one after the other
 *   labels   uint8, the SAME layout: an image volume and its label volume have the same shape, so a descriptor's vol_off, counted in
 *            elements, addresses both (as a float offset into images and as a byte offset into labels)
 * The descriptors (aesr_triplet_desc, HOST array, read during the call; 1 <= B <= 64 per call) mean what they mean for
 * aesr_triplet_assemble.  For sample b, slice s in {from, to, between} and output pixel (i, j): (u, v) = rot90^-k (i, j) as np.rot90 counts,
 * (y, x) = (oy + u, ox + v), and
 *   channel 0 = 1 / (1 + expf(gain * (cutoff - v_img))) in fp32, v_img = images[vol_off + (z_s * H + y) * W + x] or 0 outside the slice --
 *               the expression of aesr_triplet_assemble, bit for bit; aesr_labelled_triplet_assemble_raw writes v_img unchanged (the test
 *               transform: no intensity curve; gain and cutoff are ignored)
 *   channel 1 = (float) labels[the same index], 0 outside the slice: padding is background and the label channels stay out of the
 *               intensity curve (RandomIntensity(slice_mask = [1, 0, 1, 0, 1, 0])).  A label is copied: never interpolated, and any byte
 *               value passes -- what counts as a class is the label head's business.
 * Outputs are NCHW fp32: image [2B][2][width][width] (all "from" rows, then all "to" rows), between [B][2][width][width].  Every element of
 * both is written; images and labels are not modified; no other device memory is touched, no atomics, no workspace, no synchronisation
 * (capturable into a graph; desc_host may be freed when the call returns).  The values do not depend on the alignment of any pointer
 * (labels may start at any byte; the float pointers need their natural 4 bytes).  Per batch the launch reads 3 B width^2 * (4 + 1) bytes
 * and writes 3 B width^2 * 8.
 *
 * Slice indices are NOT checked against Z, which a descriptor does not carry: the caller does that (data_device.LabelledTripletAugmenter).
 * Refusals (AESR_ERR_ARG; the message names the function and the argument; nothing is launched, nothing written): a null pointer, B outside
 * 1 .. 64, width < 1, width^2 >= 2^30, a descriptor with H or W < 1, H * W >= 2^30, a negative vol_off or slice index, or k outside 0 .. 3. */
#ifndef AESR_HIP_LABELPREP_H
#define AESR_HIP_LABELPREP_H

#include <stdint.h>

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int aesr_labelled_triplet_assemble(const float* images, const uint8_t* labels, const aesr_triplet_desc* desc_host, int B, int width, float* image,
                                   float* between, void* stream);

int aesr_labelled_triplet_assemble_raw(const float* images, const uint8_t* labels, const aesr_triplet_desc* desc_host, int B, int width,
                                       float* image, float* between, void* stream);

#ifdef __cplusplus
}
#endif
#endif
