/* libaesr_hip.so -- label-head ABI (seventh header of the same library; include/aesr_hip.h holds the training and evaluation kernels, and
 * its conventions apply here unchanged: pointers are DEVICE pointers, `stream` is a hipStream_t passed as void* (NULL = the default stream),
 * every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP / AESR_ERR_UNSUPPORTED and leaves its message in
 * aesr_last_error_string()).
 *
 * The segmentation head of the multi-channel auto-encoder (networks/acai_multi_channel.py) ends in a softmax over K class logits per pixel;
 * training puts the soft-Dice loss of kwatsch/dice_loss.py on it and inference takes the arg-max label map -- csrc/seg_head.hip does all of
 * that in one pass over the logits forward and one pass backward.
 *
 *   logits, probs, dlogits   [N][H][W][K] fp32 (NHWC: the K values of a pixel are contiguous), K = 2 ... 8
 *   labels                   class ids as fp32, sample n at labels + n * label_stride (in floats), H * W contiguous values each: channel 1
 *                            of an NCHW [N][2][H][W] batch is read in place with labels = batch + H * W, label_stride = 2 * H * W
 *   argmax                   [N][H][W] int32, or NULL
 *   partial                  workspace of aesr_softmax_dice_workspace_floats(N, H, W, K) floats (fully overwritten, no initialisation needed)
 *   sums                     [N][3][K] fp64: I = sum onehot * p, R = sum onehot, P = sum p over the pixels of sample n, per class
 *   loss                     one fp32
 *
 * aesr_softmax_dice_fwd: p = exp(x - max_k x) / sum_k exp(x - max_k x); argmax = the class of the largest p, the LOWEST one among equals;
 *   loss = -(1 / (N K)) sum_{n,k} 2 I / (R + P + 1e-6)  (eps in the denominator only, mean over samples and classes, negative sign).
 *   labels == NULL is inference: only probs and argmax are written; partial, sums and loss may then be NULL and are not touched.
 * aesr_softmax_dice_bwd: gloss is the upstream gradient of the loss as a DEVICE scalar (no host read: capturable);
 *   dL/dp = -(gloss / (N K)) (2 onehot / D - 2 I / D^2) with D = R + P + 1e-6, dlogit_k = p_k (dL/dp_k - sum_j p_j dL/dp_j).
 *
 * Deviation from the reference: a label that is outside [0, K) or not integral (NaN included) belongs to NO class -- it adds to P only --
 * where torch's scatter_ in DiceLoss.forward would raise.
 *
 * The sums are made in two stages in a fixed order -- fp32 partials per workgroup of 1024 pixels, then added in fp64 in block order -- with
 * no floating-point atomics: results do not depend on scheduling and two runs give the same bits.  A pixel is one 16-byte access for K = 4
 * (two for K = 8) when logits / probs / dlogits are 16-byte aligned, 4-byte accesses otherwise; the values do not depend on the alignment.
 * The caller owns every buffer; nothing is allocated and nothing synchronises.
 *
 * Refusals: a null pointer that is not optional, a pointer that is not 4-byte (sums: 8-byte) aligned, a non-positive size, K outside
 * 2 ... 8, 2^31 elements or more (N * H * W * K, or the span of the labels), label_stride < H * W with N > 1: AESR_ERR_ARG.  An output that
 * overlaps an input or another output: AESR_ERR_UNSUPPORTED.  Nothing is written in a refusal.  The workspace query returns 0 for sizes
 * the launch entry points refuse. */
#ifndef AESR_HIP_SEG_H
#define AESR_HIP_SEG_H

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t aesr_softmax_dice_workspace_floats(int N, int H, int W, int K);

int aesr_softmax_dice_fwd(const float* logits, const float* labels, size_t label_stride, float* probs, int* argmax, float* partial,
                          double* sums, float* loss, int N, int H, int W, int K, void* stream);

int aesr_softmax_dice_bwd(const float* probs, const float* labels, size_t label_stride, const double* sums, const float* gloss,
                          float* dlogits, int N, int H, int W, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif
