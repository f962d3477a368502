/* libaesr_hip.so -- fused training-step ABI (fourth header of the same library; include/aesr_hip.h holds the training and evaluation
 * kernels, and its conventions apply here unchanged: pointers are DEVICE pointers, activations are fp32 NHWC, `stream` is a hipStream_t
 * passed as void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP and leaves its message
 * in aesr_last_error_string(); activation codes: 0 none, 1 LeakyReLU(slope), 2 ReLU, 3 sigmoid).
 *
 * The whole backward of a Cout == 1, 3x3, padding-1 convolution with bias  out = act(conv(x, W) + b)  in ONE pass over its saved input x
 * (csrc/conv_thin.hip: thin_reduce_kernel<false, true> + thin_cout1_finish_kernel), two launches.  It replaces, with bit-identical
 * results, the sequence
 *     aesr_act_bwd(dout, out, dpre, act, slope)                         dpre = dout * act'(out)
 *     aesr_conv2d_cout1_wgrad(x, dpre, dw, db, ...)                     dw, db
 *     aesr_conv2d_cout1_dgrad_pre(dpre, w_flipped, x, dx, mask_act, ..) dx = mask'(x) * conv(dpre, flipped W)
 * of include/aesr_hip.h, which reads x twice (once for dw, once as the mask of dx) and takes five launches.  x is at once the
 * convolution's saved input and the saved OUTPUT of the activation `mask_act` in front of it, whose derivative (from that output)
 * multiplies dx; mask_act = 0: no mask.  dpre is never stored: the derivative of `act` is applied while dout is staged.
 *   dw [1][Cin][3][3] and db [1] are overwritten (not accumulated), dx [N,H,W,Cin] is written in full; x, dout, out and w_flipped are not
 *   modified; dx must not overlap x.  workspace: aesr_conv2d_cout1_bwd_workspace_floats(Cin) floats, contents ignored on entry.
 * Cin must be 4 times a power of two (4..256).  A null pointer (out may be NULL only when act == 0), an empty shape, another Cin or an
 * unknown activation code: AESR_ERR_ARG, nothing is launched, nothing is written. */
#ifndef AESR_HIP_TRAIN_H
#define AESR_HIP_TRAIN_H

#include <stddef.h>

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (512 + 1) * 10 * Cin: the partial sums of the 512 workgroups (and room for their total).  0 when Cin <= 0.  Host only. */
size_t aesr_conv2d_cout1_bwd_workspace_floats(int Cin);

int aesr_conv2d_cout1_bwd(const float* x,         /* [N,H,W,Cin] saved input of the conv (= mask tensor)          */
                          const float* dout,      /* [N,H,W]     dL/d(out), behind the conv's own activation      */
                          const float* out,       /* [N,H,W]     saved conv output; may be NULL when act == NONE  */
                          const float* w_flipped, /* [9][Cin]    wexp[t][ci] = W[0,ci,8-t] (weight preparation)   */
                          float* dw, float* db, float* dx, float* workspace, int N, int H, int W, int Cin, int act, float slope,
                          int mask_act, float mask_slope, void* stream);

#ifdef __cplusplus
}
#endif
#endif
