/* libaesr_hip.so -- train-mode BatchNorm2d + AvgPool2d(2), pooled once (a further header of the same library; include/aesr_hip.h holds
 * the training kernels, and its conventions apply here unchanged: pointers are DEVICE pointers unless marked host, activations are fp32
 * NHWC, `stream` is a hipStream_t passed as void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG /
 * AESR_ERR_HIP and leaves its message in aesr_last_error_string(); statistic groups: images nstart[g] .. nstart[g + 1] - 1 form group g,
 * nstart is a host array of G + 1 ints with nstart[0] = 0, strictly increasing, nstart[G] = N; counts is a host array of G doubles, the
 * values per channel of each group).
 *
 * The fourth launch form of the BatchNorm call  out = AvgPool2d(2)(BatchNorm(y)),  for the calls that aesr_bn_stats_finalize + aesr_bn_apply
 * (mode AESR_BN_POOL) and aesr_bn_bwd serve.  The statistics pass has every 2x2 window of y in registers: it also writes the windows' means
 * m [N][H/2][W/2][C], and the forward apply and the backward reduction read m -- a quarter of y -- where they read y before:
 *
 *   aesr_bn_pool_stats_finalize   y -> m, mean / invstd / scale / shift [G][C], running statistics        (two launches)
 *   aesr_bn_pool_apply            out = scale * m + shift                                                 (one launch)
 *   aesr_bn_pool_bwd              sum g = sum_windows g_pool, sum g * xhat = sum_windows g_pool * ((m - mean) * invstd)  -> coef, dgamma,
 *                                 dbeta; then dpre as aesr_bn_bwd (that pass still reads y: xhat and act'(y) per pixel)  (three launches)
 *
 * Bit for bit the same as the three-launch route: m = aesr_bn_apply(y, scale = 1, shift = 0, AESR_BN_POOL); out for given scale / shift;
 * dpre for given coef.  The per-channel sums are taken over windows instead of pixels, so mean, invstd, scale, shift, the running
 * statistics, coef, dgamma and dbeta (and through them out and dpre) differ from that route by summation order only; every result is
 * bitwise repeatable (no atomics).  The pixels the pooling leaves out (odd H or W) count for the statistics and get dpre; they carry no
 * gradient into the sums.
 *
 * partial: G * 512 * 2 * C floats of scratch, contents ignored on entry.  A null pointer, a shape aesr_bn_pool_supported refuses or a bad
 * group table: AESR_ERR_ARG, nothing is launched, nothing is written. */
#ifndef AESR_HIP_BNPOOL_H
#define AESR_HIP_BNPOOL_H

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where the three entry points below take a call of N images of H x W x C in G groups: C a multiple of 4 with C / 4 a divisor of 256
 * (so C <= 1024), H >= 2, W >= 2, 1 <= G <= 4, N >= G, N * H * W < 2^31; else 0.  Host only. */
int aesr_bn_pool_supported(int N, int H, int W, int C, int G);

int aesr_bn_pool_stats_finalize(const float* y,              /* [N,H,W,C]                                                        */
                                float* m,                    /* [N,H/2,W/2,C] the 2x2 means, written in full                     */
                                float* partial, const double* counts_host, const float* gamma, const float* beta,
                                float* running_mean, float* running_var,       /* [C], stepped group after group when update_running; may be NULL */
                                int64_t* num_batches_tracked,                  /* advanced by G when update_running; may be NULL  */
                                float* mean, float* invstd, float* scale, float* shift,       /* [G][C], written                 */
                                int N, int H, int W, int C, int G, const int* nstart_host, float momentum, float eps, int update_running,
                                void* stream);

int aesr_bn_pool_apply(const float* m, const float* scale, const float* shift, float* out /* [N,Ho,Wo,C] */, int N, int Ho, int Wo, int C,
                       int G, const int* nstart_host, void* stream);

/* N: the leading images that carry a gradient (whole groups: nstart[G] = N); y and m may hold more images behind them.
 * gout [N,H/2,W/2,C]; mean / invstd / scale [G][C] of the forward call; coef [G][2][C], dgamma [C], dbeta [C], dpre [N,H,W,C] are written;
 * act / slope: the activation that produced y (its derivative is folded into dpre). */
int aesr_bn_pool_bwd(const float* gout, const float* y, const float* m, const float* mean, const float* invstd, const float* scale,
                     float* partial, const double* counts_host, float* coef, float* dgamma, float* dbeta, float* dpre, int N, int H, int W,
                     int C, int act, float slope, int G, const int* nstart_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
