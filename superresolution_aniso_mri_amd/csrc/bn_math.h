// The arithmetic of nn.BatchNorm2d, stated ONCE for the launch forms (device-inline only; included by bn.hip and bn_fused.hip):
//   three launches   bn.hip: statistics -> [reduce +] finalize -> apply            (backward: reduce -> [reduce +] finalize -> apply)
//   SyncBN           bn.hip: ... all-reduce of the sums, then finalize inside the apply launch  (bn_finalize_apply, bn_bwd_finalize_apply)
//   one launch       bn_fused.hip: the layer resident in LDS, one grid barrier
//   pooled once      bn.hip: the three launches with AvgPool2d(2) behind them; the statistics pass writes the 2x2 means, which the apply and the
//                    backward reduction stream instead of the activation (include/aesr_hip_bnpool.h)
// The forms differ in how the sums are reduced and in where the tables live; everything from the sums on is here.  The Makefile compiles
// with -ffp-contract=off, so an expression means the same operations in the same order wherever it is inlined: the forms agree bit for bit
// wherever they are given the same sums (tests/test_gpu_kernels.py: test_bn_groups_fwd_bwd).
#pragma once
#include "aesr_kernels.h"

// statistic group of image n: the last g with nstart[g] <= n
__device__ __forceinline__ int bn_group_of(int G, const int* nstart, int n) {
    int g = 0;
    for (int k = 1; k < G; ++k)
        if (n >= nstart[k]) g = k;
    return g;
}

// ---- forward: how the sums are taken -------------------------------------------------------------------------------------------------
// The variance is s1 / M - mean^2, and fp32 squares and fp32 running sums carry an error of 2^-24 * E[x^2], which that subtraction magnifies by
// (mean / sigma)^2: a channel at 12.8 +- 0.1 lost four digits of its invstd, a constant channel came out with a variance.  So every statistics
// pass (bn_stats_kernel, bn_stats_kernel_pool, phase 1 of bn_fused_fwd_kernel) accumulates d = v - K, sum d and sum d * d in fp32, about a
// per-channel pivot K[g][c] = the mean of eight pixels of the group in this call's y (bn_pivot4), so |mean - K| is a fraction of sigma and the
// fp32 sums are as accurate as for centred data (bn.hip adds a workgroup's up to 128 lanes in fp64 before it rounds the partial:
// with the pivot k sigma off the mean every rounding of sum d * d counts (1 + k^2) times in the variance).  Where the fp32 partials have become fp64 totals (bn_reduce_pivot_kernel,
// bn_reduce_finalize_kernel, bn_fused_fwd_kernel behind bf_totals) bn_unpivot turns them into the sums about 0 in fp64: everything from
// sums[g][2][C] on -- bn_moments, the all-reduce and the peer exchange of SyncBN, whose ranks each have a pivot of their own -- is unchanged.
// (fp64 leaves (mean / sigma)^2 * 2^-53: 5e-10 at a ratio of 2000.)  tests/test_gpu_bn_conditioning.py holds every form to it.
__device__ __forceinline__ void bn_unpivot(double sd, double qd, double M, double K, double* s0, double* s1) {
    *s0 = sd + M * K;
    *s1 = qd + 2.0 * K * sd + M * K * K;
}

// The pivot of the group with pixels [p0, p1), channels c..c+3 / channel c: the mean of BN_PIVOT_N of its pixels, one from each such part of the group and off the
// image border for the usual widths (any value near the channel's mean serves; both forms below are the same fp32 operations, so the
// statistics pass and the conversion use the same bits).  One pixel alone sits 1 sigma out on average and 3 sigma out for some channel of a
// layer, which costs well-centred channels (1 + 3^2) roundings where the sums about 0 cost them 2; eight pixels bring that distance to a third.
// An empty group has no pivot and needs none.
#define BN_PIVOT_N 8          // pixels in the pivot (a power of two: the mean is a sum and an exact scaling)
__device__ __forceinline__ size_t bn_pivot_pixel(size_t p0, size_t p1, int j) {
    const size_t M = p1 - p0, i = ((size_t)(2 * j + 1) * M) / (2 * BN_PIVOT_N) + (size_t)(17 + 37 * j);
    return p0 + (i < M ? i : M - 1);
}
__device__ __forceinline__ f32x4 bn_pivot4(const float* y, size_t p0, size_t p1, int C, int c) {
    if (p0 >= p1) return (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 v[BN_PIVOT_N];
#pragma unroll
    for (int j = 0; j < BN_PIVOT_N; ++j) v[j] = *(const f32x4*)(y + bn_pivot_pixel(p0, p1, j) * C + c);
    f32x4 t = v[0];
#pragma unroll
    for (int j = 1; j < BN_PIVOT_N; ++j) t += v[j];
    return t * (1.f / BN_PIVOT_N);
}
__device__ __forceinline__ double bn_pivot1(const float* y, size_t p0, size_t p1, int C, int c) {
    if (p0 >= p1) return 0.0;
    float v[BN_PIVOT_N];
#pragma unroll
    for (int j = 0; j < BN_PIVOT_N; ++j) v[j] = y[bn_pivot_pixel(p0, p1, j) * C + c];
    float t = v[0];
#pragma unroll
    for (int j = 1; j < BN_PIVOT_N; ++j) t += v[j];
    return (double)(t * (1.f / BN_PIVOT_N));
}

// The pivot of a whole block through LDS: the C / 4 threads of the first pixel lane load it, everybody reads it (each thread loading for
// itself asks every block's 256-512 threads for the same few cache lines: +1 us per launch).  Every thread of the block calls it; scratch holds C
// floats and is free again on return.
__device__ __forceinline__ f32x4 bn_pivot_block(const float* y, size_t p0, size_t p1, int C, float* scratch) {
    const int C4 = C >> 2, c4 = threadIdx.x % C4;
    if ((int)threadIdx.x < C4) *(f32x4*)(scratch + c4 * 4) = bn_pivot4(y, p0, p1, C, c4 * 4);
    __syncthreads();
    const f32x4 K = *(const f32x4*)(scratch + c4 * 4);
    __syncthreads();
    return K;
}

// ---- forward: sums -> mean / invstd / scale / shift / running statistics -----------------------------------------------------------
// moments of M values from their sum s0 and sum of squares s1, in fp64: mean, 1 / sqrt(biased variance + eps); returns the biased variance
__device__ __forceinline__ double bn_moments(double s0, double s1, double M, float eps, float* mean, float* invstd) {
    const double mu = s0 / M;
    double var = s1 / M - mu * mu;
    if (var < 0.0) var = 0.0;
    *mean = (float)mu;
    *invstd = (float)(1.0 / sqrt(var + (double)eps));
    return var;
}

// the variance the running statistics take (a division more: only where they are updated)
__device__ __forceinline__ double bn_unbiased(double var, double M) { return M > 1.0 ? var * M / (M - 1.0) : var; }

// the affine map of the normalisation: out = scale * y + shift
__device__ __forceinline__ float bn_scale(float gamma, float invstd) { return gamma * invstd; }
__device__ __forceinline__ float bn_shift(float beta, float mean, float scale) { return beta - mean * scale; }

// one momentum step of the running statistics (fp32, as nn.BatchNorm2d); several groups = several steps, group after group
__device__ __forceinline__ void bn_running_step(float momentum, float mean, double unbiased, float* running_mean, float* running_var) {
    *running_mean = (1.f - momentum) * *running_mean + momentum * mean;
    *running_var = (1.f - momentum) * *running_var + momentum * (float)unbiased;
}

// Finalize inside an apply launch: EVERY block derives scale / shift for all groups and channels from sums[g][2][C] (fp64; global memory or
// LDS) into its LDS tables s_sc / s_sh [g][C]; the block with first == true also writes mean / invstd / scale / shift for the backward pass
// and steps the running statistics.  P: BnFinArgs or BnFusedArgs (gamma, beta, running_*, nbt, mean, invstd, scale, shift, C, G, momentum,
// eps, update_running, counts).  NT threads; the caller barriers before it reads the tables.
template <int NT, class P>
__device__ __forceinline__ void bn_fwd_tables(const double* sums, const P& f, bool first, float* s_sc, float* s_sh) {
    const int C = f.C, GC = f.G * C;
    for (int i = threadIdx.x; i < GC; i += NT) {
        const int g = i / C, c = i - g * C;
        float m, iv;
        bn_moments(sums[(g * 2 + 0) * C + c], sums[(g * 2 + 1) * C + c], f.counts.c[g], f.eps, &m, &iv);
        const float sc = bn_scale(f.gamma[c], iv), sh = bn_shift(f.beta[c], m, sc);
        s_sc[i] = sc;
        s_sh[i] = sh;
        if (first) {
            f.mean[i] = m;
            f.invstd[i] = iv;
            f.scale[i] = sc;
            f.shift[i] = sh;
        }
    }
    if (first && f.update_running) {
        if (threadIdx.x == 0 && f.nbt) *f.nbt += f.G;
        for (int c = threadIdx.x; c < C; c += NT) {
            float rm = f.running_mean[c], rv = f.running_var[c];
            for (int g = 0; g < f.G; ++g) {             // group after group, as the reference's successive calls
                float m, iv;
                const double var = bn_moments(sums[(g * 2 + 0) * C + c], sums[(g * 2 + 1) * C + c], f.counts.c[g], f.eps, &m, &iv);
                bn_running_step(f.momentum, m, bn_unbiased(var, f.counts.c[g]), &rm, &rv);
            }
            f.running_mean[c] = rm;
            f.running_var[c] = rv;
        }
    }
}

// ---- backward: sums (s1 = sum g, s2 = sum g * xhat) -> coefficients, dgamma, dbeta ---------------------------------------------------
__device__ __forceinline__ float bn_bwd_coef(double sum, double M) { return (float)(sum / M); }

// One channel c: dgamma[c] = sum_g s2, dbeta[c] = sum_g s1 in fp64 and group order; COEF: coef[g][2][C] = sums / M on the way.
// The channel's sums are s[(g * 2 + {0, 1}) * stride + ci].
template <bool COEF>
__device__ __forceinline__ void bn_bwd_channel(const double* s, int stride, int ci, const double* M, int G, int C, int c, float* coef,
                                               float* dgamma, float* dbeta) {
    double dg = 0.0, db = 0.0;
    for (int g = 0; g < G; ++g) {
        const double s1 = s[(g * 2 + 0) * stride + ci], s2 = s[(g * 2 + 1) * stride + ci];
        if (COEF) {
            coef[(g * 2 + 0) * C + c] = bn_bwd_coef(s1, M[g]);
            coef[(g * 2 + 1) * C + c] = bn_bwd_coef(s2, M[g]);
        }
        db += s1;
        dg += s2;
    }
    dgamma[c] = (float)dg;
    dbeta[c] = (float)db;
}

// The backward counterpart of bn_fwd_tables: every block's LDS table s_k[g][2][C] = sums / M; the first block writes coef / dgamma / dbeta.
template <int NT>
__device__ __forceinline__ void bn_bwd_tables(const double* sums, const double* M, int G, int C, bool first, float* s_k, float* coef,
                                              float* dgamma, float* dbeta) {
    const int GC2 = G * 2 * C;
    for (int i = threadIdx.x; i < GC2; i += NT) {
        const float k = bn_bwd_coef(sums[i], M[i / (2 * C)]);
        s_k[i] = k;
        if (first) coef[i] = k;
    }
    if (first)
        for (int c = threadIdx.x; c < C; c += NT) bn_bwd_channel<false>(sums, C, c, M, G, C, c, nullptr, dgamma, dbeta);
}

// ---- element formulas (four channels of one pixel) --------------------------------------------------------------------------------------
// AvgPool2d(2) of the BatchNorm input: the affine map commutes with the mean, so the window is averaged first
__device__ __forceinline__ f32x4 bn_pool2x2(f32x4 v00, f32x4 v01, f32x4 v10, f32x4 v11) { return ((v00 + v01) + (v10 + v11)) * 0.25f; }

__device__ __forceinline__ f32x4 bn_fwd_elem(f32x4 v, f32x4 sc, f32x4 sh) { return v * sc + sh; }

// gradient w.r.t. the input of the activation that produced y, from gg = the gradient w.r.t. the BatchNorm output at this pixel
__device__ __forceinline__ f32x4 bn_bwd_elem(f32x4 yv, f32x4 gg, f32x4 mu, f32x4 iv, f32x4 sc, f32x4 k1, f32x4 k2, int act, float slope) {
    const f32x4 xh = (yv - mu) * iv;
    f32x4 d = sc * (gg - k1 - xh * k2);
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] *= act_grad_from_output(yv[e], act, slope);
    return d;
}
