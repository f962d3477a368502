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
