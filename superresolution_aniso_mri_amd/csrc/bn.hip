// BatchNorm2d (train + eval) with the following AvgPool2d(2) / nearest Upsample(x2) fused, NHWC, with
// *statistic groups*: one launch normalises several independent sub-batches (e.g. enc(x[2B]) and
// enc(slice_between[B]) of kwatsch/cardiac/trainer_ae.py:18,180), each with its own batch statistics,
// exactly as if the reference had called the network once per sub-batch (running statistics are
// updated group after group, in order).
//
//   stats    : per-channel sum / sum of squares partials (about a pivot, below) -> bn_reduce_pivot -> double [G][2][C] about 0
//              (under data parallel these sums are all-reduced across ranks = SyncBN)
//   finalize : mean, biased var -> invstd, scale = gamma*invstd, shift = beta - mean*scale; running stats
//              with momentum (unbiased var), num_batches_tracked (nn.BatchNorm2d semantics)
//   apply    : out = scale*pool_or_up(y) + shift          (affine commutes with the 2x2 mean)
//   backward : reduce sum(g), sum(g*xhat) -> apply dy = scale*(g - s1/M - xhat*s2/M) * act'(y)
//
// How the sums are taken: about a per-channel pivot K[g][c], the mean of eight pixels of the group in this call's y -- threads accumulate d = v - K,
// sum d and sum d * d in fp32, a workgroup's lanes meet in fp64, the partials are fp32, and the launch that turns them into fp64 totals
// (bn_reduce_pivot_kernel, bn_reduce_finalize_kernel) converts them to sums about 0 there (bn_math.h: bn_unpivot).  Sums about 0 in fp32 lose
// (mean / sigma)^2 roundings in var = E[x^2] - mean^2: a bias-dominated channel (10 +- 0.01) would get a random invstd, a constant one a
// variance.  sums[g][2][C], what SyncBN all-reduces, and everything behind it are as before; tests/test_gpu_bn_conditioning.py.
//
// Replaces nn.BatchNorm2d + nn.AvgPool2d / nn.Upsample of networks/acai_vanilla.py:58-59,90-92.
// The arithmetic from the sums on is in bn_math.h (shared with bn_fused.hip); this file adds the reductions and the streaming loops.
#include "bn_math.h"

enum { BN_MODE_NONE = 0, BN_MODE_POOL = 1, BN_MODE_UP = 2 };

// ---- forward statistics ---------------------------------------------------------------------------------
// partial[g][wg][2][C], about the group's pivot; grid = (nwg, G)
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ y, float* __restrict__ partial, int HW,
                                                       int C, BnGroups gr) {
    extern __shared__ __attribute__((aligned(16))) float red[];   // [PL][2][C]
    const int C4 = C >> 2, PL = 256 / C4;
    const int c4 = threadIdx.x % C4, pl = threadIdx.x / C4;
    const int g = blockIdx.y;
    const size_t p0 = (size_t)gr.nstart[g] * HW, p1 = (size_t)gr.nstart[g + 1] * HW;
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    const f32x4 K = bn_pivot_block(y, p0, p1, C, red);          // sums about the group's pivot (bn_math.h)
    if (pl < PL) {
        for (size_t p = p0 + (size_t)blockIdx.x * PL + pl; p < p1; p += (size_t)gridDim.x * PL) {
            const f32x4 d = *(const f32x4*)(y + p * C + c4 * 4) - K;
            s += d;
            q += d * d;
        }
        *(f32x4*)(red + (pl * 2 + 0) * C + c4 * 4) = s;
        *(f32x4*)(red + (pl * 2 + 1) * C + c4 * 4) = q;
    }
    __syncthreads();
    // the lanes meet in fp64 (up to 128 of them: an fp32 chain would cost sqrt(PL) roundings of the variance), one rounding into the partial
    for (int o = threadIdx.x; o < 2 * C; o += 256) {
        double t = 0.0;
        for (int k = 0; k < PL; ++k) t += (double)red[k * 2 * C + o];
        partial[((size_t)g * gridDim.x + blockIdx.x) * 2 * C + o] = (float)t;
    }
}

// sums[g][2][C] (double) = sum_wg partial[g][wg][2][C]
// block = 64 columns x 4 row-lanes: coalesced across columns, fixed summation order (bitwise reproducible)
__global__ __launch_bounds__(1024) void bn_reduce_kernel(const float* __restrict__ partial, double* __restrict__ sums, int nwg,
                                                         int C, int G) {
    __shared__ double red[16][64];
    const int col = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int o = blockIdx.x * 64 + col;
    const int n = G * 2 * C;
    double s = 0.0;
    if (o < n) {
        const int g = o / (2 * C), r = o - g * 2 * C;
        const float* base = partial + (size_t)g * nwg * 2 * C + r;
        const size_t rs = (size_t)2 * C;
        // 8 independent loads in flight per thread (one load per trip = a round of memory latency per row: 10 us for 512 rows)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int k = rl;
        for (; k + 7 * 16 < nwg; k += 8 * 16) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = base[(size_t)(k + u * 16) * rs];
            s0 += (double)v[0] + (double)v[4];
            s1 += (double)v[1] + (double)v[5];
            s2 += (double)v[2] + (double)v[6];
            s3 += (double)v[3] + (double)v[7];
        }
        for (; k < nwg; k += 16) s0 += (double)base[(size_t)k * rs];
        s = (s0 + s1) + (s2 + s3);
    }
    red[rl][col] = s;
    __syncthreads();
    if (rl == 0 && o < n) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][col];
        sums[o] = t;
    }
}

// The same for the forward statistics, whose partials are sums about the groups' pivots in y: a thread owns both columns of a (group,
// channel) and stores the sums about 0 (bn_math.h: bn_unpivot) -- what the all-reduce of SyncBN adds across ranks.  block = 64 x 16 as above.
__global__ __launch_bounds__(1024) void bn_reduce_pivot_kernel(const float* __restrict__ partial, double* __restrict__ sums, int nwg, int C,
                                                               const float* __restrict__ y, int HW, BnGroups gr) {
    __shared__ double red[2][16][64];
    const int col = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int o = blockIdx.x * 64 + col;
    const int n = gr.G * C;
    const int g = o < n ? o / C : 0, c = o - g * C;
    double s = 0.0, q = 0.0;
    if (o < n) {
        const float* base = partial + (size_t)g * nwg * 2 * C + c;
        const size_t rs = (size_t)2 * C;
        double s0 = 0.0, s1 = 0.0, q0 = 0.0, q1 = 0.0;
        int k = rl;
        for (; k + 3 * 16 < nwg; k += 4 * 16) {             // 8 independent loads in flight per thread
            float v[4], w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = base[(size_t)(k + u * 16) * rs];
                w[u] = base[(size_t)(k + u * 16) * rs + C];
            }
            s0 += (double)v[0] + (double)v[2];
            s1 += (double)v[1] + (double)v[3];
            q0 += (double)w[0] + (double)w[2];
            q1 += (double)w[1] + (double)w[3];
        }
        for (; k < nwg; k += 16) {
            s0 += (double)base[(size_t)k * rs];
            q0 += (double)base[(size_t)k * rs + C];
        }
        s = s0 + s1;
        q = q0 + q1;
    }
    red[0][rl][col] = s;
    red[1][rl][col] = q;
    __syncthreads();
    if (rl == 0 && o < n) {
        double ts = 0.0, tq = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            ts += red[0][k][col];
            tq += red[1][k][col];
        }
        const size_t p0 = (size_t)gr.nstart[g] * HW, p1 = (size_t)gr.nstart[g + 1] * HW;
        bn_unpivot(ts, tq, (double)(p1 - p0), bn_pivot1(y, p0, p1, C, c), &sums[(g * 2 + 0) * C + c], &sums[(g * 2 + 1) * C + c]);
    }
}

// train: stats from sums/counts (+ running update, group after group); eval: stats from the running buffers
struct BnFinArgs {
    const float* gamma; const float* beta; float* running_mean; float* running_var; long long* nbt;
    float* mean; float* invstd; float* scale; float* shift;
    int C, G;
    float momentum, eps;
    int train, update_running;
    BnCounts counts;
};

// one channel, one group: (sum, sum of squares) -> mean / invstd / scale / shift (+ running statistics)
__device__ __forceinline__ void bn_finalize_one(const BnFinArgs& f, int c, int g, double s0, double s1) {
    float m, iv;
    if (f.train) {
        const double var = bn_moments(s0, s1, f.counts.c[g], f.eps, &m, &iv);
        if (f.update_running)      // through memory: the next group's step reads what this one wrote
            bn_running_step(f.momentum, m, bn_unbiased(var, f.counts.c[g]), &f.running_mean[c], &f.running_var[c]);
    } else {
        m = f.running_mean[c];
        iv = 1.f / sqrtf(f.running_var[c] + f.eps);
    }
    f.mean[g * f.C + c] = m;
    f.invstd[g * f.C + c] = iv;
    const float sc = bn_scale(f.gamma[c], iv);
    f.scale[g * f.C + c] = sc;
    f.shift[g * f.C + c] = bn_shift(f.beta[c], m, sc);
}

__global__ void bn_finalize_kernel(const double* __restrict__ sums, BnFinArgs f) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && f.train && f.update_running && f.nbt) *f.nbt += f.G;
    if (c >= f.C) return;
    for (int g = 0; g < f.G; ++g)
        bn_finalize_one(f, c, g, f.train ? sums[(g * 2 + 0) * f.C + c] : 0.0, f.train ? sums[(g * 2 + 1) * f.C + c] : 0.0);
}

// block layout of the finalize kernels: 16 channels x 64 row-lanes
#define BNR_COLS 16
#define BNR_RL 64

// All 2*G column totals of a block's 16 channels with ONE wait on global memory: the 64 row-lanes of the block are split over the
// 2*G quantities (q = 2*g + {0: first sum, 1: second sum}), each thread strides its quantity's nwg partial rows, the partial
// sums meet in LDS and 2*G*16 threads add them up in a fixed order.  (One total at a time = four dependent rounds of global
// latency + 32 barriers: 10 us for a few KB.)  tot[q][col] is valid for every thread after the call.  G <= 4.
__device__ __forceinline__ void bn_all_totals(const float* __restrict__ partial, int nwg, int C, int G, int c, bool live,
                                              double (*red)[BNR_COLS], double (*tot)[BNR_COLS], int col, int slot) {
    const int NQ = 2 * G, RLQ = BNR_RL / NQ;
    const int q = slot % NQ, rl = slot / NQ;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (live && rl < RLQ) {
        const float* base = partial + ((size_t)(q >> 1) * nwg * 2 + (q & 1)) * C + c;      // partial[g][k][s][c], row stride 2*C
        const size_t rs = (size_t)2 * C;
        int k = rl;
        for (; k + 7 * RLQ < nwg; k += 8 * RLQ) {          // 8 independent loads in flight per thread
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = base[(k + u * RLQ) * rs];
            s0 += (double)v[0] + (double)v[4];
            s1 += (double)v[1] + (double)v[5];
            s2 += (double)v[2] + (double)v[6];
            s3 += (double)v[3] + (double)v[7];
        }
        for (; k < nwg; k += RLQ) s0 += (double)base[k * rs];
    }
    red[slot][col] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (slot < NQ) {
        double t = 0.0;
        for (int r = 0; r < RLQ; ++r) t += red[r * NQ + slot][col];
        tot[slot][col] = t;
    }
    __syncthreads();
}

// Statistics partials -> finalize in ONE launch (no SyncBN exchange in between).  block = 16 channels x 64 row-lanes.
// The partials are sums about the groups' pivots in y (HW pixels per image, groups gr): back to sums about 0 in fp64 (bn_math.h: bn_unpivot).
__global__ __launch_bounds__(1024) void bn_reduce_finalize_kernel(const float* __restrict__ partial, int nwg, const float* __restrict__ y,
                                                                  int HW, BnGroups gr, BnFinArgs f) {
    __shared__ double red[BNR_RL][BNR_COLS];
    __shared__ double tot[8][BNR_COLS];
    const int col = threadIdx.x % BNR_COLS, rl = threadIdx.x / BNR_COLS;
    const int c = blockIdx.x * BNR_COLS + col;
    const bool live = c < f.C;
    if (c == 0 && rl == 0 && f.update_running && f.nbt) *f.nbt += f.G;
    bn_all_totals(partial, nwg, f.C, f.G, c, live, red, tot, col, rl);
    if (rl == 0 && live)
        for (int g = 0; g < f.G; ++g) {                                                                     // group order: running stats
            const size_t p0 = (size_t)gr.nstart[g] * HW, p1 = (size_t)gr.nstart[g + 1] * HW;
            double s0, s1;
            bn_unpivot(tot[2 * g][col], tot[2 * g + 1][col], (double)(p1 - p0), bn_pivot1(y, p0, p1, f.C, c), &s0, &s1);
            bn_finalize_one(f, c, g, s0, s1);
        }
}

// ---- forward apply (+pool / +upsample) ----------------------------------------------------------------

// out = scale * pool_or_up(y) + shift over the whole output, grid-stride; sc_tab / sh_tab [g][C]: the finalize launch's tables in global
// memory or the block's own in LDS
__device__ __forceinline__ void bn_apply_loop(const BnApplyArgs& a, const float* sc_tab, const float* sh_tab) {
    const int C4 = a.C >> 2;
    const size_t total = (size_t)a.N * a.Ho * a.Wo * C4;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int c4 = idx % C4;
        size_t pix = idx / C4;
        const int x = pix % a.Wo;
        pix /= a.Wo;
        const int yy = pix % a.Ho;
        const int n = pix / a.Ho;
        const int g = bn_group_of(a.gr.G, a.gr.nstart, n);
        const f32x4 sc = *(const f32x4*)(sc_tab + g * a.C + c4 * 4);
        const f32x4 sh = *(const f32x4*)(sh_tab + g * a.C + c4 * 4);
        f32x4 v;
        if (a.mode == BN_MODE_POOL) {
            const float* b = a.y + (((size_t)n * a.H + 2 * yy) * a.W + 2 * x) * a.C + c4 * 4;
            v = bn_pool2x2(*(const f32x4*)b, *(const f32x4*)(b + a.C), *(const f32x4*)(b + (size_t)a.W * a.C),
                           *(const f32x4*)(b + (size_t)a.W * a.C + a.C));
        } else if (a.mode == BN_MODE_UP) {
            v = *(const f32x4*)(a.y + (((size_t)n * a.H + (yy >> 1)) * a.W + (x >> 1)) * a.C + c4 * 4);
        } else {
            v = *(const f32x4*)(a.y + (((size_t)n * a.H + yy) * a.W + x) * a.C + c4 * 4);
        }
        *(f32x4*)(a.out + idx * 4) = bn_fwd_elem(v, sc, sh);
    }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(BnApplyArgs a) { bn_apply_loop(a, a.scale, a.shift); }

// Data parallel (SyncBN): finalize + apply in ONE launch.  The all-reduced sums are [G][2][C] doubles -- a few hundred values -- so every
// block derives scale / shift for all groups and channels itself (bn_math.h: bn_fwd_tables) and block 0 alone writes mean / invstd /
// scale / shift for the backward pass and updates the running statistics, group after group.
constexpr int BN_FUSE_MAX = 1024;       // G * C values a block keeps in LDS

__global__ __launch_bounds__(256) void bn_finalize_apply_kernel(const double* __restrict__ sums, BnFinArgs f, BnApplyArgs a) {
    __shared__ __attribute__((aligned(16))) float s_sc[BN_FUSE_MAX], s_sh[BN_FUSE_MAX];
    bn_fwd_tables<256>(sums, f, blockIdx.x == 0, s_sc, s_sh);
    __syncthreads();
    bn_apply_loop(a, s_sc, s_sh);
}

// ---- backward --------------------------------------------------------------------------------------------

// MODE >= 0: compile-time mode with branch-free loads (a divergent bounds branch in front of the load kept the compiler from
// batching the loads of the unrolled pixels); MODE < 0 keeps the run-time form
template <int MODE>
__device__ __forceinline__ f32x4 bn_gather_g_t(const BnBwdArgs& a, int n, int yy, int x, int c4) {
    // gradient w.r.t. the BN output at full-resolution BN pixel (yy, x)
    const int mode = MODE < 0 ? a.mode : MODE;
    if (mode == BN_MODE_POOL) {
        const int py = yy >> 1, px = x >> 1;
        if (MODE < 0) {
            if (py >= a.Ho || px >= a.Wo) return (f32x4){0.f, 0.f, 0.f, 0.f};
            return *(const f32x4*)(a.gout + (((size_t)n * a.Ho + py) * a.Wo + px) * a.C + c4 * 4) * 0.25f;
        }
        const float w = (py < a.Ho && px < a.Wo) ? 0.25f : 0.f;          // odd H / W: the last row / column is not pooled
        return *(const f32x4*)(a.gout + (((size_t)n * a.Ho + min(py, a.Ho - 1)) * a.Wo + min(px, a.Wo - 1)) * a.C + c4 * 4) * w;
    } else if (mode == BN_MODE_UP) {
        const float* b = a.gout + (((size_t)n * a.Ho + 2 * yy) * a.Wo + 2 * x) * a.C + c4 * 4;
        return (*(const f32x4*)b + *(const f32x4*)(b + a.C)) +
               (*(const f32x4*)(b + (size_t)a.Wo * a.C) + *(const f32x4*)(b + (size_t)a.Wo * a.C + a.C));
    }
    return *(const f32x4*)(a.gout + (((size_t)n * a.H + yy) * a.W + x) * a.C + c4 * 4);
}

// exact floor(p / d) for p < 2^31 with the host's (m, k) = (ceil(2^k / d), 31 + ceil(log2 d)): one 64-bit multiply and a shift
__device__ __forceinline__ unsigned bn_fastdiv(unsigned p, unsigned long long m, int k) {
    return (unsigned)(((unsigned long long)p * m) >> k);
}

// grid = (nwg, G)
template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(BnBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int C4 = a.C >> 2, PL = 256 / C4;
    const int c4 = threadIdx.x % C4, pl = threadIdx.x / C4;
    const int g = blockIdx.y;
    const unsigned HW = a.H * a.W;
    const unsigned p0 = a.gr.nstart[g] * HW, p1 = a.gr.nstart[g + 1] * HW;       // host checks N*H*W < 2^31
    const f32x4 mu = *(const f32x4*)(a.mean + g * a.C + c4 * 4);
    const f32x4 iv = *(const f32x4*)(a.invstd + g * a.C + c4 * 4);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (pl < PL) {
        // BNR_U pixels per trip: their loads (y and the 1..4 gathered gradient pieces each) are independent, which multiplies the
        // bytes in flight per thread -- one pixel per trip left the kernel latency-bound (2.2-3.6 TB/s with 8 waves per CU)
        constexpr int U = 2;
        const unsigned S = gridDim.x * PL;
        unsigned p = p0 + blockIdx.x * PL + pl;
        f32x4 a1[U], a2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) a1[u] = a2[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (; p + (U - 1) * S < p1; p += U * S) {
            f32x4 v[U], gq[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned q = p + u * S;
                const unsigned n = bn_fastdiv(q, a.m_hw, a.k_hw);          // q / HW, q % HW, rem / W without ~40-instruction
                const unsigned rem = q - n * HW;                            // divisions (C/4 threads repeat them per pixel)
                const unsigned yy = bn_fastdiv(rem, a.m_w, a.k_w);
                v[u] = *(const f32x4*)(a.y + (size_t)q * a.C + c4 * 4);
                gq[u] = bn_gather_g_t<MODE>(a, n, yy, rem - yy * a.W, c4);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a1[u] += gq[u];
                a2[u] += gq[u] * ((v[u] - mu) * iv);
            }
        }
        for (; p < p1; p += S) {
            const unsigned n = bn_fastdiv(p, a.m_hw, a.k_hw);
            const unsigned rem = p - n * HW;
            const unsigned yy = bn_fastdiv(rem, a.m_w, a.k_w), x = rem - yy * a.W;
            const f32x4 gg = bn_gather_g_t<MODE>(a, n, yy, x, c4);
            const f32x4 xh = (*(const f32x4*)(a.y + (size_t)p * a.C + c4 * 4) - mu) * iv;
            s1 += gg;
            s2 += gg * xh;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s1 += a1[u];
            s2 += a2[u];
        }
        *(f32x4*)(red + (pl * 2 + 0) * a.C + c4 * 4) = s1;
        *(f32x4*)(red + (pl * 2 + 1) * a.C + c4 * 4) = s2;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * a.C; o += 256) {
        float t = 0.f;
        for (int k = 0; k < PL; ++k) t += red[k * 2 * a.C + o];
        a.partial[((size_t)g * gridDim.x + blockIdx.x) * 2 * a.C + o] = t;
    }
}

// coef[g][2][C] = sums/M ; dgamma[c] = sum_g s2 ; dbeta[c] = sum_g s1
__global__ void bn_bwd_finalize_kernel(const double* __restrict__ sums, BnCounts counts,
                                       float* __restrict__ coef, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                       int C, int G) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_bwd_channel<true>(sums, C, c, counts.c, G, C, c, coef, dgamma, dbeta);
}

// backward-reduce partials -> coef / dgamma / dbeta in ONE launch (same math as bn_reduce + bn_bwd_finalize)
__global__ __launch_bounds__(1024) void bn_bwd_reduce_finalize_kernel(const float* __restrict__ partial, int nwg, BnCounts counts,
                                                                      float* __restrict__ coef, float* __restrict__ dgamma,
                                                                      float* __restrict__ dbeta, int C, int G) {
    __shared__ double red[BNR_RL][BNR_COLS];
    const int col = threadIdx.x % BNR_COLS, rl = threadIdx.x / BNR_COLS;
    const int c = blockIdx.x * BNR_COLS + col;
    const bool live = c < C;
    __shared__ double tot[8][BNR_COLS];
    bn_all_totals(partial, nwg, C, G, c, live, red, tot, col, rl);
    if (rl == 0 && live) bn_bwd_channel<true>(&tot[0][0], BNR_COLS, col, counts.c, G, C, c, coef, dgamma, dbeta);
}

// dpre = scale * (g - k1 - xhat * k2) * act'(y) over the whole layer, grid-stride; k_tab [g][2][C]: coef in global memory or the block's
// own table in LDS
template <int MODE>
__device__ __forceinline__ void bn_bwd_apply_loop(const BnBwdArgs& a, const float* k_tab) {
    const int C4 = a.C >> 2;
    const size_t total = (size_t)a.N * a.H * a.W * C4;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int c4 = idx % C4;
        size_t pix = idx / C4;
        const int x = pix % a.W;
        pix /= a.W;
        const int yy = pix % a.H;
        const int n = pix / a.H;
        const int g = bn_group_of(a.gr.G, a.gr.nstart, n);
        const f32x4 mu = *(const f32x4*)(a.mean + g * a.C + c4 * 4);
        const f32x4 iv = *(const f32x4*)(a.invstd + g * a.C + c4 * 4);
        const f32x4 sc = *(const f32x4*)(a.scale + g * a.C + c4 * 4);
        const f32x4 k1 = *(const f32x4*)(k_tab + (g * 2 + 0) * a.C + c4 * 4);
        const f32x4 k2 = *(const f32x4*)(k_tab + (g * 2 + 1) * a.C + c4 * 4);
        const f32x4 yv = *(const f32x4*)(a.y + idx * 4);
        const f32x4 gg = bn_gather_g_t<MODE>(a, n, yy, x, c4);
        *(f32x4*)(a.dpre + idx * 4) = bn_bwd_elem(yv, gg, mu, iv, sc, k1, k2, a.act, a.slope);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnBwdArgs a) { bn_bwd_apply_loop<MODE>(a, a.coef); }

// the same for the backward pass: coef = sums / M per block in LDS, block 0 writes coef / dgamma / dbeta (bn_math.h: bn_bwd_tables)
template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_finalize_apply_kernel(const double* __restrict__ sums, BnCounts counts, float* __restrict__ coef,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta, int G, BnBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float s_k[2 * BN_FUSE_MAX];       // [g][2][C]
    bn_bwd_tables<256>(sums, counts.c, G, a.C, blockIdx.x == 0, s_k, coef, dgamma, dbeta);
    __syncthreads();
    bn_bwd_apply_loop<MODE>(a, s_k);
}

// ---- BatchNorm + AvgPool2d(2), pool once (include/aesr_hip_bnpool.h) ------------------------------------------------
// The fourth launch form, for the three-launch route in POOL mode.  The statistics pass has every 2x2 window in registers anyway: it also
// writes the window's mean m [N][Ho][Wo][C], and the two other streaming passes that needed y only through that mean read m instead:
//   forward   bn_stats_kernel_pool -> bn_reduce_finalize_kernel -> bn_apply_kernel_pooled          out = scale * m + shift
//   backward  bn_bwd_reduce_kernel_pooled -> bn_bwd_reduce_finalize_kernel -> bn_bwd_apply_kernel<BN_MODE_POOL>
// Every pixel of a window carries the gradient g_pool / 4 and the pixels the pooling leaves out (odd H / W) carry none, so
//   sum g = sum_windows g_pool        sum g * xhat = sum_windows g_pool * ((m - mean) * invstd).
// m, and out / dpre for given tables, are bit for bit the three-launch route's (the same expressions of bn_math.h); the per-channel sums are
// taken over windows instead of pixels, which moves them by summation order only.

// partial[g][wg][2][C] as bn_stats_kernel; grid = (nwg, G).  A thread owns (channel quad, 2x2 window): four independent 16-byte loads per trip.
// ODD: H or W is odd, the pooling leaves a row / column out (even sizes compile without that loop).
template <bool ODD>
__global__ __launch_bounds__(256) void bn_stats_kernel_pool(BnPoolStatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float red[];   // [PL][2][C]
    const int C = a.C, C4 = C >> 2, PL = 256 / C4;
    const int c4 = threadIdx.x % C4, pl = threadIdx.x / C4;
    const int g = blockIdx.y;
    const unsigned HoWo = a.Ho * a.Wo;                            // host checks N*H*W < 2^31
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    const size_t HW = (size_t)a.H * a.W;
    const f32x4 K = bn_pivot_block(a.y, a.gr.nstart[g] * HW, a.gr.nstart[g + 1] * HW, C, red);      // sums about the group's pivot
    if (pl < PL) {
        const unsigned S = gridDim.x * PL;
        const size_t row = (size_t)a.W * C;
        const unsigned w1 = a.gr.nstart[g + 1] * HoWo;
        for (unsigned w = a.gr.nstart[g] * HoWo + blockIdx.x * PL + pl; w < w1; w += S) {
            const unsigned n = bn_fastdiv(w, a.m_win, a.k_win);
            const unsigned rem = w - n * HoWo;
            const unsigned py = bn_fastdiv(rem, a.m_wo, a.k_wo), px = rem - py * a.Wo;
            const float* b = a.y + (((size_t)n * a.H + 2 * py) * a.W + 2 * px) * C + c4 * 4;
            const f32x4 v00 = *(const f32x4*)b, v01 = *(const f32x4*)(b + C);
            const f32x4 v10 = *(const f32x4*)(b + row), v11 = *(const f32x4*)(b + row + C);
            const f32x4 d00 = v00 - K, d01 = v01 - K, d10 = v10 - K, d11 = v11 - K;
            s += (d00 + d01) + (d10 + d11);
            q += (d00 * d00 + d01 * d01) + (d10 * d10 + d11 * d11);
            *(f32x4*)(a.m + (size_t)w * C + c4 * 4) = bn_pool2x2(v00, v01, v10, v11);
        }
        // what the pooling leaves out still counts for the statistics: the last column (odd W: H pixels per image), then the rest of the
        // last row (odd H: 2 * Wo pixels)
        const unsigned Tc = (a.W & 1) ? a.H : 0, T = Tc + ((a.H & 1) ? 2 * a.Wo : 0);
        if (ODD && T) {
            const unsigned t1 = a.gr.nstart[g + 1] * T;
            for (unsigned t = a.gr.nstart[g] * T + blockIdx.x * PL + pl; t < t1; t += S) {
                const unsigned n = t / T, r = t - n * T;
                const unsigned yy = r < Tc ? r : a.H - 1, x = r < Tc ? a.W - 1 : r - Tc;
                const f32x4 d = *(const f32x4*)(a.y + (((size_t)n * a.H + yy) * a.W + x) * C + c4 * 4) - K;
                s += d;
                q += d * d;
            }
        }
        *(f32x4*)(red + (pl * 2 + 0) * C + c4 * 4) = s;
        *(f32x4*)(red + (pl * 2 + 1) * C + c4 * 4) = q;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * C; o += 256) {          // in fp64, as bn_stats_kernel
        double t = 0.0;
        for (int k = 0; k < PL; ++k) t += (double)red[k * 2 * C + o];
        a.partial[((size_t)g * gridDim.x + blockIdx.x) * 2 * C + o] = (float)t;
    }
}

// out = scale * m + shift, flat over the pooled tensor; per = vectors per image.  The stride is a multiple of 256 and 256 one of C/4, so a
// thread keeps its channel quad; the group follows from the groups' first vectors (nstart is padded with N behind the last group).
// U independent vectors in flight per thread.
template <int U>
__global__ __launch_bounds__(256) void bn_apply_kernel_pooled(const float* __restrict__ m, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, float* __restrict__ out, size_t per, int C,
                                                              BnGroups gr) {
    const int c4 = threadIdx.x % (C >> 2);
    const size_t total = gr.nstart[gr.G] * per, b1 = gr.nstart[1] * per, b2 = gr.nstart[2] * per, b3 = gr.nstart[3] * per;
    const size_t S = (size_t)gridDim.x * 256;
    size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; idx + (U - 1) * S < total; idx += U * S) {
        f32x4 v[U], sc[U], sh[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = idx + u * S;
            const int g = (int)(i >= b1) + (int)(i >= b2) + (int)(i >= b3);
            v[u] = *(const f32x4*)(m + i * 4);
            sc[u] = *(const f32x4*)(scale + g * C + c4 * 4);
            sh[u] = *(const f32x4*)(shift + g * C + c4 * 4);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) *(f32x4*)(out + (idx + u * S) * 4) = bn_fwd_elem(v[u], sc[u], sh[u]);
    }
    for (; idx < total; idx += S) {
        const int g = (int)(idx >= b1) + (int)(idx >= b2) + (int)(idx >= b3);
        const f32x4 sc = *(const f32x4*)(scale + g * C + c4 * 4);
        const f32x4 sh = *(const f32x4*)(shift + g * C + c4 * 4);
        *(f32x4*)(out + idx * 4) = bn_fwd_elem(*(const f32x4*)(m + idx * 4), sc, sh);
    }
}

// partial[g][wg][2][C] as bn_bwd_reduce_kernel; grid = (nwg, G).  Both operands are read flat, U windows in flight per thread.
template <int U>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel_pooled(const float* __restrict__ gout, const float* __restrict__ m,
                                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                   float* __restrict__ partial, unsigned HoWo, int C, BnGroups gr) {
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int C4 = C >> 2, PL = 256 / C4;
    const int c4 = threadIdx.x % C4, pl = threadIdx.x / C4;
    const int g = blockIdx.y;
    const unsigned w1 = gr.nstart[g + 1] * HoWo;
    const f32x4 mu = *(const f32x4*)(mean + g * C + c4 * 4);
    const f32x4 iv = *(const f32x4*)(invstd + g * C + c4 * 4);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (pl < PL) {
        const unsigned S = gridDim.x * PL;
        unsigned w = gr.nstart[g] * HoWo + blockIdx.x * PL + pl;
        f32x4 a1[U], a2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) a1[u] = a2[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (; w + (U - 1) * S < w1; w += U * S) {
            f32x4 mv[U], gq[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t o = (size_t)(w + u * S) * C + c4 * 4;
                gq[u] = *(const f32x4*)(gout + o);
                mv[u] = *(const f32x4*)(m + o);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a1[u] += gq[u];
                a2[u] += gq[u] * ((mv[u] - mu) * iv);
            }
        }
        for (; w < w1; w += S) {
            const size_t o = (size_t)w * C + c4 * 4;
            const f32x4 gg = *(const f32x4*)(gout + o);
            s1 += gg;
            s2 += gg * ((*(const f32x4*)(m + o) - mu) * iv);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s1 += a1[u];
            s2 += a2[u];
        }
        *(f32x4*)(red + (pl * 2 + 0) * C + c4 * 4) = s1;
        *(f32x4*)(red + (pl * 2 + 1) * C + c4 * 4) = s2;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * C; o += 256) {
        float t = 0.f;
        for (int k = 0; k < PL; ++k) t += red[k * 2 * C + o];
        partial[((size_t)g * gridDim.x + blockIdx.x) * 2 * C + o] = t;
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------
static int bn_check_c(int C, const char* who) {
    if (C % 4 != 0 || 256 % (C / 4) != 0 || C > 1024) {
        aesr_set_error("%s: unsupported channel count %d (need C/4 | 256)", who, C);
        return AESR_ERR_ARG;
    }
    return AESR_OK;
}

// blocks of a streaming (grid-stride) kernel over `pixels` pixels of C channels, four channels per thread
static dim3 bn_stream_grid(size_t pixels, int C) {
    const size_t total = pixels * (C / 4);
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    return dim3(grid);
}

// the three compile-time modes of a backward kernel template
#define BN_LAUNCH_MODE(kernel, mode, grid, shm, st, ...)                                                       \
    do {                                                                                                       \
        if ((mode) == BN_MODE_POOL) hipLaunchKernelGGL(kernel<BN_MODE_POOL>, grid, dim3(256), shm, st, __VA_ARGS__); \
        else if ((mode) == BN_MODE_UP) hipLaunchKernelGGL(kernel<BN_MODE_UP>, grid, dim3(256), shm, st, __VA_ARGS__);  \
        else hipLaunchKernelGGL(kernel<0>, grid, dim3(256), shm, st, __VA_ARGS__);                             \
    } while (0)

int aesr_launch_bn_stats(const float* y, float* partial, int HW, int C, const BnGroups& gr, int nwg, hipStream_t st) {
    if (int e = bn_check_c(C, "bn_stats")) return e;
    const int PL = 256 / (C / 4);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(nwg, gr.G), dim3(256), (size_t)PL * 2 * C * sizeof(float), st, y, partial, HW, C, gr);
    AESR_LAUNCH_CHECK("bn_stats");
    return AESR_OK;
}

int aesr_launch_bn_reduce(const float* partial, double* sums, int nwg, int C, int G, hipStream_t st) {
    hipLaunchKernelGGL(bn_reduce_kernel, dim3(ceil_div(G * 2 * C, 64)), dim3(1024), 0, st, partial, sums, nwg, C, G);
    AESR_LAUNCH_CHECK("bn_reduce");
    return AESR_OK;
}

// the partials of aesr_launch_bn_stats over the same y / HW / groups -> sums about 0
int aesr_launch_bn_reduce_pivot(const float* partial, double* sums, int nwg, int C, const float* y, int HW, const BnGroups& gr, hipStream_t st) {
    hipLaunchKernelGGL(bn_reduce_pivot_kernel, dim3(ceil_div(gr.G * C, 64)), dim3(1024), 0, st, partial, sums, nwg, C, y, HW, gr);
    AESR_LAUNCH_CHECK("bn_reduce_pivot");
    return AESR_OK;
}

static BnFinArgs bn_fin_args(const double* counts, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             long long* nbt, float* mean, float* invstd, float* scale, float* shift, int C, int G, float momentum,
                             float eps, int train, int update_running) {
    BnFinArgs f;
    f.gamma = gamma; f.beta = beta; f.running_mean = running_mean; f.running_var = running_var; f.nbt = nbt;
    f.mean = mean; f.invstd = invstd; f.scale = scale; f.shift = shift; f.C = C; f.G = G; f.momentum = momentum; f.eps = eps;
    f.train = train; f.update_running = update_running;
    f.counts = bn_counts(counts, G);
    return f;
}

int aesr_launch_bn_finalize(const double* sums, const double* counts, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, long long* nbt, float* mean, float* invstd,
                            float* scale, float* shift, int C, int G, float momentum, float eps, int train,
                            int update_running, hipStream_t st) {
    const BnFinArgs f = bn_fin_args(counts, gamma, beta, running_mean, running_var, nbt, mean, invstd, scale, shift, C, G, momentum,
                                    eps, train, update_running);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, st, sums, f);
    AESR_LAUNCH_CHECK("bn_finalize");
    return AESR_OK;
}

// y / HW / gr: what the statistics launch that wrote the partials was given (the pivots are read back from y)
int aesr_launch_bn_reduce_finalize(const float* partial, int nwg, const float* y, int HW, const BnGroups& gr, const double* counts,
                                   const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, long long* nbt, float* mean, float* invstd,
                                   float* scale, float* shift, int C, float momentum, float eps, int update_running, hipStream_t st) {
    const BnFinArgs f = bn_fin_args(counts, gamma, beta, running_mean, running_var, nbt, mean, invstd, scale, shift, C, gr.G, momentum,
                                    eps, 1, update_running);
    hipLaunchKernelGGL(bn_reduce_finalize_kernel, dim3(ceil_div(C, BNR_COLS)), dim3(BNR_COLS * BNR_RL), 0, st, partial, nwg, y, HW, gr, f);
    AESR_LAUNCH_CHECK("bn_reduce_finalize");
    return AESR_OK;
}

int aesr_launch_bn_bwd_reduce_finalize(const float* partial, int nwg, const double* counts, float* coef, float* dgamma,
                                       float* dbeta, int C, int G, hipStream_t st) {
    hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel, dim3(ceil_div(C, BNR_COLS)), dim3(BNR_COLS * BNR_RL), 0, st, partial, nwg,
                       bn_counts(counts, G), coef, dgamma, dbeta, C, G);
    AESR_LAUNCH_CHECK("bn_bwd_reduce_finalize");
    return AESR_OK;
}

int aesr_launch_bn_apply(const BnApplyArgs& a, hipStream_t st) {
    if (int e = bn_check_c(a.C, "bn_apply")) return e;
    hipLaunchKernelGGL(bn_apply_kernel, bn_stream_grid((size_t)a.N * a.Ho * a.Wo, a.C), dim3(256), 0, st, a);
    AESR_LAUNCH_CHECK("bn_apply");
    return AESR_OK;
}

static void bn_magic(unsigned d, unsigned long long* m, int* k) {
    int L = 0;
    while ((1u << L) < d) ++L;
    *k = 31 + L;
    const unsigned __int128 one = (unsigned __int128)1 << *k;
    *m = (unsigned long long)((one + d - 1) / d);
}

int aesr_launch_bn_bwd_reduce(const BnBwdArgs& a_in, int nwg, hipStream_t st) {
    BnBwdArgs a = a_in;
    bn_magic((unsigned)(a.H * a.W), &a.m_hw, &a.k_hw);
    bn_magic((unsigned)a.W, &a.m_w, &a.k_w);
    if (int e = bn_check_c(a.C, "bn_bwd_reduce")) return e;
    const int PL = 256 / (a.C / 4);
    BN_LAUNCH_MODE(bn_bwd_reduce_kernel, a.mode, dim3(nwg, a.gr.G), (size_t)PL * 2 * a.C * sizeof(float), st, a);
    AESR_LAUNCH_CHECK("bn_bwd_reduce");
    return AESR_OK;
}

int aesr_launch_bn_bwd_finalize(const double* sums, const double* counts, float* coef, float* dgamma, float* dbeta, int C,
                                int G, hipStream_t st) {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, st, sums, bn_counts(counts, G), coef, dgamma, dbeta, C, G);
    AESR_LAUNCH_CHECK("bn_bwd_finalize");
    return AESR_OK;
}

int aesr_launch_bn_bwd_apply(const BnBwdArgs& a, hipStream_t st) {
    if (int e = bn_check_c(a.C, "bn_bwd_apply")) return e;
    BN_LAUNCH_MODE(bn_bwd_apply_kernel, a.mode, bn_stream_grid((size_t)a.N * a.H * a.W, a.C), 0, st, a);
    AESR_LAUNCH_CHECK("bn_bwd_apply");
    return AESR_OK;
}

// finalize + apply / backward finalize + apply in one launch (data parallel, train mode); false: too many values for the LDS tables
bool aesr_bn_fused_ok(int C, int G) { return G * C <= BN_FUSE_MAX && G >= 1 && G <= 4; }

int aesr_launch_bn_finalize_apply(const double* sums, const double* counts, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, long long* nbt, float* mean, float* invstd, float* scale, float* shift, float momentum,
                                  float eps, int update_running, int G, const BnApplyArgs& a, hipStream_t st) {
    if (int e = bn_check_c(a.C, "bn_finalize_apply")) return e;
    const BnFinArgs f = bn_fin_args(counts, gamma, beta, running_mean, running_var, nbt, mean, invstd, scale, shift, a.C, G, momentum, eps, 1,
                                    update_running);
    hipLaunchKernelGGL(bn_finalize_apply_kernel, bn_stream_grid((size_t)a.N * a.Ho * a.Wo, a.C), dim3(256), 0, st, sums, f, a);
    AESR_LAUNCH_CHECK("bn_finalize_apply");
    return AESR_OK;
}

int aesr_launch_bn_bwd_finalize_apply(const double* sums, const double* counts, float* coef, float* dgamma, float* dbeta, int G,
                                      const BnBwdArgs& a, hipStream_t st) {
    if (int e = bn_check_c(a.C, "bn_bwd_finalize_apply")) return e;
    BN_LAUNCH_MODE(bn_bwd_finalize_apply_kernel, a.mode, bn_stream_grid((size_t)a.N * a.H * a.W, a.C), 0, st, sums, bn_counts(counts, G), coef,
                   dgamma, dbeta, G, a);
    AESR_LAUNCH_CHECK("bn_bwd_finalize_apply");
    return AESR_OK;
}

// BatchNorm + AvgPool2d(2), pool once.  (Last in the file, and the kernels templates: their instantiations follow the older ones, whose
// listings keep their label numbers -- scripts/isa_same.py compares them line by line.)
int aesr_launch_bn_pool_stats(const BnPoolStatsArgs& a_in, int nwg, hipStream_t st) {
    BnPoolStatsArgs a = a_in;
    if (int e = bn_check_c(a.C, "bn_pool_stats")) return e;
    bn_magic((unsigned)(a.Ho * a.Wo), &a.m_win, &a.k_win);
    bn_magic((unsigned)a.Wo, &a.m_wo, &a.k_wo);
    const int PL = 256 / (a.C / 4);
    const size_t shm = (size_t)PL * 2 * a.C * sizeof(float);
    if ((a.H | a.W) & 1) hipLaunchKernelGGL(bn_stats_kernel_pool<true>, dim3(nwg, a.gr.G), dim3(256), shm, st, a);
    else hipLaunchKernelGGL(bn_stats_kernel_pool<false>, dim3(nwg, a.gr.G), dim3(256), shm, st, a);
    AESR_LAUNCH_CHECK("bn_pool_stats");
    return AESR_OK;
}

int aesr_launch_bn_pool_apply(const float* m, const float* scale, const float* shift, float* out, int HoWo, int C, const BnGroups& gr,
                              hipStream_t st) {
    if (int e = bn_check_c(C, "bn_pool_apply")) return e;
    hipLaunchKernelGGL(bn_apply_kernel_pooled<2>, bn_stream_grid((size_t)gr.nstart[gr.G] * HoWo, C), dim3(256), 0, st, m, scale, shift, out,
                       (size_t)HoWo * (C / 4), C, gr);
    AESR_LAUNCH_CHECK("bn_pool_apply");
    return AESR_OK;
}

int aesr_launch_bn_pool_bwd_reduce(const float* gout, const float* m, const float* mean, const float* invstd, float* partial, int HoWo, int C,
                                   const BnGroups& gr, int nwg, hipStream_t st) {
    if (int e = bn_check_c(C, "bn_pool_bwd_reduce")) return e;
    const int PL = 256 / (C / 4);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel_pooled<4>, dim3(nwg, gr.G), dim3(256), (size_t)PL * 2 * C * sizeof(float), st, gout, m, mean, invstd,
                       partial, (unsigned)HoWo, C, gr);
    AESR_LAUNCH_CHECK("bn_pool_bwd_reduce");
    return AESR_OK;
}
