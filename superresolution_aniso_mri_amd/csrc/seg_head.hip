// The label head of the multi-channel auto-encoder on the device: softmax over the K class logits of every pixel, the soft-Dice sums and
// loss of kwatsch/dice_loss.py (reference :4-33), the arg-max label map, and the backward of all of it.  include/aesr_hip_seg.h.
//
//   forward    one pass over logits [N][H][W][K]: p = softmax(x) with the row maximum subtracted, arg-max (ties to the lowest class),
//              and per workgroup the fp32 partial sums  I_k = sum onehot_k p_k,  R_k = sum onehot_k,  P_k = sum p_k  of its SEG_PPB pixels;
//              a second, one-workgroup launch adds the partials of each sample in fp64 in block order and forms
//              loss = -(1 / (N K)) sum_{n,k} 2 I / (R + P + 1e-6).
//   backward   one pass: q_k = dL/dp_k = -(g / (N K)) (2 onehot_k / D_k - 2 I_k / D_k^2), D = R + P + 1e-6 (the two per-class factors are
//              computed once per workgroup in fp64), dlogit_k = p_k (q_k - sum_j p_j q_j).
// A pixel is one 16-byte load when K = 4 (two when K = 8) if logits / probs / dlogits are 16-byte aligned; any other K or alignment takes
// 4-byte accesses with the same arithmetic, so values never depend on a pointer's alignment.  No atomics: which pixel a thread takes and
// the order of every sum are fixed by (H, W, K) alone, so two runs give the same bits.
#include "aesr_kernels.h"
#include "aesr_hostcheck.h"
#include "../../include/aesr_hip_seg.h"

#define SEG_THREADS 256
#define SEG_PPT 4                                // pixels per thread: four independent loads in flight
#define SEG_PPB (SEG_THREADS * SEG_PPT)          // pixels per workgroup (<= 2^16 terms per fp32 partial)
#define SEG_EPS 1.0e-6

template <int K, bool VEC>
__device__ __forceinline__ void seg_load(const float* __restrict__ p, float (&x)[K]) {
    if (VEC) {
#pragma unroll
        for (int c = 0; c < K / 4; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * c);
            x[4 * c + 0] = v.x;
            x[4 * c + 1] = v.y;
            x[4 * c + 2] = v.z;
            x[4 * c + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = p[k];
    }
}

template <int K, bool VEC>
__device__ __forceinline__ void seg_store(float* __restrict__ p, const float (&x)[K]) {
    if (VEC) {
#pragma unroll
        for (int c = 0; c < K / 4; ++c)
            *reinterpret_cast<f32x4*>(p + 4 * c) = (f32x4){x[4 * c + 0], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]};
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] = x[k];
    }
}

// workgroup b of sample n takes the pixels [b * SEG_PPB, (b + 1) * SEG_PPB) of that sample; thread t the pixels b * SEG_PPB + j * 256 + t
template <int K, bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                              size_t label_stride, float* __restrict__ probs, int* __restrict__ argmax,
                                                              float* __restrict__ partial, int HW, int nb) {
    __shared__ float red[SEG_THREADS / 64][3 * K];
    const int n = blockIdx.x / nb, b = blockIdx.x - n * nb;
    const size_t img = (size_t)n * HW;
    float sI[K], sR[K], sP[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sI[k] = sR[k] = sP[k] = 0.f;
#pragma unroll
    for (int j = 0; j < SEG_PPT; ++j) {
        const int pix = b * SEG_PPB + j * SEG_THREADS + (int)threadIdx.x;
        if (pix < HW) {
            float x[K];
            seg_load<K, VEC>(logits + (img + pix) * K, x);
            float m = x[0];
#pragma unroll
            for (int k = 1; k < K; ++k) m = fmaxf(m, x[k]);
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                x[k] = expf(x[k] - m);
                s += x[k];
            }
            int best = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) x[k] = x[k] / s;
#pragma unroll
            for (int k = 1; k < K; ++k) best = x[k] > x[best] ? k : best;          // strict: a tie stays with the lower class
            seg_store<K, VEC>(probs + (img + pix) * K, x);
            if (argmax) argmax[img + pix] = best;
            if (labels) {
                const float l = labels[(size_t)n * label_stride + pix];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const bool hit = l == (float)k;             // a label outside [0, K) or not integral belongs to no class
                    sI[k] += hit ? x[k] : 0.f;
                    sR[k] += hit ? 1.f : 0.f;
                    sP[k] += x[k];
                }
            }
        }
    }
    if (!labels) return;          // uniform over the grid: inference, no sums
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float a = wave_sum(sI[k]), r = wave_sum(sR[k]), p = wave_sum(sP[k]);
        if (lane == 0) {
            red[wave][k] = a;
            red[wave][K + k] = r;
            red[wave][2 * K + k] = p;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * K) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < SEG_THREADS / 64; ++w) s += red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * (3 * K) + threadIdx.x] = s;
    }
}

// one workgroup: sums[n][which][k] (which = I, R, P) = the nb partials of sample n added in fp64 in block order; then the loss.  The loads
// of SEG_FIN_CHUNK partials are issued together and added in order afterwards: one memory latency per chunk instead of one per partial.
#define SEG_FIN_THREADS 1024
#define SEG_FIN_CHUNK 16
__global__ __launch_bounds__(SEG_FIN_THREADS) void seg_finish_kernel(const float* __restrict__ partial, double* __restrict__ sums,
                                                                     float* __restrict__ loss, int N, int nb, int K) {
    __shared__ double red[SEG_FIN_THREADS];
    const int row = 3 * K;
    for (int e = threadIdx.x; e < N * row; e += SEG_FIN_THREADS) {
        const int n = e / row, c = e - n * row;
        const float* p = partial + (size_t)n * nb * row + c;
        double s = 0.0;
        for (int b0 = 0; b0 < nb; b0 += SEG_FIN_CHUNK) {
            float v[SEG_FIN_CHUNK];
#pragma unroll
            for (int j = 0; j < SEG_FIN_CHUNK; ++j) v[j] = b0 + j < nb ? p[(size_t)(b0 + j) * row] : 0.f;
#pragma unroll
            for (int j = 0; j < SEG_FIN_CHUNK; ++j) s += (double)v[j];          // + 0.0 past the last block: changes nothing
        }
        sums[e] = s;
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = threadIdx.x; i < N * K; i += SEG_FIN_THREADS) {
        const int n = i / K, k = i - n * K;
        const double* s = sums + (size_t)n * row;
        acc += 2.0 * s[k] / (s[K + k] + s[2 * K + k] + SEG_EPS);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = SEG_FIN_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(-red[0] / ((double)N * (double)K));
}

template <int K, bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ labels,
                                                              size_t label_stride, const double* __restrict__ sums,
                                                              const float* __restrict__ gloss, float* __restrict__ dlogits, int HW, int nb,
                                                              double inv_nk) {
    __shared__ float coef[2][K];          // q_k = coef[0][k] * onehot_k + coef[1][k]
    const int n = blockIdx.x / nb, b = blockIdx.x - n * nb;
    if ((int)threadIdx.x < K) {
        const double* s = sums + (size_t)n * (3 * K);
        const int k = threadIdx.x;
        const double D = s[K + k] + s[2 * K + k] + SEG_EPS, c = (double)*gloss * inv_nk;
        coef[0][k] = (float)(-c * 2.0 / D);
        coef[1][k] = (float)(c * 2.0 * s[k] / (D * D));
    }
    __syncthreads();
    float ca[K], cb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        ca[k] = coef[0][k];
        cb[k] = coef[1][k];
    }
    const size_t img = (size_t)n * HW;
#pragma unroll
    for (int j = 0; j < SEG_PPT; ++j) {
        const int pix = b * SEG_PPB + j * SEG_THREADS + (int)threadIdx.x;
        if (pix < HW) {
            float p[K], q[K];
            seg_load<K, VEC>(probs + (img + pix) * K, p);
            const float l = labels[(size_t)n * label_stride + pix];
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                q[k] = (l == (float)k ? ca[k] : 0.f) + cb[k];
                dot += p[k] * q[k];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) q[k] = p[k] * (q[k] - dot);
            seg_store<K, VEC>(dlogits + (img + pix) * K, q);
        }
    }
}

static inline int seg_blocks_per_sample(int H, int W) { return ceil_div(H * W, SEG_PPB); }

// the checks the launch entry points share; `fn` is the entry point's name in the message
static int seg_check(const char* fn, int N, int H, int W, int K) {
    AESR_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: N, H, W = %d, %d, %d must all be positive", fn, N, H, W);
    AESR_CHECK_ARG(K >= 2 && K <= 8, "%s: K=%d classes, 2 to 8 are supported", fn, K);
    AESR_CHECK_ARG((double)N * H * W * K < 2147483648.0, "%s: N * H * W * K = %d x %d x %d x %d has 2^31 elements or more", fn, N, H, W, K);
    return AESR_OK;
}

#define SEG_DISPATCH(KERNEL, vec, ...)                                                                        \
    switch (K) {                                                                                              \
        case 2: hipLaunchKernelGGL((KERNEL<2, false>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__); break;   \
        case 3: hipLaunchKernelGGL((KERNEL<3, false>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__); break;   \
        case 4:                                                                                               \
            if (vec) hipLaunchKernelGGL((KERNEL<4, true>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__);      \
            else hipLaunchKernelGGL((KERNEL<4, false>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__);         \
            break;                                                                                            \
        case 5: hipLaunchKernelGGL((KERNEL<5, false>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__); break;   \
        case 6: hipLaunchKernelGGL((KERNEL<6, false>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__); break;   \
        case 7: hipLaunchKernelGGL((KERNEL<7, false>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__); break;   \
        default:                                                                                              \
            if (vec) hipLaunchKernelGGL((KERNEL<8, true>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__);      \
            else hipLaunchKernelGGL((KERNEL<8, false>), grid, dim3(SEG_THREADS), 0, st, __VA_ARGS__);         \
            break;                                                                                            \
    }

extern "C" {

size_t aesr_softmax_dice_workspace_floats(int N, int H, int W, int K) {
    if (N <= 0 || H <= 0 || W <= 0 || K < 2 || K > 8 || (double)N * H * W * K >= 2147483648.0) return 0;
    return (size_t)N * seg_blocks_per_sample(H, W) * 3 * K;
}

int aesr_softmax_dice_fwd(const float* logits, const float* labels, size_t label_stride, float* probs, int* argmax, float* partial,
                          double* sums, float* loss, int N, int H, int W, int K, void* stream) {
    const int rc = seg_check("aesr_softmax_dice_fwd", N, H, W, K);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(logits, "aesr_softmax_dice_fwd: logits is a null pointer");
    AESR_CHECK_ARG(probs, "aesr_softmax_dice_fwd: probs is a null pointer");
    AESR_CHECK_ARG((uintptr_t)logits % 4 == 0 && (uintptr_t)probs % 4 == 0 && (uintptr_t)argmax % 4 == 0 && (uintptr_t)labels % 4 == 0 &&
                       (uintptr_t)partial % 4 == 0 && (uintptr_t)loss % 4 == 0,
                   "aesr_softmax_dice_fwd: a device pointer is not 4-byte aligned");
    const int HW = H * W, nb = seg_blocks_per_sample(H, W);
    const size_t bytes = (size_t)4 * N * HW * K;
    if (labels) {
        AESR_CHECK_ARG(partial && sums && loss, "aesr_softmax_dice_fwd: labels are given, so partial, sums and loss must be too");
        AESR_CHECK_ARG((uintptr_t)sums % 8 == 0, "aesr_softmax_dice_fwd: sums is not 8-byte aligned");
        AESR_CHECK_ARG(label_stride >= (size_t)HW || N == 1, "aesr_softmax_dice_fwd: label_stride=%zu is smaller than H * W = %d", label_stride, HW);
        AESR_CHECK_ARG((double)(N - 1) * (double)label_stride + HW < 2147483648.0, "aesr_softmax_dice_fwd: the labels span 2^31 elements or more");
    }
    const size_t lab_bytes = labels ? 4 * ((size_t)(N - 1) * label_stride + HW) : 0;
    if (aesr_overlap(probs, bytes, logits, bytes) || aesr_overlap(probs, bytes, labels, lab_bytes) ||
        aesr_overlap(argmax, (size_t)4 * N * HW, logits, bytes) || aesr_overlap(argmax, (size_t)4 * N * HW, labels, lab_bytes) ||
        aesr_overlap(argmax, (size_t)4 * N * HW, probs, bytes)) {
        aesr_set_error("aesr_softmax_dice_fwd: an output overlaps an input or another output");
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned int)(N * nb));          // <= N * H * W < 2^31
    const bool vec = (uintptr_t)logits % 16 == 0 && (uintptr_t)probs % 16 == 0;
    SEG_DISPATCH(seg_fwd_kernel, vec, logits, labels, label_stride, probs, argmax, partial, HW, nb)
    AESR_LAUNCH_CHECK("softmax_dice_fwd");
    if (labels) {
        hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(SEG_FIN_THREADS), 0, st, (const float*)partial, sums, loss, N, nb, K);
        AESR_LAUNCH_CHECK("softmax_dice_finish");
    }
    return AESR_OK;
}

int aesr_softmax_dice_bwd(const float* probs, const float* labels, size_t label_stride, const double* sums, const float* gloss,
                          float* dlogits, int N, int H, int W, int K, void* stream) {
    const int rc = seg_check("aesr_softmax_dice_bwd", N, H, W, K);
    if (rc != AESR_OK) return rc;
    AESR_CHECK_ARG(probs && labels && sums && gloss && dlogits, "aesr_softmax_dice_bwd: a null pointer");
    AESR_CHECK_ARG((uintptr_t)probs % 4 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)gloss % 4 == 0 && (uintptr_t)dlogits % 4 == 0,
                   "aesr_softmax_dice_bwd: a device pointer is not 4-byte aligned");
    AESR_CHECK_ARG((uintptr_t)sums % 8 == 0, "aesr_softmax_dice_bwd: sums is not 8-byte aligned");
    const int HW = H * W, nb = seg_blocks_per_sample(H, W);
    AESR_CHECK_ARG(label_stride >= (size_t)HW || N == 1, "aesr_softmax_dice_bwd: label_stride=%zu is smaller than H * W = %d", label_stride, HW);
    AESR_CHECK_ARG((double)(N - 1) * (double)label_stride + HW < 2147483648.0, "aesr_softmax_dice_bwd: the labels span 2^31 elements or more");
    const size_t bytes = (size_t)4 * N * HW * K;
    if (aesr_overlap(dlogits, bytes, probs, bytes) || aesr_overlap(dlogits, bytes, labels, 4 * ((size_t)(N - 1) * label_stride + HW)) ||
        aesr_overlap(dlogits, bytes, sums, (size_t)8 * N * 3 * K) || aesr_overlap(dlogits, bytes, gloss, 4)) {
        aesr_set_error("aesr_softmax_dice_bwd: dlogits overlaps an input");
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned int)(N * nb));
    const bool vec = (uintptr_t)probs % 16 == 0 && (uintptr_t)dlogits % 16 == 0;
    const double inv_nk = 1.0 / ((double)N * (double)K);
    SEG_DISPATCH(seg_bwd_kernel, vec, probs, labels, label_stride, sums, gloss, dlogits, HW, nb, inv_nk)
    AESR_LAUNCH_CHECK("softmax_dice_bwd");
    return AESR_OK;
}

}  // extern "C"
