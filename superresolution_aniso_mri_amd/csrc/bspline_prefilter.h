// The recursive cubic B-spline pre-filter of one line (scipy.ndimage.spline_filter1d(order = 3, mode = 'mirror') in double) and the
// whole-sample mirror it stands on: stated once for bspline_prefilter.hip, z_expand.hip and reslice_taps.hip.  Device functions only.
#pragma once
#include <math.h>

#pragma clang fp contract(off)

#define BSP_POLE (sqrt(3.0) - 2.0)
#define BSP_GAIN 6.0

// whole-sample mirror of period 2 n - 2: c b | a b c d | c b, repeated while i is outside; n == 1: always 0
__device__ __forceinline__ int aesr_mirror_index(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// the first anti-causal value from the last two causal ones
__device__ __forceinline__ double bsp_anticausal_start(double prev2, double prev) {
    const double z1 = BSP_POLE;
    return z1 / (z1 * z1 - 1.0) * (z1 * prev2 + prev);
}

// Coefficients c[i * stride] of the n samples x[i * stride]: gain 6, exact mirror initialisation over the whole line with the powers of
// the pole as running products, causal and anti-causal recursion; n == 1 copies.  x may BE c (the in-place passes): x[i] is read for the
// last time before c[i] is first written.  Where they are distinct the caller's own __restrict__ pointers say so.
template <typename S>
__device__ __forceinline__ void bsp_prefilter_line(const S* x, double* c, int n, size_t stride) {
    if (n == 1) {
        c[0] = (double)x[0];
        return;
    }
    const double z1 = BSP_POLE, gain = BSP_GAIN;
    double zn1 = 1.0;
    for (int i = 0; i < n - 1; ++i) zn1 *= z1;          // z1^(n-1) as a running product
    double c0 = (double)x[0] * gain + zn1 * ((double)x[(size_t)(n - 1) * stride] * gain), zi = z1;
    for (int i = 1; i < n - 1; ++i) {
        c0 += zi * ((double)x[(size_t)i * stride] * gain + zn1 * ((double)x[(size_t)(n - 1 - i) * stride] * gain));
        zi *= z1;
    }
    c0 /= 1.0 - zn1 * zn1;
    c[0] = c0;
    double prev = c0, prev2 = c0;
    for (int i = 1; i < n; ++i) {          // causal
        prev2 = prev;
        prev = (double)x[(size_t)i * stride] * gain + z1 * prev;
        c[(size_t)i * stride] = prev;
    }
    double next = bsp_anticausal_start(prev2, prev);
    c[(size_t)(n - 1) * stride] = next;
    for (int i = n - 2; i >= 0; --i) {          // anti-causal
        next = z1 * (next - c[(size_t)i * stride]);
        c[(size_t)i * stride] = next;
    }
}
