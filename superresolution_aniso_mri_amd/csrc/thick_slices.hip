// Thick-slice simulation of an isotropic brain volume [Z][H][W] (the reference's datasets/common_brains.py:37-44 simulate_thick_slices:
// scipy.ndimage.gaussian_filter1d along z of every (y, x) column, sigma = thickness / 2.355), optionally keeping only every z_step-th
// slice (what the loaders' [::downsample_steps] keeps): out[o] = blur(in)[o * z_step].  include/aesr_hip_dataprep.h.
//   - the (y, x) columns are independent, so a slice is a flat row of H * W pixels; lanes run along it: 16 bytes per lane (VEC) when
//     W % 4 == 0 and both pointers are 16-byte aligned, 4 bytes per lane otherwise;
//   - a workgroup (256 threads) owns a strip of 256 pixels and a run of OB output slices.  It stages the (OB - 1) z_step + 2 r + 1 input
//     slices that run needs in LDS (a slice of the strip is 1 KiB: at most TS_WINDOW = 48 slices, 48 KiB), the reflect boundary
//     (d c b a | a b c d, repeated while the index is outside) resolved while staging; with z_step > 2 r + 1 the slices no tap reaches
//     are skipped.  Every input element then comes from HBM / L2 once per workgroup, not once per tap;
//   - each output is the centre tap plus the pairs (in[z - l] + in[z + l]) * w[l] from the outermost inwards, accumulated in double
//     without contraction and rounded to fp32 once: scipy's order for fp32 input, so the result can equal scipy's bit for bit.
// The weights travel by value in the kernel arguments (33 doubles): no workspace, no copy, no synchronisation, no atomics, no scratch.
#include <math.h>

#include "../../include/aesr_hip_dataprep.h"
#include "aesr_kernels.h"

#pragma clang fp contract(off)

#define TS_MAXR 16
#define TS_THREADS 256
#define TS_WINDOW 48         // input slices staged per workgroup

struct TsWeights { double w[2 * TS_MAXR + 1]; };          // w[0 .. 2 r] as scipy lays them out; w[r] is the centre

// index i of the reflect-extended line of n samples: the extension is symmetric about -1/2 and has period 2 n (unsigned: n < 2^31)
__device__ __forceinline__ int ts_reflect(int i, int n) {
    if (i < 0) i = -1 - i;
    const unsigned int p = 2u * (unsigned int)n, m = (unsigned int)i % p;
    return (int)(m < (unsigned int)n ? m : p - 1u - m);
}

// T = f32x4 (SU = 64 units of 16 bytes per staged slice) or float (SU = 256 units of 4 bytes).  units: units per slice (H * W / 4 or
// H * W).  grid.x: strips, grid.y: runs of OB output slices.
template <typename T, int SU>
__global__ __launch_bounds__(TS_THREADS) void thick_slices_kernel(const T* __restrict__ in, T* __restrict__ out, TsWeights wt, int Z, int Zo,
                                                                  unsigned int units, int step, int r, int OB) {
    __shared__ T win[TS_WINDOW * SU];
    constexpr int NV = sizeof(T) / sizeof(float);
    const unsigned int u0 = blockIdx.x * SU;
    const int o0 = blockIdx.y * OB, nob = min(OB, Zo - o0);
    const int n_in = (nob - 1) * step + 2 * r + 1;          // <= TS_WINDOW: the launcher chose OB for it
    const int zlo = o0 * step - r;
    const bool sparse = step > 2 * r + 1;
    for (int idx = threadIdx.x; idx < n_in * SU; idx += TS_THREADS) {
        const int s = idx / SU;
        const unsigned int u = u0 + (idx & (SU - 1));
        if (u >= units || (sparse && s % step > 2 * r)) continue;
        win[idx] = in[(size_t)ts_reflect(zlo + s, Z) * units + u];
    }
    __syncthreads();
    const double wc = wt.w[r];
    for (int idx = threadIdx.x; idx < nob * SU; idx += TS_THREADS) {
        const int j = idx / SU, ul = idx & (SU - 1);
        const unsigned int u = u0 + ul;
        if (u >= units) continue;
        const float* __restrict__ c = (const float*)(win + (j * step + r) * SU + ul);
        double acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = (double)c[v] * wc;
        for (int l = r; l >= 1; --l) {
            const double w = wt.w[r - l];
            const float* __restrict__ a = c - l * (SU * NV);
            const float* __restrict__ b = c + l * (SU * NV);
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] += ((double)a[v] + (double)b[v]) * w;
        }
        T res;
#pragma unroll
        for (int v = 0; v < NV; ++v) ((float*)&res)[v] = (float)acc[v];
        out[(size_t)(o0 + j) * units + u] = res;
    }
}

extern "C" {

int aesr_thick_slices_out_slices(int Z, int z_step) { return Z > 0 && z_step >= 1 ? Z / z_step + (Z % z_step != 0) : 0; }

int aesr_thick_slices_store_bytes(int W, const float* in, const float* out) {
    return W > 0 && W % 4 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0 ? 16 : 4;
}

int aesr_thick_slices(const float* in, float* out, int Z, int H, int W, int z_step, const double* weights_host, int radius, void* stream) {
    AESR_CHECK_ARG(in, "aesr_thick_slices: in is a null pointer");
    AESR_CHECK_ARG(out, "aesr_thick_slices: out is a null pointer");
    AESR_CHECK_ARG(weights_host, "aesr_thick_slices: weights_host is a null pointer");
    AESR_CHECK_ARG(Z > 0 && H > 0 && W > 0, "aesr_thick_slices: Z, H, W = %d, %d, %d must all be positive", Z, H, W);
    AESR_CHECK_ARG(z_step >= 1, "aesr_thick_slices: z_step=%d must be at least 1", z_step);
    AESR_CHECK_ARG((size_t)Z * H * W < ((size_t)1 << 31), "aesr_thick_slices: Z * H * W = %d x %d x %d has 2^31 elements or more", Z, H, W);
    AESR_CHECK_ARG(radius >= 0, "aesr_thick_slices: radius=%d is negative", radius);
    if (radius > TS_MAXR) {
        aesr_set_error("aesr_thick_slices: radius=%d exceeds the supported %d (slice thickness above ~9.7)", radius, TS_MAXR);
        return AESR_ERR_UNSUPPORTED;
    }
    TsWeights wt;
    double sum = 0.0;
    for (int k = 0; k <= 2 * TS_MAXR; ++k) wt.w[k] = 0.0;
    for (int k = 0; k <= 2 * radius; ++k) {
        AESR_CHECK_ARG(weights_host[k] == weights_host[2 * radius - k], "aesr_thick_slices: weights_host is not symmetric (entry %d)", k);
        wt.w[k] = weights_host[k];
        sum += weights_host[k];
    }
    AESR_CHECK_ARG(fabs(sum - 1.0) <= 1e-12, "aesr_thick_slices: weights_host sums to %.17g, not to 1", sum);
    const int Zo = aesr_thick_slices_out_slices(Z, z_step);
    // the longest run of output slices whose input window fits the staged TS_WINDOW slices (>= 1: 2 * TS_MAXR + 1 <= TS_WINDOW)
    int OB = (TS_WINDOW - 2 * radius - 1) / z_step + 1;
    if (OB > Zo) OB = Zo;
    const size_t HW = (size_t)H * W;
    const bool vec = aesr_thick_slices_store_bytes(W, in, out) == 16;
    const unsigned int units = (unsigned int)(vec ? HW / 4 : HW);
    const dim3 grid((units + (vec ? 64 : 256) - 1) / (vec ? 64 : 256), (unsigned int)ceil_div(Zo, OB));
    AESR_CHECK_ARG(grid.y <= 65535, "aesr_thick_slices: Z=%d with z_step=%d needs %u runs of output slices (at most 65535)", Z, z_step, grid.y);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL((thick_slices_kernel<f32x4, 64>), grid, dim3(TS_THREADS), 0, st, (const f32x4*)in, (f32x4*)out, wt, Z, Zo, units, z_step,
                           radius, OB);
    else
        hipLaunchKernelGGL((thick_slices_kernel<float, 256>), grid, dim3(TS_THREADS), 0, st, in, out, wt, Z, Zo, units, z_step, radius, OB);
    AESR_LAUNCH_CHECK("thick_slices");
    return AESR_OK;
}

}  // extern "C"
