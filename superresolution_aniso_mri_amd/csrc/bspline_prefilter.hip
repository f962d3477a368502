// The recursive cubic B-spline pre-filter: scipy.ndimage.spline_filter1d(order = 3, mode = 'mirror') in double along z (fp32 samples to fp64
// coefficients: aesr_bspline_prefilter_z, include/aesr_hip_baselines.h) and then in place along y and x (aesr_bspline_prefilter_3d,
// include/aesr_hip_reslice_taps.h).  bspline_prefilter.h has the recursion of a line.
//   - z: one thread per (frame, y, x) column; y: one thread per (frame, z, x) line.  Lanes are neighbouring columns: every load and store
//     of a wave is one contiguous row segment;
//   - x: the line is the contiguous axis.  A workgroup owns 64 rows and moves them through LDS in blocks of 64 rows x 32 columns (rows
//     padded to 33 doubles: the 32 lanes of a half-wave fall on 32 different bank pairs), loaded and stored with all 256 threads along the
//     rows, so global traffic is in 256-byte row segments; one lane per row then runs the recursion over the block in LDS and carries its
//     state to the next block.  Three sweeps: the exact causal start (two running sums over the whole line), causal ascending, anti-causal
//     descending; a line that fits one block is loaded and stored once.  A line is read and written by one workgroup only.
// No workspace beyond the caller's `coef`, no copy, no synchronisation, no atomics, no scratch.
#include "../../include/aesr_hip_baselines.h"
#include "../../include/aesr_hip_reslice_taps.h"
#include "aesr_kernels.h"
#include "aesr_hostcheck.h"
#include "bspline_prefilter.h"

#pragma clang fp contract(off)

#define BSP_THREADS 256
#define PFX_ROWS 64            // rows of a workgroup of the x pass
#define PFX_CW 32              // columns of a staged block
#define PFX_LD (PFX_CW + 1)    // padded row of the staged block, in doubles

// z: cols = N * HW columns, column c of frame n starts at n * Z * HW + c and has stride HW
__global__ __launch_bounds__(BSP_THREADS) void bspline_prefilter_kernel(const float* __restrict__ in, double* __restrict__ coef, unsigned int cols,
                                                                        unsigned int HW, int Z) {
    const unsigned int col = blockIdx.x * BSP_THREADS + threadIdx.x;
    if (col >= cols) return;
    const size_t off = (size_t)(col / HW) * Z * HW + col % HW;
    bsp_prefilter_line(in + off, coef + off, Z, HW);
}

// y: cols = N * Z * W lines of H coefficients with stride W, in place
__global__ __launch_bounds__(BSP_THREADS) void bspline_prefilter_y_kernel(double* __restrict__ coef, unsigned int cols, unsigned int W, int H) {
    const unsigned int col = blockIdx.x * BSP_THREADS + threadIdx.x;
    if (col >= cols) return;
    double* c = coef + (size_t)(col / W) * H * W + col % W;
    bsp_prefilter_line(c, c, H, W);
}

// x: PFX_ROWS rows per workgroup through LDS in blocks of PFX_CW columns.  rows = N * Z * H lines of W >= 2 coefficients, in place.
// With z = the pole, L = W: the causal start is c0 = 6 (S1 + z^(L-1) S2) / (1 - z^(2L-2)), S1 = sum_{i=0}^{L-1} z^i x[i] and
// S2 = sum_{j=1}^{L-2} z^(L-1-j) x[j] (the mirrored half of the period), S2 by Horner's rule so that both run in ascending order.
__global__ __launch_bounds__(BSP_THREADS) void bspline_prefilter_x_kernel(double* __restrict__ coef, unsigned int rows, int W) {
    __shared__ double tile[PFX_ROWS * PFX_LD];
    const unsigned int row0 = blockIdx.x * PFX_ROWS;
    const int nrows = (int)min((unsigned int)PFX_ROWS, rows - row0);          // > 0: the launcher sized the grid for it
    double* __restrict__ base = coef + (size_t)row0 * W;
    const int nch = (W + PFX_CW - 1) / PFX_CW;
    const int r = (int)threadIdx.x;
    const bool owner = r < nrows;          // this lane runs the recursion of row r
    double* __restrict__ mine = tile + (owner ? r : 0) * PFX_LD;
    const double z1 = BSP_POLE, gain = BSP_GAIN;

    // all threads: block `ch` of the rows <-> LDS; the barriers keep a block's recursion apart from its load and store
    auto load = [&](int ch) {
        __syncthreads();
        for (int idx = (int)threadIdx.x; idx < PFX_ROWS * PFX_CW; idx += BSP_THREADS) {
            const int rr = idx / PFX_CW, x = ch * PFX_CW + idx % PFX_CW;
            if (rr < nrows && x < W) tile[rr * PFX_LD + idx % PFX_CW] = base[(size_t)rr * W + x];
        }
        __syncthreads();
    };
    auto store = [&](int ch) {
        __syncthreads();
        for (int idx = (int)threadIdx.x; idx < PFX_ROWS * PFX_CW; idx += BSP_THREADS) {
            const int rr = idx / PFX_CW, x = ch * PFX_CW + idx % PFX_CW;
            if (rr < nrows && x < W) base[(size_t)rr * W + x] = tile[rr * PFX_LD + idx % PFX_CW];
        }
    };

    // sweep 1: the causal start
    double s1 = 0.0, s2 = 0.0, zi = 1.0;          // zi = z1^i
    for (int ch = 0; ch < nch; ++ch) {
        load(ch);
        if (owner) {
            const int x0 = ch * PFX_CW, n = min(PFX_CW, W - x0);
            for (int j = 0; j < n; ++j) {
                const int i = x0 + j;
                const double v = mine[j];
                s1 += zi * v;
                if (i >= 1 && i <= W - 2) s2 = s2 * z1 + v;
                if (i < W - 1) zi *= z1;          // ends as z1^(W-1)
            }
        }
    }
    const double zn1 = zi;
    double prev = gain * (s1 + zn1 * (s2 * z1)) / (1.0 - zn1 * zn1), prev2 = prev;
    // sweep 2: causal, ascending.  A line of one block is still in LDS.
    for (int ch = 0; ch < nch; ++ch) {
        if (nch > 1) load(ch);
        if (owner) {
            const int x0 = ch * PFX_CW, n = min(PFX_CW, W - x0);
            for (int j = 0; j < n; ++j) {
                if (x0 + j > 0) {
                    prev2 = prev;
                    prev = mine[j] * gain + z1 * prev;
                }
                mine[j] = prev;
            }
        }
        if (nch > 1) store(ch);
    }
    // sweep 3: anti-causal, descending; prev2, prev are the last two causal values
    double next = bsp_anticausal_start(prev2, prev);
    for (int ch = nch - 1; ch >= 0; --ch) {
        if (nch > 1) load(ch);
        if (owner) {
            const int x0 = ch * PFX_CW, n = min(PFX_CW, W - x0);
            for (int j = n - 1; j >= 0; --j) {
                if (x0 + j < W - 1) next = z1 * (next - mine[j]);
                mine[j] = next;
            }
        }
        store(ch);
    }
}

// the checks the two entry points share; `fn` is the entry point's name in the message
static int bsp_check(const char* fn, const float* in, const double* coef, int N, int Z, int H, int W) {
    AESR_CHECK_ARG(in, "%s: in is a null pointer", fn);
    AESR_CHECK_ARG(coef, "%s: coef is a null pointer", fn);
    AESR_CHECK_ARG((uintptr_t)in % 4 == 0, "%s: in is not 4-byte aligned", fn);
    AESR_CHECK_ARG((uintptr_t)coef % 8 == 0, "%s: coef is not 8-byte aligned", fn);
    AESR_CHECK_ARG(N > 0 && Z > 0 && H > 0 && W > 0, "%s: N, Z, H, W = %d, %d, %d, %d must all be positive", fn, N, Z, H, W);
    AESR_CHECK_ARG((double)N * Z * H * W < 2147483648.0, "%s: N * Z * H * W = %d x %d x %d x %d has 2^31 elements or more", fn, N, Z, H, W);
    return AESR_OK;
}

// fp32 -> fp64 along z; Z == 1 copies
static int bsp_launch_z(const float* in, double* coef, int N, int Z, int H, int W, hipStream_t st) {
    const unsigned int HW = (unsigned int)H * W, cols = HW * N;
    hipLaunchKernelGGL(bspline_prefilter_kernel, dim3((cols + BSP_THREADS - 1) / BSP_THREADS), dim3(BSP_THREADS), 0, st, in, coef, cols, HW, Z);
    AESR_LAUNCH_CHECK("bspline_prefilter_z");
    return AESR_OK;
}

extern "C" {

int aesr_bspline_prefilter_z(const float* in, double* coef, int N, int Z, int H, int W, void* stream) {
    if (const int rc = bsp_check("aesr_bspline_prefilter_z", in, coef, N, Z, H, W)) return rc;
    return bsp_launch_z(in, coef, N, Z, H, W, (hipStream_t)stream);
}

int aesr_bspline_prefilter_3d(const float* in, double* coef, int N, int Z, int H, int W, void* stream) {
    if (const int rc = bsp_check("aesr_bspline_prefilter_3d", in, coef, N, Z, H, W)) return rc;
    const size_t count = (size_t)N * Z * H * W;
    if (aesr_overlap(coef, 8 * count, in, 4 * count)) {
        aesr_set_error("aesr_bspline_prefilter_3d: coef overlaps in");
        return AESR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = bsp_launch_z(in, coef, N, Z, H, W, st)) return rc;
    if (H > 1) {
        const unsigned int cols = (unsigned int)N * Z * W;
        hipLaunchKernelGGL(bspline_prefilter_y_kernel, dim3((cols + BSP_THREADS - 1) / BSP_THREADS), dim3(BSP_THREADS), 0, st, coef, cols, (unsigned int)W, H);
        AESR_LAUNCH_CHECK("bspline_prefilter_3d (y)");
    }
    if (W > 1) {
        const unsigned int rows = (unsigned int)N * Z * H;
        hipLaunchKernelGGL(bspline_prefilter_x_kernel, dim3((rows + PFX_ROWS - 1) / PFX_ROWS), dim3(BSP_THREADS), 0, st, coef, rows, W);
        AESR_LAUNCH_CHECK("bspline_prefilter_3d (x)");
    }
    return AESR_OK;
}

}  // extern "C"
