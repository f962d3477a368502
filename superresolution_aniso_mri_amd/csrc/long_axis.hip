// Long-axis (through-plane) views of a volume pair for the evaluation (evaluate/metrics.py:65-243 of the reference swaps axis 0 with
// eval_axis on the host, slice-tests `np.sum(reference[s]) == 0` and then scores slice by slice):
//   axis 1:  view[h][z][w] = v[z][h][w]      a permutation of whole rows of W floats
//   axis 2:  view[w][h][z] = v[z][h][w]      per h a Z x W -> W x Z transpose
// for the reference and the reconstruction at once, plus black[s] = 1 iff every element of ref_view[s] is exactly 0 (+0.0 or -0.0; a NaN
// is not 0).  Every element is moved as a 32-bit word, untouched: the views are bitwise np.swapaxes(v, 0, axis).  Each input is read
// once and each view written once; the flags come from the words a workgroup has in its registers anyway.
//   axis 1: one workgroup per (slice h, volume): it owns the whole slice, so its flag is one __syncthreads_or.  Loads and stores are
//           contiguous along w (16 bytes per lane when W % 4 == 0 and the pointers allow it).
//   axis 2: tiles of LA_TW = 64 columns x up to LA_ROWS = 128 (h, z) rows go through LDS: read along w (256 contiguous bytes per wave
//           instruction), written along (h, z), which is contiguous in the view for a fixed w -- one tile covers all of Z when Z <= 64 and
//           then as many h as fit, so a wave stores runs of up to 512 bytes even for Z = 10.  LDS rows are padded by one word: the
//           column read has stride 65 words and is conflict-free.  A slice w is spread over many workgroups, so the launcher presets
//           black[] to 1 (a memset node of W bytes in front of the kernel) and every workgroup that met a non-zero word in column w
//           stores 0 there: byte stores of one value, whichever workgroup comes first -- no atomics, nothing depends on scheduling.
#include "aesr_kernels.h"

#define LA_TW 64
#define LA_ROWS 128
#define LA_THREADS1 512

template <typename T> __device__ __forceinline__ bool la_nonzero(T v);
template <> __device__ __forceinline__ bool la_nonzero<float>(float v) { return v != 0.f; }
template <> __device__ __forceinline__ bool la_nonzero<f32x4>(f32x4 v) { return v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f; }

// T = float (WT = W) or f32x4 (WT = W / 4).  grid (H, 2): blockIdx.y = 0 reference (sets black[h]), 1 reconstruction.
template <typename T>
__global__ __launch_bounds__(LA_THREADS1) void long_axis_rows_kernel(const T* __restrict__ ref, const T* __restrict__ rec,
                                                                      T* __restrict__ ref_view, T* __restrict__ rec_view,
                                                                      unsigned char* __restrict__ black, int Z, int H, int WT) {
    const int h = blockIdx.x;
    const bool is_ref = blockIdx.y == 0;
    const T* __restrict__ src = (is_ref ? ref : rec) + (size_t)h * WT;
    T* __restrict__ dst = (is_ref ? ref_view : rec_view) + (size_t)h * Z * WT;
    const size_t zstride = (size_t)H * WT;
    const int n = Z * WT;                           // < 2^30 (checked by the entry point)
    int any = 0;
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += LA_THREADS1) {
        const int z = i / WT, c = i - z * WT;
        const T v = src[(size_t)z * zstride + c];
        dst[i] = v;
        any |= la_nonzero<T>(v);
    }
    if (is_ref) {                                   // uniform per workgroup
        any = __syncthreads_or(any);
        if (threadIdx.x == 0) black[h] = any ? 0 : 1;
    }
}

// 1-D grid: tile = ((vol * nzc + zc) * nht + ht) * nwt + wt, w tiles fastest.  TZ = min(Z, 64) z per tile, TH = LA_ROWS / TZ h per
// tile; tile row r = hl * TZ + zl.  black[] was preset to 1.
__global__ __launch_bounds__(256) void long_axis_transpose_kernel(const float* __restrict__ ref, const float* __restrict__ rec,
                                                                  float* __restrict__ ref_view, float* __restrict__ rec_view,
                                                                  unsigned char* __restrict__ black, int Z, int H, int W, int TZ, int TH,
                                                                  int nwt, int nht, int nzc) {
    __shared__ float tile[LA_ROWS][LA_TW + 1];
    __shared__ int nz[LA_TW], srow[LA_ROWS], drow[LA_ROWS];
    unsigned int t = blockIdx.x;
    const int wt = t % nwt;
    t /= nwt;
    const int ht = t % nht;
    t /= nht;
    const int zc = t % nzc;
    const bool is_ref = t / nzc == 0;
    const float* __restrict__ src = is_ref ? ref : rec;
    float* __restrict__ dst = is_ref ? ref_view : rec_view;
    const int w0 = wt * LA_TW, h0 = ht * TH, z0 = zc * TZ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = TH * TZ;                       // <= LA_ROWS
    // where tile row r comes from and goes to (-1: outside the volume): the only divisions of the kernel, one per row
    if (threadIdx.x < LA_ROWS) {
        const int r = threadIdx.x, hl = r / TZ, zl = r - hl * TZ;
        const int h = h0 + hl, z = z0 + zl;
        const bool ok = r < rows && h < H && z < Z;
        srow[r] = ok ? (z * H + h) * W : -1;        // < 2^30 (checked by the entry point)
        drow[r] = ok ? h * Z + z : -1;
    }
    if (threadIdx.x < LA_TW) nz[threadIdx.x] = 0;
    __syncthreads();
    // read: a wave takes a row, its lanes run along w
    int any = 0;
    const bool w_ok = w0 + lane < W;
#pragma unroll 8
    for (int r = wave; r < rows; r += 4) {
        const int off = srow[r];                    // the same for the whole wave
        float v = 0.f;
        if (w_ok && off >= 0) v = src[(size_t)off + w0 + lane];
        tile[r][lane] = v;
        any |= v != 0.f;
    }
    if (is_ref && any) nz[lane] = 1;                // every writer stores the same value
    __syncthreads();
    // write: a wave takes a column w, its lanes run along the rows = along (h, z) of the view
    const int d0 = drow[lane], d1 = drow[lane + 64];
    const size_t HZ = (size_t)H * Z;
#pragma unroll 4
    for (int wl = wave; wl < LA_TW; wl += 4) {
        if (w0 + wl >= W) break;
        float* __restrict__ col = dst + (size_t)(w0 + wl) * HZ;
        if (d0 >= 0) col[d0] = tile[lane][wl];
        if (d1 >= 0) col[d1] = tile[lane + 64][wl];
    }
    if (is_ref && threadIdx.x < LA_TW && w0 + (int)threadIdx.x < W && nz[threadIdx.x]) black[w0 + threadIdx.x] = 0;
}

int aesr_launch_long_axis_views(const float* ref, const float* rec, float* ref_view, float* rec_view, unsigned char* black, int Z, int H,
                                int W, int axis, hipStream_t st) {
    if (axis == 1) {
        const uintptr_t bits = (uintptr_t)ref | (uintptr_t)rec | (uintptr_t)ref_view | (uintptr_t)rec_view;
        if (W % 4 == 0 && bits % 16 == 0)
            hipLaunchKernelGGL(long_axis_rows_kernel<f32x4>, dim3(H, 2), dim3(LA_THREADS1), 0, st, (const f32x4*)ref, (const f32x4*)rec,
                               (f32x4*)ref_view, (f32x4*)rec_view, black, Z, H, W / 4);
        else
            hipLaunchKernelGGL(long_axis_rows_kernel<float>, dim3(H, 2), dim3(LA_THREADS1), 0, st, ref, rec, ref_view, rec_view, black, Z, H, W);
        AESR_LAUNCH_CHECK("long_axis_rows");
        return AESR_OK;
    }
    const int TZ = Z < 64 ? Z : 64, TH = LA_ROWS / TZ;              // TZ <= 64: TH >= 2
    const int nwt = ceil_div(W, LA_TW), nht = ceil_div(H, TH), nzc = ceil_div(Z, TZ);
    // tiles <= 2 * ceil(W/64) * ceil(H/TH) * ceil(Z/TZ) with Z*H*W < 2^30: far below the 2^31 - 1 limit of grid.x
    const size_t tiles = (size_t)2 * nzc * nht * nwt;
    AESR_CHECK_ARG(tiles < ((size_t)1 << 31), "aesr_long_axis_views: %d x %d x %d needs %zu tiles", Z, H, W, tiles);
    hipError_t e = hipMemsetAsync(black, 1, (size_t)W, st);
    if (e != hipSuccess) {
        aesr_set_error("long_axis_views: memset failed: %s", hipGetErrorString(e));
        return AESR_ERR_HIP;
    }
    hipLaunchKernelGGL(long_axis_transpose_kernel, dim3((unsigned int)tiles), dim3(256), 0, st, ref, rec, ref_view, rec_view, black, Z, H, W,
                       TZ, TH, nwt, nht, nzc);
    AESR_LAUNCH_CHECK("long_axis_transpose");
    return AESR_OK;
}
