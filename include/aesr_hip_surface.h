/* libaesr_hip.so -- segmentation-score ABI (eighth header of the same library; include/aesr_hip.h holds the training and evaluation kernels,
 * and its conventions apply here unchanged: pointers are DEVICE pointers unless called host arrays, `stream` is a hipStream_t passed as
 * void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP / AESR_ERR_UNSUPPORTED and leaves
 * its message in aesr_last_error_string()).
 *
 * The overlap counts and surface distances a segmentation is judged by (Dice and its relatives, Hausdorff distance, its 95th percentile,
 * average symmetric surface distance), for N volume pairs and C classes in one launch sequence -- csrc/seg_metrics.hip.
 *
 * Definitions.  result, reference are label volumes [N][Z][H][W] of class ids stored as fp32 (the convention of aesr_hip_seg.h: a value
 * that is not integral, NaN, or not in `classes` belongs to no class).  For class c the masks are A = (result == c), B = (reference == c).
 *   counts   [N][C][7] int64: |A|, |B|, |A n B|, |A u B|, the voxel total Z*H*W, the number of border voxels of A, of B.
 *   border   of a mask M for ndim in {2, 3} and connectivity in 1 ... ndim: a voxel of M with at least one neighbour not in M, the
 *            neighbours being the offsets o != 0, o in {-1, 0, 1}^ndim, |o|_1 <= connectivity; a neighbour outside the array is not in M.
 *            ndim = 2: every slice is an image of its own (no z neighbours, no z distance).  ndim = 3 with Z = 1: every object voxel is
 *            border.
 *   lists    for every border voxel p of the source mask in raster order (z, y, x ascending), the distance to the nearest border voxel q
 *            of the other mask, sqrt(min_q (dz*sz)^2 + ((dy*sy)^2 + (dx*sx)^2)) with spacing = (sz, sy, sx): all in fp64, each term the
 *            square of the rounded product, the additions in exactly that association, nothing contracted.  The minimum is taken axis by
 *            axis (x, then y, then z), which equals the minimum over all q bit for bit because rounding and + are monotone.  With
 *            ndim = 2 a border voxel whose slice holds no border voxel of the other mask gets +infinity.
 *            List (n, c, d), d = 0: from the border of A to the border of B (result -> reference), d = 1: from B to A.  Its length is
 *            the border count of its source mask when A and B are both non-empty, else 0.  The lists are packed back to back in the
 *            order l = (n * C + c) * 2 + d; the caller derives every offset from `counts`.
 *   stats    [N][C][2][2] fp64: per list its sum and its maximum (0, 0 for an empty list).
 *
 * Two phases, because list sizes are not known before the borders are:
 *   aesr_surface_borders    classify + border + counts.  Writes `counts` (fully overwritten) and the border section of the workspace.
 *                           It alone serves callers that want only the overlap ratios.
 *   (the caller copies `counts` to the host -- the only synchronisation -- and sizes `distances`)
 *   aesr_surface_distances  distance transforms and the packed lists.  `workspace` and `counts` are those of the borders call with the
 *                           same N, Z, H, W, C, ndim, unchanged in between; `counts_host` is the HOST copy of `counts`.  Writes the
 *                           first sum-of-list-lengths doubles of `distances` (every one of them; nothing beyond) and all of `stats`.
 *
 * Memory contract: result, reference N*Z*H*W floats each, read only; workspace aesr_surface_workspace_bytes(N, Z, H, W, C) bytes, 16-byte
 * aligned, needs no initialisation, every byte that is read was written by the same call sequence; counts 7*N*C int64, 8-byte aligned;
 * distances `capacity` doubles, 8-byte aligned (may be NULL when the lengths sum to 0); stats 4*N*C doubles, 8-byte aligned; classes a
 * host array of C ints, spacing a host array of 3 doubles.  Labels are read with 16-byte accesses when result and reference are 16-byte
 * aligned and Z*H*W is a multiple of 4, with 4-byte accesses otherwise; the values are identical either way.  All sums are
 * integer or made in a fixed order, there are no floating-point atomics: two runs give the same bits.  The caller owns every buffer;
 * nothing is allocated and nothing synchronises.
 *
 * Refusals, all before anything touches the device, nothing written: a null pointer, a pointer not aligned as above (labels: 4 bytes),
 * a non-positive size, C outside 1 ... 8, ndim outside {2, 3}, connectivity outside 1 ... ndim, a spacing that is not positive and
 * finite, duplicate class ids, a class id beyond +-2^24, N*Z*H*W of 2^31 or more (or 2*N*C), counts_host that is inconsistent (negative entries,
 * more border voxels than voxels) or needs more than `capacity` doubles: AESR_ERR_ARG.  W above 4096 (one line's border bitmask lives in
 * LDS), an output or the workspace overlapping an input or another output: AESR_ERR_UNSUPPORTED.  The workspace query returns 0 for
 * sizes the launch entry points refuse. */
#ifndef AESR_HIP_SURFACE_H
#define AESR_HIP_SURFACE_H

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESR_SURFACE_MAX_CLASSES 8
#define AESR_SURFACE_COUNTS 7
#define AESR_SURFACE_MAX_W 4096

size_t aesr_surface_workspace_bytes(int N, int Z, int H, int W, int C);

int aesr_surface_borders(const float* result, const float* reference, void* workspace, long long* counts, int N, int Z, int H, int W,
                         const int* classes, int C, int ndim, int connectivity, void* stream);

int aesr_surface_distances(void* workspace, const long long* counts, const long long* counts_host, double* distances, size_t capacity,
                           double* stats, int N, int Z, int H, int W, int C, int ndim, const double* spacing, void* stream);

#ifdef __cplusplus
}
#endif
#endif
