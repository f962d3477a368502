/* libaesr_hip.so -- connected-component ABI (eleventh header of the same library; include/aesr_hip.h holds the training and evaluation kernels,
 * and its conventions apply here unchanged: pointers are DEVICE pointers unless called host arrays, `stream` is a hipStream_t passed as
 * void* (NULL = the default stream), every launch entry point returns 0 or AESR_ERR_ARG / AESR_ERR_HIP / AESR_ERR_UNSUPPORTED and leaves
 * its message in aesr_last_error_string()).  The conventions and refusals are those of include/aesr_hip_surface.h; every one of them is
 * listed again below.
 *
 * Exact connected-component labelling of label volumes for all frames and classes in one launch sequence, the per-component table, the
 * overlaps of two labelled volumes and a table gather: what object-wise scores and largest-component clean-up stand on --
 * csrc/components.hip.
 *
 * Definitions.  vol is a label volume [N][Z][H][W] of class ids stored as fp32 (the convention of aesr_hip_seg.h / aesr_hip_surface.h: a
 * value that is NaN, not integral, or not in `classes` belongs to no class).
 *   adjacency   two voxels are adjacent for ndim in {2, 3} and connectivity in 1 ... ndim when their offset o != 0 lies in {-1, 0, 1}^ndim
 *               with |o|_1 <= connectivity: scipy's generate_binary_structure(ndim, connectivity).
 *   units       ndim = 2: every slice is an image of its own, a unit is a slice, U = N * Z, unit u = n * Z + z.  ndim = 3: a unit is a
 *               frame, U = N.  (The rule by which aesr_hip_surface.h scores slices.)
 *   components  a component is a maximal set of voxels of one unit that have the same class and are connected through adjacent voxels of
 *               that class.  A voxel belongs to at most one class and only equal classes merge, so one pass serves all C classes.
 *   numbering   per (unit, class) the components are numbered 1 ... n in raster order (z, y, x ascending) of each component's first
 *               voxel: exactly scipy.ndimage.label of the mask (vol == class) of that unit.
 *
 * Outputs.
 *   labels        int32 [N][Z][H][W]: 0 where the voxel has no class, otherwise its component's number within its (unit, class).
 *   n_components  int32 [U][C].
 *   table         int64 [R][8], one row per component in the order (unit, class, number), R = the sum of n_components: voxel count, the
 *                 half-open bounding box z0, z1, y0, y1, x0, x1 (scipy's find_objects; with ndim = 2, z1 = z0 + 1; z counts within the
 *                 frame), and the linear index (z * H + y) * W + x of the component's first voxel within its frame.
 *   overlap runs  of two labelled volumes A and B of the same shape, classes and ndim: the tuple (unit, class index, label_A, label_B) at
 *                 every voxel that has the same class in A and in B and whose x-predecessor in the same row does not carry the same
 *                 tuple, packed in raster order as int32 [K][4].  The set of distinct tuples is exactly the set of (component of A,
 *                 component of B) pairs that share a voxel; K is bounded by the number of x-runs.
 *   apply table   out[p] = labels[p] == 0 ? 0 : table[offset[unit][class] + labels[p] - 1], offset being the exclusive prefix of
 *                 n_components in the order (unit, class); out is fp32 and table a device array of fp32.  Component NUMBERS travel through
 *                 fp32 when a caller puts them into such a table (the pair relabelling of evaluate/object_metrics.py does), which is why
 *                 more than 2^24 components in one (unit, class) are refused by the entry points that take the host counts.
 *
 * Phases, because table sizes are not known before the labelling is:
 *   aesr_components_label          labels, n_components (both fully overwritten) and the workspace.
 *   (the caller copies n_components to the host -- the only synchronisation -- and sizes `table`)
 *   aesr_components_tables         all R rows of `table`; it writes their initial values itself.  vol, labels, n_components are those of
 *                                  the label call with the same sizes, classes and ndim; n_components_host is the HOST copy.
 *   aesr_components_apply_table    the gather above, all of `out`.
 *   aesr_components_overlap_count  count[0] = K, and the run ranks in the workspace.
 *   (the caller copies count to the host and sizes `runs`)
 *   aesr_components_overlap_runs   the first K tuples of `runs`, nothing beyond; the four volumes and the workspace are those of the count
 *                                  call, unchanged in between.
 *
 * Memory contract: vol N*Z*H*W floats, read only, 4-byte aligned; labels N*Z*H*W int32, 4-byte aligned; n_components U*C int32, 4-byte
 * aligned; workspace aesr_components_workspace_bytes(N, Z, H, W, C) bytes, 16-byte aligned, needs no initialisation, every byte that is read
 * was written by the same call sequence (one workspace may serve all six calls; the tables / apply section, the overlap section and the
 * labelling section do not share bytes); table 8*capacity int64, 8-byte aligned; count one int64, 8-byte aligned; runs 4*capacity int32,
 * 4-byte aligned (may be NULL when count_host is 0); the fp32 table table_len floats and out N*Z*H*W floats, 4-byte aligned; classes and
 * n_components_host host arrays.  Label values are read with 16-byte accesses by the tile kernel when vol and the workspace are 16-byte
 * aligned and W is a multiple of 4, with 4-byte accesses otherwise; the values are identical either way.  Everything is integer: component
 * roots are minimum linear indices, so the labels do not depend on the order in which atomics arrive; table entries are integer sums,
 * minima and maxima; packing is by raster rank.  Two runs give the same bits.  The caller owns every buffer; nothing is allocated and
 * nothing synchronises.
 *
 * Refusals, all before anything touches the device, nothing written: a null pointer, a pointer not aligned as above, a non-positive
 * size, C outside 1 ... 8, ndim outside {2, 3}, connectivity outside 1 ... ndim, duplicate class ids, a class id beyond +-2^24,
 * N*Z*H*W of 2^31 or more (or N*Z*C), host counts that are inconsistent (negative, more components than the unit has voxels, count_host above the
 * number of voxels) or need more rows / floats / tuples than `capacity` / `table_len`: AESR_ERR_ARG.  An output or the workspace
 * overlapping an input or another output, more than 2^24 components in one (unit, class) of n_components_host: AESR_ERR_UNSUPPORTED.
 * The workspace query returns 0 for sizes the launch entry points refuse. */
#ifndef AESR_HIP_COMPONENTS_H
#define AESR_HIP_COMPONENTS_H

#include "aesr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESR_COMPONENTS_MAX_CLASSES 8
#define AESR_COMPONENTS_COLUMNS 8
#define AESR_COMPONENTS_MAX_PER_CLASS 16777216

size_t aesr_components_workspace_bytes(int N, int Z, int H, int W, int C);

int aesr_components_label(const float* vol, int* labels, int* n_components, void* workspace, int N, int Z, int H, int W, const int* classes,
                          int C, int ndim, int connectivity, void* stream);

int aesr_components_tables(const float* vol, const int* labels, const int* n_components, const int* n_components_host, void* workspace,
                           long long* table, size_t capacity, int N, int Z, int H, int W, const int* classes, int C, int ndim, void* stream);

int aesr_components_overlap_count(const float* vol_a, const int* labels_a, const float* vol_b, const int* labels_b, void* workspace,
                                  long long* count, int N, int Z, int H, int W, const int* classes, int C, int ndim, void* stream);

int aesr_components_overlap_runs(const float* vol_a, const int* labels_a, const float* vol_b, const int* labels_b, void* workspace,
                                 long long count_host, int* runs, size_t capacity, int N, int Z, int H, int W, const int* classes, int C,
                                 int ndim, void* stream);

int aesr_components_apply_table(const float* vol, const int* labels, const int* n_components, const int* n_components_host, void* workspace,
                                const float* table, size_t table_len, float* out, int N, int Z, int H, int W, const int* classes, int C,
                                int ndim, void* stream);

#ifdef __cplusplus
}
#endif
#endif
