// What the affine reslicing files share (reslice.hip, reslice_taps.hip): the tile of a workgroup, the position rule -- one device function,
// so that every interpolator samples bit-identical positions -- and the host's checks of the two shapes.  Static inline only: no symbol.
#pragma once
#include "aesr_common.h"

#pragma clang fp contract(off)

#define RSL_THREADS 256
#define RSL_LX 64          // lanes along the output x: one wave is one row segment of a tile

struct RslAffine {
    double m[12];          // rows of the 3x4 matrix: source (x, y, z) = M * (xo, yo, zo, 1)
};

// A tile is RSL_LX lanes x 4 rows of one output slice; grid.x: tiles_x * tiles_y * Zo tiles, x fastest (zo < Zo: the launcher sized the
// grid for it).  The voxel of this thread; false when it lies beyond the slice's edge.
__device__ __forceinline__ bool rsl_tile_voxel(unsigned int tiles_x, unsigned int tiles_y, int Ho, int Wo, int& xo, int& yo, unsigned int& zo) {
    const unsigned int tx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
    const unsigned int ty = rest % tiles_y;
    zo = rest / tiles_y;
    xo = (int)(tx * RSL_LX + (threadIdx.x & (RSL_LX - 1)));
    yo = (int)(ty * (RSL_THREADS / RSL_LX) + threadIdx.x / RSL_LX);
    return xo < Wo && yo < Ho;
}

// p = (x, y, z) of output voxel (xo, yo, zo): per row ((m0 xo + m1 yo) + m2 zo) + m3 in fp64, never contracted
__device__ __forceinline__ void rsl_affine_position(const RslAffine& A, int xo, int yo, int zo, double p[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
        p[a] = ((A.m[4 * a] * (double)xo + A.m[4 * a + 1] * (double)yo) + A.m[4 * a + 2] * (double)zo) + A.m[4 * a + 3];
}

// The host's checks of the source and output shapes, in two steps because each entry point has checks of its own between them; `fn` is the
// entry point's name in the message.
static inline int rsl_check_sizes(const char* fn, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo) {
    AESR_CHECK_ARG(N > 0, "%s: N=%d must be positive", fn, N);
    AESR_CHECK_ARG(Zs > 0 && Hs > 0 && Ws > 0, "%s: Zs, Hs, Ws = %d, %d, %d must all be positive", fn, Zs, Hs, Ws);
    AESR_CHECK_ARG(Zo > 0 && Ho > 0 && Wo > 0, "%s: Zo, Ho, Wo = %d, %d, %d must all be positive", fn, Zo, Ho, Wo);
    return AESR_OK;
}

static inline int rsl_check_counts(const char* fn, int N, int Zs, int Hs, int Ws, int Zo, int Ho, int Wo) {
    AESR_CHECK_ARG((double)N * Zs * Hs * Ws < 2147483648.0, "%s: N * Zs * Hs * Ws = %d x %d x %d x %d has 2^31 elements or more", fn, N, Zs, Hs, Ws);
    AESR_CHECK_ARG((double)N * Zo * Ho * Wo < 2147483648.0, "%s: N * Zo * Ho * Wo = %d x %d x %d x %d has 2^31 elements or more", fn, N, Zo, Ho, Wo);
    return AESR_OK;
}
