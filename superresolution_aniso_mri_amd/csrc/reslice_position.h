// The position rule the affine reslicing kernels share (reslice.hip, reslice_taps.hip): one device function, so that every interpolator
// samples bit-identical positions.
#pragma once

#pragma clang fp contract(off)

struct RslAffine {
    double m[12];          // rows of the 3x4 matrix: source (x, y, z) = M * (xo, yo, zo, 1)
};

// p = (x, y, z) of output voxel (xo, yo, zo): per row ((m0 xo + m1 yo) + m2 zo) + m3 in fp64, never contracted
__device__ __forceinline__ void rsl_affine_position(const RslAffine& A, int xo, int yo, int zo, double p[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
        p[a] = ((A.m[4 * a] * (double)xo + A.m[4 * a + 1] * (double)yo) + A.m[4 * a + 2] * (double)zo) + A.m[4 * a + 3];
}
