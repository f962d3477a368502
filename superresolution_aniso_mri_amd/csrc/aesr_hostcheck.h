// Host-side argument checks that several entry-point files share (reslice.hip, seg_head.hip, seg_metrics.hip, components.hip), and the
// label-class table the two label-volume files hand to their kernels.  Everything here is static inline: no symbol of its own.
#pragma once
#include "aesr_common.h"
#include "../../include/aesr_hip_components.h"
#include "../../include/aesr_hip_surface.h"

// true when the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte; a null pointer or an empty range overlaps nothing
static inline bool aesr_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

struct AesrBuf {
    const void* p;
    size_t bytes;
    bool out;          // written by the call: an output or the workspace
};

// true when an output (or the workspace) overlaps any other buffer of the call; two inputs may share memory
static inline bool aesr_any_overlap(const AesrBuf* bufs, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if ((bufs[i].out || bufs[j].out) && aesr_overlap(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes)) return true;
    return false;
}

static inline size_t aesr_up16(size_t v) { return (v + 15) / 16 * 16; }

// ---- label classes: the ids of the classes a call asks for, as the floats the label volumes hold ---------------------------------------
#define AESR_MAX_CLASSES 8
static_assert(AESR_SURFACE_MAX_CLASSES == AESR_MAX_CLASSES && AESR_COMPONENTS_MAX_CLASSES == AESR_MAX_CLASSES,
              "both label-volume headers promise AESR_MAX_CLASSES classes");

struct AesrClasses {
    float v[AESR_MAX_CLASSES];
};

// index of the class whose id v is, -1 for none
__device__ __forceinline__ int aesr_class_of(float v, const AesrClasses& cls, int C) {
    int k = -1;
#pragma unroll
    for (int c = 0; c < AESR_MAX_CLASSES; ++c)
        if (c < C && v == cls.v[c]) k = c;          // NaN equals nothing; ids are distinct, so at most one hit
    return k;
}

// the class ids alone (classes != NULL, 1 <= C <= AESR_MAX_CLASSES: the caller has checked both): each exact in fp32 and listed once; fills cls
static inline int aesr_fill_classes(const char* fn, const int* classes, int C, AesrClasses* cls) {
    for (int c = 0; c < AESR_MAX_CLASSES; ++c) cls->v[c] = 0.f;
    for (int c = 0; c < C; ++c) {
        AESR_CHECK_ARG(classes[c] >= -(1 << 24) && classes[c] <= (1 << 24), "%s: class id %d is not exact in fp32", fn, classes[c]);
        for (int d = 0; d < c; ++d) AESR_CHECK_ARG(classes[d] != classes[c], "%s: class id %d is listed twice", fn, classes[c]);
        cls->v[c] = (float)classes[c];
    }
    return AESR_OK;
}
