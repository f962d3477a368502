// Host-side planning of the convolution kernels (conv_plan.hip): size limits, channel padding, the tile planners and what they share --
// one plan cache and one reader for the override variables.  No device code.
#pragma once
#include <stdlib.h>

#include <map>
#include <mutex>

#include "aesr_kernels.h"

void cout_padding(int Cout, int* CoutP, int* NB);
static inline int plane_stride(int n) { return round_up(n, 64) + 4; }    // = 4 (mod 64): 16 channel planes hit 16 distinct bank quads

// Every convolution entry point and query decides FIRST, in 64 bits, whether the tensors stay inside the kernels' 32-bit element offsets (the
// launchers refuse 0x1C000000 elements and more): the planners do their tile arithmetic in int and must never see sizes beyond that
// (found by the host-side sanitizer sweep of round 6, tests/test_host_sanitized.py: ceil_div(INT_MAX, 2) in plan_wino from a query).
bool conv_dims_ok(int N, int H, int W, int Cin, int Cout);
#define AESR_CHECK_DIMS(who, N, H, W, Cin, Cout)                                                                                            \
    do {                                                                                                                                    \
        if (!conv_dims_ok(N, H, W, Cin, Cout)) {                                                                                            \
            aesr_set_error("%s: %d x %d x %d with %d -> %d channels is empty or beyond the kernels' 32-bit element offsets (469M elements)", who, N, H, \
                           W, Cin, Cout);                                                                                                   \
            return AESR_ERR_UNSUPPORTED;                                                                                                    \
        }                                                                                                                                   \
    } while (0)

// A planner override: n integers "a,b,.." from the environment variable `name` into v.  True when all n are there; otherwise v is all
// zero, which every planner reads as "not forced".  Read on EVERY call and made part of the cache key below, so that a variable takes
// effect whenever it is set, whatever the process planned before.
static inline bool env_ints(const char* name, int* v, int n) {
    const char* e = getenv(name);
    int got = 0;
    for (; e && got < n; ++got) {
        char* end;
        v[got] = (int)strtol(e, &end, 10);
        if (end == e || (got + 1 < n && *end != ',')) break;
        e = end + 1;
    }
    if (got == n) return true;
    for (int i = 0; i < n; ++i) v[i] = 0;
    return false;
}

// Plans by key (shape and parsed overrides): found, or computed once under the lock.
template <class Key, class Plan>
class PlanCache {
    std::mutex mu_;
    std::map<Key, Plan> plans_;

  public:
    template <class F>
    Plan get(const Key& key, F compute) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = plans_.find(key);
        if (it == plans_.end()) it = plans_.emplace(key, compute()).first;
        return it->second;
    }
};

struct ConvPlan { int TI, TH, TW, NB, MBW, CinP, CoutP, ksplit; };
ConvPlan plan_conv(int N, int Ho, int Wo, int Cin, int Cout, int KS);

struct WinoPlan { int TI, THt, TWt, CinP, CoutP; double cost; };
WinoPlan plan_wino(int N, int H, int W, int Cin, int Cout);

struct WgradPlan { int variant, COT, CinP, CoutP, TH, TW, S, nslab, PWS, TWS, PSX, PSD; size_t slab_floats; };
bool wgrad_wino_ok(int Cin, int Cout, int KS, int pad);
WgradPlan plan_wgrad(int N, int Ho, int Wo, int Cin, int Cout, int KS, int pad = -1);
