// The tile planners of the convolution kernels (conv_plan.h): host code only.
#include "conv_plan.h"

#include <stdio.h>

#include <tuple>

void cout_padding(int Cout, int* CoutP, int* NB) {
    if (Cout <= 16) { *CoutP = 16; *NB = 1; }
    else if (Cout <= 32) { *CoutP = 32; *NB = 2; }
    else { *CoutP = round_up(Cout, 64); *NB = 4; }
}

bool conv_dims_ok(int N, int H, int W, int Cin, int Cout) {
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return false;
    if (N > (1 << 24) || H > (1 << 15) || W > (1 << 15) || Cin > (1 << 15) || Cout > (1 << 15)) return false;
    const unsigned long long px = (unsigned long long)N * (unsigned)(H + 2) * (unsigned)(W + 2);       // <= 2^24 * 2^16 * 2^16: no overflow
    return px * (unsigned long long)(Cin > Cout ? Cin : Cout) < 0x1C000000ull;
}

// Pick the output tile (TI images x TH x TW) of the one 512-thread workgroup per CU that minimises estimated MFMA time: idle M-block
// slots at tile edges (the network's sizes are 162, 81, 40 ...) and the work-item quantisation over the CUs.  (Two 4-wave workgroups per
// CU measured 2-5 % slower on all but the 32->32 160x160 layer, profiles/r01_igemm_nt256.txt: not built.)
// AESR_IGEMM_TILE="TI,TH,TW" and AESR_IGEMM_KSPLIT force the tile and the K-split (experiments, tests).
ConvPlan plan_conv(int N, int Ho, int Wo, int Cin, int Cout, int KS) {
    int ft[3], fks;
    env_ints("AESR_IGEMM_TILE", ft, 3);
    env_ints("AESR_IGEMM_KSPLIT", &fks, 1);
    static PlanCache<std::tuple<int, int, int, int, int, int, int, int, int, int>, ConvPlan> cache;
    return cache.get(std::make_tuple(N, Ho, Wo, Cin, Cout, KS, ft[0], ft[1], ft[2], fks), [&] {
        ConvPlan p;
        cout_padding(Cout, &p.CoutP, &p.NB);
        p.CinP = round_up(Cin, 16);
        p.MBW = (p.NB == 4) ? 2 : 4;                     // M-blocks per wave
        const int ncout = p.CoutP / (16 * p.NB);
        const int NT = 512, NW = NT / 64;
        double best = 1e300;
        p.TI = 1; p.TH = 1; p.TW = 1;
        const int maxpix = 16 * NW * p.MBW;
        // LDS per workgroup: patch (80 B per pixel) + the chunk's weights + bias; 6 staging pieces of 16 B per thread
        const int lds_budget = 160 * 1024 - (KS * KS * 4 * 16 * p.NB * 16 + p.CoutP * 4);
        int maxpatch = lds_budget / 80;
        if (maxpatch > 760) maxpatch = 760;
        auto consider = [&](int TI, int TH, int TW) {
            const int PP = TI * (TH + KS - 1) * (TW + KS - 1);
            const int TP = TI * TH * TW;
            if (TP > maxpix || PP > maxpatch) return;
            const int nblk = ceil_div(TP, 16);
            const long nwg = (long)ceil_div(N, TI) * ceil_div(Ho, TH) * ceil_div(Wo, TW) * ncout;
            // per CU and 16-channel chunk: the MFMA time of a SIMD (2 waves x blocks x NB x taps x 4 k-steps x 32 cycles)
            // plus the staging / barrier phases in which the matrix pipe idles (phase stamps: ~4.5k cycles with one
            // workgroup per CU)
            const double nch = p.CinP / 16;
            const double per = nch * (ceil_div(nblk, NW) * 2.0 * p.NB * KS * KS * 4 * 32 + 4500.0) + 3000.0;
            const double slots = 256.0;
            const double rounds = nwg <= 8 * slots ? (double)ceil_div((int)nwg, (int)slots) : (double)nwg / slots;
            const double t = per * rounds;
            if (t < best * 0.999 || (t < best * 1.001 && TP > p.TI * p.TH * p.TW)) {
                if (t < best) best = t;
                p.TI = TI; p.TH = TH; p.TW = TW;
            }
        };
        if (Ho * Wo <= maxpix && (Ho + KS - 1) * (Wo + KS - 1) <= maxpatch) {
            for (int TI = 1; TI <= N && TI * Ho * Wo <= maxpix; ++TI) consider(TI, Ho, Wo);
        }
        for (int TH = 1; TH <= Ho && TH <= 64; ++TH)
            for (int TW = 1; TW <= Wo && TW <= 64; ++TW) consider(1, TH, TW);
        if (ft[0] || ft[1] || ft[2]) { p.TI = ft[0]; p.TH = ft[1] < Ho ? ft[1] : Ho; p.TW = ft[2] < Wo ? ft[2] : Wo; }
        // K-split for layers whose work items under-fill the 256 persistent workgroups (VGG conv4/5 at 20x20 / 10x10): slices of
        // the input channels become extra work items that write raw partial sums, a fix-up pass adds them (+bias, activation,
        // mask).  Used only when the caller passes a workspace (aesr_conv2d_fwd_ws / _dgrad_ws).
        p.ksplit = 1;
        const long items = (long)ceil_div(N, p.TI) * ceil_div(Ho, p.TH) * ceil_div(Wo, p.TW) * ncout;
        const int nch = p.CinP / 16, nblk = ceil_div(p.TI * p.TH * p.TW, 16);
        const double chunk = ceil_div(nblk, 8) * 2.0 * p.NB * KS * KS * 4 * 32 + 4500.0;
        const double out_bytes = (double)N * Ho * Wo * Cout * 4;
        double bestt = 1e300;
        for (int ks = 1; ks <= 4; ++ks) {
            if (nch % ks != 0 || nch / ks < 4 || (Cout & 3)) continue;
            if (ks > 1 && items * ks > 4 * 256) break;
            const double rounds = (double)ceil_div((int)(items * ks), 256);
            double t = rounds * ((nch / ks) * chunk + 3000.0);
            if (ks > 1) t += (ks + 2) * out_bytes / 2000.0 + 12000.0;        // fix-up traffic at ~4 TB/s + a launch
            if (t < bestt * 0.97) { bestt = t; p.ksplit = ks; }
        }
        if (fks >= 1 && nch % fks == 0) p.ksplit = fks;
        if (getenv("AESR_PLAN_DEBUG"))
            fprintf(stderr, "[aesr plan] conv N=%d %dx%d Cin=%d Cout=%d KS=%d -> NT=%d TI=%d TH=%d TW=%d NB=%d nblk=%d items=%ld ksplit=%d\n", N, Ho,
                    Wo, Cin, Cout, KS, NT, p.TI, p.TH, p.TW, p.NB, nblk, items, p.ksplit);
        return p;
    });
}

// Winograd F(2x2,3x3) work-item shape: TI images x THt x TWt tiles (<= 128 tiles = 8 waves x 16), patch within LDS (two buffers)
// and within 5 staging pieces per thread.  Cost = work-item rounds over the 256 CUs x chunk time; a chunk costs one or two
// wave-passes per SIMD (waves whose 16 tiles are all invalid skip the arithmetic).  AESR_WINO_TILE="TI,THt,TWt" forces the shape.
WinoPlan plan_wino(int N, int H, int W, int Cin, int Cout) {
    int ft[3];
    env_ints("AESR_WINO_TILE", ft, 3);
    static PlanCache<std::tuple<int, int, int, int, int, int, int, int>, WinoPlan> cache;
    return cache.get(std::make_tuple(N, H, W, Cin, Cout, ft[0], ft[1], ft[2]), [&] {
        WinoPlan p;
        p.CinP = round_up(Cin, 16);
        p.CoutP = round_up(Cout, 32);
        const int Ht = ceil_div(H, 2), Wt = ceil_div(W, 2), ncot = p.CoutP / 32, nch = p.CinP / 16;
        p.TI = 1; p.THt = 1; p.TWt = 1; p.cost = 1e300;
        auto consider = [&](int TI, int THt, int TWt) {
            const int TP = TI * THt * TWt, PP = TI * (2 * THt + 2) * (2 * TWt + 2);
            if (TP > 128 || PP * 4 > 512 * 5 || aesr_wino_lds_bytes(PP) > (size_t)160 * 1024) return;
            const long items = (long)ceil_div(N, TI) * ceil_div(Ht, THt) * ceil_div(Wt, TWt) * ncot;
            const double passes = ceil_div(ceil_div(TP, 16), 4);
            const double per = nch * (passes * 128 * 32.0 + 1200.0) + 2500.0;
            const double rounds = items <= 8 * 256 ? (double)ceil_div((int)items, 256) : (double)items / 256.0;
            const double t = per * rounds;
            if (t < p.cost * 0.999 || (t < p.cost * 1.001 && TP > p.TI * p.THt * p.TWt)) {
                if (t < p.cost) p.cost = t;
                p.TI = TI; p.THt = THt; p.TWt = TWt;
            }
        };
        for (int TI = 1; TI <= N && TI * Ht * Wt <= 128; ++TI) consider(TI, Ht, Wt);
        for (int THt = 1; THt <= Ht && THt <= 64; ++THt)
            for (int TWt = 1; TWt <= Wt && TWt <= 64; ++TWt) consider(1, THt, TWt);
        if (ft[0] || ft[1] || ft[2]) { p.TI = ft[0]; p.THt = ft[1] < Ht ? ft[1] : Ht; p.TWt = ft[2] < Wt ? ft[2] : Wt; }
        if (getenv("AESR_PLAN_DEBUG"))
            fprintf(stderr, "[aesr plan] wino N=%d %dx%d Cin=%d Cout=%d -> TI=%d THt=%d TWt=%d (tiles %d, patch %d px) cost %.0f\n", N, H, W, Cin, Cout,
                    p.TI, p.THt, p.TWt, p.TI * p.THt * p.TWt, p.TI * (2 * p.THt + 2) * (2 * p.TWt + 2), p.cost);
        return p;
    });
}

// Winograd F(2x2,3x3) weight gradient (conv_wgrad_wino.hip, variant 2): 3x3 / padding 1 with both channel counts multiples of 32.
// One 4-wave workgroup per CU walks spatial tiles of TH x TW output pixels (TH even, TW a multiple of 8, within the register
// prefetch slots); S splits x (ci, co) chunks ~ 256 workgroups.  AESR_WGRAD_WINO=0 keeps the direct kernels: read once per process.
bool wgrad_wino_ok(int Cin, int Cout, int KS, int pad) {
    static const bool enabled = [] { const char* e = getenv("AESR_WGRAD_WINO"); return !(e && atoi(e) == 0); }();
    return enabled && KS == 3 && pad == 1 && Cin % 32 == 0 && Cout % 32 == 0;
}

// f: AESR_WGRAD_WINO_TILE="TH,TW", AESR_WGRAD_WINO_S and AESR_WGRAD_WINO_SMAX (0: not forced)
static WgradPlan plan_wgrad_wino(int N, int H, int W, int Cin, int Cout, const int* f) {
    WgradPlan p;
    p.variant = 2;
    p.COT = 32;
    p.CinP = Cin;
    p.CoutP = Cout;
    const int nchunks = (Cin / 32) * (Cout / 32);
    int S = 256 / nchunks;
    if (S >= 8) S &= ~7;                       // multiple of 8: XCD-aware workgroup order
    if (S < 1) S = 1;
    double best = 1e300;
    p.TH = 16; p.TW = 8; p.S = S;
    for (int v = 0; v < 2; ++v) {
        const int TH = v ? 8 : 16, TW = v ? 16 : 8;                 // the kernel's two tiles (aesr_wgrad_wino_tile_ok): 8 k-steps, 2 per wave
        const int ntiles = N * ceil_div(H, TH) * ceil_div(W, TW);
        const int s = S < ntiles ? S : ntiles;
        // per visit: 128 MFMAs of a wave (4 096 cycles) + ~270 other instructions, which this chip does not overlap with them
        const double t = (double)ceil_div(ntiles, s) * (4096.0 + 1300.0);
        if (t < best) { best = t; p.TH = TH; p.TW = TW; p.S = s; }
    }
    if (aesr_wgrad_wino_tile_ok(f[0], f[1])) {
        p.TH = f[0]; p.TW = f[1];
        const int ntiles = N * ceil_div(H, p.TH) * ceil_div(W, p.TW);
        p.S = S < ntiles ? S : ntiles;
    }
    if (f[2] > 0) p.S = f[2];
    if (f[3] > 0 && p.S > f[3]) p.S = f[3];        // cap the slab count of every layer (fewer, longer-lived workgroups; fewer slabs to sum)
    p.PWS = round_up(p.TW + 2, 4);             // LDS row strides in pixels (conv_wgrad_wino.hip)
    p.TWS = round_up(p.TW, 4);
    p.PSX = p.PSD = 0;
    p.nslab = p.S;
    p.slab_floats = (size_t)p.nslab * 10 * p.CinP * p.CoutP;
    if (getenv("AESR_PLAN_DEBUG"))
        fprintf(stderr, "[plan_wgrad] wino N=%d %dx%d %d->%d: tile %dx%d S=%d tiles=%d\n", N, H, W, Cin, Cout, p.TH, p.TW, p.S,
                N * ceil_div(H, p.TH) * ceil_div(W, p.TW));
    return p;
}

// Direct weight gradient (conv_wgrad.hip); AESR_WGRAD_TILE="TH,TW" and AESR_WGRAD_S (splits per (ci, co) chunk) force its plan.
WgradPlan plan_wgrad(int N, int Ho, int Wo, int Cin, int Cout, int KS, int pad) {
    const bool wino = wgrad_wino_ok(Cin, Cout, KS, pad);
    int f[4] = {};
    env_ints(wino ? "AESR_WGRAD_WINO_TILE" : "AESR_WGRAD_TILE", f, 2);
    env_ints(wino ? "AESR_WGRAD_WINO_S" : "AESR_WGRAD_S", f + 2, 1);
    if (wino) env_ints("AESR_WGRAD_WINO_SMAX", f + 3, 1);
    static PlanCache<std::tuple<int, int, int, int, int, int, int, int, int, int>, WgradPlan> cache;
    return cache.get(std::make_tuple(N, Ho, Wo, Cin, Cout, wino ? -KS : KS, f[0], f[1], f[2], f[3]), [&] {
        if (wino) return plan_wgrad_wino(N, Ho, Wo, Cin, Cout, f);
        WgradPlan p;
        p.variant = Cout > 32 ? 1 : 0;
        p.COT = p.variant ? 64 : 32;
        const int cibw = p.variant ? 2 : 1;
        p.CinP = round_up(Cin, 32);
        p.CoutP = round_up(Cout, p.COT);
        const size_t max_lds = 52 * 1024;        // three workgroups per CU
        const int nchunks = (p.CinP / 32) * (p.CoutP / p.COT);
        const int S0 = round_up(768 / nchunks > 0 ? 768 / nchunks : 1, 8);      // multiple of 8: XCD-aware workgroup order
        double best = 1e300;
        p.TH = 1; p.TW = 8; p.S = 1;
        for (int TW = 8; TW <= 64; TW += 8) {
            if (TW - 8 >= Wo) break;
            for (int TH = 1; TH <= 32 && TH <= Ho; ++TH) {
                const int PH = TH + KS - 1, PWp = TW + KS - 1, PWS = PWp + (PWp & 1);
                // the kernel prefetches a whole tile into registers: WG_NX / WG_ND float4 slots per thread (conv_wgrad.hip)
                if (PH * PWp * 8 > 256 * (p.variant ? 4 : 6) || TH * TW * (p.COT / 4) > 256 * (p.variant ? 5 : 6)) break;
                const size_t ldsb = ((size_t)32 * plane_stride(PH * PWS) + (size_t)p.COT * plane_stride(TH * TW)) * 4;
                if (ldsb > max_lds) break;
                const int ntiles = N * ceil_div(Ho, TH) * ceil_div(Wo, TW);
                const int S = S0 < ntiles ? S0 : ntiles;
                const double rounds = (double)ceil_div(ntiles, S);
                // three workgroups share a SIMD's matrix pipe; per tile about 4.5k cycles of LDS-write phase, barriers and
                // address work are not hidden (fitted to the phase stamps of AESR_WGRAD_DBG on the layers of the AE)
                const double mf = 3.0 * (TH * TW / 8) * (2 * KS * KS * cibw) * 32.0;
                const double t = rounds * (mf + 4500.0);
                if (t < best) { best = t; p.TH = TH; p.TW = TW; p.S = S; }
            }
        }
        if (f[0] > 0 && f[1] > 0 && f[1] % 8 == 0) {
            p.TH = f[0] < Ho ? f[0] : Ho; p.TW = f[1];
            const int ntiles = N * ceil_div(Ho, p.TH) * ceil_div(Wo, p.TW);
            p.S = S0 < ntiles ? S0 : ntiles;
        }
        const int ntiles = N * ceil_div(Ho, p.TH) * ceil_div(Wo, p.TW);
        if (f[2] > 0) p.S = f[2] < ntiles ? f[2] : ntiles;
        p.PWS = p.TW + KS - 1 + ((p.TW + KS - 1) & 1);
        p.TWS = p.TW;
        p.PSX = plane_stride((p.TH + KS - 1) * p.PWS);
        p.PSD = plane_stride(p.TH * p.TW);
        p.nslab = p.S;
        if (getenv("AESR_PLAN_DEBUG"))
            fprintf(stderr, "[plan_wgrad] N=%d %dx%d %d->%d k%d: tile %dx%d S=%d tiles=%d rounds=%d lds=%zu\n", N, Ho, Wo, Cin, Cout, KS, p.TH,
                    p.TW, p.S, ntiles, ceil_div(ntiles, p.S), ((size_t)32 * p.PSX + (size_t)p.COT * p.PSD) * 4);
        p.slab_floats = (size_t)p.nslab * (KS * KS + 1) * p.CinP * p.CoutP;
        return p;
    });
}
