// The tile code the three Winograd F(2x2, 3x3) forward / data-gradient kernels share (conv_wino.hip, conv_wino_res.hip,
// conv_wino_ring.hip): buffer access, the magic division, the in-register input transform V = B^T d B and the item epilogue
// (output transform, activation, derivative mask, stores).  What differs between the kernels -- how patches and filter chunks
// reach LDS, the order of the MFMA positions, the launchers -- stays with them.
//
// The multi-statement pieces are MACROS, not functions: these kernels sit at 256 registers, and the register allocator's result
// depends on the shape of the code it is handed.  The tile store as a __forceinline__ function template (accumulators by reference)
// spilled 8 registers in every data-gradient instantiation of conv_wino_ring_f32 (0 before) and took the stamped 16-cout
// conv_wino_res_f32 from 196 to 229 registers; as a macro the listings are instruction for instruction those of the three copies
// it replaced (profiles/wino_shared_tile_isa.txt, scripts/isa_same.py).
#pragma once
#include "aesr_common.h"

constexpr int WINO_OOB = 0x70000000;            // byte offset that every buffer descriptor rejects (see conv_igemm.hip)

// global -> LDS without registers: lane l of the wave writes 16 bytes at lds_wave_base + 16 l (lds_wave_base is wave-uniform: M0);
// uniform_off is the instruction's scalar offset
__device__ __forceinline__ void wino_dma(__amdgpu_buffer_rsrc_t rs, float* lds_wave_base, int byte_off, int uniform_off = 0) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, byte_off, uniform_off, 0, 0);
}
__device__ __forceinline__ f32x4 wino_ld(__amdgpu_buffer_rsrc_t rs, int byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 0));
}
// Whatever a caller adds to the address (the ring kernel's slab offset of a channel split) is added to the per-lane offset, NOT
// passed as the instruction's scalar offset.  With an SGPR soffset the compiler (ROCm 7.2 clang) leaves out the wait state between
// "buffer_store_dwordx4 v[128:131], v, s[..], sN offen" and the next VALU instruction that overwrites v[128:131] -- its hazard
// recognizer holds that this store-data hazard "only exists if the instruction is not using a register in the soffset field" --
// and on gfx950 the store then picks up the NEW contents in part of its lanes: odd output channels of tiles 12..15 came out wrong
// (scripts/diag_ring_tail.py; the ISA of the two forms differs by exactly that s_nop).  With soffset = 0 the compiler inserts the
// wait state.
__device__ __forceinline__ void wino_st(__amdgpu_buffer_rsrc_t rs, int byte_off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int, v), rs, byte_off, 0, 0);
}

// divisions by launch constants as multiply-high with the host's magic numbers (x / d == mulhi(x, ceil(2^32 / d)) for
// x * d < 2^32): a runtime integer division costs ~40 instructions, and they sit on item boundaries, where no MFMA overlaps them
#define WINO_DIV(x, m) ((m) ? (int)__umulhi((unsigned)(x), (m)) : (int)(x))          /* m == 0: divisor 1 */

// slope of the branch-free none / ReLU / LeakyReLU form max(x, x * slope); ACT_NONE / ACT_SIGMOID: identity
__device__ __forceinline__ float wino_slope(int act, float slope) { return act == ACT_LRELU ? slope : (act == ACT_RELU ? 0.f : 1.f); }

// ---- input transform of the raw tile f32x4 t[4][4] (a lane's 4 x 4 pixels, 4 channels each) ----
// row half, in place: t = B^T d
#define WINO_ROW_HALF(t)                                                            \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                              \
        const f32x4 d0_ = t[0][j_], d1_ = t[1][j_], d2_ = t[2][j_], d3_ = t[3][j_]; \
        t[0][j_] = aesr_sub4(d0_, d2_);                                             \
        t[1][j_] = d1_ + d2_;                                                       \
        t[2][j_] = aesr_sub4(d2_, d1_);                                             \
        t[3][j_] = aesr_sub4(d1_, d3_);                                             \
    }
// column half, position by position (the kernels compute it one position ahead of the MFMAs that consume it): V[i][j] = (t[i] B)[j]
#define WINO_V(t, i, j) ((j) == 0 ? aesr_sub4(t[i][0], t[i][2]) : (j) == 1 ? t[i][1] + t[i][2] : (j) == 2 ? aesr_sub4(t[i][2], t[i][1]) : aesr_sub4(t[i][1], t[i][3]))

// ---- item epilogue of a lane: output transform Y = A^T M A of its tile, activation, (data gradient) derivative mask, store ----
// The lane holds the 16 positions of ONE Winograd tile = the 2 x 2 outputs at (n, y0, x0), for the 4 output channels
// co0 + nb * 16 + 4 g of each of its NB accumulator sets.  okn: the lane has a tile (false: nothing is read or stored);
// so: byte offset of a channel split's slab, on the plain and the 2x2-summing stores (the POST forms take no split).
// POST: eval-mode BatchNorm (a per-channel affine behind the activation) and the AvgPool2d(2) that follows it -- a lane's 2 x 2
// tile IS one pooling window.  It restates bn_math.h's order of operations (bn_pool2x2, bn_fwd_elem) on its own registers.
// From the enclosing scope: a (WinoArgs), acc[16][NB], rs_out, rs_ys, outH, outW, nslope, mslope, sigm.
#define WINO_STORE_TILE(NB, MASK, POST, okn, n, y0, x0, co0, g, so)                                                                          \
    {                                                                                                                                        \
        int ob[2][2];                                                                                                                        \
        _Pragma("unroll") for (int p = 0; p < 2; ++p)                                                                                        \
            _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                                                    \
                ob[p][q] = ((okn) && (y0) + p < a.H && (x0) + q < a.W) ? (((n) * a.H + (y0) + p) * a.W + (x0) + q) * a.Cout * 4 : WINO_OOB; \
        _Pragma("unroll") for (int nb = 0; nb < (NB); ++nb) {                                                                                \
            const int co = (co0) + nb * 16 + 4 * (g);                                                                                        \
            const int cob = co < a.Cout ? co * 4 : WINO_OOB;                                                                                 \
            f32x4 ys[2][2];                                                                                                                  \
            if (MASK) {                                                                                                                      \
                _Pragma("unroll") for (int p = 0; p < 2; ++p)                                                                                \
                    _Pragma("unroll") for (int q = 0; q < 2; ++q) ys[p][q] = wino_ld(rs_ys, ob[p][q] + cob);                                 \
            }                                                                                                                                \
            f32x4 P[2][4];                                                                                                                   \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                                  \
                P[0][j] = acc[0 + j][nb] + acc[4 + j][nb] + acc[8 + j][nb];                                                                  \
                P[1][j] = aesr_sub4(aesr_sub4(acc[4 + j][nb], acc[8 + j][nb]), acc[12 + j][nb]);                                             \
            }                                                                                                                                \
            if (a.out_sum2) {                                                                                                                \
                /* adjoint of the nearest Upsample(x2) in front of this layer's forward: the 2x2 tile collapses to one pixel (the sum */    \
                /* of A^T M A over its four entries = the corner combination below); no activation, no mask */                              \
                const f32x4 s = aesr_sub4((P[0][0] + P[1][0]) + 2.f * (P[0][1] + P[1][1]), P[0][3] + P[1][3]);                               \
                const int obs = ((okn) && (y0) < a.H && (x0) < a.W) ? (((n) * outH + ((y0) >> 1)) * outW + ((x0) >> 1)) * a.Cout * 4 : WINO_OOB; \
                wino_st(rs_out, obs + cob + (so), s);                                                                                        \
                continue;                                                                                                                    \
            }                                                                                                                                \
            f32x4 psc = {1.f, 1.f, 1.f, 1.f}, psh = {0.f, 0.f, 0.f, 0.f}, prow = psh, pm = psh; /* pooled: row sums as they come (8 registers, not 16) */ \
            if ((POST) && co < a.Cout) {                                                                                                     \
                psc = *(const f32x4*)(a.post_scale + co);                                                                                    \
                psh = *(const f32x4*)(a.post_shift + co);                                                                                    \
            }                                                                                                                                \
            _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                                                                  \
                f32x4 Y[2];                                                                                                                  \
                Y[0] = P[p][0] + P[p][1] + P[p][2];                                                                                          \
                Y[1] = aesr_sub4(aesr_sub4(P[p][1], P[p][2]), P[p][3]);                                                                      \
                _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                                              \
                    f32x4 o = Y[q];                                                                                                          \
                    /* none / ReLU / LeakyReLU as ONE branch-free form, max(x, x * slope) for 0 <= slope <= 1; a per-element switch on */    \
                    /* the activation code costs a chain of uniform branches per element (~1000 instructions per item) */                   \
                    const f32x4 os = o * nslope;                                                                                             \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], os[e]);                                                 \
                    if (sigm) {                                                                                                              \
                        _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = 1.f / (1.f + expf(-o[e]));                                      \
                    }                                                                                                                        \
                    if (MASK) {                                                                                                              \
                        _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] *= (ys[p][q][e] > 0.f ? 1.f : mslope);                            \
                    }                                                                                                                        \
                    if (POST) {                                                                                                              \
                        if (a.post_pool) prow = q == 0 ? o : prow + o;                                                                       \
                        else wino_st(rs_out, ob[p][q] + cob, o * psc + psh); /* bn.hip bn_apply: v * scale + shift */                        \
                    } else {                                                                                                                 \
                        wino_st(rs_out, ob[p][q] + cob + (so), o);                                                                           \
                    }                                                                                                                        \
                }                                                                                                                            \
                if ((POST) && a.post_pool) pm = p == 0 ? prow : pm + prow;                                                                   \
            }                                                                                                                                \
            if ((POST) && a.post_pool) {                                                                                                     \
                /* AvgPool2d(2) of the activated tile, then the affine: the arithmetic and order of bn.hip's bn_apply (pooling mode); */     \
                /* a window that sticks out of an odd image has no output (floor) */                                                        \
                const f32x4 m = pm * 0.25f; /* ((o00 + o01) + (o10 + o11)) * 0.25 */                                                         \
                const int obs = ((okn) && (y0) + 1 < a.H && (x0) + 1 < a.W) ? (((n) * outH + ((y0) >> 1)) * outW + ((x0) >> 1)) * a.Cout * 4 : WINO_OOB; \
                wino_st(rs_out, obs + cob, m * psc + psh);                                                                                   \
            }                                                                                                                                \
        }                                                                                                                                    \
    }

// The same epilogue where only the positions 4 i + j with i, j in {0, 1, 3} exist (conv_wino_res.hip, NINE: the layers behind a folded
// Upsample(x2); no mask, no POST).  A macro of its own, so that the expansion above stays what it is.
//  * plain stores (in_up2 forward): the missing accumulators are exact +0 in the 16-position form, and this is WINO_STORE_TILE's
//    expression tree with those terms left out: P[0][j] = acc[j] + acc[4 + j] (+ 0), P[1][j] = (acc[4 + j] - 0) - acc[12 + j],
//    Y[0] = P[p][0] + P[p][1] (+ 0), Y[1] = (P[p][1] - 0) - P[p][3] -- the same bits.
//  * out_sum2: s = 1^T A^T M A 1 with 1^T A^T = [1, 2, 0, -1]:  Q[j] = (acc[j] + 2 acc[4 + j]) - acc[12 + j] for j in {0, 1, 3},
//    s = (Q[0] + 2 Q[1]) - Q[3].  Row 2 and column 2 of M have weight 0 (WINO_STORE_TILE adds and subtracts them): equal in exact
//    arithmetic, rounded differently.
#define WINO_STORE_TILE9(NB, okn, n, y0, x0, co0, g, so)                                                                                     \
    {                                                                                                                                        \
        int ob[2][2];                                                                                                                        \
        _Pragma("unroll") for (int p = 0; p < 2; ++p)                                                                                        \
            _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                                                    \
                ob[p][q] = ((okn) && (y0) + p < a.H && (x0) + q < a.W) ? (((n) * a.H + (y0) + p) * a.W + (x0) + q) * a.Cout * 4 : WINO_OOB; \
        _Pragma("unroll") for (int nb = 0; nb < (NB); ++nb) {                                                                                \
            const int co = (co0) + nb * 16 + 4 * (g);                                                                                        \
            const int cob = co < a.Cout ? co * 4 : WINO_OOB;                                                                                 \
            if (a.out_sum2) {                                                                                                                \
                const f32x4 Q0 = aesr_sub4(acc[0][nb] + 2.f * acc[4][nb], acc[12][nb]);                                                      \
                const f32x4 Q1 = aesr_sub4(acc[1][nb] + 2.f * acc[5][nb], acc[13][nb]);                                                      \
                const f32x4 Q3 = aesr_sub4(acc[3][nb] + 2.f * acc[7][nb], acc[15][nb]);                                                      \
                const f32x4 s = aesr_sub4(Q0 + 2.f * Q1, Q3);                                                                                \
                const int obs = ((okn) && (y0) < a.H && (x0) < a.W) ? (((n) * outH + ((y0) >> 1)) * outW + ((x0) >> 1)) * a.Cout * 4 : WINO_OOB; \
                wino_st(rs_out, obs + cob + (so), s);                                                                                        \
                continue;                                                                                                                    \
            }                                                                                                                                \
            f32x4 P[2][4];                                                                                                                   \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                                  \
                if (j == 2) continue;                                                                                                        \
                P[0][j] = acc[0 + j][nb] + acc[4 + j][nb];                                                                                   \
                P[1][j] = aesr_sub4(acc[4 + j][nb], acc[12 + j][nb]);                                                                        \
            }                                                                                                                                \
            _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                                                                  \
                f32x4 Y[2];                                                                                                                  \
                Y[0] = P[p][0] + P[p][1];                                                                                                    \
                Y[1] = aesr_sub4(P[p][1], P[p][3]);                                                                                          \
                _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                                              \
                    f32x4 o = Y[q];                                                                                                          \
                    const f32x4 os = o * nslope;                                                                                             \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], os[e]);                                                 \
                    if (sigm) {                                                                                                              \
                        _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = 1.f / (1.f + expf(-o[e]));                                      \
                    }                                                                                                                        \
                    wino_st(rs_out, ob[p][q] + cob + (so), o);                                                                               \
                }                                                                                                                            \
            }                                                                                                                                \
        }                                                                                                                                    \
    }
