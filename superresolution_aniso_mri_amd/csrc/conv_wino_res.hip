// Winograd F(2x2, 3x3) convolution for layers with FEW input channels (Cin <= 64): the transformed filter stays resident in LDS
// and every wave runs on its own -- no barrier after the prologue.
//
// The general kernel (conv_wino.hip) streams 16-channel chunks of patch + U through LDS for an 8-wave work item and meets at a
// barrier per chunk.  With Cin = 32 an item is only 2 chunks long, so the item epilogue (output transform, activation, stores,
// re-zeroing 128 accumulators, the next item's address work) -- during which all 8 waves leave the matrix pipe idle TOGETHER --
// was 30 % of the kernel (AESR_WINO_DBG stamps: 7.9 k of 27 k cycles per item), and on gfx950 the f32 MFMA shares its pipe with the
// vector ALU (scripts/micro/mfma_gap.hip), so nothing hides inside a wave either.  Here:
//  * all of U for the workgroup's output channels (64 KB: 32 couts x <= 32 input channels, or 16 couts x <= 64) is loaded ONCE per
//    workgroup; workgroup b serves the cout tile b % ncot for its whole life;
//  * a work item belongs to ONE wave: 4 x 4 Winograd tiles (8 x 8 outputs) x 32 output channels, the same 128 accumulators per
//    wave as in conv_wino.hip.  The wave fetches its own 10 x 10-pixel patch by DMA (buffer_load ... lds, one instruction per
//    patch row of 16 pixel slots, 4 instructions of address work each) into its own 10 KB of LDS and waits only on its own
//    vmcnt: the patch buffer is free again as soon as its 16 ds_read_b128 have returned (the raw tile lives in registers while
//    it is transformed), so the NEXT chunk's patch is requested before this chunk's 128 MFMAs start -- single buffered, a whole
//    chunk of matrix work ahead;
//  * the two waves of a SIMD drift apart (the older one is served first), so one's epilogue, stores and mask loads run beside
//    the other's MFMAs without any scheduling effort;
//  * patch rows are pitched 1040 B and the DMA source swaps channel quads q <-> q ^ 1 in pixels 4..7 and 12..15 of a row: the
//    16 lanes of a ds_read_b128 phase (16 tiles, one channel quad) then hit 16 different 16-byte bank groups -- conflict free
//    (conv_wino.hip pays 4-way conflicts for its register-free DMA).
// Everything else (U packing, the per-lane transforms, the bias in the accumulator of position (1,1), the derivative mask, the
// folded Upsample in both directions) is conv_wino.hip's; results are bit-identical in exact arithmetic and equal to rounding.
//
// Replaces the ATen/cuDNN conv2d calls behind networks/acai_vanilla.py:55-56,87-88,96 (the 32-channel layers) forward and as
// data gradient.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

#include "aesr_kernels.h"
#include "conv_wino_tile.h"

constexpr int WR_NT = 512;          // threads per workgroup: 8 independent waves, 2 per SIMD
// TN = output channels of a workgroup: 32 (K side <= 32 channels: <= 64 KB of filter) or 16 (K side <= 64 channels: 64 KB)
constexpr int WR_RP = 260;          // floats between patch rows: 16 pixel slots x 16 channels + 4 (shifts a row by one 16-byte bank group)
constexpr int WR_PFL = 10 * WR_RP;  // floats of a wave's patch buffer (10 rows)

// the k-th position that is computed: all 16, or (NINE) the nine 4 i + j with i, j in {0, 1, 3}
template <bool NINE>
__host__ __device__ constexpr int wr_xi(int k) { return NINE ? 4 * (k / 3 == 2 ? 3 : k / 3) + (k % 3 == 2 ? 3 : k % 3) : k; }

// POST: eval-mode BatchNorm (a per-channel affine behind the activation) and the AvgPool2d(2) that follows it, in the epilogue -- a lane
// holds one 2 x 2 output tile, which IS one pooling window; an instantiation of its own, so that the training kernels' code is untouched
// STAMP (debug, AESR_WINO_RES_DBG=1): wall-clock stamps (s_memrealtime, 10 ns) of the phases of every wave's FIRST item -> a.dbgbuf as
// [workgroup][wave][16] 64-bit ticks: 0 entry, 1 DMAs of the prologue issued, 2 behind the prologue barrier, 3 + 2 c patch of chunk c landed,
// 4 + 2 c MFMAs of chunk c issued (c < 4), 11 stores of the item issued, 12 exit, 13 items of the wave
// NINE (the layers behind a nearest Upsample(x2): in_up2 forward, out_sum2 data gradient; AESR_WINO_UP2_NINE=0 selects the 16-position
// instantiation): only the positions xi = 4 i + j with i, j in {0, 1, 3} are computed -- 9 U reads, 9 column transforms, 36 NB MFMAs per
// chunk instead of 64 NB.
//  * in_up2: a tile starts at an even pixel, so its patch rows (2k-1, 2k, 2k+1, 2k+2) are the stored rows (k-1, k, k, k+1): rows 1 and 2
//    are the same numbers (at every border too: H and W are even), and so are columns 1 and 2.  Row 2 of B^T is d2 - d1: V[2][.] and
//    V[.][2] are exactly +0, M = sum U V there is +0 (an accumulator that starts from +0 never becomes -0), and the output transform
//    without those 7 terms gives every bit it gave with them (x + 0 == x unless x is -0, and no partial sum below can be: each has an
//    operand that started from +0; x - 0 == x always).
//  * out_sum2: the stored value is the SUM of the tile's 2 x 2 outputs, 1^T A^T M A 1 with 1^T A^T = [1, 2, 0, -1]: row 2 and column 2
//    of M carry weight 0.  The 16-position form adds and subtracts them (they cancel in exact arithmetic only); without them dx moves
//    by rounding, towards the exact value.
template <int WR_TN, bool MASK, bool POST = false, bool STAMP = false, bool NINE = false>
__global__ __launch_bounds__(WR_NT, 2) void conv_wino_res_f32(WinoArgs a) {
    static_assert(!NINE || (!MASK && !POST && !STAMP), "the nine-position form: plain forward / 2x2-summing data gradient only");
    constexpr int WR_NB = WR_TN / 16;
    constexpr int NPOS = NINE ? 9 : 16;             // positions computed; the k-th of them is wr_xi<NINE>(k)
    constexpr int WR_WFL = 16 * 4 * WR_TN * 4;      // floats of one U chunk (16 positions x 16 ci x TN co)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned long long stamp[14] = {};
    int stamped_items = 0;
#define WR_STAMP(k)                                                          \
    if constexpr (STAMP) {                                                   \
        if (stamped_items == 0) stamp[k] = __builtin_amdgcn_s_memrealtime(); \
    }
    WR_STAMP(0)
    const int l15 = lane & 15, g = lane >> 4;
    const int ncot = a.CoutP / WR_TN, nchunks = a.CinP >> 4;
    // Workgroup -> (cout tile, spatial worker).  Workgroups b and b + 8 share an XCD (round-robin placement: speed only, never
    // correctness): where the grid allows, XCD x takes a CONTIGUOUS run of blocks per round and all cout tiles of a block sit on it,
    // so the 10 x 10 patches of neighbouring blocks (1.56 x the image) and the re-reads by the other cout tiles hit that XCD's L2
    // instead of crossing the fabric (round 2 PMC: 2.4 x the algorithmic bytes read).  Otherwise: cout tile = b % ncot as before.
    const bool xmap = a.xcd_map != 0;
    const int xcd = blockIdx.x & 7, lw = blockIdx.x >> 3;
    const int cot = xmap ? lw % ncot : blockIdx.x % ncot;
    const int wgc = xmap ? lw / ncot : blockIdx.x / ncot;               // spatial worker (inside the XCD / of the grid)
    const int nwgc = xmap ? (gridDim.x >> 3) / ncot : gridDim.x / ncot;
    const int co0 = cot * WR_TN;
    float* const ldsW = lds;                                        // [nchunks][16 positions][4][32][4]
    float* const ldsP = lds + nchunks * WR_WFL + wave * WR_PFL;     // this wave's patch: [10 rows][16 pixel slots][16 ch] (+ pitch)
    float* const ldsBias = lds + nchunks * WR_WFL + 8 * WR_PFL;     // [32]

    const int sh = a.in_up2 ? 1 : 0;
    const int inH = a.H >> sh, inW = a.W >> sh;                                              // stored size of the input tensor
    const bool halfout = a.out_sum2 || (POST && a.post_pool);
    const int outH = halfout ? a.H >> 1 : a.H, outW = halfout ? a.W >> 1 : a.W;              // stored size of the output tensor
    const int inimg = inH * inW * a.Cin * 4, inrow = inW * a.Cin * 4;                        // bytes of an input image / row
    // (sizes through readfirstlane: a 64-bit product lands in vector registers, and a resource there costs a waterfall loop per access)
    const int wbytes = __builtin_amdgcn_readfirstlane(16 * a.CinP * a.CoutP * 4);
    const int obytes = __builtin_amdgcn_readfirstlane(a.N * outH * outW * a.Cout * 4), ybytes = __builtin_amdgcn_readfirstlane(a.N * a.H * a.W * a.Cout * 4);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)a.upk, 0, wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void*)a.out, 0, obytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_ys = __builtin_amdgcn_make_buffer_rsrc((void*)(MASK ? a.ysave : a.out), 0, ybytes, 0x00020000);

    // ---- prologue: the workgroup's U block(s) and bias, once ----
    // (the bias is only REQUESTED here: parked in LDS behind the DMA issue below -- written first, its global round trip (~1 us on a cold
    // line) stood in front of every DMA of the launch: stamps of profiles/r04_small_shard_budget.txt, section 11)
    float bias_v = 0.f;
    if (tid < WR_TN && a.bias && co0 + tid < a.Cout) bias_v = a.bias[co0 + tid];
    // packed layout [chunk][32-cout tile][position][ci / 4][32 couts][4]: a 16-cout workgroup takes one half of every 32-cout row
    auto filter_chunk = [&](int cc) {
        const int wbase = (int)(((size_t)cc * (a.CoutP / 32) + (co0 >> 5)) * (8192 * 4)) + ((co0 >> 4) & 1) * (WR_TN == 16 ? 256 : 0);
#pragma unroll
        for (int j = 0; j < WR_WFL / 4 / WR_NT; ++j) {
            const int pc = tid + WR_NT * j;                        // 16-byte piece -> (row of TN couts x 4, piece in the row)
            wino_dma(rs_w, ldsW + cc * WR_WFL + j * (WR_NT * 4) + wave * 256, wbase + ((pc / WR_TN) * 128 + (pc % WR_TN) * 4) * 4);
        }
    };
    for (int cc = 0; cc < nchunks; ++cc) filter_chunk(cc);

    // ---- per-lane maps ----
    // DMA: lane -> pixel slot lane >> 2 of a patch row, channel quad (lane & 3) ^ ((slot >> 2) & 1)
    const int dpx = lane >> 2, dq = (lane & 3) ^ ((dpx >> 2) & 1);
    const int lcd = (((dpx - sh) >> sh) * a.Cin + 4 * dq) * 4;          // bytes from (row start + item column origin); arithmetic shift: -1 stays -1
    // MFMA B operand: lane -> tile l15 = (ty, tx) of the 4 x 4 block, channel quad g; patch pixel (2 ty + i, 2 tx + j)
    const int ty = l15 >> 2, tx = l15 & 3;
    const int offA = (2 * ty) * WR_RP + (2 * tx) * 16 + ((g ^ (tx >> 1)) << 2);                  // columns j = 0, 1
    const int offB = (2 * ty) * WR_RP + (2 * tx) * 16 + ((g ^ (((2 * tx + 2) >> 2) & 1)) << 2);  // columns j = 2, 3
    const float* wbl = ldsW + (g * WR_TN + l15) * 4;                    // + chunk * WFL + xi * 512 + nb * 64

    const float mslope = wino_slope(a.mask_act, a.slope), nslope = wino_slope(a.act, a.slope);
    const bool sigm = a.act == ACT_SIGMOID;

    // item k of this wave: block wgc + nwgc * (wave + 8 k) of the N x BY x BX blocks of 8 x 8 outputs (a partial last round lands on
    // wave 0 of many workgroups, not on all waves of a few)
    // XCD map: round k, XCD x = blocks [(8 k + x) * 8 nwgc, + 8 nwgc), wave w of worker s takes block w * nwgc + s of them
    // The workgroup's items in the order they are dealt: slot j -> block; wave w takes slots w, w + 8, ...  The two waves of a SIMD do NOT progress
    // alike -- the older one (waves 0..3) is served first and ran its equally long list in 74 us where waves 4..7 took 90 (stamps of 32 -> 32 @
    // 162 x 162 x 36, profiles/r05_res_wave_exit.txt) -- but dealing the slots through an LDS counter (a wave takes the next undealt slot
    // when it finishes an item: profiles/EXPERIMENTS.md) bought only 1 % there and cost 1 % on small layers: the SIMD finishes items at one
    // rate whichever wave owns them; the younger wave simply runs faster once it is alone.  Slots are monotonic in the block index, so the
    // first slot past the end ends a wave.
    auto item_of = [&](int j) { return xmap ? xcd * (8 * nwgc) + wgc + nwgc * (j & 7) + 64 * nwgc * (j >> 3) : wgc + nwgc * j; };
    int item = item_of(wave);
    int slot = wave;
    // the patch of (item, chunk) -> this wave's LDS buffer: 10 DMAs; out-of-range rows / columns deliver zeros
    int in_n = 0, in_y0 = 0, in_x0 = 0;
    auto locate = [&](int it) {
        in_n = WINO_DIV(it, a.m_bpi);
        const int rem = it - in_n * a.bpi;
        const int by = WINO_DIV(rem, a.m_regs_x);
        in_y0 = by * 8;
        in_x0 = (rem - by * a.regs_x) * 8;
    };
    auto fetch = [&](int, int cc) {
        const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.in + (size_t)in_n * inimg), 0, inimg, 0x00020000);
        const unsigned gx = (unsigned)(in_x0 - 1 + dpx);
        const int off = (dpx < 10 && gx < (unsigned)a.W && cc * 16 + 4 * dq < a.Cin) ? lcd + ((in_x0 >> sh) - 1 + sh) * a.Cin * 4 + cc * 64 : WINO_OOB;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const int urow = ((in_y0 - 1 + r) >> sh) * inrow;           // row -1 stays -1: outside the image's resource
            wino_dma(rs_in, ldsP + r * WR_RP, off + urow);
        }
    };
    if (item < a.nblk) {
        locate(item);
        fetch(item, 0);
    }
    WR_STAMP(1)
    if (tid < WR_TN) ldsBias[tid] = bias_v;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // explicit: this wave's share of the filter DMAs has landed before it arrives
    __syncthreads();            // U and bias are in LDS (every wave waited for its own part)
    WR_STAMP(2)

    f32x4 acc[16][WR_NB];
    int cc = 0;
    bool after_stores = false;
    while (item < a.nblk) {
        // ---- the 4x4 input pixels of this lane's tile, 4 channels each ----
        // the DMAs of this patch are the oldest outstanding memory operations; the previous item's stores may still be in flight
        if (after_stores) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * WR_NB) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (STAMP) {
            if (stamped_items == 0 && cc < 4) stamp[3 + 2 * cc] = __builtin_amdgcn_s_memrealtime();
        }
        f32x4 t[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) t[i][j] = *(const f32x4*)(ldsP + (j < 2 ? offA : offB) + i * WR_RP + j * 16);
        const float* wb = wbl + cc * WR_WFL;
        // PP positions per MFMA group: with ONE accumulator register set per position (16-cout workgroups) the four MFMAs of a position
        // form a dependent chain -- 40 cycles each instead of the 32 of independent ones -- so two positions are interleaved there
        // (three of the nine: an odd count leaves no lone chain behind)
        constexpr int PP = (WR_NB == 1) ? (NINE ? 3 : 2) : 1;
        f32x4 wnx[PP][WR_NB];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
#pragma unroll
            for (int nb = 0; nb < WR_NB; ++nb) wnx[pp][nb] = *(const f32x4*)(wb + wr_xi<NINE>(pp) * (4 * WR_TN * 4) + nb * 64);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // the patch is in registers: request the next one (next chunk, or chunk 0 of the next item) into the same buffer
        const int cur_n = in_n, cur_y0 = in_y0, cur_x0 = in_x0;
        const bool last = cc + 1 == nchunks;
        if (last) {
            slot += 8;
            item = item_of(slot);
            if (item < a.nblk) {
                locate(item);
                fetch(item, 0);
            }
        } else {
            fetch(item, cc + 1);
        }
        // row half of the transform (B^T d); NINE: nothing reads t[2][.], and the compiler drops its subtractions
        WINO_ROW_HALF(t)
        // column half, one position ahead of the MFMAs that consume it: V[i][j] = (t[i] B)[j].  In the FIRST chunk of an item the
        // MFMA of each accumulator's first use takes 0 (the bias in position (1,1)) as its C operand: nothing is zeroed between items
        auto positions = [&](auto firstc) {
            constexpr bool FIRST = decltype(firstc)::value;
            f32x4 vnx[PP];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) vnx[pp] = WINO_V(t, wr_xi<NINE>(pp) >> 2, wr_xi<NINE>(pp) & 3);
#pragma unroll
            for (int grp = 0; grp < NPOS / PP; ++grp) {
                f32x4 wc[PP][WR_NB], vc[PP];
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) {
                    vc[pp] = vnx[pp];
#pragma unroll
                    for (int nb = 0; nb < WR_NB; ++nb) wc[pp][nb] = wnx[pp][nb];
                }
                if (grp + 1 < NPOS / PP) {
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp) {
                        const int xn = wr_xi<NINE>((grp + 1) * PP + pp);
#pragma unroll
                        for (int nb = 0; nb < WR_NB; ++nb) wnx[pp][nb] = *(const f32x4*)(wb + xn * (4 * WR_TN * 4) + nb * 64);
                        vnx[pp] = WINO_V(t, xn >> 2, xn & 3);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp)
#pragma unroll
                        for (int nb = 0; nb < WR_NB; ++nb) {
                            const int xi = wr_xi<NINE>(grp * PP + pp);
                            f32x4 c = acc[xi][nb];
                            if (FIRST && r == 0) c = xi == 5 ? *(const f32x4*)(ldsBias + nb * 16 + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
                            acc[xi][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[pp][nb][r], vc[pp][r], c, 0, 0, 0);
                        }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (cc == 0) positions(std::true_type{});
        else positions(std::false_type{});
        if constexpr (STAMP) {
            if (stamped_items == 0 && cc < 4) stamp[4 + 2 * cc] = __builtin_amdgcn_s_memrealtime();
        }
        after_stores = false;
        if (!last) {
            ++cc;
            continue;
        }
        cc = 0;
        // ---- item finished: output transform Y = A^T M A, activation, (data gradient) derivative mask, store ----------
        {
            const int y0 = cur_y0 + 2 * ty, x0 = cur_x0 + 2 * tx;
            if constexpr (NINE) {
                WINO_STORE_TILE9(WR_NB, true, cur_n, y0, x0, co0, g, 0)
            } else {
                WINO_STORE_TILE(WR_NB, MASK, POST, true, cur_n, y0, x0, co0, g, 0)
            }
        }
        after_stores = !MASK && !halfout;           // exactly 4 NB stores follow the next patch's DMAs
        WR_STAMP(11)
        if constexpr (STAMP) ++stamped_items;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // no DMA may still be writing this workgroup's LDS when it is released
    if constexpr (STAMP) {
        stamp[12] = __builtin_amdgcn_s_memrealtime();
        stamp[13] = (unsigned long long)stamped_items;
        if (lane == 0) {
            unsigned long long* dst = (unsigned long long*)a.dbgbuf + ((size_t)blockIdx.x * 8 + wave) * 16;
#pragma unroll
            for (int k = 0; k < 14; ++k) dst[k] = stamp[k];
        }
    }
#undef WR_STAMP
}

// Output channels per workgroup.  64 K-side channels only fit with 16; with <= 32 both do, and the choice is about balance: a
// 16-cout work item is 0.55 of a 32-cout one (half the MFMAs, the same transforms), so it wins when it saves rounds of
// items over the 2 048 waves -- at 6 images of 160 x 160: 2 400 items = 2 rounds, or 4 800 half items = 3 x 0.55 = 1.65
static int wino_res_tn(const WinoArgs& a) {
    if (a.CinP > 32) return 16;
    static const int forced = getenv("AESR_WINO_RES_TN") ? atoi(getenv("AESR_WINO_RES_TN")) : 0;
    if (forced == 16 || forced == 32) return forced;
    const long nblk = (long)a.N * ceil_div(a.H, 8) * ceil_div(a.W, 8);
    const double c32 = (double)((nblk * (a.CoutP / 32) + 2047) / 2048), c16 = 0.55 * (double)((nblk * (a.CoutP / 16) + 2047) / 2048);
    return c16 < c32 ? 16 : 32;
}
// (the 4 floats behind the bias are spare: once an item counter; kept so that a launch asks for the LDS size it was measured with)
static size_t wino_res_lds_bytes(int CinP, int TN) { return ((size_t)(CinP >> 4) * (256 * TN) + 8 * WR_PFL + 32 + 4) * sizeof(float); }

bool aesr_wino_res_ok(const WinoArgs& a) {
    // AESR_WINO_RES: 0 = never, 1 = K side <= 32 channels only, unset / 2 = up to 64 channels (16-cout workgroups)
    static const int level = getenv("AESR_WINO_RES") ? atoi(getenv("AESR_WINO_RES")) : 2;
    if (level <= 0 || a.CinP % 16 != 0 || a.CoutP % 32 != 0 || a.CoutP / 16 > 256) return false;
    if (a.CinP <= 32) return true;
    // 16-cout workgroups pay twice the transform work per MFMA: worth it only where the 8 x 8-output blocks tile the image with
    // little waste (measured: 40 x 40 and 80 x 80 layers 5-13 % faster than the streamed kernel, 81 x 81 (+18 % padding) 5 % slower)
    const double waste = (double)(ceil_div(a.H, 8) * 8) * (ceil_div(a.W, 8) * 8) / ((double)a.H * a.W);
    return level >= 2 && a.CinP <= 64 && waste <= 1.10;
}

// debug launch (AESR_WINO_RES_DBG=1, forward without mask): the stamped instantiation, then a host sync and ONE line on stderr -- where the
// time of a launch goes for the waves that had work (profiles/r04_small_shard_budget.txt, section 11)
template <int WR_TN>
static int wino_res_stamped(const WinoArgs& b_in, int grid, size_t shmem, hipStream_t st) {
    static unsigned long long* dbuf = nullptr;
    static std::vector<unsigned long long> host;
    const size_t n = (size_t)grid * 8 * 16;
    if (grid > 1024) return AESR_ERR_ARG;
    if (!dbuf && hipMalloc(&dbuf, (size_t)1024 * 8 * 16 * sizeof(unsigned long long)) != hipSuccess) return AESR_ERR_HIP;
    (void)hipFuncSetAttribute((const void*)conv_wino_res_f32<WR_TN, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    WinoArgs b = b_in;
    b.dbgbuf = (float*)dbuf;
    (void)hipMemsetAsync(dbuf, 0, n * sizeof(unsigned long long), st);
    hipLaunchKernelGGL((conv_wino_res_f32<WR_TN, false, false, true>), dim3(grid), dim3(WR_NT), shmem, st, b);
    AESR_LAUNCH_CHECK("conv_wino_res_f32 (stamped)");
    (void)hipStreamSynchronize(st);
    host.resize(n);
    (void)hipMemcpy(host.data(), dbuf, n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    unsigned long long t_first = ~0ull, t_last = 0;
    for (size_t w = 0; w < (size_t)grid * 8; ++w) {
        const unsigned long long* s_ = &host[w * 16];
        if (s_[0] && s_[0] < t_first) t_first = s_[0];
        if (s_[12] > t_last) t_last = s_[12];
    }
    const int nch = b.CinP / 16 < 4 ? b.CinP / 16 : 4;
    double sum[16] = {}, ramp_max = 0;
    int busy = 0, items = 0;
    for (size_t w = 0; w < (size_t)grid * 8; ++w) {
        const unsigned long long* s_ = &host[w * 16];
        if (!s_[13]) continue;
        ++busy;
        items += (int)s_[13];
        const double ramp = (double)(s_[0] - t_first);
        if (ramp > ramp_max) ramp_max = ramp;
        sum[0] += ramp;                                     // entry behind the first wave of the grid
        sum[1] += (double)(s_[1] - s_[0]);                  // address work + issue of the filter and first-patch DMAs
        sum[2] += (double)(s_[2] - s_[1]);                  // wait for them + the barrier
        unsigned long long prev = s_[2];
        for (int c = 0; c < nch; ++c) {
            sum[3 + 2 * c] += (double)(s_[3 + 2 * c] - prev);               // wait for the patch of chunk c
            sum[4 + 2 * c] += (double)(s_[4 + 2 * c] - s_[3 + 2 * c]);      // LDS reads, next DMAs, transform, MFMAs of chunk c
            prev = s_[4 + 2 * c];
        }
        sum[11] += (double)(s_[11] - prev);                 // output transform, activation, stores issued
        sum[12] += (double)(s_[12] - s_[11]);               // further items of the wave + drain of the stores
    }
    const double q = busy ? 0.01 / busy : 0.0;              // ticks of 10 ns -> us per busy wave
    fprintf(stderr, "[wino-res stamps] %d->%d N=%d %dx%d TN=%d grid=%d: %d of %d waves busy, %d items | span %.2f us | per busy wave (first item), us: "
            "entry behind first wave %.2f (max %.2f) | DMA issue %.2f | prologue wait+barrier %.2f |", b.Cin, b.Cout, b.N, b.H, b.W, WR_TN, grid, busy,
            grid * 8, items, (double)(t_last - t_first) * 0.01, sum[0] * q, ramp_max * 0.01, sum[1] * q, sum[2] * q);
    for (int c = 0; c < nch; ++c) fprintf(stderr, " chunk %d: wait %.2f work %.2f |", c, sum[3 + 2 * c] * q, sum[4 + 2 * c] * q);
    fprintf(stderr, " epilogue %.2f | rest of the wave %.2f\n", sum[11] * q, sum[12] * q);
    // do the eight waves of a workgroup (wave w and w + 4 share a SIMD) finish their -- equally long -- item lists at the same time?
    double ex[8] = {}, ex_min[8], ex_max[8] = {};
    int nw[8] = {};
    for (int w = 0; w < 8; ++w) ex_min[w] = 1e30;
    for (size_t w = 0; w < (size_t)grid * 8; ++w) {
        const unsigned long long* s_ = &host[w * 16];
        if (!s_[13]) continue;
        const double e = (double)(s_[12] - t_first) * 0.01;
        const int k = (int)(w & 7);
        ex[k] += e; ++nw[k];
        if (e < ex_min[k]) ex_min[k] = e;
        if (e > ex_max[k]) ex_max[k] = e;
    }
    fprintf(stderr, "[wino-res stamps] exit of wave w behind the grid's first entry, us (mean [min .. max] over the workgroups):");
    for (int w = 0; w < 8; ++w)
        if (nw[w]) fprintf(stderr, "  w%d %.1f [%.1f .. %.1f]", w, ex[w] / nw[w], ex_min[w], ex_max[w]);
    fprintf(stderr, "\n");
    return AESR_OK;
}

template <int WR_TN, bool MASK, bool POST = false, bool NINE = false>
static int wino_res_launch_one(const WinoArgs& a, hipStream_t st) {
    const size_t shmem = wino_res_lds_bytes(a.CinP, WR_TN);
    static bool attr_set[AESR_MAX_DEVICES] = {};
    if (int e = aesr_lds_opt_in((const void*)conv_wino_res_f32<WR_TN, MASK, POST, false, NINE>, "conv_wino_res_f32", attr_set)) return e;
    const int ncot = a.CoutP / WR_TN;
    int grid = 256 / ncot * ncot;                          // one workgroup per CU, a whole number of them per cout tile
    if (const char* e = getenv("AESR_WINO_GRID")) grid = atoi(e) / ncot * ncot;
    // Few blocks (a small data-parallel shard, the deep layers): at most FOUR per workgroup.  Waves 0..3 of a workgroup sit on the four
    // SIMDs of its CU (wave i -> SIMD i % 4: measured, scripts/res_stamps.py), so four one-item waves each have a matrix pipe to themselves;
    // the round-2 rule packed eight per workgroup and two one-item waves shared every SIMD (2.2 -> 1.5 us per 16-channel chunk at 6 images).
    static const int wpw = getenv("AESR_WINO_RES_WPW") ? atoi(getenv("AESR_WINO_RES_WPW")) : 4;
    const int per_cot = ceil_div(a.nblk, wpw >= 1 && wpw <= 8 ? wpw : 4);
    if (grid / ncot > per_cot) grid = per_cot * ncot;
    if (grid < ncot) grid = ncot;
    WinoArgs b = a;
    static const int xmap_on = getenv("AESR_WINO_XCD") ? atoi(getenv("AESR_WINO_XCD")) : 1;
    // (the XCD map hands every XCD a contiguous run of 8 x its workers blocks per round: with fewer blocks than waves it would fill the first
    // XCDs' workgroups with eight blocks each and leave the others idle)
    b.xcd_map = (xmap_on && grid % (8 * ncot) == 0 && a.nblk >= 8 * (grid / ncot)) ? 1 : 0;
    if constexpr (!MASK && !POST && !NINE) {
        if (getenv("AESR_WINO_RES_DBG")) return wino_res_stamped<WR_TN>(b, grid, shmem, st);
    }
    hipLaunchKernelGGL((conv_wino_res_f32<WR_TN, MASK, POST, false, NINE>), dim3(grid), dim3(WR_NT), shmem, st, b);
    AESR_LAUNCH_CHECK("conv_wino_res_f32");
    return AESR_OK;
}

// AESR_WINO_UP2_NINE=0: the upsample-folded layers run the 16-position instantiations, forward, data gradient and weight gradient
// (conv_wgrad_wino.hip) alike; read once
bool aesr_wino_up2_nine() {
    static const bool on = [] { const char* e = getenv("AESR_WINO_UP2_NINE"); return !(e && *e && atoi(e) == 0); }();
    return on;
}

// called by aesr_launch_conv_wino (which has validated the arguments) when aesr_wino_res_ok(a)
int aesr_launch_conv_wino_res(const WinoArgs& a_in, hipStream_t st) {
    WinoArgs a = a_in;
    a.TI = 1; a.THt = 4; a.TWt = 4;
    a.regs_y = ceil_div(a.H, 8);
    a.regs_x = ceil_div(a.W, 8);
    a.bpi = a.regs_y * a.regs_x;
    a.nblk = a.N * a.bpi;
    const int TN = wino_res_tn(a);
    a.nitems = a.nblk * (a.CoutP / TN);
    a.m_bpi = aesr_magic_u32(a.bpi); a.m_regs_x = aesr_magic_u32(a.regs_x);
    // the wave's item index runs up to nblk + 8 * 256 past the end before it is compared: exactness of the multiply-high division
    if (((unsigned long long)a.nblk + 4096) * (unsigned)(a.bpi + a.regs_x) >= ((unsigned long long)1 << 31) || (size_t)a.H * a.W * a.Cin * 4 >= (size_t)0x10000000) {
        aesr_set_error("conv_wino_res: %d blocks exceed the exact range of the item decomposition (or images of 256 MB and more)", a.nblk);
        return AESR_ERR_UNSUPPORTED;
    }
    if (wino_res_lds_bytes(a.CinP, TN) > (size_t)160 * 1024) {
        aesr_set_error("conv_wino_res: %d input channels do not fit the resident filter", a.CinP);
        return AESR_ERR_ARG;
    }
    if (a.post_scale) {
        if (a.ysave || a.out_sum2 || !a.post_shift) {
            aesr_set_error("conv_wino_res: the folded eval-mode BatchNorm is a forward epilogue (no derivative mask, no 2x2-summing output)");
            return AESR_ERR_ARG;
        }
        return TN == 32 ? wino_res_launch_one<32, false, true>(a, st) : wino_res_launch_one<16, false, true>(a, st);
    }
    // behind a folded Upsample(x2), either direction: the nine-position form (aesr_launch_conv_wino has checked that H and W are even;
    // out_sum2 comes without mask, activation and bias).  Named last: the compiler emits kernels in the order they are first named, and
    // the listings of the 16-position ones stay what they were.
    if (!((a.in_up2 || a.out_sum2) && !a.ysave && aesr_wino_up2_nine())) {
        if (TN == 32) return a.ysave ? wino_res_launch_one<32, true>(a, st) : wino_res_launch_one<32, false>(a, st);
        return a.ysave ? wino_res_launch_one<16, true>(a, st) : wino_res_launch_one<16, false>(a, st);
    }
    return TN == 32 ? wino_res_launch_one<32, false, false, true>(a, st) : wino_res_launch_one<16, false, false, true>(a, st);
}
