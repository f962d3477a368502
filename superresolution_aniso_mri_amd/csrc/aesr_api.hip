// extern "C" entry points of libaesr_hip.so (declared in include/aesr_hip.h); the tile planners they ask are in conv_plan.hip.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/aesr_hip.h"
#include "../../include/aesr_hip_bnpool.h"
#include "../../include/aesr_hip_dataprep.h"
#include "../../include/aesr_hip_train.h"
#include "aesr_kernels.h"
#include "conv_plan.h"

// ---- error string ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void aesr_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static bool fill_groups(BnGroups* gr, int G, const int* nstart_host) {
    if (G < 1 || G > 4 || !nstart_host) return false;
    gr->G = G;
    for (int i = 0; i <= G; ++i) gr->nstart[i] = nstart_host[i];
    for (int i = G + 1; i < 5; ++i) gr->nstart[i] = nstart_host[G];
    return true;
}

// ---- what the convolution entry points share ----------------------------------------------------------------------
// The one shape check: filter and padding legal, tensors inside the kernels' offsets (conv_dims_ok), a non-empty output.  Ho and Wo
// are set whenever the filter is legal.  Queries answer 0 for anything but GEOM_OK; launches turn the code into their own message.
enum { GEOM_OK = 0, GEOM_FILTER, GEOM_DIMS, GEOM_SMALL };
static int conv_geom(int N, int H, int W, int Cin, int Cout, int KS, int pad, int* Ho, int* Wo) {
    if ((KS != 1 && KS != 3) || pad < 0 || pad >= KS) return GEOM_FILTER;
    *Ho = (int)((long long)H + 2 * pad - KS + 1);       // (H, W are unchecked here: no int overflow)
    *Wo = (int)((long long)W + 2 * pad - KS + 1);
    if (!conv_dims_ok(N, H, W, Cin, Cout)) return GEOM_DIMS;
    return *Ho > 0 && *Wo > 0 ? GEOM_OK : GEOM_SMALL;
}

// Padded sizes and column tile of a packed filter: kin / nout are the K-side and output channel counts (swapped for the data gradient)
struct PackGeom { int KinP, NoutP, TN; };
static PackGeom pack_geom(int Cout, int Cin, int transpose, bool wino) {
    const int kin = transpose ? Cout : Cin, nout = transpose ? Cin : Cout;
    PackGeom g;
    g.KinP = round_up(kin, 16);
    if (wino) {
        g.NoutP = round_up(nout, 32);
        g.TN = 32;
    } else {
        int NB;
        cout_padding(nout, &g.NoutP, &NB);
        g.TN = 16 * NB;
    }
    return g;
}

// The planned part of a Winograd launch or query; pointers, activation and the folded forms are the caller's
static WinoArgs wino_args(int N, int H, int W, int kin, int nout, const WinoPlan& p) {
    WinoArgs a = {};
    a.N = N; a.H = H; a.W = W; a.Cin = kin; a.CinP = p.CinP; a.Cout = nout; a.CoutP = p.CoutP;
    a.TI = p.TI; a.THt = p.THt; a.TWt = p.TWt;
    a.plan_cost = p.cost;
    a.ksplit = 1;
    return a;
}

// Job tables: chunks of the table's capacity, each zeroed, filled (fill(job, index, entry, &blocks): 0 or the refusal), given its
// block0 offsets and launched; stops at the first error.
template <class Table, class Job, class Fill>
static int run_job_table(const Job* jobs, int njobs, Fill fill, int (*launch)(const Table&, hipStream_t), void* stream) {
    const int cap = (int)(sizeof(Table().job) / sizeof(Table().job[0]));
    for (int j0 = 0; j0 < njobs; j0 += cap) {
        Table t;
        memset(&t, 0, sizeof(t));
        t.njobs = njobs - j0 < cap ? njobs - j0 : cap;
        for (int k = 0; k < t.njobs; ++k) {
            int blocks = 0;
            if (int e = fill(jobs[j0 + k], j0 + k, t.job[k], &blocks)) return e;
            t.job[k].block0 = t.nblocks;
            t.nblocks += blocks;
        }
        if (int e = launch(t, (hipStream_t)stream)) return e;
    }
    return AESR_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------
extern "C" {

int aesr_version(void) { return AESR_ABI_VERSION; }
const char* aesr_last_error_string(void) { return g_err; }

size_t aesr_conv2d_packed_floats(int Cout, int Cin, int KS, int transpose) {
    const PackGeom g = pack_geom(Cout, Cin, transpose, false);
    return (size_t)KS * KS * g.KinP * g.NoutP;
}

int aesr_conv2d_pack(const float* w, float* packed, int Cout, int Cin, int KS, int transpose, void* stream) {
    AESR_CHECK_ARG(w && packed && Cout > 0 && Cin > 0 && (KS == 1 || KS == 3), "aesr_conv2d_pack: bad arguments");
    const PackGeom g = pack_geom(Cout, Cin, transpose, false);
    return aesr_launch_pack_weights(w, packed, Cout, Cin, KS, g.KinP, g.NoutP, g.TN, transpose, (hipStream_t)stream);
}

static int blocks_of(size_t threads) { return threads > (size_t)256 * 256 ? 256 : (int)((threads + 255) / 256); }

int aesr_conv2d_pack_many(const aesr_pack_job* jobs_host, int njobs, void* stream) {
    AESR_CHECK_ARG(jobs_host && njobs > 0, "aesr_conv2d_pack_many: no jobs");
    return run_job_table<PackTable>(jobs_host, njobs, [](const aesr_pack_job& jb, int j, PackJob& o, int* blocks) -> int {
        AESR_CHECK_ARG(jb.w && jb.packed && jb.Cout > 0 && jb.Cin > 0 && (jb.KS == 1 || jb.KS == 3), "aesr_conv2d_pack_many: bad job %d", j);
        const PackGeom g = pack_geom(jb.Cout, jb.Cin, jb.transpose, false);
        o.w = jb.w; o.p = jb.packed; o.Cout = jb.Cout; o.Cin = jb.Cin; o.KS = jb.KS; o.KinP = g.KinP; o.NoutP = g.NoutP; o.TN = g.TN;
        o.transpose = jb.transpose;
        *blocks = blocks_of(((size_t)jb.KS * jb.KS * g.KinP * g.NoutP + 3) / 4);         // 4 elements per thread
        return AESR_OK;
    }, aesr_launch_pack_many, stream);
}

int aesr_weight_prep_many(const aesr_prep_job* jobs_host, int njobs, void* stream) {
    AESR_CHECK_ARG(jobs_host && njobs > 0, "aesr_weight_prep_many: no jobs");
    return run_job_table<PrepTable>(jobs_host, njobs, [](const aesr_prep_job& jb, int j, PrepJob& o, int* blocks) -> int {
        AESR_CHECK_ARG(jb.w && jb.out && jb.Cout > 0 && jb.Cin > 0, "aesr_weight_prep_many: bad job %d", j);
        o.w = jb.w; o.aux0 = jb.aux0; o.aux1 = jb.aux1; o.out = jb.out; o.kind = jb.kind; o.Cout = jb.Cout; o.Cin = jb.Cin; o.KS = jb.KS;
        o.transpose = jb.transpose;
        size_t threads = 0;
        if (jb.kind == AESR_PREP_PACK || jb.kind == AESR_PREP_WINO_PACK) {     // as aesr_conv2d_pack_many / aesr_conv2d_wino_pack_many
            const bool wino = jb.kind == AESR_PREP_WINO_PACK;
            AESR_CHECK_ARG(wino || jb.KS == 1 || jb.KS == 3, "aesr_weight_prep_many: job %d: KS=%d", j, jb.KS);
            AESR_CHECK_ARG(!wino || jb.KS == 3, "aesr_weight_prep_many: job %d: the Winograd transform is for 3x3 filters", j);
            const PackGeom g = pack_geom(jb.Cout, jb.Cin, jb.transpose, wino);
            o.KinP = g.KinP; o.NoutP = g.NoutP; o.TN = g.TN;
            threads = wino ? (size_t)g.KinP * g.NoutP : ((size_t)jb.KS * jb.KS * g.KinP * g.NoutP + 3) / 4;       // direct: 4 elements per thread
        } else if (jb.kind == AESR_PREP_STEM_FOLD) {           // as aesr_stemconv_fold: Cout = C1, Cin = Cs, aux0 / aux1 = stem weight / bias
            AESR_CHECK_ARG(jb.aux0, "aesr_weight_prep_many: job %d: stem fold needs the stem weight", j);
            threads = (size_t)9 * jb.Cout;
        } else if (jb.kind == AESR_PREP_COUT1_FLIP) {
            threads = (size_t)9 * jb.Cin;
        } else {
            aesr_set_error("aesr_weight_prep_many: job %d: unknown kind %d", j, jb.kind);
            return AESR_ERR_ARG;
        }
        *blocks = blocks_of(threads);
        return AESR_OK;
    }, aesr_launch_prep_many, stream);
}

// ---- implicit-GEMM path ----------------------------------------------------------------------------------------------
static int run_igemm(const float* in, const float* packed, const float* bias, const float* ysave, float* out, int N, int H,
                     int W, int Cin, int Cout, int KS, int pad, int act, int mask_act, float slope, float* workspace,
                     hipStream_t st) {
    int Ho, Wo;
    const int g = conv_geom(N, H, W, Cin, Cout, KS, pad, &Ho, &Wo);
    if (g == GEOM_DIMS) AESR_CHECK_DIMS("aesr_conv2d (implicit GEMM)", N, H, W, Cin, Cout);
    AESR_CHECK_ARG(g == GEOM_OK, "aesr_conv2d: the %d x %d input is smaller than the %d x %d filter", H, W, KS, KS);
    const ConvPlan p = plan_conv(N, Ho, Wo, Cin, Cout, KS);
    IgemmArgs a = {};
    a.in = in; a.wpk = packed; a.bias = bias; a.ysave = ysave; a.out = out;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.CinP = p.CinP; a.Cout = Cout; a.CoutP = p.CoutP; a.Ho = Ho; a.Wo = Wo; a.pad = pad;
    a.TI = p.TI; a.TH = p.TH; a.TW = p.TW; a.tiles_y = ceil_div(Ho, p.TH); a.tiles_x = ceil_div(Wo, p.TW);
    a.act = act; a.mask_act = mask_act; a.slope = slope; a.ksplit = 1;
    if (workspace && p.ksplit > 1) {
        // raw partial sums of the k slices -> workspace, then the fix-up pass (bias, activation, derivative mask)
        a.ksplit = p.ksplit; a.out = workspace; a.bias = nullptr; a.ysave = nullptr; a.act = ACT_NONE; a.mask_act = ACT_NONE;
        if (int e = aesr_launch_conv_igemm(a, KS, p.NB, p.MBW, st)) return e;
        return aesr_launch_conv_ksplit_fixup(workspace, bias, ysave, out, (size_t)N * Ho * Wo * Cout, Cout, p.ksplit, act, mask_act,
                                             slope, st);
    }
    return aesr_launch_conv_igemm(a, KS, p.NB, p.MBW, st);
}

// forward (in = x, aux = bias) or data gradient (in = dy [N,Ho,Wo,Cout], packed = the flipped filter, aux = the saved x for the derivative
// mask): dx = conv(dy, flipped w) with Cout and Cin swapped and padding KS-1-pad -> [N,H,W,Cin]
static int igemm_entry(const char* who, bool dgrad, const float* in, const float* packed, const float* aux, float* out, float* workspace,
                       int N, int H, int W, int Cin, int Cout, int KS, int pad, int act, float slope, void* stream) {
    AESR_CHECK_ARG(in && packed && out && N > 0 && H > 0 && W > 0, "%s: null pointer or empty shape", who);
    AESR_CHECK_ARG((dgrad ? Cout : Cin) % 4 == 0 && Cin > 0 && Cout > 0, "%s: %s=%d must be a positive multiple of 4", who, dgrad ? "Cout" : "Cin",
                   dgrad ? Cout : Cin);
    int Ho, Wo;
    AESR_CHECK_ARG(conv_geom(N, H, W, Cin, Cout, KS, pad, &Ho, &Wo) != GEOM_FILTER, "%s: unsupported KS=%d pad=%d", who, KS, pad);
    if (dgrad) return run_igemm(in, packed, nullptr, aux, out, N, Ho, Wo, Cout, Cin, KS, KS - 1 - pad, ACT_NONE, act, slope, workspace, (hipStream_t)stream);
    return run_igemm(in, packed, aux, nullptr, out, N, H, W, Cin, Cout, KS, pad, act, ACT_NONE, slope, workspace, (hipStream_t)stream);
}

int aesr_conv2d_fwd_ws(const float* in, const float* packed, const float* bias, float* out, float* workspace, int N, int H, int W,
                       int Cin, int Cout, int KS, int pad, int act, float slope, void* stream) {
    return igemm_entry("aesr_conv2d_fwd_ws", false, in, packed, bias, out, workspace, N, H, W, Cin, Cout, KS, pad, act, slope, stream);
}

int aesr_conv2d_fwd(const float* in, const float* packed, const float* bias, float* out, int N, int H, int W, int Cin,
                    int Cout, int KS, int pad, int act, float slope, void* stream) {
    return igemm_entry("aesr_conv2d_fwd", false, in, packed, bias, out, nullptr, N, H, W, Cin, Cout, KS, pad, act, slope, stream);
}

int aesr_conv2d_dgrad_ws(const float* dy, const float* packed_t, const float* x_saved, float* dx, float* workspace, int N, int H,
                         int W, int Cin, int Cout, int KS, int pad, int mask_act, float slope, void* stream) {
    return igemm_entry("aesr_conv2d_dgrad_ws", true, dy, packed_t, x_saved, dx, workspace, N, H, W, Cin, Cout, KS, pad, mask_act, slope, stream);
}

int aesr_conv2d_dgrad(const float* dy, const float* packed_t, const float* x_saved, float* dx, int N, int H, int W, int Cin,
                      int Cout, int KS, int pad, int mask_act, float slope, void* stream) {
    return igemm_entry("aesr_conv2d_dgrad", true, dy, packed_t, x_saved, dx, nullptr, N, H, W, Cin, Cout, KS, pad, mask_act, slope, stream);
}

size_t aesr_conv2d_workspace_floats(int N, int H, int W, int Cin, int Cout, int KS, int pad) {
    int Ho, Wo;
    if (conv_geom(N, H, W, Cin, Cout, KS, pad, &Ho, &Wo) != GEOM_OK) return 0;
    const ConvPlan p = plan_conv(N, Ho, Wo, Cin, Cout, KS);
    return p.ksplit > 1 ? (size_t)p.ksplit * N * Ho * Wo * Cout : 0;
}

size_t aesr_conv2d_dgrad_workspace_floats(int N, int H, int W, int Cin, int Cout, int KS, int pad) {
    int Ho, Wo;
    if (conv_geom(N, H, W, Cin, Cout, KS, pad, &Ho, &Wo) != GEOM_OK) return 0;
    return aesr_conv2d_workspace_floats(N, Ho, Wo, Cout, Cin, KS, KS - 1 - pad);        // the forward kernel on dy, as igemm_entry runs it
}

// ---- Winograd F(2x2,3x3) path --------------------------------------------------------------------------------------
int aesr_conv2d_wino_supported(int Cin, int Cout, int KS, int pad, int transpose) {
    const int kin = transpose ? Cout : Cin, nout = transpose ? Cin : Cout;
    return KS == 3 && pad == 1 && kin > 0 && nout > 0 && kin % 16 == 0 && nout % 32 == 0;
}

// a query's arguments: false where the layer is no Winograd layer or beyond the kernels' offsets
static bool wino_query(int N, int H, int W, int Cin, int Cout, int KS, int pad, int transpose, WinoArgs* a) {
    if (!aesr_conv2d_wino_supported(Cin, Cout, KS, pad, transpose) || !conv_dims_ok(N, H, W, Cin, Cout)) return false;
    const int kin = transpose ? Cout : Cin, nout = transpose ? Cin : Cout;
    *a = wino_args(N, H, W, kin, nout, plan_wino(N, H, W, kin, nout));
    return true;
}

int aesr_conv2d_wino_kernel(int N, int H, int W, int Cin, int Cout, int KS, int pad, int transpose) {
    WinoArgs a;
    if (!wino_query(N, H, W, Cin, Cout, KS, pad, transpose, &a)) return 0;
    if (aesr_wino_res_ok(a)) return 2;
    a.ws_floats = ~(size_t)0;           // a query: as called with the workspace aesr_conv2d_wino_workspace_floats asks for
    return aesr_wino_ring_takes(a) ? 3 : 1;
}

size_t aesr_conv2d_wino_workspace_floats(int N, int H, int W, int Cin, int Cout, int transpose) {
    WinoArgs a;
    if (!wino_query(N, H, W, Cin, Cout, 3, 1, transpose, &a) || aesr_wino_res_ok(a)) return 0;
    return aesr_wino_ring_workspace_floats(a);
}

unsigned int aesr_conv2d_wino_ring_timeouts(void) {
    (void)hipDeviceSynchronize();
    return aesr_wino_ring_timeouts();
}

size_t aesr_conv2d_wino_packed_floats(int Cout, int Cin, int transpose) {
    const PackGeom g = pack_geom(Cout, Cin, transpose, true);
    return (size_t)16 * g.KinP * g.NoutP;
}

int aesr_conv2d_wino_pack_many(const aesr_pack_job* jobs_host, int njobs, void* stream) {
    AESR_CHECK_ARG(jobs_host && njobs > 0, "aesr_conv2d_wino_pack_many: no jobs");
    return run_job_table<PackTable>(jobs_host, njobs, [](const aesr_pack_job& jb, int j, PackJob& o, int* blocks) -> int {
        AESR_CHECK_ARG(jb.w && jb.packed && jb.Cout > 0 && jb.Cin > 0 && jb.KS == 3, "aesr_conv2d_wino_pack_many: bad job %d", j);
        const PackGeom g = pack_geom(jb.Cout, jb.Cin, jb.transpose, true);
        o.w = jb.w; o.p = jb.packed; o.Cout = jb.Cout; o.Cin = jb.Cin; o.KS = 3; o.KinP = g.KinP; o.NoutP = g.NoutP; o.TN = g.TN;
        o.transpose = jb.transpose;
        *blocks = blocks_of((size_t)g.KinP * g.NoutP);
        return AESR_OK;
    }, aesr_launch_wino_pack_many, stream);
}

static int run_wino(const float* in, const float* upk, const float* bias, const float* ysave, float* out, int N, int H, int W,
                    int Cin, int Cout, int act, int mask_act, float slope, hipStream_t st, int in_up2 = 0, int out_sum2 = 0,
                    float* ws = nullptr, size_t ws_floats = 0) {
    AESR_CHECK_DIMS("aesr_conv2d_wino", N, H, W, Cin, Cout);
    WinoArgs a = wino_args(N, H, W, Cin, Cout, plan_wino(N, H, W, Cin, Cout));
    a.in = in; a.upk = upk; a.bias = bias; a.ysave = ysave; a.out = out;
    a.act = act; a.mask_act = mask_act; a.slope = slope; a.in_up2 = in_up2; a.out_sum2 = out_sum2;
    a.ws = ws_floats ? ws : nullptr; a.ws_floats = ws ? ws_floats : 0;
    return aesr_launch_conv_wino(a, st);
}

int aesr_conv2d_wino_fwd(const float* in, const float* upacked, const float* bias, float* out, int N, int H, int W, int Cin,
                         int Cout, int act, float slope, void* stream) {
    AESR_CHECK_ARG(in && upacked && out && N > 0 && H > 0 && W > 0, "aesr_conv2d_wino_fwd: null pointer or empty shape");
    AESR_CHECK_ARG(aesr_conv2d_wino_supported(Cin, Cout, 3, 1, 0), "aesr_conv2d_wino_fwd: needs Cin %% 16 == 0 and Cout %% 32 == 0 (got %d -> %d)", Cin, Cout);
    return run_wino(in, upacked, bias, nullptr, out, N, H, W, Cin, Cout, act, ACT_NONE, slope, (hipStream_t)stream);
}

int aesr_conv2d_wino_dgrad(const float* dy, const float* upacked_t, const float* x_saved, float* dx, int N, int H, int W, int Cin,
                           int Cout, int mask_act, float slope, void* stream) {
    AESR_CHECK_ARG(dy && upacked_t && dx && N > 0 && H > 0 && W > 0, "aesr_conv2d_wino_dgrad: null pointer or empty shape");
    AESR_CHECK_ARG(aesr_conv2d_wino_supported(Cin, Cout, 3, 1, 1), "aesr_conv2d_wino_dgrad: needs Cout %% 16 == 0 and Cin %% 32 == 0 (got %d -> %d)", Cin, Cout);
    // dx = conv(dy [N,H,W,Cout], flipped / transposed filter), padding 1 -> [N,H,W,Cin]
    return run_wino(dy, upacked_t, nullptr, x_saved, dx, N, H, W, Cout, Cin, ACT_NONE, mask_act, slope, (hipStream_t)stream);
}

int aesr_conv2d_wino_fwd_ws(const float* in, const float* upacked, const float* bias, float* out, float* workspace, size_t workspace_floats,
                            int N, int H, int W, int Cin, int Cout, int act, float slope, void* stream) {
    AESR_CHECK_ARG(in && upacked && out && N > 0 && H > 0 && W > 0, "aesr_conv2d_wino_fwd_ws: null pointer or empty shape");
    AESR_CHECK_ARG(aesr_conv2d_wino_supported(Cin, Cout, 3, 1, 0), "aesr_conv2d_wino_fwd_ws: needs Cin %% 16 == 0 and Cout %% 32 == 0 (got %d -> %d)", Cin, Cout);
    return run_wino(in, upacked, bias, nullptr, out, N, H, W, Cin, Cout, act, ACT_NONE, slope, (hipStream_t)stream, 0, 0, workspace, workspace_floats);
}

int aesr_conv2d_wino_dgrad_ws(const float* dy, const float* upacked_t, const float* x_saved, float* dx, float* workspace, size_t workspace_floats,
                              int N, int H, int W, int Cin, int Cout, int mask_act, float slope, void* stream) {
    AESR_CHECK_ARG(dy && upacked_t && dx && N > 0 && H > 0 && W > 0, "aesr_conv2d_wino_dgrad_ws: null pointer or empty shape");
    AESR_CHECK_ARG(aesr_conv2d_wino_supported(Cin, Cout, 3, 1, 1), "aesr_conv2d_wino_dgrad_ws: needs Cout %% 16 == 0 and Cin %% 32 == 0 (got %d -> %d)", Cin, Cout);
    return run_wino(dy, upacked_t, nullptr, x_saved, dx, N, H, W, Cout, Cin, ACT_NONE, mask_act, slope, (hipStream_t)stream, 0, 0, workspace, workspace_floats);
}

/* conv + activation + eval-mode BatchNorm (per-channel scale / shift) [+ AvgPool2d(2)] as one launch: the resident-filter kernel, and the
   ring kernel where it takes the layer WITHOUT a workspace (no channel split: the epilogue has to see the finished sums) */
int aesr_conv2d_wino_fwd_bn_supported(int N, int H, int W, int Cin, int Cout) {
    WinoArgs a;
    if (!wino_query(N, H, W, Cin, Cout, 3, 1, 0, &a)) return 0;
    return aesr_wino_res_ok(a) || aesr_wino_ring_takes(a) ? 1 : 0;          /* a.ws_floats = 0: as the call below runs it */
}

int aesr_conv2d_wino_fwd_bn(const float* in, const float* upacked, const float* bias, const float* bn_scale, const float* bn_shift, float* out, int N,
                            int H, int W, int Cin, int Cout, int act, float slope, int pool, void* stream) {
    AESR_CHECK_ARG(in && upacked && bn_scale && bn_shift && out && N > 0 && H > 0 && W > 0, "aesr_conv2d_wino_fwd_bn: null pointer or empty shape");
    AESR_CHECK_ARG(!pool || (H >= 2 && W >= 2), "aesr_conv2d_wino_fwd_bn: pooling needs H, W >= 2");
    AESR_CHECK_ARG(aesr_conv2d_wino_fwd_bn_supported(N, H, W, Cin, Cout), "aesr_conv2d_wino_fwd_bn: %d -> %d at %d x %d x %d is not a resident-filter or ring-kernel layer "
                   "(aesr_conv2d_wino_fwd_bn_supported)", Cin, Cout, N, H, W);
    WinoArgs a = wino_args(N, H, W, Cin, Cout, plan_wino(N, H, W, Cin, Cout));
    a.in = in; a.upk = upacked; a.bias = bias; a.out = out;
    a.act = act; a.mask_act = ACT_NONE; a.slope = slope;
    a.post_scale = bn_scale; a.post_shift = bn_shift; a.post_pool = pool ? 1 : 0;
    return aesr_launch_conv_wino(a, (hipStream_t)stream);
}

/* nearest Upsample(x2) in front of the convolution folded into the kernels (H, W = the convolution's = upsampled size, even) */
int aesr_conv2d_wino_fwd_up2(const float* in_half, const float* upacked, const float* bias, float* out, int N, int H, int W, int Cin,
                             int Cout, int act, float slope, void* stream) {
    AESR_CHECK_ARG(in_half && upacked && out && N > 0 && H > 0 && W > 0 && !((H | W) & 1), "aesr_conv2d_wino_fwd_up2: null pointer, empty or odd shape");
    AESR_CHECK_ARG(aesr_conv2d_wino_supported(Cin, Cout, 3, 1, 0), "aesr_conv2d_wino_fwd_up2: needs Cin %% 16 == 0 and Cout %% 32 == 0 (got %d -> %d)", Cin, Cout);
    return run_wino(in_half, upacked, bias, nullptr, out, N, H, W, Cin, Cout, act, ACT_NONE, slope, (hipStream_t)stream, 1, 0);
}

int aesr_conv2d_wino_dgrad_sum2(const float* dy, const float* upacked_t, float* dx_half, int N, int H, int W, int Cin, int Cout,
                                void* stream) {
    AESR_CHECK_ARG(dy && upacked_t && dx_half && N > 0 && H > 0 && W > 0 && !((H | W) & 1), "aesr_conv2d_wino_dgrad_sum2: null pointer, empty or odd shape");
    AESR_CHECK_ARG(aesr_conv2d_wino_supported(Cin, Cout, 3, 1, 1), "aesr_conv2d_wino_dgrad_sum2: needs Cout %% 16 == 0 and Cin %% 32 == 0 (got %d -> %d)", Cin, Cout);
    return run_wino(dy, upacked_t, nullptr, nullptr, dx_half, N, H, W, Cout, Cin, ACT_NONE, ACT_NONE, 0.f, (hipStream_t)stream, 0, 1);
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
size_t aesr_conv2d_wgrad_workspace_floats(int N, int H, int W, int Cin, int Cout, int KS, int pad) {
    int Ho, Wo;
    if (conv_geom(N, H, W, Cin, Cout, KS, pad, &Ho, &Wo) != GEOM_OK) return 0;
    return plan_wgrad(N, Ho, Wo, Cin, Cout, KS, pad).slab_floats;
}

static int wgrad_impl(const float* x, const float* dy, float* dw, float* db, float* workspace, int N, int H, int W, int Cin,
                      int Cout, int KS, int pad, void* stream, int x_up2) {
    AESR_CHECK_ARG(x && dy && workspace && N > 0, "aesr_conv2d_wgrad: null pointer or empty shape");
    AESR_CHECK_ARG(Cin % 4 == 0 && Cout % 4 == 0, "aesr_conv2d_wgrad: Cin=%d, Cout=%d must be multiples of 4", Cin, Cout);
    int Ho, Wo;
    const int g = conv_geom(N, H, W, Cin, Cout, KS, pad, &Ho, &Wo);
    AESR_CHECK_ARG(g != GEOM_FILTER, "aesr_conv2d_wgrad: unsupported KS=%d pad=%d", KS, pad);
    if (g == GEOM_DIMS) AESR_CHECK_DIMS("aesr_conv2d_wgrad", N, H, W, Cin, Cout);
    AESR_CHECK_ARG(g == GEOM_OK, "aesr_conv2d_wgrad: the %d x %d input is smaller than the %d x %d filter", H, W, KS, KS);
    const WgradPlan p = plan_wgrad(N, Ho, Wo, Cin, Cout, KS, pad);
    WgradArgs a;
    a.x = x; a.dy = dy; a.slab = workspace;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.CinP = p.CinP; a.Cout = Cout; a.CoutP = p.CoutP; a.Ho = Ho; a.Wo = Wo; a.pad = pad;
    a.TH = p.TH; a.TW = p.TW; a.tiles_y = ceil_div(Ho, p.TH); a.tiles_x = ceil_div(Wo, p.TW);
    a.ntiles = N * a.tiles_y * a.tiles_x; a.S = p.S;
    a.PWS = p.PWS; a.TWS = p.TWS; a.PSX = p.PSX; a.PSD = p.PSD; a.dbgbuf = nullptr; a.x_up2 = x_up2;
    if (p.variant == 2) {
        if (int e = aesr_launch_conv_wgrad_wino(a, (hipStream_t)stream)) return e;
    } else if (int e = aesr_launch_conv_wgrad(a, KS, p.variant, (hipStream_t)stream)) {
        return e;
    }
    if (!dw) return AESR_OK;            // partial-slab form (aesr_conv2d_wgrad_partial): the caller reduces later
    return aesr_launch_wgrad_reduce(workspace, dw, db, p.nslab, KS, Cin, p.CinP, Cout, p.CoutP, (hipStream_t)stream);
}

int aesr_conv2d_wgrad(const float* x, const float* dy, float* dw, float* db, float* workspace, int N, int H, int W, int Cin,
                      int Cout, int KS, int pad, void* stream) {
    return wgrad_impl(x, dy, dw, db, workspace, N, H, W, Cin, Cout, KS, pad, stream, 0);
}

int aesr_conv2d_wgrad_partial(const float* x, const float* dy, float* workspace, int N, int H, int W, int Cin, int Cout, int KS,
                              int pad, int x_up2, void* stream) {
    AESR_CHECK_ARG(!x_up2 || (wgrad_wino_ok(Cin, Cout, KS, pad) && !((H | W) & 1)), "aesr_conv2d_wgrad_partial: the folded upsampling needs "
                   "the Winograd weight-gradient kernel (3x3, padding 1, Cin, Cout multiples of 32) and an even size");
    return wgrad_impl(x, dy, nullptr, nullptr, workspace, N, H, W, Cin, Cout, KS, pad, stream, x_up2);
}

int aesr_conv2d_wgrad_reduce_many(const aesr_wgrad_reduce_job* jobs_host, int njobs, void* stream) {
    AESR_CHECK_ARG(jobs_host && njobs > 0, "aesr_conv2d_wgrad_reduce_many: no jobs");
    return run_job_table<ReduceTable>(jobs_host, njobs, [](const aesr_wgrad_reduce_job& jb, int j, ReduceJob& o, int* blocks) -> int {
        AESR_CHECK_ARG(jb.workspace && jb.dw && jb.N > 0 && (jb.KS == 1 || jb.KS == 3), "aesr_conv2d_wgrad_reduce_many: bad job %d", j);
        int Ho, Wo;
        AESR_CHECK_ARG(conv_geom(jb.N, jb.H, jb.W, jb.Cin, jb.Cout, jb.KS, jb.pad, &Ho, &Wo) == GEOM_OK, "aesr_conv2d_wgrad_reduce_many: job %d: bad shape", j);
        const WgradPlan p = plan_wgrad(jb.N, Ho, Wo, jb.Cin, jb.Cout, jb.KS, jb.pad);      // the plan the partial launch used
        o.slab = jb.workspace; o.dw = jb.dw; o.db = jb.db; o.nslab = p.nslab; o.KS2 = jb.KS * jb.KS; o.Cin = jb.Cin; o.CinP = p.CinP;
        o.Cout = jb.Cout; o.CoutP = p.CoutP;
        *blocks = ceil_div(o.KS2 * jb.Cin * jb.Cout + (jb.db ? jb.Cout : 0), 64);
        return AESR_OK;
    }, aesr_launch_wgrad_reduce_many, stream);
}

int aesr_conv2d_wgrad_up2_supported(int Cin, int Cout) { return wgrad_wino_ok(Cin, Cout, 3, 1) ? 1 : 0; }

int aesr_conv2d_wgrad_up2(const float* x_half, const float* dy, float* dw, float* db, float* workspace, int N, int H, int W, int Cin,
                          int Cout, void* stream) {
    AESR_CHECK_ARG(wgrad_wino_ok(Cin, Cout, 3, 1) && !((H | W) & 1), "aesr_conv2d_wgrad_up2: needs the Winograd weight-gradient kernel "
                   "(Cin, Cout multiples of 32; got %d -> %d) and an even size", Cin, Cout);
    return wgrad_impl(x_half, dy, dw, db, workspace, N, H, W, Cin, Cout, 3, 1, stream, 1);
}

int aesr_conv2d_smallcin_fwd(const float* in, const float* w, const float* bias, const float* y_saved, float* out, int N,
                             int H, int W, int Cin, int Cout, int KS, int pad, int act, int mask_act, float slope,
                             int transpose, int bcast, const float* ca_host, const float* cb_host, void* stream) {
    AESR_CHECK_ARG(in && w && out && N > 0 && Cin >= 1 && Cin <= 4 && Cout > 0, "aesr_conv2d_smallcin_fwd: need 1 <= Cin <= 4");
    AESR_CHECK_ARG(!bcast || (ca_host && cb_host), "aesr_conv2d_smallcin_fwd: bcast needs ca/cb");
    SmallArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in; a.w = w; a.bias = bias; a.ysave = y_saved; a.out = out;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KS = KS; a.pad = pad;
    a.Ho = H + 2 * pad - KS + 1; a.Wo = W + 2 * pad - KS + 1;
    a.act = act; a.mask_act = mask_act; a.slope = slope; a.transpose = transpose; a.bcast = bcast;
    for (int i = 0; i < Cin && bcast; ++i) { a.ca[i] = ca_host[i]; a.cb[i] = cb_host[i]; }
    return aesr_launch_smallcin_fwd(a, (hipStream_t)stream);
}

int aesr_conv2d_smallcin_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, int KS,
                               int pad, int bcast, const float* ca_host, void* stream) {
    AESR_CHECK_ARG(dy && w && dx && N > 0 && Cin >= 1 && Cin <= 4 && Cout > 0, "aesr_conv2d_smallcin_dgrad: need 1 <= Cin <= 4");
    AESR_CHECK_ARG(!bcast || ca_host, "aesr_conv2d_smallcin_dgrad: bcast needs ca");
    SmallDgradArgs a;
    memset(&a, 0, sizeof(a));
    a.dy = dy; a.w = w; a.dx = dx; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KS = KS; a.pad = pad; a.bcast = bcast;
    a.Ho = H + 2 * pad - KS + 1; a.Wo = W + 2 * pad - KS + 1;
    for (int i = 0; i < Cin && bcast; ++i) a.ca[i] = ca_host[i];
    return aesr_launch_smallcin_dgrad(a, (hipStream_t)stream);
}

#define SMALL_WGRAD_NWG 512
size_t aesr_small_wgrad_workspace_floats(int nout) { return (size_t)SMALL_WGRAD_NWG * nout; }

int aesr_conv2d_smallcin_wgrad(const float* in, const float* dout, float* dw, float* db, float* workspace, int N, int H,
                               int W, int Cin, int Cout, int pad, void* stream) {
    AESR_CHECK_ARG(in && dout && dw && db && workspace && Cin >= 1 && Cin <= 4, "aesr_conv2d_smallcin_wgrad: need 1 <= Cin <= 4");
    AESR_CHECK_ARG(Cout >= 4 && Cout % 4 == 0 && 256 % (Cout / 4) == 0 && Cout <= 256,
                   "aesr_conv2d_smallcin_wgrad: Cout=%d must be a multiple of 4 with Cout/4 dividing 256", Cout);
    SmallWgradArgs a;
    a.in = in; a.dout = dout; a.partial = workspace; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.pad = pad;
    a.Ho = H + 2 * pad; a.Wo = W + 2 * pad;
    if (int e = aesr_launch_smallcin_wgrad(a, SMALL_WGRAD_NWG, (hipStream_t)stream)) return e;
    return aesr_launch_sum_partials(workspace, SMALL_WGRAD_NWG, Cout * (Cin + 1), dw, Cout * Cin, db, (hipStream_t)stream);
}

int aesr_conv2d_cout1_fwd(const float* x, const float* w, const float* bias, float* out, int N, int H, int W, int Cin, int act,
                          float slope, void* stream) {
    AESR_CHECK_ARG(x && w && out && N > 0 && H > 0 && W > 0, "aesr_conv2d_cout1_fwd: null pointer or empty shape");
    AESR_CHECK_ARG(Cin > 0 && Cin % 4 == 0 && Cin <= 256, "aesr_conv2d_cout1_fwd: Cin=%d must be a multiple of 4 (<= 256)", Cin);
    if (((Cin / 4) & (Cin / 4 - 1)) == 0)
        return aesr_launch_thin_collapse(x, w, bias, out, N, H, W, Cin, act, slope, (hipStream_t)stream);
    Cout1FwdArgs a;
    a.x = x; a.w = w; a.bias = bias; a.out = out; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.act = act; a.slope = slope;
    a.TH = H < 16 ? H : 16; a.TW = W < 16 ? W : 16;
    while (((size_t)(a.TH + 2) * (a.TW + 2) * (Cin + 4) + 9 * Cin) * 4 > 64 * 1024 && a.TH > 1) a.TH /= 2;
    a.tiles_y = ceil_div(H, a.TH); a.tiles_x = ceil_div(W, a.TW);
    return aesr_launch_cout1_fwd(a, (hipStream_t)stream);
}

#define THIN_NWG 512
static bool thin_channels_ok(int C) { return C >= 4 && C <= 256 && C % 4 == 0 && ((C / 4) & (C / 4 - 1)) == 0; }

size_t aesr_conv2d_cout1_workspace_floats(int Cin) {
    const size_t legacy = (size_t)SMALL_WGRAD_NWG * (Cin * 9 + 1);
    const size_t thin = (size_t)(THIN_NWG + 1) * 10 * Cin;
    return legacy > thin ? legacy : thin;
}

int aesr_conv2d_cout1_wgrad(const float* x, const float* dy, float* dw, float* db, float* workspace, int N, int H, int W,
                            int Cin, void* stream) {
    AESR_CHECK_ARG(x && dy && dw && db && workspace, "aesr_conv2d_cout1_wgrad: null pointer");
    AESR_CHECK_ARG(N > 0 && H > 0 && W > 0, "aesr_conv2d_cout1_wgrad: empty shape");
    if (thin_channels_ok(Cin)) {
        // dW[0,ci,ky,kx] = sum_u X[u,ci] * dy[u - (ky-1, kx-1)]  ->  thin reduce of X against dy, taps flipped
        ThinArgs a;
        memset(&a, 0, sizeof(a));
        a.s = dy; a.t = x; a.partial = workspace;
        a.N = N; a.Hs = H; a.Ws = W; a.Ho = H; a.Wo = W; a.C = Cin; a.ps = 0; a.with_be = 0;
        float* R = workspace + (size_t)THIN_NWG * 10 * Cin;
        if (int e = aesr_launch_thin_reduce(a, THIN_NWG, (hipStream_t)stream)) return e;
        if (int e = aesr_launch_sum_partials(workspace, THIN_NWG, 10 * Cin, R, 10 * Cin, nullptr, (hipStream_t)stream)) return e;
        return aesr_launch_thin_cout1_finish(R, dw, db, Cin, (hipStream_t)stream);
    }
    AESR_CHECK_ARG(Cin >= 4 && Cin <= 128 && 256 % Cin == 0, "aesr_conv2d_cout1_wgrad: Cin=%d must divide 256 (and be >= 4)", Cin);
    Cout1WgradArgs a;
    a.x = x; a.dy = dy; a.partial = workspace; a.N = N; a.H = H; a.W = W; a.Cin = Cin;
    a.TH = H < 16 ? H : 16; a.TW = W < 16 ? W : 16;
    while ((size_t)(a.TH + 2) * (a.TW + 2) * (Cin + 1) * 4 > 60 * 1024 && a.TH > 1) a.TH /= 2;
    a.tiles_y = ceil_div(H, a.TH); a.tiles_x = ceil_div(W, a.TW); a.ntiles = N * a.tiles_y * a.tiles_x;
    int nwg = a.ntiles < SMALL_WGRAD_NWG ? a.ntiles : SMALL_WGRAD_NWG;
    if (int e = aesr_launch_cout1_wgrad(a, nwg, (hipStream_t)stream)) return e;
    return aesr_launch_sum_partials(workspace, nwg, Cin * 9 + 1, dw, Cin * 9, db, (hipStream_t)stream);
}

// flip_ws: where to flip w into first (aesr_conv2d_cout1_dgrad), or nullptr for a filter that is flipped already (.._pre)
static int cout1_dgrad(const char* who, const float* dy, const float* w, float* flip_ws, const float* y_saved, float* dx, int N, int H, int W,
                       int Cin, int mask_act, float slope, void* stream) {
    AESR_CHECK_ARG(dy && w && dx && N > 0 && H > 0 && W > 0, "%s: null pointer or empty shape", who);
    AESR_CHECK_ARG(thin_channels_ok(Cin), "%s: Cin=%d must be 4 times a power of two (4..256)", who, Cin);
    if (flip_ws)
        if (int e = aesr_launch_thin_cout1_flip(w, flip_ws, Cin, (hipStream_t)stream)) return e;
    ThinArgs a;
    memset(&a, 0, sizeof(a));
    a.s = dy; a.w = flip_ws ? flip_ws : w; a.ysave = y_saved; a.out = dx;
    a.N = N; a.Hs = H; a.Ws = W; a.Ho = H; a.Wo = W; a.C = Cin; a.ps = 0;
    a.act = ACT_NONE; a.mask_act = y_saved ? mask_act : ACT_NONE; a.slope = slope;
    return aesr_launch_thin_expand(a, (hipStream_t)stream);
}

int aesr_conv2d_cout1_dgrad(const float* dy, const float* w, const float* y_saved, float* dx, float* workspace, int N, int H,
                            int W, int Cin, int mask_act, float slope, void* stream) {
    AESR_CHECK_ARG(workspace, "aesr_conv2d_cout1_dgrad: null pointer or empty shape");
    return cout1_dgrad("aesr_conv2d_cout1_dgrad", dy, w, workspace, y_saved, dx, N, H, W, Cin, mask_act, slope, stream);
}

int aesr_conv2d_cout1_dgrad_pre(const float* dy, const float* w_flipped, const float* y_saved, float* dx, int N, int H, int W, int Cin,
                                int mask_act, float slope, void* stream) {
    return cout1_dgrad("aesr_conv2d_cout1_dgrad_pre", dy, w_flipped, nullptr, y_saved, dx, N, H, W, Cin, mask_act, slope, stream);
}

// ---- include/aesr_hip_train.h: the Cout == 1 convolution's backward in one pass over its saved input --------------------------------
size_t aesr_conv2d_cout1_bwd_workspace_floats(int Cin) { return Cin > 0 ? (size_t)(THIN_NWG + 1) * 10 * Cin : 0; }

int aesr_conv2d_cout1_bwd(const float* x, const float* dout, const float* out, const float* w_flipped, float* dw, float* db, float* dx,
                          float* workspace, int N, int H, int W, int Cin, int act, float slope, int mask_act, float mask_slope,
                          void* stream) {
    AESR_CHECK_ARG(x && dout && w_flipped && dw && db && dx && workspace, "aesr_conv2d_cout1_bwd: null pointer");
    AESR_CHECK_ARG(N > 0 && H > 0 && W > 0, "aesr_conv2d_cout1_bwd: empty shape");
    AESR_CHECK_ARG(thin_channels_ok(Cin), "aesr_conv2d_cout1_bwd: Cin=%d must be 4 times a power of two (4..256)", Cin);
    AESR_CHECK_ARG(act >= ACT_NONE && act <= ACT_SIGMOID && mask_act >= ACT_NONE && mask_act <= ACT_SIGMOID,
                   "aesr_conv2d_cout1_bwd: unknown activation (act=%d, mask_act=%d)", act, mask_act);
    AESR_CHECK_ARG(out || act == ACT_NONE, "aesr_conv2d_cout1_bwd: out (the saved output) is needed for act=%d", act);
    // weight gradient = thin reduce of x against dpre = dout * act'(out), taps flipped (aesr_conv2d_cout1_wgrad); data gradient = the
    // expand of dpre with the flipped filter, masked by the derivative of the activation that produced x (aesr_conv2d_cout1_dgrad_pre):
    // both from the one read of x
    ThinArgs a;
    memset(&a, 0, sizeof(a));
    a.s = dout; a.sout = act == ACT_NONE ? nullptr : out; a.t = x; a.partial = workspace; a.w = w_flipped; a.out = dx;
    a.N = N; a.Hs = H; a.Ws = W; a.Ho = H; a.Wo = W; a.C = Cin; a.ps = 0; a.with_be = 0;
    a.act = act; a.slope = slope; a.mask_act = mask_act; a.mask_slope = mask_slope;
    if (int e = aesr_launch_thin_reduce_dx(a, THIN_NWG, (hipStream_t)stream)) return e;
    return aesr_launch_thin_cout1_finish_sum(workspace, THIN_NWG, dw, db, Cin, (hipStream_t)stream);
}

size_t aesr_stemconv_folded_floats(int C1) { return (size_t)2 * 9 * C1; }

int aesr_stemconv_fold(const float* w_stem, const float* b_stem, const float* w1, float* folded, int Cs, int C1, void* stream) {
    AESR_CHECK_ARG(w_stem && w1 && folded && Cs > 0 && C1 > 0, "aesr_stemconv_fold: bad arguments");
    return aesr_launch_thin_stem_fold(w_stem, b_stem, w1, folded, Cs, C1, (hipStream_t)stream);
}

int aesr_stemconv_fwd(const float* x, const float* folded, const float* b1, float* out, int N, int H, int W, int C1,
                      int stem_pad, int act, float slope, void* stream) {
    AESR_CHECK_ARG(x && folded && out && N > 0 && H > 0 && W > 0 && stem_pad >= 0, "aesr_stemconv_fwd: bad arguments");
    AESR_CHECK_ARG(thin_channels_ok(C1), "aesr_stemconv_fwd: C1=%d must be 4 times a power of two (4..256)", C1);
    ThinArgs a;
    memset(&a, 0, sizeof(a));
    a.s = x; a.w = folded; a.be = folded + (size_t)9 * C1; a.b = b1; a.out = out;
    a.N = N; a.Hs = H; a.Ws = W; a.Ho = H + 2 * stem_pad; a.Wo = W + 2 * stem_pad; a.C = C1; a.ps = stem_pad;
    a.act = act; a.mask_act = ACT_NONE; a.slope = slope;
    return aesr_launch_thin_expand(a, (hipStream_t)stream);
}

size_t aesr_stemconv_workspace_floats(int C1) { return (size_t)(THIN_NWG + 1) * 19 * C1; }

int aesr_stemconv_wgrad(const float* x, const float* g, const float* w_stem, const float* b_stem, const float* w1,
                        float* dw_stem, float* db_stem, float* dw1, float* db1, float* workspace, int N, int H, int W, int Cs,
                        int C1, int stem_pad, void* stream) {
    AESR_CHECK_ARG(x && g && w_stem && w1 && dw_stem && dw1 && workspace, "aesr_stemconv_wgrad: null pointer");
    AESR_CHECK_ARG(N > 0 && H > 0 && W > 0 && Cs > 0 && stem_pad >= 0, "aesr_stemconv_wgrad: bad shape");
    AESR_CHECK_ARG(thin_channels_ok(C1), "aesr_stemconv_wgrad: C1=%d must be 4 times a power of two (4..256)", C1);
    AESR_CHECK_ARG(!db_stem || b_stem, "aesr_stemconv_wgrad: db_stem needs b_stem");
    ThinArgs a;
    memset(&a, 0, sizeof(a));
    a.s = x; a.t = g; a.partial = workspace;
    a.N = N; a.Hs = H; a.Ws = W; a.Ho = H + 2 * stem_pad; a.Wo = W + 2 * stem_pad; a.C = C1; a.ps = stem_pad; a.with_be = 1;
    float* R = workspace + (size_t)THIN_NWG * 19 * C1;
    if (int e = aesr_launch_thin_reduce(a, THIN_NWG, (hipStream_t)stream)) return e;
    if (int e = aesr_launch_sum_partials(workspace, THIN_NWG, 19 * C1, R, 19 * C1, nullptr, (hipStream_t)stream)) return e;
    return aesr_launch_thin_stem_finish(R, w_stem, b_stem, w1, dw_stem, db_stem, dw1, db1, Cs, C1, (hipStream_t)stream);
}

int aesr_resample2_fwd(const float* x, float* out, int N, int H, int W, int C, int mode, void* stream) {
    AESR_CHECK_ARG(x && out && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "aesr_resample2_fwd: bad arguments (C %% 4 == 0)");
    AESR_CHECK_ARG(mode >= AESR_RS_POOL && mode <= AESR_RS_BILINEAR, "aesr_resample2_fwd: unknown mode %d", mode);
    AESR_CHECK_ARG(mode != AESR_RS_POOL || (H >= 2 && W >= 2), "aesr_resample2_fwd: pooling needs H, W >= 2");
    return aesr_launch_resample2(x, nullptr, nullptr, out, N, H, W, C, mode, 0, ACT_NONE, 0.f, (hipStream_t)stream);
}

int aesr_resample2_bwd(const float* gout, const float* x_saved, float* dx, int N, int H, int W, int C, int mode, int mask_act,
                       float slope, void* stream) {
    AESR_CHECK_ARG(gout && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "aesr_resample2_bwd: bad arguments (C %% 4 == 0)");
    AESR_CHECK_ARG(mode >= AESR_RS_POOL && mode <= AESR_RS_BILINEAR, "aesr_resample2_bwd: unknown mode %d", mode);
    AESR_CHECK_ARG(mode != AESR_RS_POOL || (H >= 2 && W >= 2), "aesr_resample2_bwd: pooling needs H, W >= 2");
    return aesr_launch_resample2(nullptr, gout, x_saved, dx, N, H, W, C, mode, 1, x_saved ? mask_act : ACT_NONE, slope,
                                 (hipStream_t)stream);
}

int aesr_bn_stats(const float* y, float* partial, double* sums, int HW, int C, int G, const int* nstart_host, void* stream) {
    BnGroups gr;
    AESR_CHECK_ARG(y && partial && sums && fill_groups(&gr, G, nstart_host), "aesr_bn_stats: bad arguments");
    if (int e = aesr_launch_bn_stats(y, partial, HW, C, gr, AESR_BN_NWG, (hipStream_t)stream)) return e;
    return aesr_launch_bn_reduce_pivot(partial, sums, AESR_BN_NWG, C, y, HW, gr, (hipStream_t)stream);
}

int aesr_bn_finalize(const double* sums, const double* counts_host, const float* gamma, const float* beta, float* running_mean,
                     float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd, float* scale, float* shift,
                     int C, int G, float momentum, float eps, int train, int update_running, void* stream) {
    AESR_CHECK_ARG(gamma && beta && mean && invstd && scale && shift && G >= 1 && G <= 4, "aesr_bn_finalize: bad arguments");
    AESR_CHECK_ARG(!train || (sums && counts_host), "aesr_bn_finalize: train mode needs sums and counts");
    AESR_CHECK_ARG(train || (running_mean && running_var), "aesr_bn_finalize: eval mode needs running stats");
    return aesr_launch_bn_finalize(sums, counts_host, gamma, beta, running_mean, running_var, (long long*)num_batches_tracked, mean,
                                   invstd, scale, shift, C, G, momentum, eps, train, update_running && running_mean && running_var,
                                   (hipStream_t)stream);
}

int aesr_bn_stats_finalize(const float* y, float* partial, const double* counts_host, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                           float* scale, float* shift, int HW, int C, int G, const int* nstart_host, float momentum, float eps,
                           int update_running, void* stream) {
    BnGroups gr;
    AESR_CHECK_ARG(y && partial && counts_host && fill_groups(&gr, G, nstart_host), "aesr_bn_stats_finalize: bad arguments");
    AESR_CHECK_ARG(gamma && beta && mean && invstd && scale && shift, "aesr_bn_stats_finalize: null pointer");
    if (int e = aesr_launch_bn_stats(y, partial, HW, C, gr, AESR_BN_NWG, (hipStream_t)stream)) return e;
    return aesr_launch_bn_reduce_finalize(partial, AESR_BN_NWG, y, HW, gr, counts_host, gamma, beta, running_mean, running_var,
                                          (long long*)num_batches_tracked, mean, invstd, scale, shift, C, momentum, eps,
                                          update_running && running_mean && running_var, (hipStream_t)stream);
}

static void bn_out_dims(int H, int W, int mode, int* Ho, int* Wo) {
    if (mode == AESR_BN_POOL) { *Ho = H / 2; *Wo = W / 2; }
    else if (mode == AESR_BN_UP) { *Ho = 2 * H; *Wo = 2 * W; }
    else { *Ho = H; *Wo = W; }
}

// The argument blocks of the apply / backward kernels: pointers, dims (with the output's) and groups; false: bad groups.  The entry points
// check their own pointers (each needs another subset) and what else they refuse.
static bool bn_apply_args(BnApplyArgs* a, const float* y, const float* scale, const float* shift, float* out, int N, int H, int W, int C,
                          int mode, int G, const int* nstart_host) {
    a->y = y; a->scale = scale; a->shift = shift; a->out = out; a->N = N; a->H = H; a->W = W; a->C = C; a->mode = mode;
    bn_out_dims(H, W, mode, &a->Ho, &a->Wo);
    return fill_groups(&a->gr, G, nstart_host);
}

static bool bn_bwd_args(BnBwdArgs* a, const float* gout, const float* y, const float* mean, const float* invstd, const float* scale,
                        float* coef, float* partial, float* dpre, int N, int H, int W, int C, int mode, int act, float slope, int G,
                        const int* nstart_host) {
    memset(a, 0, sizeof(*a));
    a->gout = gout; a->y = y; a->mean = mean; a->invstd = invstd; a->scale = scale; a->coef = coef; a->partial = partial; a->dpre = dpre;
    a->N = N; a->H = H; a->W = W; a->C = C; a->mode = mode; a->act = act; a->slope = slope;
    bn_out_dims(H, W, mode, &a->Ho, &a->Wo);
    return fill_groups(&a->gr, G, nstart_host);
}

int aesr_bn_apply(const float* y, const float* scale, const float* shift, float* out, int N, int H, int W, int C, int mode,
                  int G, const int* nstart_host, void* stream) {
    BnApplyArgs a;
    AESR_CHECK_ARG(y && scale && shift && out && bn_apply_args(&a, y, scale, shift, out, N, H, W, C, mode, G, nstart_host),
                   "aesr_bn_apply: bad arguments");
    AESR_CHECK_ARG(a.Ho > 0 && a.Wo > 0, "aesr_bn_apply: empty output");
    return aesr_launch_bn_apply(a, (hipStream_t)stream);
}

int aesr_bn_fused_supported(int C, int G) { return aesr_bn_fused_ok(C, G) ? 1 : 0; }

int aesr_bn_fused1_supported(int N, int H, int W, int C, int mode, int G, int backward) {
    if (mode != AESR_BN_NONE && mode != AESR_BN_POOL) return 0;
    return aesr_bn_fused1_ok(N, H, W, C, mode == AESR_BN_POOL, G, backward) ? 1 : 0;
}

size_t aesr_bn_fused1_workspace_floats(int C, int G) { return (size_t)256 * G * 2 * C; }
size_t aesr_bn_fused1_barrier_words(void) { return 16 * 32; }
unsigned int aesr_bn_fused1_timeouts(void) { return aesr_bn_fused_timeouts_impl(); }

// the caller's exchange arguments of the *_p2p entry points, as given (fill_p2p checks them)
struct BnP2P { void* const* peers_host; int world, rank, slot; const unsigned int* gen_dev; };

static int fill_p2p(BnFusedArgs* a, const BnP2P& p, const char* who) {
    if (!p.peers_host || !p.gen_dev || p.world < 1 || p.world > 8 || p.rank < 0 || p.rank >= p.world || p.slot < 0 || p.slot >= AESR_P2P_SLOTS) {
        aesr_set_error("%s: bad exchange arguments (world %d, rank %d, slot %d of %d)", who, p.world, p.rank, p.slot, AESR_P2P_SLOTS);
        return AESR_ERR_ARG;
    }
    a->world = p.world; a->rank = p.rank; a->slot = p.slot; a->gen = p.gen_dev;
    for (int r = 0; r < p.world; ++r) {
        if (!p.peers_host[r]) {
            aesr_set_error("%s: the region of rank %d is not mapped", who, r);
            return AESR_ERR_ARG;
        }
        a->peers[r] = (unsigned char*)p.peers_host[r];
    }
    return AESR_OK;
}

// what the forward and the backward entry share: dims, groups, counts, workspace, barrier state and (p2p) the exchange
static int bn_fused1_args(BnFusedArgs* a, const char* who, float* workspace, unsigned int* barrier_state, const double* counts_host, int N, int H,
                          int W, int C, int mode, const BnGroups& gr, const BnP2P* p2p) {
    if (mode != AESR_BN_NONE && mode != AESR_BN_POOL) {
        aesr_set_error(p2p ? "%s: mode %d" : "%s: mode %d (the un-folded Upsample takes the three-launch path)", who, mode);
        return AESR_ERR_ARG;
    }
    a->rec = workspace; a->bar = barrier_state; a->N = N; a->H = H; a->W = W; a->C = C; a->pool = mode == AESR_BN_POOL;
    bn_out_dims(H, W, mode, &a->Ho, &a->Wo);
    a->G = gr.G;
    a->counts = bn_counts(counts_host, gr.G);
    memcpy(a->nstart, gr.nstart, sizeof(a->nstart));
    return p2p ? fill_p2p(a, *p2p, who) : AESR_OK;
}

static int bn_fused1_fwd(const char* who, const float* y, float* out, float* workspace, unsigned int* barrier_state, const double* counts_host,
                         const float* gamma, const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                         float* invstd, float* scale, float* shift, int N, int H, int W, int C, int mode, int G, const int* nstart_host,
                         float momentum, float eps, int update_running, const BnP2P* p2p, void* stream) {
    BnGroups gr;
    BnFusedArgs a = {};
    AESR_CHECK_ARG(y && out && workspace && barrier_state && counts_host && gamma && beta && mean && invstd && scale && shift &&
                       fill_groups(&gr, G, nstart_host) && gr.nstart[G] == N, "%s: bad arguments", who);
    if (int e = bn_fused1_args(&a, who, workspace, barrier_state, counts_host, N, H, W, C, mode, gr, p2p)) return e;
    a.y = y; a.out = out; a.gamma = gamma; a.beta = beta; a.running_mean = running_mean; a.running_var = running_var;
    a.nbt = (long long*)num_batches_tracked; a.mean = mean; a.invstd = invstd; a.scale = scale; a.shift = shift;
    a.momentum = momentum; a.eps = eps; a.update_running = update_running && running_mean && running_var; a.act = ACT_NONE;
    return aesr_launch_bn_fused(a, 0, (hipStream_t)stream);
}

static int bn_fused1_bwd(const char* who, const float* gout, const float* y, const float* mean, const float* invstd, const float* scale,
                         float* workspace, unsigned int* barrier_state, const double* counts_host, float* coef, float* dgamma, float* dbeta,
                         float* dpre, int N, int H, int W, int C, int mode, int act, float slope, int G, const int* nstart_host, const BnP2P* p2p,
                         void* stream) {
    BnGroups gr;
    BnFusedArgs a = {};
    AESR_CHECK_ARG(gout && y && mean && invstd && scale && workspace && barrier_state && counts_host && coef && dgamma && dbeta && dpre &&
                       fill_groups(&gr, G, nstart_host) && gr.nstart[G] == N, "%s: bad arguments", who);
    if (int e = bn_fused1_args(&a, who, workspace, barrier_state, counts_host, N, H, W, C, mode, gr, p2p)) return e;
    a.y = y; a.gout = gout; a.out = dpre; a.mean_in = mean; a.invstd_in = invstd; a.scale_in = scale; a.coef = coef; a.dgamma = dgamma;
    a.dbeta = dbeta; a.act = act; a.slope = slope;
    return aesr_launch_bn_fused(a, 1, (hipStream_t)stream);
}

int aesr_bn_fused1_fwd(const float* y, float* out, float* workspace, unsigned int* barrier_state, const double* counts_host, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                       float* scale, float* shift, int N, int H, int W, int C, int mode, int G, const int* nstart_host, float momentum, float eps,
                       int update_running, void* stream) {
    return bn_fused1_fwd("aesr_bn_fused1_fwd", y, out, workspace, barrier_state, counts_host, gamma, beta, running_mean, running_var,
                         num_batches_tracked, mean, invstd, scale, shift, N, H, W, C, mode, G, nstart_host, momentum, eps, update_running, nullptr, stream);
}

int aesr_bn_fused1_bwd(const float* gout, const float* y, const float* mean, const float* invstd, const float* scale, float* workspace,
                       unsigned int* barrier_state, const double* counts_host, float* coef, float* dgamma, float* dbeta, float* dpre, int N, int H,
                       int W, int C, int mode, int act, float slope, int G, const int* nstart_host, void* stream) {
    return bn_fused1_bwd("aesr_bn_fused1_bwd", gout, y, mean, invstd, scale, workspace, barrier_state, counts_host, coef, dgamma, dbeta, dpre, N, H, W,
                         C, mode, act, slope, G, nstart_host, nullptr, stream);
}

/* ---- the same two with the SyncBN exchange inside: data parallel over peer-mapped regions ---- */
size_t aesr_p2p_region_bytes(int world) { return world > 0 && world <= 8 ? (size_t)AESR_P2P_SLOTS * 2 * world * AESR_P2P_REC_BYTES : 0; }

int aesr_p2p_tick(unsigned int* gen_dev, void* stream) {
    AESR_CHECK_ARG(gen_dev, "aesr_p2p_tick: null pointer");
    return aesr_launch_p2p_tick(gen_dev, (hipStream_t)stream);
}

int aesr_bn_fused1_fwd_p2p(const float* y, float* out, float* workspace, unsigned int* barrier_state, const double* counts_host, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                           float* scale, float* shift, int N, int H, int W, int C, int mode, int G, const int* nstart_host, float momentum, float eps,
                           int update_running, void* const* peers_host, int world, int rank, int slot, const unsigned int* gen_dev, void* stream) {
    const BnP2P p2p = {peers_host, world, rank, slot, gen_dev};
    return bn_fused1_fwd("aesr_bn_fused1_fwd_p2p", y, out, workspace, barrier_state, counts_host, gamma, beta, running_mean, running_var,
                         num_batches_tracked, mean, invstd, scale, shift, N, H, W, C, mode, G, nstart_host, momentum, eps, update_running, &p2p, stream);
}

int aesr_bn_fused1_bwd_p2p(const float* gout, const float* y, const float* mean, const float* invstd, const float* scale, float* workspace,
                           unsigned int* barrier_state, const double* counts_host, float* coef, float* dgamma, float* dbeta, float* dpre, int N, int H,
                           int W, int C, int mode, int act, float slope, int G, const int* nstart_host, void* const* peers_host, int world, int rank,
                           int slot, const unsigned int* gen_dev, void* stream) {
    const BnP2P p2p = {peers_host, world, rank, slot, gen_dev};
    return bn_fused1_bwd("aesr_bn_fused1_bwd_p2p", gout, y, mean, invstd, scale, workspace, barrier_state, counts_host, coef, dgamma, dbeta, dpre, N, H,
                         W, C, mode, act, slope, G, nstart_host, &p2p, stream);
}

int aesr_bn_finalize_apply(const double* sums, const double* counts_host, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd, float* scale, float* shift,
                           const float* y, float* out, int N, int H, int W, int C, int mode, int G, const int* nstart_host, float momentum,
                           float eps, int update_running, void* stream) {
    BnApplyArgs a;
    AESR_CHECK_ARG(sums && counts_host && gamma && beta && mean && invstd && scale && shift && y && out &&
                       bn_apply_args(&a, y, scale, shift, out, N, H, W, C, mode, G, nstart_host), "aesr_bn_finalize_apply: bad arguments");
    AESR_CHECK_ARG(aesr_bn_fused_ok(C, G), "aesr_bn_finalize_apply: %d groups x %d channels exceed the kernel's tables (aesr_bn_fused_supported)", G, C);
    AESR_CHECK_ARG(a.Ho > 0 && a.Wo > 0, "aesr_bn_finalize_apply: empty output");
    return aesr_launch_bn_finalize_apply(sums, counts_host, gamma, beta, running_mean, running_var, (long long*)num_batches_tracked, mean, invstd,
                                         scale, shift, momentum, eps, update_running && running_mean && running_var, G, a, (hipStream_t)stream);
}

int aesr_bn_bwd_reduce(const float* gout, const float* y, const float* mean, const float* invstd, float* partial, double* sums,
                       int N, int H, int W, int C, int mode, int G, const int* nstart_host, void* stream) {
    BnBwdArgs a;
    AESR_CHECK_ARG(gout && y && mean && invstd && partial && sums &&
                       bn_bwd_args(&a, gout, y, mean, invstd, nullptr, nullptr, partial, nullptr, N, H, W, C, mode, 0, 0.f, G, nstart_host),
                   "aesr_bn_bwd_reduce: bad arguments");
    AESR_CHECK_ARG((double)N * H * W < 2147483648.0, "aesr_bn_bwd_reduce: more than 2^31 pixels");
    if (int e = aesr_launch_bn_bwd_reduce(a, AESR_BN_NWG, (hipStream_t)stream)) return e;
    return aesr_launch_bn_reduce(partial, sums, AESR_BN_NWG, C, G, (hipStream_t)stream);
}

int aesr_bn_bwd_apply(const float* gout, const float* y, const float* mean, const float* invstd, const float* scale,
                      const double* sums, const double* counts_host, float* coef, float* dgamma, float* dbeta, float* dpre, int N,
                      int H, int W, int C, int mode, int act, float slope, int G, const int* nstart_host, void* stream) {
    BnBwdArgs a;
    AESR_CHECK_ARG(gout && y && mean && invstd && scale && sums && counts_host && coef && dgamma && dbeta && dpre &&
                       bn_bwd_args(&a, gout, y, mean, invstd, scale, coef, nullptr, dpre, N, H, W, C, mode, act, slope, G, nstart_host),
                   "aesr_bn_bwd_apply: bad arguments");
    if (aesr_bn_fused_ok(C, G))          // coef / dgamma / dbeta from the sums in the apply kernel's prologue: one launch
        return aesr_launch_bn_bwd_finalize_apply(sums, counts_host, coef, dgamma, dbeta, G, a, (hipStream_t)stream);
    if (int e = aesr_launch_bn_bwd_finalize(sums, counts_host, coef, dgamma, dbeta, C, G, (hipStream_t)stream)) return e;
    return aesr_launch_bn_bwd_apply(a, (hipStream_t)stream);
}

int aesr_bn_bwd(const float* gout, const float* y, const float* mean, const float* invstd, const float* scale, float* partial,
                const double* counts_host, float* coef, float* dgamma, float* dbeta, float* dpre, int N, int H, int W, int C,
                int mode, int act, float slope, int G, const int* nstart_host, void* stream) {
    BnBwdArgs a;
    AESR_CHECK_ARG(gout && y && mean && invstd && scale && partial && counts_host && coef && dgamma && dbeta && dpre &&
                       bn_bwd_args(&a, gout, y, mean, invstd, scale, coef, partial, dpre, N, H, W, C, mode, act, slope, G, nstart_host),
                   "aesr_bn_bwd: bad arguments");
    AESR_CHECK_ARG((double)N * H * W < 2147483648.0, "aesr_bn_bwd: more than 2^31 pixels");
    if (int e = aesr_launch_bn_bwd_reduce(a, AESR_BN_NWG, (hipStream_t)stream)) return e;
    if (int e = aesr_launch_bn_bwd_reduce_finalize(partial, AESR_BN_NWG, counts_host, coef, dgamma, dbeta, C, G, (hipStream_t)stream))
        return e;
    return aesr_launch_bn_bwd_apply(a, (hipStream_t)stream);
}

// ---- include/aesr_hip_bnpool.h: BatchNorm + AvgPool2d(2), pooled once in the statistics pass ------------------------------------------
int aesr_bn_pool_supported(int N, int H, int W, int C, int G) {
    if (C < 4 || C % 4 != 0 || C > 1024 || 256 % (C / 4) != 0) return 0;        // what the kernels' (channel quad, lane) layout takes
    if (H < 2 || W < 2 || G < 1 || G > 4 || N < G) return 0;
    return (double)N * H * W < 2147483648.0 ? 1 : 0;
}

// the shape and the group table of an entry point of this header: groups non-empty, in order, covering exactly the N images
static bool bn_pool_groups(BnGroups* gr, int N, int H, int W, int C, int G, const int* nstart_host) {
    if (!aesr_bn_pool_supported(N, H, W, C, G) || !fill_groups(gr, G, nstart_host)) return false;
    if (gr->nstart[0] != 0 || gr->nstart[G] != N) return false;
    for (int g = 0; g < G; ++g)
        if (gr->nstart[g + 1] <= gr->nstart[g]) return false;
    return true;
}

int aesr_bn_pool_stats_finalize(const float* y, float* m, float* partial, const double* counts_host, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                                float* scale, float* shift, int N, int H, int W, int C, int G, const int* nstart_host, float momentum,
                                float eps, int update_running, void* stream) {
    BnPoolStatsArgs a;
    memset(&a, 0, sizeof(a));
    AESR_CHECK_ARG(y && m && partial && counts_host && gamma && beta && mean && invstd && scale && shift,
                   "aesr_bn_pool_stats_finalize: null pointer");
    AESR_CHECK_ARG(bn_pool_groups(&a.gr, N, H, W, C, G, nstart_host),
                   "aesr_bn_pool_stats_finalize: N=%d H=%d W=%d C=%d G=%d or the group table is not supported (aesr_bn_pool_supported)", N, H, W, C, G);
    a.y = y; a.m = m; a.partial = partial; a.H = H; a.W = W; a.C = C; a.Ho = H / 2; a.Wo = W / 2;
    if (int e = aesr_launch_bn_pool_stats(a, AESR_BN_NWG, (hipStream_t)stream)) return e;
    return aesr_launch_bn_reduce_finalize(partial, AESR_BN_NWG, y, H * W, a.gr, counts_host, gamma, beta, running_mean, running_var,
                                          (long long*)num_batches_tracked, mean, invstd, scale, shift, C, momentum, eps,
                                          update_running && running_mean && running_var, (hipStream_t)stream);
}

int aesr_bn_pool_apply(const float* m, const float* scale, const float* shift, float* out, int N, int Ho, int Wo, int C, int G,
                       const int* nstart_host, void* stream) {
    BnGroups gr;
    AESR_CHECK_ARG(m && scale && shift && out, "aesr_bn_pool_apply: null pointer");
    AESR_CHECK_ARG(Ho >= 1 && Wo >= 1 && (double)Ho * Wo < 536870912.0 && bn_pool_groups(&gr, N, 2 * Ho, 2 * Wo, C, G, nstart_host),
                   "aesr_bn_pool_apply: N=%d Ho=%d Wo=%d C=%d G=%d or the group table is not supported (aesr_bn_pool_supported)", N, Ho, Wo, C, G);
    return aesr_launch_bn_pool_apply(m, scale, shift, out, Ho * Wo, C, gr, (hipStream_t)stream);
}

int aesr_bn_pool_bwd(const float* gout, const float* y, const float* m, const float* mean, const float* invstd, const float* scale,
                     float* partial, const double* counts_host, float* coef, float* dgamma, float* dbeta, float* dpre, int N, int H, int W,
                     int C, int act, float slope, int G, const int* nstart_host, void* stream) {
    BnBwdArgs a;
    AESR_CHECK_ARG(gout && y && m && mean && invstd && scale && partial && counts_host && coef && dgamma && dbeta && dpre,
                   "aesr_bn_pool_bwd: null pointer");
    AESR_CHECK_ARG(act >= ACT_NONE && act <= ACT_SIGMOID, "aesr_bn_pool_bwd: unknown activation code %d", act);
    AESR_CHECK_ARG(bn_bwd_args(&a, gout, y, mean, invstd, scale, coef, partial, dpre, N, H, W, C, AESR_BN_POOL, act, slope, G, nstart_host) &&
                       bn_pool_groups(&a.gr, N, H, W, C, G, nstart_host),
                   "aesr_bn_pool_bwd: N=%d H=%d W=%d C=%d G=%d or the group table is not supported (aesr_bn_pool_supported)", N, H, W, C, G);
    if (int e = aesr_launch_bn_pool_bwd_reduce(gout, m, mean, invstd, partial, a.Ho * a.Wo, C, a.gr, AESR_BN_NWG, (hipStream_t)stream)) return e;
    if (int e = aesr_launch_bn_bwd_reduce_finalize(partial, AESR_BN_NWG, counts_host, coef, dgamma, dbeta, C, G, (hipStream_t)stream))
        return e;
    return aesr_launch_bn_bwd_apply(a, (hipStream_t)stream);
}

int aesr_maxpool2_fwd(const float* x, float* out, int N, int H, int W, int C, void* stream) {
    AESR_CHECK_ARG(x && out && N > 0 && H >= 2 && W >= 2 && C % 4 == 0, "aesr_maxpool2_fwd: bad arguments (C %% 4 == 0, H,W >= 2)");
    return aesr_launch_maxpool2_fwd(x, out, N, H, W, C, (hipStream_t)stream);
}

int aesr_maxpool2_bwd(const float* gout, const float* x, const float* gadd, float* dx, int N, int H, int W, int C, int relu_mask,
                      void* stream) {
    AESR_CHECK_ARG(gout && x && dx && N > 0 && H >= 2 && W >= 2 && C % 4 == 0, "aesr_maxpool2_bwd: bad arguments");
    return aesr_launch_maxpool2_bwd(gout, x, gadd, dx, N, H, W, C, relu_mask, (hipStream_t)stream);
}

int aesr_scale_expand_fwd(const float* x, float* out4, size_t n, const float* ca_host, const float* cb_host, void* stream) {
    AESR_CHECK_ARG(x && out4 && ca_host && cb_host && n > 0 && n < ((size_t)1 << 29), "aesr_scale_expand_fwd: bad arguments");
    return aesr_launch_scale_expand(x, out4, (int)n, ca_host, cb_host, 0, (hipStream_t)stream);
}

int aesr_scale_expand_bwd(const float* d4, float* dx, size_t n, const float* ca_host, void* stream) {
    AESR_CHECK_ARG(d4 && dx && ca_host && n > 0 && n < ((size_t)1 << 29), "aesr_scale_expand_bwd: bad arguments");
    return aesr_launch_scale_expand(d4, dx, (int)n, ca_host, nullptr, 1, (hipStream_t)stream);
}

int aesr_lpips_tap_fwd(const float* f, const float* lin_w, float* partial, int B, int HW, int C, void* stream) {
    AESR_CHECK_ARG(f && lin_w && partial && B > 0 && HW > 0, "aesr_lpips_tap_fwd: bad arguments");
    return aesr_launch_lpips_tap_fwd(f, lin_w, partial, B, HW, C, (hipStream_t)stream);
}

int aesr_lpips_tap_bwd(const float* f, const float* lin_w, const float* gd, float* gf0, int B, int HW, int C, void* stream) {
    AESR_CHECK_ARG(f && lin_w && gd && gf0 && B > 0 && HW > 0, "aesr_lpips_tap_bwd: bad arguments");
    return aesr_launch_lpips_tap_bwd(f, lin_w, gd, gf0, B, HW, C, (hipStream_t)stream);
}

int aesr_lpips_finalize(const float* const* partials_host, const int* hw_host, int ntaps, float* d, int B, void* stream) {
    AESR_CHECK_ARG(partials_host && hw_host && d && ntaps >= 1 && ntaps <= 8 && B > 0, "aesr_lpips_finalize: bad arguments");
    return aesr_launch_lpips_finalize(partials_host, hw_host, ntaps, d, B, (hipStream_t)stream);
}

int aesr_space_to_depth2(const float* x, float* out, int N, int H, int W, int C, void* stream) {
    AESR_CHECK_ARG(x && out && N > 0 && H >= 2 && W >= 2 && C % 4 == 0, "aesr_space_to_depth2: bad arguments (C %% 4 == 0, H,W >= 2)");
    return aesr_launch_s2d(x, out, N, H, W, C, 0, (hipStream_t)stream);
}

int aesr_depth_to_space2(const float* g, float* dx, int N, int H, int W, int C, void* stream) {
    AESR_CHECK_ARG(g && dx && N > 0 && H >= 2 && W >= 2 && C % 4 == 0, "aesr_depth_to_space2: bad arguments (C %% 4 == 0, H,W >= 2)");
    return aesr_launch_s2d(g, dx, N, H, W, C, 1, (hipStream_t)stream);
}

int aesr_lerp_fwd(const float* z, const float* a_from, const float* a_to, float* zmix, int B, size_t per, void* stream) {
    AESR_CHECK_ARG(z && a_from && a_to && zmix && B > 0 && per % 4 == 0, "aesr_lerp_fwd: bad arguments (per %% 4 == 0)");
    return aesr_launch_lerp_fwd(z, a_from, a_to, zmix, B, per, (hipStream_t)stream);
}

int aesr_lerp_bwd(const float* dzmix, const float* a_from, const float* a_to, float* dz, int B, size_t per, void* stream) {
    AESR_CHECK_ARG(dzmix && a_from && a_to && dz && B > 0 && per % 4 == 0, "aesr_lerp_bwd: bad arguments (per %% 4 == 0)");
    return aesr_launch_lerp_bwd(dzmix, a_from, a_to, dz, B, per, (hipStream_t)stream);
}

int aesr_lerp_cat_fwd(const float* z, const float* a_from, const float* a_to, float* zcat, int B, size_t per, void* stream) {
    AESR_CHECK_ARG(z && a_from && a_to && zcat && z != zcat && B > 0 && per % 4 == 0, "aesr_lerp_cat_fwd: bad arguments (per %% 4 == 0)");
    return aesr_launch_lerp_cat_fwd(z, a_from, a_to, zcat, B, per, (hipStream_t)stream);
}

int aesr_lerp_multi(const float* z, float* out, int Z, size_t per_slice, const float* alphas_host, int n, int act, float slope,
                    void* stream) {
    AESR_CHECK_ARG(z && out && alphas_host && Z >= 2 && per_slice > 0 && per_slice % 4 == 0, "aesr_lerp_multi: bad arguments (two slices or more, per_slice %% 4 == 0)");
    AESR_CHECK_ARG(n >= 1 && n <= 16, "aesr_lerp_multi: %d mixing coefficients per call (1..16)", n);
    AESR_CHECK_ARG(act == ACT_NONE || act == ACT_RELU || (act == ACT_LRELU && slope >= 0.f && slope <= 1.f),
                   "aesr_lerp_multi: activation %d (none, ReLU, or LeakyReLU with a slope in [0, 1])", act);
    const float nslope = act == ACT_LRELU ? slope : (act == ACT_RELU ? 0.f : 1.f);
    return aesr_launch_lerp_multi(z, out, Z, per_slice, alphas_host, n, nslope, (hipStream_t)stream);
}

int aesr_interleave_clamp(const float* orig, const float* synth, float* out, int Z, int n, size_t per_slice, float lo, float hi, void* stream) {
    AESR_CHECK_ARG(orig && out && Z >= 1 && n >= 0 && per_slice > 0 && per_slice % 4 == 0 && (synth || n == 0 || Z == 1) && orig != out && synth != out,
                   "aesr_interleave_clamp: bad arguments (per_slice %% 4 == 0, out apart from its inputs)");
    AESR_CHECK_ARG(lo <= hi, "aesr_interleave_clamp: empty range [%g, %g]", (double)lo, (double)hi);
    return aesr_launch_interleave_clamp(orig, synth, out, Z, Z > 1 ? n : 0, per_slice, lo, hi, (hipStream_t)stream);
}

int aesr_lerp_cat_bwd(const float* g, const float* a_from, const float* a_to, float* dz, int B, size_t per, void* stream) {
    AESR_CHECK_ARG(g && a_from && a_to && dz && g != dz && B > 0 && per % 4 == 0, "aesr_lerp_cat_bwd: bad arguments (per %% 4 == 0)");
    return aesr_launch_lerp_cat_bwd(g, a_from, a_to, dz, B, per, (hipStream_t)stream);
}

int aesr_mse_fwd(const float* a, const float* b, double* partial, float* loss, size_t n, void* stream) {
    AESR_CHECK_ARG(a && b && partial && loss && n > 0, "aesr_mse_fwd: bad arguments");
    return aesr_launch_mse_fwd(a, b, partial, AESR_MSE_NPART, loss, n, (hipStream_t)stream);
}

int aesr_mse3_fwd(const float* a1, const float* b1, size_t n1, const float* a2, const float* b2, size_t n2, const float* a3,
                  const float* b3, size_t n3, const float* lam, double* workspace, float* out4, void* stream) {
    AESR_CHECK_ARG(a1 && b1 && n1 > 0 && a2 && b2 && n2 > 0 && (!a3 || (b3 && n3 > 0)) && lam && workspace && out4, "aesr_mse3_fwd: bad arguments");
    const float* a[3] = {a1, a2, a3};
    const float* b[3] = {b1, b2, a3 ? b3 : nullptr};
    const size_t n[3] = {n1, n2, a3 ? n3 : 1};
    return aesr_launch_mse3_fwd(a, b, n, lam, workspace, out4, (hipStream_t)stream);
}

int aesr_mse3_bwd(const float* a1, const float* b1, size_t n1, const float* a2, const float* b2, size_t n2, const float* lam,
                  const float* gloss, float* d1, float* d2, void* stream) {
    AESR_CHECK_ARG(a1 && b1 && n1 > 0 && a2 && b2 && n2 > 0 && lam && gloss && d1 && d2, "aesr_mse3_bwd: bad arguments");
    return aesr_launch_mse3_bwd(a1, b1, n1, a2, b2, n2, lam, gloss, d1, d2, (hipStream_t)stream);
}

int aesr_mse_bwd(const float* a, const float* b, const float* gloss, float* da, size_t n, void* stream) {
    AESR_CHECK_ARG(a && b && gloss && da && n > 0, "aesr_mse_bwd: bad arguments");
    return aesr_launch_mse_bwd(a, b, gloss, da, n, (hipStream_t)stream);
}

int aesr_l1_fwd(const float* a, const float* b, double* partial, float* loss, size_t n, void* stream) {
    AESR_CHECK_ARG(a && b && partial && loss && n > 0, "aesr_l1_fwd: bad arguments");
    return aesr_launch_l1_fwd(a, b, partial, AESR_MSE_NPART, loss, n, (hipStream_t)stream);
}

int aesr_l1_bwd(const float* a, const float* b, const float* gloss, float* da, size_t n, void* stream) {
    AESR_CHECK_ARG(a && b && gloss && da && n > 0, "aesr_l1_bwd: bad arguments");
    return aesr_launch_l1_bwd(a, b, gloss, da, n, (hipStream_t)stream);
}

int aesr_row_mean_fwd(const float* x, float* out, int N, size_t M, void* stream) {
    AESR_CHECK_ARG(x && out && N > 0 && M > 0, "aesr_row_mean_fwd: bad arguments");
    return aesr_launch_row_mean_fwd(x, out, N, M, (hipStream_t)stream);
}

int aesr_row_mean_bwd(const float* g, float* dx, int N, size_t M, void* stream) {
    AESR_CHECK_ARG(g && dx && N > 0 && M > 0, "aesr_row_mean_bwd: bad arguments");
    return aesr_launch_row_mean_bwd(g, dx, N, M, (hipStream_t)stream);
}

int aesr_lap_blur5(const float* in, const float* add, float* out, int P, int H, int W, float gain, int adjoint, void* stream) {
    AESR_CHECK_ARG(in && out && P > 0 && H >= 3 && W >= 3, "aesr_lap_blur5: bad arguments (reflect padding by 2 needs H, W >= 3)");
    AESR_CHECK_ARG(in != out, "aesr_lap_blur5: in-place filtering is not supported");
    return aesr_launch_lap_blur5(in, add, out, P, H, W, gain, adjoint ? 1 : 0, (hipStream_t)stream);
}

int aesr_lap_down2(const float* in, float* out, int P, int H, int W, void* stream) {
    AESR_CHECK_ARG(in && out && P > 0 && H > 0 && W > 0, "aesr_lap_down2: bad arguments");
    return aesr_launch_lap_down2(in, out, P, H, W, (hipStream_t)stream);
}

int aesr_lap_zero_insert2(const float* in, float* out, int P, int h, int w, int H, int W, void* stream) {
    AESR_CHECK_ARG(in && out && P > 0 && h > 0 && w > 0 && (H + 1) / 2 == h && (W + 1) / 2 == w,
                   "aesr_lap_zero_insert2: need h == ceil(H/2), w == ceil(W/2)");
    return aesr_launch_lap_zero_insert2(in, out, P, h, w, H, W, (hipStream_t)stream);
}

int aesr_act_bwd(const float* dout, const float* y, float* dpre, size_t n, int act, float slope, void* stream) {
    AESR_CHECK_ARG(dout && y && dpre && n > 0, "aesr_act_bwd: bad arguments");
    return aesr_launch_act_bwd(dout, y, dpre, n, act, slope, (hipStream_t)stream);
}

void aesr_adam_state_init(float* state_host8, double steps_done, double beta1, double beta2) {
    // the same chain of double multiplications the kernel runs step after step (NOT pow): an optimizer resumed from a checkpoint
    // continues bit for bit like the one that was never stopped
    double b1p = beta1, b2p = beta2;
    for (long k = 0; k < (long)steps_done; ++k) {
        b1p = aesr_adam_next_power(b1p, beta1);
        b2p = aesr_adam_next_power(b2p, beta2);
    }
    state_host8[0] = (float)steps_done;
    state_host8[1] = (float)(1.0 - b1p);
    state_host8[2] = (float)sqrt(1.0 - b2p);
    state_host8[3] = 0.f;
    memcpy(state_host8 + 4, &b1p, sizeof(double));
    memcpy(state_host8 + 6, &b2p, sizeof(double));
}

int aesr_adam_step(float* p, float* g, float* exp_avg, float* exp_avg_sq, float* state, size_t n, float lr, double beta1,
                   double beta2, float eps, float weight_decay, int zero_grad, void* stream) {
    AESR_CHECK_ARG(p && g && exp_avg && exp_avg_sq && state && n > 0, "aesr_adam_step: bad arguments");
    return aesr_launch_adam(p, g, exp_avg, exp_avg_sq, state, n, lr, beta1, beta2, eps, weight_decay, zero_grad, (hipStream_t)stream);
}

// descriptor checks and table fill shared by aesr_triplet_assemble and aesr_triplet_assemble_raw (include/aesr_hip_dataprep.h)
static int triplet_table(const char* who, const float* volumes, const aesr_triplet_desc* desc_host, int B, int width, const float* image,
                         const float* between, TripletTable& t) {
    AESR_CHECK_ARG(volumes && desc_host && image && between && width > 0, "%s: null pointer or empty shape", who);
    AESR_CHECK_ARG(B >= 1 && B <= TRIPLET_MAX, "%s: B=%d must be 1..%d per call", who, B, TRIPLET_MAX);
    memset(&t, 0, sizeof(t));
    for (int b = 0; b < B; ++b) {
        const aesr_triplet_desc& s = desc_host[b];
        AESR_CHECK_ARG(s.H > 0 && s.W > 0 && s.vol_off >= 0 && s.z_from >= 0 && s.z_to >= 0 && s.z_between >= 0 && s.k >= 0 && s.k <= 3,
                       "%s: bad descriptor %d", who, b);
        TripletDesc& d = t.d[b];
        d.vol_off = s.vol_off; d.H = s.H; d.W = s.W; d.z_from = s.z_from; d.z_to = s.z_to; d.z_between = s.z_between;
        d.oy = s.oy; d.ox = s.ox; d.k = s.k; d.gain = s.gain; d.cutoff = s.cutoff;
    }
    return AESR_OK;
}

int aesr_triplet_assemble(const float* volumes, const aesr_triplet_desc* desc_host, int B, int width, float* image,
                          float* between, void* stream) {
    TripletTable t;
    const int rc = triplet_table("aesr_triplet_assemble", volumes, desc_host, B, width, image, between, t);
    return rc != AESR_OK ? rc : aesr_launch_triplet_assemble(volumes, t, B, width, image, between, (hipStream_t)stream);
}

int aesr_triplet_assemble_raw(const float* volumes, const aesr_triplet_desc* desc_host, int B, int width, float* image, float* between,
                              void* stream) {
    TripletTable t;
    const int rc = triplet_table("aesr_triplet_assemble_raw", volumes, desc_host, B, width, image, between, t);
    return rc != AESR_OK ? rc : aesr_launch_triplet_assemble_raw(volumes, t, B, width, image, between, (hipStream_t)stream);
}

size_t aesr_ssim_workspace_doubles(int Z, int H, int W) { return (size_t)Z * ceil_div(H, 16) * ceil_div(W, 16) * 2; }

int aesr_ssim_mse(const float* a, const float* b, double* workspace, double* ssim, double* mse, int Z, int H, int W, int win,
                  double data_range, double k1, double k2, void* stream) {
    AESR_CHECK_ARG(a && b && workspace && ssim && mse && Z > 0 && H > 0 && W > 0, "aesr_ssim_mse: null pointer or empty shape");
    AESR_CHECK_ARG(win >= 3 && win <= 11 && (win & 1) && win <= H && win <= W,
                   "aesr_ssim_mse: win=%d must be odd, 3..11 and not larger than the image (%dx%d)", win, H, W);
    AESR_CHECK_ARG(data_range > 0.0, "aesr_ssim_mse: data_range must be positive");
    return aesr_launch_ssim_mse(a, b, workspace, ssim, mse, Z, H, W, win, data_range, k1, k2, (hipStream_t)stream);
}

int aesr_long_axis_views(const float* ref, const float* rec, float* ref_view, float* rec_view, unsigned char* black, int Z, int H, int W,
                         int axis, void* stream) {
    AESR_CHECK_ARG(ref && rec && ref_view && rec_view && black, "aesr_long_axis_views: null pointer");
    AESR_CHECK_ARG(axis == 1 || axis == 2, "aesr_long_axis_views: axis=%d must be 1 or 2 (axis 0 is the volume itself)", axis);
    AESR_CHECK_ARG(Z > 0 && H > 0 && W > 0, "aesr_long_axis_views: empty shape %d x %d x %d", Z, H, W);
    AESR_CHECK_ARG((size_t)Z * H < ((size_t)1 << 30) && (size_t)Z * H * W < ((size_t)1 << 30),
                   "aesr_long_axis_views: %d x %d x %d has 2^30 elements or more", Z, H, W);
    return aesr_launch_long_axis_views(ref, rec, ref_view, rec_view, black, Z, H, W, axis, (hipStream_t)stream);
}

// (the shapes aesr_vif_mscale takes; anything else has no workspace: the layout arithmetic is int -- sanitizer sweep, round 6)
size_t aesr_vif_workspace_bytes(int Z, int H, int W) {
    return (Z > 0 && Z <= 65535 && H > 0 && W > 0 && (size_t)H * W < ((size_t)1 << 30)) ? aesr_vif_workspace_bytes_impl(Z, H, W) : 0;
}

int aesr_vif_mscale(const float* ref, const float* dist, void* workspace, double* vif, int Z, int H, int W, const double* weights_host,
                    const int* radii_host, double sigma_nsq, void* stream) {
    AESR_CHECK_ARG(ref && dist && workspace && vif && weights_host && radii_host, "aesr_vif_mscale: null pointer");
    AESR_CHECK_ARG(Z > 0 && Z <= 65535 && H > 0 && W > 0 && (size_t)H * W < ((size_t)1 << 30), "aesr_vif_mscale: unsupported shape %d x %d x %d", Z, H, W);
    AESR_CHECK_ARG(sigma_nsq > 0.0, "aesr_vif_mscale: sigma_nsq must be positive");
    return aesr_launch_vif_mscale(ref, dist, workspace, vif, Z, H, W, weights_host, radii_host, sigma_nsq, (hipStream_t)stream);
}

}  // extern "C"
