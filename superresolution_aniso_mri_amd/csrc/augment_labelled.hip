// On-device batch assembly + augmentation of LABELLED training triplets (include/aesr_hip_labelprep.h): the reference's
// ACDCDatasetEDESPairs.__getitem__ (datasets/ACDC/data_with_labels.py:141-192: [image, labels] of the from / to / between slices, six
// channels) under train_cardiac_aesr.py:83-105 -- AdjustToPatchSize, CenterCrop, RandomCrop, RandomIntensity(slice_mask=[1,0,1,0,1,0]),
// RandomRotation -- and the 6-channel branch of prepare_batch_pairs (datasets/ACDC/data4d_simple.py:349-353), as ONE launch over two
// device-resident caches of the same layout: float32 images and uint8 label maps.
//   out[b][s][0][i][j] = sigm( gain_b * (img_b[z_s][oy_b + u][ox_b + v] - cutoff_b) ),   (u, v) = rot90^-k (i, j)   (csrc/augment.hip)
//   out[b][s][1][i][j] = (float) lab_b[z_s][oy_b + u][ox_b + v]
// Outside the slice the image sample is 0 and goes through the curve (the padding does in the reference); the label is 0 and does NOT
// (the slice mask leaves the label channels out of the curve: padding is background).  A label is a byte that is copied: never
// interpolated, never compared with a class count.  RAW: channel 0 is the image sample unchanged (the test transform).
// The source coordinates of a pixel are computed once and serve both channels; a lane stores 4 bytes per channel, a wave two 256-byte
// row segments.  NCHW: `image` [2B][2][W][W] (all "from" rows, then all "to" rows), `between` [B][2][W][W].
#include <string.h>

#include "../../include/aesr_hip_labelprep.h"
#include "aesr_kernels.h"

template <bool RAW>
__global__ __launch_bounds__(256) void labelled_triplet_assemble_kernel(const float* __restrict__ vol, const uint8_t* __restrict__ lab,
                                                                        TripletTable t, int B, int W, float* __restrict__ image,
                                                                        float* __restrict__ between) {
    const int b = blockIdx.z, s = blockIdx.y;
    const TripletDesc d = t.d[b];
    const int z = s == 0 ? d.z_from : (s == 1 ? d.z_to : d.z_between);
    const size_t slice = (size_t)d.vol_off + (size_t)z * d.H * d.W;          // one offset, in elements, addresses both caches
    const float* src = vol + slice;
    const uint8_t* lsrc = lab + slice;
    const size_t plane = (size_t)W * W;
    float* dst = (s == 2 ? between + (size_t)b * 2 * plane : image + (size_t)(s * B + b) * 2 * plane);
    for (int p = blockIdx.x * 256 + threadIdx.x; p < W * W; p += gridDim.x * 256) {
        const int i = p / W, j = p - i * W;
        int u, v;                                   // np.rot90(X, k, axes=(1, 2)): out[i][j] = X[u][v]
        if (d.k == 0) { u = i; v = j; }
        else if (d.k == 1) { u = j; v = W - 1 - i; }
        else if (d.k == 2) { u = W - 1 - i; v = W - 1 - j; }
        else { u = W - 1 - j; v = i; }
        const int y = d.oy + u, x = d.ox + v;
        float val = 0.f, cls = 0.f;
        if (y >= 0 && y < d.H && x >= 0 && x < d.W) {
            const size_t o = (size_t)y * d.W + x;
            val = src[o];
            cls = (float)lsrc[o];
        }
        dst[p] = RAW ? val : 1.f / (1.f + expf(d.gain * (d.cutoff - val)));
        dst[plane + p] = cls;
    }
}

template <bool RAW>
static int labelled_assemble(const char* who, const float* images, const uint8_t* labels, const aesr_triplet_desc* desc_host, int B, int width,
                             float* image, float* between, void* stream) {
    AESR_CHECK_ARG(images && labels && desc_host && image && between, "%s: null pointer", who);
    AESR_CHECK_ARG(B >= 1 && B <= TRIPLET_MAX, "%s: B=%d must be 1..%d per call", who, B, TRIPLET_MAX);
    AESR_CHECK_ARG(width >= 1, "%s: width=%d must be positive", who, width);
    AESR_CHECK_ARG((size_t)width * width < ((size_t)1 << 30), "%s: width=%d: a %d x %d slice has 2^30 elements or more", who, width, width, width);
    TripletTable t;
    memset(&t, 0, sizeof(t));
    for (int b = 0; b < B; ++b) {
        const aesr_triplet_desc& s = desc_host[b];
        AESR_CHECK_ARG(s.H > 0 && s.W > 0 && (size_t)s.H * s.W < ((size_t)1 << 30), "%s: descriptor %d: slice size %d x %d", who, b, s.H, s.W);
        AESR_CHECK_ARG(s.vol_off >= 0 && s.z_from >= 0 && s.z_to >= 0 && s.z_between >= 0, "%s: descriptor %d: negative offset or slice index", who, b);
        AESR_CHECK_ARG(s.k >= 0 && s.k <= 3, "%s: descriptor %d: k=%d must be 0..3", who, b, s.k);
        TripletDesc& d = t.d[b];
        d.vol_off = s.vol_off; d.H = s.H; d.W = s.W; d.z_from = s.z_from; d.z_to = s.z_to; d.z_between = s.z_between;
        d.oy = s.oy; d.ox = s.ox; d.k = s.k; d.gain = s.gain; d.cutoff = s.cutoff;
    }
    int gx = ceil_div(width * width, 256);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(labelled_triplet_assemble_kernel<RAW>, dim3(gx, 3, B), dim3(256), 0, (hipStream_t)stream, images, labels, t, B, width,
                       image, between);
    AESR_LAUNCH_CHECK(who);
    return AESR_OK;
}

extern "C" {

int aesr_labelled_triplet_assemble(const float* images, const uint8_t* labels, const aesr_triplet_desc* desc_host, int B, int width, float* image,
                                   float* between, void* stream) {
    return labelled_assemble<false>("aesr_labelled_triplet_assemble", images, labels, desc_host, B, width, image, between, stream);
}

int aesr_labelled_triplet_assemble_raw(const float* images, const uint8_t* labels, const aesr_triplet_desc* desc_host, int B, int width,
                                       float* image, float* between, void* stream) {
    return labelled_assemble<true>("aesr_labelled_triplet_assemble_raw", images, labels, desc_host, B, width, image, between, stream);
}

}  // extern "C"
