// NHWC f32 convolutions for the SuperPoint VGG encoder / heads (gfx950).
#pragma once
#include "common.h"

// Route of a launch: which kernel instantiation the launchers below chose, CONV_ROUTE(kind), and the fused features it ran with (a
// mask of ConvFeature bits: here most of the hand-written index arithmetic sits in the features, not in the choice of kernel).  The
// launch sites store both in the handle (imcui_hip_conv_last_route / _route_counts / _route_features), so the report cannot disagree
// with what ran; host code only.  Values are part of the test interface (imcui_hip/backend.py CONV_ROUTE_KINDS, CONV_FEATURES).
enum ConvRouteKind {
    CR_NONE = 0,             // nothing launched (a refused call, an empty map)
    CR_F32 = 1,              // conv3x3_kernel (exact f32)
    CR_SPLIT_N2 = 2,         // conv3x3_split_kernel<false, 2>
    CR_SPLIT_N4 = 3,         // conv3x3_split_kernel<false, 4>
    CR_SPLIT_N2_SINGLE = 4,  // conv3x3_split_kernel<false, 2, true>
    CR_SPLIT_N4_SINGLE = 5,  // conv3x3_split_kernel<false, 4, true>
    CR_TALL = 6,             // conv3x3_tall_kernel<false>
    CR_TALL_SINGLE = 7,      // conv3x3_tall_kernel<false, true>
    CR_FUSED_8ROW = 8,       // conv3x3_split_kernel<true, 2>
    CR_FUSED_TALL = 9,       // conv3x3_tall_kernel<true>
    CR_CONV1A = 10,          // conv1a_kernel
    CR_NKIND = 11
};
enum ConvFeature {
    CF_POOL = 1,            // fused 2x2 max-pool
    CF_RESID = 2,           // residual map added before the activation
    CF_RESID2 = 4,          // second residual map
    CF_LEAKY = 8,           // activation code 2
    CF_RELU_IN = 16,        // relu bit 2: ReLU on the input while it is staged
    CF_CIN_STRIDE = 32,     // cin_stride != Cin
    CF_COUT_LIVE = 64,      // cout_live < Cout
    CF_HEAD = 128,          // fused point-map head
    CF_HEAD_NO_OUT = 256,   // ... without the 128-channel map
    CF_HEAD_RAW = 512       // ... with the raw 4-channel output
};
#define CONV_ROUTE(kind) (kind)
static_assert(CR_NKIND <= IMCUI_CONV_ROUTE_SLOTS, "route table of imcui_hip_s too small");
static inline void conv_route_note(imcui_hip_s* h, int kind, int features) {
    const int r = CONV_ROUTE(kind);
    h->conv_last_route = r;
    ++h->conv_route_count[r];
    h->conv_route_features[r] |= features;
}

// 3x3, pad 1, stride 1, +bias, +ReLU, optional fused 2x2/2 max-pool.
// in  : [B, H, W, Cin]  (NHWC), Cin % 32 == 0
// wp  : packed weights  [Cin/32][9 taps][8 cq][Cout][4]   (see pack_conv3x3)
// out : [B, H, W, Cout] or, with pool, [B, H/2, W/2, Cout];  Cout % 64 == 0
int conv3x3_launch(imcui_hip_s* h, const float* in, const float* wp, const float* bias, float* out, int B, int H, int W,
                   int Cin, int Cout, int relu, int pool, hipStream_t stream);

// DPT head fused into the epilogue of its last 3x3 convolution (128 channels, ReLU): 1x1 convolution to 4 channels (w [4][128], b [4])
// + point-map post-processing -> pts [B*H*W][3] = xyz / |xyz| * expm1(|xyz|), conf [B*H*W] = 1 + exp(c), raw [B*H*W][4] optional.
// With a head the 128-channel map is written only if `out` is not null.
struct ConvHead {
    const float* w = nullptr;
    const float* b = nullptr;
    float* pts = nullptr;
    float* conf = nullptr;
    float* raw = nullptr;
};

// split-precision variant (imcui_hip_s::precision == 1): weights pre-split into f16 hi / lo planes
//   wh/wl : [Cin/32][9 taps][4 octets][Cout][8 halves] of w * 2^e ; wscale -> 2^-e (device scalar)
//   relu  : activation code 0 none / 1 ReLU / 2 LeakyReLU(0.01);  resid (optional, no pooling): a map of the output's shape
//           added before the activation (residual blocks of the dense matchers' backbones)
int conv3x3_split_launch(imcui_hip_s* h, const float* in, const unsigned short* wh, const unsigned short* wl,
                         const float* wscale, const float* bias, float* out, int B, int H, int W, int Cin, int Cout,
                         int relu, int pool, hipStream_t stream, const float* resid = nullptr, int cin_stride = 0, int cout_live = 0,
                         int single = 0, const float* resid2 = nullptr, const ConvHead* head = nullptr);
// relu bit 2 (value 4): ReLU applied to the INPUT map while it is staged (the producer left it un-activated);  resid2: a second map
// added after resid (out = act(conv + resid + resid2))
// cin_stride: floats between two pixels of `in` when the map stores more channels than the Cin that are used (0 = Cin)
// cout_live: output channels >= cout_live are zero padding of the layer (zero weights and bias): their 32-channel fragments
// are not multiplied, the channels are stored as zeros (0 = Cout)
// single: one f16 product per element pair (hi planes only) instead of three, see GemmP.single
// SuperPoint conv1a (1->64, VALU, evaluated on the fly for the patch) fused into conv1b (64->64, split MFMA):
// image [B,H,W] -> relu(conv1b(relu(conv1a(image)))) (+2x2 max-pool), NHWC out
int conv1ab_fused_split_launch(imcui_hip_s* h, const float* image, const float* w1a, const float* b1a,
                               const unsigned short* wh, const unsigned short* wl, const float* wscale, const float* bias,
                               float* out, int B, int H, int W, int pool, hipStream_t stream);
// host: OIHW -> the split layout above; returns 2^-e
float pack_conv3x3_split(const float* w_oihw, int Cout, int Cin, unsigned short* hi, unsigned short* lo);
// host: the same from the implicit-GEMM layout [Cout][9 taps][Cin] (pack_conv_gemm); planes of 9 * Cin * Cout halves each
float pack_conv3x3_split_from_gemm(const float* w_gemm, int Cout, int Cin, unsigned short* hi, unsigned short* lo, int cin_used = 0);

// first layer: 1 -> 64 channels, 3x3, pad 1, +bias, +ReLU.  in [B,H,W] ; w [9][64] ; out [B,H,W,64]
int conv1a_launch(imcui_hip_s* h, const float* in, const float* w, const float* bias, float* out, int B, int H, int W,
                  hipStream_t stream);

// host-side packers (OIHW -> device layouts above)
void pack_conv3x3(const float* w_oihw, int Cout, int Cin, float* dst);
void pack_conv1a(const float* w_oihw, float* dst);  // [64,1,3,3] -> [9][64]
