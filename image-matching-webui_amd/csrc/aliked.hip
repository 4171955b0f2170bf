// ALIKED forward on MI355X (aliked-n16 / aliked-n16rot): the four-block encoder (3x3 convolutions with folded BatchNorm and SELU,
// deformable 3x3 convolutions in blocks 3 and 4), the score head, DKD (simple_nms, border, threshold with the mean fallback, the
// n_limit / top-k cut, soft-argmax refinement) and the sparse deformable descriptor head (SDDH).  Replaces `self.model(data)` of
// imcui/hloc/extractors/aliked.py:24-32 (LightGlue's ALIKED.forward).
//
// Data flow (NHWC maps; Hp x Wp = the image replicate-padded to multiples of 32, InputPadder's even split):
//   block1 3 -> 16 -> 16 at 1/1            fp32 FMA on the VALU, LDS tiles (K = 27 / 144: too shallow for the matrix pipe)
//   block2 16 -> 32 -> 32 at 1/2           implicit-GEMM 3x3 (gemm.hip, both arithmetic modes), 1x1 shortcut + SELU on the VALU
//   block3 32 -> 64 -> 64 at 1/8, block4 64 -> 128 -> 128 at 1/32: offset convolution (18 channels, VALU), ak_deform_kernel (clamp,
//          bilinear gather, zero outside) -> rows [pixels][9 cin], then the shared GEMM (K = 288 .. 1152)
//   f_i = SELU(conv1x1_i(x_i)), 32 channels, stored at 1/2, 1/8, 1/32 -- NOT at 1/1
//   score head: layer 0 (1x1 over the concatenation of bilinear up-samplings) is linear, so it is evaluated branch-wise:
//          W_a f1 + up2(W_b f2) + up8(W_c f3) + up32(W_d f4), 8 channels; f1 is formed in registers from x1.  Then 8 -> 4 -> 4 -> 1.
//   The 128-channel map x1234 and its normalised copy are never formed: the descriptor head evaluates the four branches and the
//   per-pixel L2 norm at the 9 + 16 positions a key-point reads (ak_feat_*), one wave per position, in TWO launches per batch:
//   ak_sddh_offsets_kernel (patches + offset MLP) and ak_sddh_desc_kernel (samples, sf_conv, aggregation on MFMA, L2 norm).
// Summation orders are fixed and every grid is sized by shapes or capacities: an image's result does not depend on its batch, and
// there is no host synchronisation.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "ak_shared.h"
#include "imcui_hip.h"
#include "netpack.h"

#define AK_M 16          // SDDH sample positions
#define AK_KB0 8         // key-points per workgroup step of ak_sddh_offsets_kernel
#define AK_KB1 32        // key-points per workgroup step of ak_sddh_desc_kernel (one 32-row MFMA tile)
#define AK_NLIMIT 20000  // upstream's n_limit_max

// ------------------------------------------------------------------ tensor table (upstream state-dict order)
static const TensorTable& ak_tensors() {
    static const TensorTable table = [] {
        TensorTable t;
        const int ch[5] = {3, 16, 32, 64, 128};
        for (int b = 1; b <= 4; ++b) {
            const int cin = ch[b - 1], cout = ch[b];
            const std::string p = "block" + std::to_string(b);
            for (int j = 1; j <= 2; ++j) {
                const int ci = j == 1 ? cin : cout;
                const std::string c = p + ".conv" + std::to_string(j);
                if (b >= 3) {
                    t.add(c + ".offset_conv.weight", (size_t)18 * ci * 9);
                    t.add(c + ".offset_conv.bias", 18);
                    t.add(c + ".regular_conv.weight", (size_t)cout * ci * 9);
                } else {
                    t.add(c + ".weight", (size_t)cout * ci * 9);
                }
                for (const char* s : {"weight", "bias", "running_mean", "running_var"}) t.add(p + ".bn" + std::to_string(j) + "." + s, cout);
            }
            if (b >= 2) t.add(p + ".downsample.weight", (size_t)cout * cin);
        }
        for (int i = 1; i <= 4; ++i) t.add("conv" + std::to_string(i) + ".weight", (size_t)32 * ch[i]);
        t.add("score_head.0.weight", 8 * 128);
        t.add("score_head.2.weight", 4 * 8 * 9);
        t.add("score_head.4.weight", 4 * 4 * 9);
        t.add("score_head.6.weight", 1 * 4 * 9);
        t.add("desc_head.agg_weights", (size_t)AK_M * 128 * 128);  // (a parameter of the head itself: before its sub-modules)
        t.add("desc_head.offset_conv.0.weight", (size_t)32 * 128 * 9);
        t.add("desc_head.offset_conv.0.bias", 32);
        t.add("desc_head.offset_conv.2.weight", 32 * 32);
        t.add("desc_head.offset_conv.2.bias", 32);
        t.add("desc_head.sf_conv.weight", 128 * 128);
        return t;
    }();
    return table;
}
extern "C" int imcui_hip_aliked_num_tensors(void) { return ak_tensors().size(); }
extern "C" const char* imcui_hip_aliked_tensor_name(int i) { return ak_tensors().name(i); }

// ------------------------------------------------------------------ packed weight layout
// VALU 3x3 layers: w [tap][cin][cout], bias [cout].  0 / 1: block 1; 2..5: the offset convolutions of block3.conv1 / conv2,
// block4.conv1 / conv2; 6..8: score_head.2 / .4 / .6
#define AK_NV 9
static const int AK_VCIN[AK_NV] = {3, 16, 32, 64, 64, 128, 8, 4, 4};
static const int AK_VCOUT[AK_NV] = {16, 16, 18, 18, 18, 18, 4, 4, 1};
// GEMM layers [N][K]: 0 / 1: block 2 (implicit 3x3, input channels stored as 32); 2..5: the deformable products
#define AK_NG 6
static const int AK_GN[AK_NG] = {32, 32, 64, 64, 128, 128};
static const int AK_GK[AK_NG] = {288, 288, 288, 576, 576, 1152};
// 1x1 layers on the VALU, stored transposed [cin][cout]: 0..2 the shortcuts of blocks 2..4, 3..6 conv1..4, 7..10 the four 32-column
// slices of score_head.0, 11 desc_head.offset_conv.2 (with bias)
#define AK_NP 12
static const int AK_PCIN[AK_NP] = {16, 32, 64, 16, 32, 64, 128, 32, 32, 32, 32, 32};
static const int AK_PCOUT[AK_NP] = {32, 64, 128, 32, 32, 32, 32, 8, 8, 8, 8, 32};

struct AkLayout {
    size_t vw[AK_NV], vb[AK_NV];
    GemmLayerOff g[AK_NG];
    size_t pw[AK_NP], pb;
    // descriptor head, f32, K-major: dh0t [9 taps x 128][32] + dh0b [32] (offset_conv.0), sft [128 k][128 n] (sf_conv), agg [16][128 c][128 d]
    size_t dh0t, dh0b, sft, agg;
    size_t total;
};
static AkLayout ak_layout() {
    AkLayout l;
    PackCursor c;
    for (int i = 0; i < AK_NV; ++i) {  // (block1.conv1 first: offset 0 of the packed buffer, see imcui_hip.h)
        l.vw[i] = c.get((size_t)9 * AK_VCIN[i] * AK_VCOUT[i]);
        l.vb[i] = c.get(AK_VCOUT[i]);
    }
    for (int i = 0; i < AK_NG; ++i) l.g[i].place(c, AK_GN[i], AK_GK[i]);
    for (int i = 0; i < AK_NP; ++i) l.pw[i] = c.get((size_t)AK_PCIN[i] * AK_PCOUT[i]);
    l.pb = c.get(32);
    l.dh0t = c.get((size_t)1152 * 32);
    l.dh0b = c.get(32);
    l.sft = c.get((size_t)128 * 128);
    l.agg = c.get((size_t)AK_M * 128 * 128);
    l.total = c.off;
    return l;
}
extern "C" size_t imcui_hip_aliked_packed_floats(void) { return ak_layout().total; }

// t: host pointers of the tensors in imcui_hip_aliked_tensor_name order (shapes checked by the caller)
extern "C" int imcui_hip_aliked_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    const int nt = imcui_hip_aliked_num_tensors();
    for (int i = 0; i < nt; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const AkLayout l = ak_layout();
    memset(packed, 0, l.total * sizeof(float));
    auto T = [&](const char* name) { return t[ak_tensors().find(name)]; };
    std::vector<float> sc, sh, tmp;
    // (the four tensors of a BatchNorm follow each other in the table)
    auto fold = [&](const std::string& bn, int cout) { bn_fold_f32(t + ak_tensors().find(bn + ".weight"), cout, sc, sh); };
    // OIHW 3x3 -> [tap][cin][cout] with a per-output scale
    auto pack_valu = [&](int v, const float* w, const float* scale, const float* bias) {
        const int cin = AK_VCIN[v], cout = AK_VCOUT[v];
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int k = 0; k < 9; ++k) packed[l.vw[v] + ((size_t)k * cin + ci) * cout + co] = w[((size_t)co * cin + ci) * 9 + k] * (scale ? scale[co] : 1.0f);
        if (bias) memcpy(packed + l.vb[v], bias, cout * sizeof(float));
    };
    auto pack_gemm = [&](int g, const float* w_nk, const float* bias) {  // w_nk already [N][K]
        memcpy(packed + l.g[g].w, w_nk, (size_t)AK_GN[g] * AK_GK[g] * sizeof(float));
        if (bias) memcpy(packed + l.g[g].b, bias, AK_GN[g] * sizeof(float));
        l.g[g].split_planes(packed, AK_GN[g], AK_GK[g]);
    };
    // a 3x3 convolution followed by a folded BatchNorm as a GEMM layer (cin stored as cpad channels)
    auto pack_conv_bn = [&](int g, const float* w, int cout, int cin, int cpad, const char* bn) {
        fold(bn, cout);
        tmp.assign((size_t)cout * 9 * cpad, 0.0f);
        pack_conv_gemm(w, cout, cin, 3, cpad, tmp.data());
        for (int co = 0; co < cout; ++co)
            for (int k = 0; k < 9 * cpad; ++k) tmp[(size_t)co * 9 * cpad + k] *= sc[co];
        pack_gemm(g, tmp.data(), sh.data());
    };
    auto pack_pw = [&](int p, const float* w, int ldw, int col0) {  // w [cout][ldw], columns [col0, col0 + cin) -> [cin][cout]
        for (int co = 0; co < AK_PCOUT[p]; ++co)
            for (int ci = 0; ci < AK_PCIN[p]; ++ci) packed[l.pw[p] + (size_t)ci * AK_PCOUT[p] + co] = w[(size_t)co * ldw + col0 + ci];
    };
    fold("block1.bn1", 16);
    pack_valu(0, T("block1.conv1.weight"), sc.data(), sh.data());
    fold("block1.bn2", 16);
    pack_valu(1, T("block1.conv2.weight"), sc.data(), sh.data());
    pack_conv_bn(0, T("block2.conv1.weight"), 32, 16, 32, "block2.bn1");
    pack_conv_bn(1, T("block2.conv2.weight"), 32, 32, 32, "block2.bn2");
    const int ch[5] = {3, 16, 32, 64, 128};
    for (int b = 3; b <= 4; ++b)
        for (int j = 1; j <= 2; ++j) {
            const int cin = j == 1 ? ch[b - 1] : ch[b], cout = ch[b], idx = (b - 3) * 2 + (j - 1);
            char n0[64], n1[64], n2[64], n3[64];
            snprintf(n0, sizeof n0, "block%d.conv%d.offset_conv.weight", b, j);
            snprintf(n1, sizeof n1, "block%d.conv%d.offset_conv.bias", b, j);
            snprintf(n2, sizeof n2, "block%d.conv%d.regular_conv.weight", b, j);
            snprintf(n3, sizeof n3, "block%d.bn%d", b, j);
            pack_valu(2 + idx, T(n0), nullptr, T(n1));
            pack_conv_bn(2 + idx, T(n2), cout, cin, cin, n3);
        }
    pack_valu(6, T("score_head.2.weight"), nullptr, nullptr);
    pack_valu(7, T("score_head.4.weight"), nullptr, nullptr);
    pack_valu(8, T("score_head.6.weight"), nullptr, nullptr);
    {
        const float* w0 = T("desc_head.offset_conv.0.weight");  // [32][128][3][3] -> [tap][c][32]
        for (int o = 0; o < 32; ++o)
            for (int c = 0; c < 128; ++c)
                for (int k = 0; k < 9; ++k) packed[l.dh0t + ((size_t)k * 128 + c) * 32 + o] = w0[((size_t)o * 128 + c) * 9 + k];
        memcpy(packed + l.dh0b, T("desc_head.offset_conv.0.bias"), 32 * sizeof(float));
        const float* sf = T("desc_head.sf_conv.weight");  // [n][k] -> [k][n]
        for (int n = 0; n < 128; ++n)
            for (int k = 0; k < 128; ++k) packed[l.sft + (size_t)k * 128 + n] = sf[(size_t)n * 128 + k];
        memcpy(packed + l.agg, T("desc_head.agg_weights"), (size_t)AK_M * 128 * 128 * sizeof(float));  // [m][c][d]: already K-major
    }
    pack_pw(0, T("block2.downsample.weight"), 16, 0);
    pack_pw(1, T("block3.downsample.weight"), 32, 0);
    pack_pw(2, T("block4.downsample.weight"), 64, 0);
    pack_pw(3, T("conv1.weight"), 16, 0);
    pack_pw(4, T("conv2.weight"), 32, 0);
    pack_pw(5, T("conv3.weight"), 64, 0);
    pack_pw(6, T("conv4.weight"), 128, 0);
    for (int i = 0; i < 4; ++i) pack_pw(7 + i, T("score_head.0.weight"), 128, 32 * i);
    pack_pw(11, T("desc_head.offset_conv.2.weight"), 32, 0);
    memcpy(packed + l.pb, T("desc_head.offset_conv.2.bias"), 32 * sizeof(float));
    return IMCUI_OK;
}

// in-place SELU of a contiguous buffer
__global__ __launch_bounds__(256) void ak_selu_kernel(float* __restrict__ x, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 v = reinterpret_cast<float4*>(x)[i];
        reinterpret_cast<float4*>(x)[i] = make_float4(ak_selu(v.x), ak_selu(v.y), ak_selu(v.z), ak_selu(v.w));
    }
}

// 1x1 convolution on the VALU: out[p][co] = act(add[p][co] + sum_ci in[p][ci] wt[ci][co]); one thread per (pixel, output channel),
// channels summed in ascending order.  `add` may alias `out`.  act: 0 none, 1 SELU.
__global__ __launch_bounds__(256) void ak_pw_kernel(const float* __restrict__ in, int ldi, int cin, const float* __restrict__ wt, const float* add,
                                                    int lda, float* out, int ldo, int cout, int act, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int co = (int)(i % cout);
        const long p = i / cout;
        const float* x = in + p * ldi;
        float acc = 0.0f;
        for (int ci = 0; ci < cin; ++ci) acc = fmaf(x[ci], wt[ci * cout + co], acc);
        if (add) acc += add[p * lda + co];
        out[p * ldo + co] = act ? ak_selu(acc) : acc;
    }
}

// ------------------------------------------------------------------ deformable 3x3 convolution, gather stage
// x [B,h,w,C] NHWC, off [B,h,w,18] (offset_conv's output; channel 2k = dy, 2k + 1 = dx of tap k, torchvision's order), clamped to
// +-clampv.  A[pixel][tap][C] = bilinear sample of x at (y - 1 + ky + dy, x - 1 + kx + dx), zero outside (torchvision's
// bilinear_interpolate: 0 beyond one pixel outside, missing corners contribute 0).  One thread per (pixel, tap, 4 channels).
__global__ __launch_bounds__(256) void ak_deform_kernel(const float* __restrict__ x, const float* __restrict__ off, float* __restrict__ A, int h, int w,
                                                        int C, float clampv, long n4) {
    const int C4 = C >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        long t = i / C4;
        const int k = (int)(t % 9);
        const long m = t / 9;
        const int px = (int)(m % w);
        const long q = m / w;
        const int py = (int)(q % h);
        const long b = q / h;
        const float dy = fminf(fmaxf(off[m * 18 + 2 * k], -clampv), clampv), dx = fminf(fmaxf(off[m * 18 + 2 * k + 1], -clampv), clampv);
        const float fy = (float)(py - 1 + k / 3) + dy, fx = (float)(px - 1 + k % 3) + dx;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (fy > -1.0f && fy < (float)h && fx > -1.0f && fx < (float)w) {
            const int yl = (int)floorf(fy), xl = (int)floorf(fx);
            const float ly = fy - (float)yl, lx = fx - (float)xl, hy = 1.0f - ly, hx = 1.0f - lx;
            const float* base = x + b * (long)h * w * C + c;
            const float wgt[4] = {hy * hx, hy * lx, ly * hx, ly * lx};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = yl + (j >> 1), xx = xl + (j & 1);
                if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
                    const float4 v = *reinterpret_cast<const float4*>(base + ((long)yy * w + xx) * C);
                    o.x = fmaf(wgt[j], v.x, o.x);
                    o.y = fmaf(wgt[j], v.y, o.y);
                    o.z = fmaf(wgt[j], v.z, o.z);
                    o.w = fmaf(wgt[j], v.w, o.w);
                }
            }
        }
        *reinterpret_cast<float4*>(A + i * 4) = o;
    }
}

// ------------------------------------------------------------------ score head, layer 0 (1x1 over x1234) evaluated branch-wise
// s8[p] = SELU(W_a SELU(W_1 x1[p]) + up2(g2)[p] + up8(g3)[p] + up32(g4)[p]), g_i = W_i-slice f_i at the branch's own resolution.
// One thread per pixel of the padded map; c1t [16][32] and sat [32][8] in LDS.
__global__ __launch_bounds__(256) void ak_score8_kernel(const float* __restrict__ x1, const float* __restrict__ c1t, const float* __restrict__ sat,
                                                        const float* __restrict__ g2, const float* __restrict__ g3, const float* __restrict__ g4,
                                                        float* __restrict__ s8, int Hp, int Wp, long npix) {
    __shared__ float w1[16 * 32], wa[32 * 8];
    for (int i = threadIdx.x; i < 512; i += 256) w1[i] = c1t[i];
    wa[threadIdx.x] = sat[threadIdx.x];
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % Wp);
    const long q = p / Wp;
    const int y = (int)(q % Hp);
    const long b = q / Hp;
    float xi[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(x1 + p * 16 + c * 4);
        xi[4 * c] = v.x, xi[4 * c + 1] = v.y, xi[4 * c + 2] = v.z, xi[4 * c + 3] = v.w;
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < 32; ++c) {
        float f = 0.0f;
#pragma unroll
        for (int ci = 0; ci < 16; ++ci) f = fmaf(xi[ci], w1[ci * 32 + c], f);
        f = ak_selu(f);
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[o] = fmaf(f, wa[c * 8 + o], acc[o]);
    }
    const float* gs[3] = {g2, g3, g4};
    const int sh[3] = {1, 3, 5};
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const int hl = Hp >> sh[l], wl = Wp >> sh[l];
        const AkTap ty = ak_tap(y, hl, Hp), tx = ak_tap(x, wl, Wp);
        const float* g = gs[l] + b * (long)hl * wl * 8;
#pragma unroll
        for (int o4 = 0; o4 < 2; ++o4) {
            const float4 v00 = *reinterpret_cast<const float4*>(g + ((long)ty.i0 * wl + tx.i0) * 8 + o4 * 4);
            const float4 v01 = *reinterpret_cast<const float4*>(g + ((long)ty.i0 * wl + tx.i1) * 8 + o4 * 4);
            const float4 v10 = *reinterpret_cast<const float4*>(g + ((long)ty.i1 * wl + tx.i0) * 8 + o4 * 4);
            const float4 v11 = *reinterpret_cast<const float4*>(g + ((long)ty.i1 * wl + tx.i1) * 8 + o4 * 4);
            acc[o4 * 4 + 0] += ty.l0 * (tx.l0 * v00.x + tx.l1 * v01.x) + ty.l1 * (tx.l0 * v10.x + tx.l1 * v11.x);
            acc[o4 * 4 + 1] += ty.l0 * (tx.l0 * v00.y + tx.l1 * v01.y) + ty.l1 * (tx.l0 * v10.y + tx.l1 * v11.y);
            acc[o4 * 4 + 2] += ty.l0 * (tx.l0 * v00.z + tx.l1 * v01.z) + ty.l1 * (tx.l0 * v10.z + tx.l1 * v11.z);
            acc[o4 * 4 + 3] += ty.l0 * (tx.l0 * v00.w + tx.l1 * v01.w) + ty.l1 * (tx.l0 * v10.w + tx.l1 * v11.w);
        }
    }
    float4* o = reinterpret_cast<float4*>(s8 + p * 8);
    o[0] = make_float4(ak_selu(acc[0]), ak_selu(acc[1]), ak_selu(acc[2]), ak_selu(acc[3]));
    o[1] = make_float4(ak_selu(acc[4]), ak_selu(acc[5]), ak_selu(acc[6]), ak_selu(acc[7]));
}

// ------------------------------------------------------------------ the feature map, evaluated where it is read
// feature_map[y][x] = F.normalize(x1234)[y + pt][x + pl] on the cropped h x w grid.  One wave per position; lane l holds channels
// 2l, 2l + 1 of the 128: lanes 0..15 branch 1 (f1 = SELU(W_1 x1), formed here), 16..31 / 32..47 / 48..63 the up-sampled f2 / f3 / f4.
struct AkMaps {
    const float *x1, *f2, *f3, *f4, *c1t;
    int Hp, Wp, h, w, pt, pl;
};
// un-normalised channels (2 lane .. 2 lane + 1) of x1234 at a pixel of the cropped map; the coordinates have to be inside it
__device__ __forceinline__ float2 ak_feat_raw(const AkMaps& m, long b, int y, int x, int lane) {
    const int py = y + m.pt, px = x + m.pl;
    const int br = lane >> 4, c = (lane & 15) * 2;
    float2 v;
    if (br == 0) {
        const float* xi = m.x1 + ((b * m.Hp + py) * (long)m.Wp + px) * 16;
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int ci = 0; ci < 16; ++ci) {
            const float u = xi[ci];
            a0 = fmaf(u, m.c1t[ci * 32 + c], a0);
            a1 = fmaf(u, m.c1t[ci * 32 + c + 1], a1);
        }
        v = make_float2(ak_selu(a0), ak_selu(a1));
    } else {
        const int sh = br == 1 ? 1 : (br == 2 ? 3 : 5);
        const float* f = br == 1 ? m.f2 : (br == 2 ? m.f3 : m.f4);
        const int hl = m.Hp >> sh, wl = m.Wp >> sh;
        const AkTap ty = ak_tap(py, hl, m.Hp), tx = ak_tap(px, wl, m.Wp);
        f += b * (long)hl * wl * 32 + c;
        const float2 v00 = *reinterpret_cast<const float2*>(f + ((long)ty.i0 * wl + tx.i0) * 32);
        const float2 v01 = *reinterpret_cast<const float2*>(f + ((long)ty.i0 * wl + tx.i1) * 32);
        const float2 v10 = *reinterpret_cast<const float2*>(f + ((long)ty.i1 * wl + tx.i0) * 32);
        const float2 v11 = *reinterpret_cast<const float2*>(f + ((long)ty.i1 * wl + tx.i1) * 32);
        v.x = ty.l0 * (tx.l0 * v00.x + tx.l1 * v01.x) + ty.l1 * (tx.l0 * v10.x + tx.l1 * v11.x);
        v.y = ty.l0 * (tx.l0 * v00.y + tx.l1 * v01.y) + ty.l1 * (tx.l0 * v10.y + tx.l1 * v11.y);
    }
    return v;
}
__device__ __forceinline__ float2 ak_feat_norm(float2 v) {
    const float d = fmaxf(sqrtf(wave_sum(v.x * v.x + v.y * v.y)), 1e-12f);
    return make_float2(v.x / d, v.y / d);
}
__device__ __forceinline__ float2 ak_feat_pixel(const AkMaps& m, long b, int y, int x, int lane) {
    if (y < 0 || y >= m.h || x < 0 || x >= m.w) return make_float2(0.f, 0.f);  // (wave-uniform)
    return ak_feat_norm(ak_feat_raw(m, b, y, x, lane));
}

// key-point position in pixels of the cropped map as SDDH forms it from the normalised key-point: (kn / 2 + 0.5) * (w - 1, h - 1)
__device__ __forceinline__ float2 ak_kpt_wh(const float* kn, const AkMaps& m) {
    return make_float2((kn[0] / 2.0f + 0.5f) * (float)(m.w - 1), (kn[1] / 2.0f + 0.5f) * (float)(m.h - 1));
}

// bilinear sample of feature_map at key-point p (pixels of the cropped map) + offset, through SDDH's normalise / grid_sample round
// trip (align_corners=True, zero outside); lane's two channels.  Wave-uniform arguments.
__device__ __forceinline__ float2 ak_sample_at(const AkMaps& m, long b, float2 p, float ox, float oy, int lane) {
    const float wm = (float)(m.w - 1), hm = (float)(m.h - 1);
    const float gx = 2.0f * (p.x + ox) / wm - 1.0f, gy = 2.0f * (p.y + oy) / hm - 1.0f;
    const float fx = (gx + 1.0f) / 2.0f * wm, fy = (gy + 1.0f) / 2.0f * hm;
    const float x0f = floorf(fx), y0f = floorf(fy);
    float2 o = make_float2(0.f, 0.f);
    if (x0f >= -1.0f && x0f < (float)m.w && y0f >= -1.0f && y0f < (float)m.h) {  // otherwise all four corners are outside
        const int x0 = (int)x0f, y0 = (int)y0f;
        const float lx = fx - x0f, ly = fy - y0f;
        const float wgt[4] = {(1.0f - lx) * (1.0f - ly), lx * (1.0f - ly), (1.0f - lx) * ly, lx * ly};  // nw, ne, sw, se
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 v = ak_feat_pixel(m, b, y0 + (j >> 1), x0 + (j & 1), lane);
            o.x = fmaf(v.x, wgt[j], o.x);
            o.y = fmaf(v.y, wgt[j], o.y);
        }
    }
    return o;
}

// SDDH, launch 1 of 2: the offsets of every key-point.  A workgroup takes AK_KB0 key-points per step (grid-stride over the image's
// key-point COUNT, read on the device): the nine 128-channel patch vectors around trunc(p) are evaluated into LDS (one wave per
// position), thread (key-point, j) sums offset_conv.0's row j over the 1152 patch values in ascending order (fp32 FMA; weights
// K-major, so a wave reads 128 contiguous bytes per k), SELU, offset_conv.2, clamp.  The 32 offsets (x, y of the 16 samples) of
// key-point i are parked in floats 0..31 of its own descriptor row, which launch 2 reads before it writes the descriptor.
__global__ __launch_bounds__(256) void ak_sddh_offsets_kernel(AkMaps m, const float* __restrict__ knorm, const int* __restrict__ nkpts, int kcap,
                                                              const float* __restrict__ w0t, const float* __restrict__ b0,
                                                              const float* __restrict__ w2t, const float* __restrict__ b2, float clampv,
                                                              float* __restrict__ desc) {
    __shared__ float P[AK_KB0][1152];
    __shared__ float Hd[AK_KB0][32];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nk = min(nkpts[b], kcap);
    for (int k0 = blockIdx.x * AK_KB0; k0 < nk; k0 += gridDim.x * AK_KB0) {
        __syncthreads();
        for (int e = wv; e < AK_KB0 * 9; e += 4) {
            const int kp = e / 9, tap = e - kp * 9;
            const int i = k0 + kp;
            float2 v = make_float2(0.f, 0.f);
            if (i < nk) {
                const float2 p = ak_kpt_wh(knorm + ((long)b * kcap + i) * 2, m);
                v = ak_feat_pixel(m, b, (int)p.y - 1 + tap / 3, (int)p.x - 1 + tap % 3, lane);
            }
            P[kp][tap * 128 + 2 * lane] = v.x;
            P[kp][tap * 128 + 2 * lane + 1] = v.y;
        }
        __syncthreads();
        const int kp = tid >> 5, j = tid & 31;
        float acc = b0[j];
        for (int k = 0; k < 1152; ++k) acc = fmaf(P[kp][k], w0t[k * 32 + j], acc);
        Hd[kp][j] = ak_selu(acc);
        __syncthreads();
        float o = b2[j];
#pragma unroll
        for (int q = 0; q < 32; ++q) o = fmaf(Hd[kp][q], w2t[q * 32 + j], o);
        if (k0 + kp < nk) desc[((long)b * kcap + k0 + kp) * 128 + j] = fminf(fmaxf(o, -clampv), clampv);
    }
}

// SDDH, launch 2 of 2: samples, sf_conv, SELU, aggregation and the L2 norm for AK_KB1 = 32 key-points per workgroup step
// (grid-stride over the capacity: steps past the count only write the zero rows).  For sample m = 0..15: the 32 sampled vectors
// S [32][128] go to LDS (one wave per position); G = SELU(S sf^T) and D += G agg[m] run on v_mfma_f32_32x32x2_f32, wave w owning
// output columns 32 w .. 32 w + 31 (A fragments from LDS, B fragments K-major from global: 128 contiguous bytes per half wave).
// The f32 matrix pipe serves BOTH arithmetic modes here: 1.1 MFLOP per key-point is small against its 157 TFLOP/s, and the two
// modes then give the same descriptors.  Sums run over k ascending inside m ascending.
__global__ __launch_bounds__(256) void ak_sddh_desc_kernel(AkMaps m, const float* __restrict__ knorm, const int* __restrict__ nkpts, int kcap,
                                                           const float* __restrict__ sft, const float* __restrict__ agg, float* __restrict__ desc) {
    constexpr int LD = 129;  // odd row stride: the 32 rows of an A fragment hit distinct banks
    __shared__ float S[AK_KB1 * LD];
    __shared__ float G[AK_KB1 * LD];
    __shared__ float Off[AK_KB1][32];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int nk = min(nkpts[b], kcap);
    for (int k0 = blockIdx.x * AK_KB1; k0 < kcap; k0 += gridDim.x * AK_KB1) {
        float* out = desc + ((long)b * kcap + k0) * 128;
        if (k0 >= nk) {  // rows past the count are zero
            for (int e = tid; e < AK_KB1 * 128; e += 256)
                if (k0 + e / 128 < kcap) out[e] = 0.0f;
            continue;
        }
        __syncthreads();
        for (int e = tid; e < AK_KB1 * 32; e += 256) Off[e >> 5][e & 31] = (k0 + (e >> 5) < nk) ? out[(long)(e >> 5) * 128 + (e & 31)] : 0.0f;
        __syncthreads();
        f32x16 dacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[r] = 0.0f;
        for (int s = 0; s < AK_M; ++s) {
            for (int kp = wv; kp < AK_KB1; kp += 4) {
                float2 v = make_float2(0.f, 0.f);
                if (k0 + kp < nk) {
                    const float2 p = ak_kpt_wh(knorm + ((long)b * kcap + k0 + kp) * 2, m);
                    v = ak_sample_at(m, b, p, Off[kp][2 * s], Off[kp][2 * s + 1], lane);
                }
                S[kp * LD + 2 * lane] = v.x;
                S[kp * LD + 2 * lane + 1] = v.y;
            }
            __syncthreads();
            f32x16 g;
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = 0.0f;
            for (int k = 0; k < 128; k += 2) g = mfma32(S[lo * LD + k + hi], sft[(k + hi) * 128 + 32 * wv + lo], g);
#pragma unroll
            for (int r = 0; r < 16; ++r) G[frag_row(r, hi) * LD + 32 * wv + lo] = ak_selu(g[r]);
            __syncthreads();
            const float* am = agg + (size_t)s * 128 * 128;
            for (int k = 0; k < 128; k += 2) dacc = mfma32(G[lo * LD + k + hi], am[(k + hi) * 128 + 32 * wv + lo], dacc);
        }
        __syncthreads();  // (every wave is done reading G)
#pragma unroll
        for (int r = 0; r < 16; ++r) G[frag_row(r, hi) * LD + 32 * wv + lo] = dacc[r];
        __syncthreads();
        for (int kp = wv; kp < AK_KB1; kp += 4) {  // F.normalize(dim=1); one wave per row
            if (k0 + kp >= kcap) break;
            float2 v = make_float2(G[kp * LD + 2 * lane], G[kp * LD + 2 * lane + 1]);
            if (k0 + kp < nk) {
                const float d = fmaxf(sqrtf(wave_sum(v.x * v.x + v.y * v.y)), 1e-12f);
                v = make_float2(v.x / d, v.y / d);
            } else {
                v = make_float2(0.f, 0.f);
            }
            *reinterpret_cast<float2*>(out + (long)kp * 128 + 2 * lane) = v;
        }
    }
}

// ------------------------------------------------------------------ DKD: the cut and the refinement
// The cut and the refinement, one workgroup per image.  More than `limit` candidates: the `limit` highest scores stay (radix select of
// the limit-th largest key; among candidates equal to it the lowest flat indices).  The kept candidates leave in row-major order.
// Each is refined on the spot: soft-argmax over the (2r+1)^2 patch of the raw score map (temperature 0.1), normalised position,
// key-point score = bilinear sample of the score map there (align_corners=True), pixel position (w-1, h-1) (n + 1) / 2.
__global__ __launch_bounds__(1024) void ak_select_kernel(const float* __restrict__ cscore, const int* __restrict__ cidx, int ccap,
                                                         const int* __restrict__ ncand, int limit_, int kcap, const float* __restrict__ score, int h, int w,
                                                         int r, float* __restrict__ kpts, float* __restrict__ knorm, float* __restrict__ scores,
                                                         int* __restrict__ nkpts, int* __restrict__ status) {
    __shared__ int wcnt[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* cs = cscore + (long)b * ccap;
    const int* ci = cidx + (long)b * ccap;
    const float* sm = score + (long)b * h * w;
    const int n = min(ncand[b], ccap);
    bool filter = false;
    unsigned kth = 0;
    int need_eq = 0;
    int limit = n;
    if (n > limit_) {
        filter = true;
        limit = limit_;
        // the limit-th largest key (1 <= limit_ < n: the host passes max_keypoints > 0 or AK_NLIMIT); need_eq = how many candidates
        // equal to it are kept (the first ones in row-major order)
        kth = radix_select_kth<1024, unsigned>([&](int i) { return order_key(cs[i]); }, n, limit_, &need_eq);
    }
    if (limit > kcap) {
        if (tid == 0) atomicOr(status, 2);  // output capacity too small
        limit = kcap;
    }
    float* kp = kpts + (long)b * kcap * 2;
    float* kn = knorm + (long)b * kcap * 2;
    float* sc = scores + (long)b * kcap;
    int run = 0, eqrun = 0;
    for (int base = 0; base < n; base += 1024) {
        if (run >= limit) break;
        const int i = base + tid;
        bool gt = !filter && i < n, eq = false;
        int idx = 0;
        if (i < n) {
            idx = ci[i];
            if (filter) {
                const unsigned key = order_key(cs[i]);
                gt = key > kth;
                eq = key == kth;
            }
        }
        int etot = 0, tot, eqpos = 0;
        if (filter) eqpos = eqrun + block_ordered_rank<16>(eq, wcnt, &etot);  // (uniform: no key equals a cut that was not made)
        const bool keep = gt || (eq && eqpos < need_eq);
        const int pos = run + block_ordered_rank<16>(keep, wcnt, &tot);
        if (keep && pos < limit) {
            const int x = idx % w, y = idx / w;  // (inside the border band: the patch is inside the map)
            float mx = -INFINITY;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) mx = fmaxf(mx, sm[(long)(y + dy) * w + x + dx]);
            float se = 0.0f, sx = 0.0f, sy = 0.0f;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const float e = expf((sm[(long)(y + dy) * w + x + dx] - mx) / 0.1f);
                    se += e;
                    sx = fmaf(e, (float)dx, sx);
                    sy = fmaf(e, (float)dy, sy);
                }
            const float wm = (float)(w - 1), hm = (float)(h - 1);
            const float nx = ((float)x + sx / se) / wm * 2.0f - 1.0f, ny = ((float)y + sy / se) / hm * 2.0f - 1.0f;
            // grid_sample(score_map, align_corners=True, zeros padding)
            const float fx = (nx + 1.0f) / 2.0f * wm, fy = (ny + 1.0f) / 2.0f * hm;
            const float x0f = floorf(fx), y0f = floorf(fy);
            const int x0 = (int)x0f, y0 = (int)y0f;
            const float lx = fx - x0f, ly = fy - y0f;
            float v = 0.0f;
            const float wgt[4] = {(1.0f - lx) * (1.0f - ly), lx * (1.0f - ly), (1.0f - lx) * ly, lx * ly};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = y0 + (j >> 1), xx = x0 + (j & 1);
                if (yy >= 0 && yy < h && xx >= 0 && xx < w) v = fmaf(sm[(long)yy * w + xx], wgt[j], v);
            }
            kn[2 * pos + 0] = nx;
            kn[2 * pos + 1] = ny;
            kp[2 * pos + 0] = wm * (nx + 1.0f) / 2.0f;
            kp[2 * pos + 1] = hm * (ny + 1.0f) / 2.0f;
            sc[pos] = v;
        }
        run += tot;
        eqrun += etot;
        // Not needed for the counts (block_ordered_rank ends in a barrier): it keeps the waves of a batch together.  Without it a wave
        // that is done early enters the next batch while others still gather their patches, and the kernel measured 1.2 - 1.7 us
        // (2 - 3 %) slower at 3000 - 4000 key-points per image; with it 1 us faster than with the base kept in LDS behind two barriers.
        __syncthreads();
    }
    const int cnt = min(run, limit);
    for (int i = cnt + tid; i < kcap; i += 1024) {
        kp[2 * i + 0] = 0.0f;
        kp[2 * i + 1] = 0.0f;
        kn[2 * i + 0] = 0.0f;
        kn[2 * i + 1] = 0.0f;
        sc[i] = 0.0f;
    }
    if (tid == 0) nkpts[b] = cnt;
}

// ------------------------------------------------------------------ workspace
struct AkWs {
    float *a16, *x1, *p1, *t2, *x2, *f2, *g2, *p2, *off3, *A3, *t3, *x3, *f3, *g3, *p3, *off4, *A4, *t4, *x4, *f4, *g4;
    float *score, *nms, *knorm;
    AkDkdWs dkd;
    int* status;
    size_t total;
    bool ok;
};

static AkWs ak_carve(void* ws, size_t bytes, int B, int h, int w, int kcap) {
    WsAlloc a(ws, bytes);
    AkWs s;
    const size_t P0 = (size_t)ak_pad32(h) * ak_pad32(w), P1 = P0 / 4, P3 = P0 / 64, P5 = P0 / 1024;
    s.a16 = a.get<float>(B * P0 * 16);  // block 1's intermediate; afterwards the score head's 8 + 4 + 4 channel maps
    s.x1 = a.get<float>(B * P0 * 16);
    s.p1 = a.get<float>(B * P1 * 32);
    s.t2 = a.get<float>(B * P1 * 32);
    s.x2 = a.get<float>(B * P1 * 32);
    s.f2 = a.get<float>(B * P1 * 32);
    s.g2 = a.get<float>(B * P1 * 8);
    s.p2 = a.get<float>(B * P3 * 32);
    s.off3 = a.get<float>(B * P3 * 18);
    s.A3 = a.get<float>(B * P3 * 576);
    s.t3 = a.get<float>(B * P3 * 64);
    s.x3 = a.get<float>(B * P3 * 64);
    s.f3 = a.get<float>(B * P3 * 32);
    s.g3 = a.get<float>(B * P3 * 8);
    s.p3 = a.get<float>(B * P5 * 64);
    s.off4 = a.get<float>(B * P5 * 18);
    s.A4 = a.get<float>(B * P5 * 1152);
    s.t4 = a.get<float>(B * P5 * 128);
    s.x4 = a.get<float>(B * P5 * 128);
    s.f4 = a.get<float>(B * P5 * 32);
    s.g4 = a.get<float>(B * P5 * 8);
    s.score = a.get<float>((size_t)B * h * w);
    s.nms = a.get<float>((size_t)B * h * w);
    s.dkd.carve(a, B, h, w);
    s.knorm = a.get<float>((size_t)B * kcap * 2);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

// survivors of simple_nms are more than `radius` apart (Chebyshev) unless scores tie exactly
extern "C" int imcui_hip_aliked_max_keypoints_bound(int H, int W, int nms_radius) {
    const int r = nms_radius < 0 ? 0 : nms_radius;
    return cdiv(H, r + 1) * cdiv(W, r + 1);
}
// (sized for kcap up to every pixel: the key-point list in the workspace is 2 floats per entry)
extern "C" size_t imcui_hip_aliked_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ak_carve(nullptr, 0, B, H, W, imcui_hip_aliked_max_keypoints_bound(H, W, 0)).total;
}

extern "C" int imcui_hip_aliked_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, int nms_radius,
                                        float threshold, int max_keypoints, int kcap, float* keypoints, float* scores, float* descriptors,
                                        int* num_keypoints, int* status, float* score_map, float* keypoints_norm, float* dbg_x3, float* dbg_x4,
                                        void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "aliked: B=%d above 1024", B);
    if (nms_radius < 1 || nms_radius > 4) return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "aliked: nms_radius=%d not supported (1..4)", nms_radius);
    if (H < 32 || W < 32) return imcui_set_err(h, IMCUI_ERR_ARG, "aliked: H=%d W=%d must be at least 32", H, W);
    if ((long)B * ak_pad32(H) * ak_pad32(W) > 0x7fffffffL) return imcui_set_err(h, IMCUI_ERR_ARG, "aliked: B=%d images of %dx%d exceed 2^31 pixels per call", B, H, W);
    if (kcap <= 0 || !packed || !image || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "aliked: null argument or kcap<=0");
    if ((long)kcap > (long)H * W) return imcui_set_err(h, IMCUI_ERR_ARG, "aliked: kcap=%d above H*W", kcap);
    const int Hp = ak_pad32(H), Wp = ak_pad32(W);
    const int pt = (Hp - H) / 2, pl = (Wp - W) / 2;
    AkWs s = ak_carve(ws, ws_bytes, B, H, W, kcap);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "aliked: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const AkLayout l = ak_layout();
    const float* P = packed;
    const bool split = h->precision == 1;
    int rc;
    auto px = [&](int sh) { return (long)(Hp >> sh) * (Wp >> sh); };
    // GEMM layer L (+ folded-BatchNorm bias) on the rows of A -> out [M, N]; cin > 0: A is the NHWC map [B, Hp >> sh, Wp >> sh, cin] and
    // the layer its implicit 3x3 convolution (pad 1), else A holds the gathered rows [M, K]
    auto gemm = [&](int L, const float* A, int sh, int cin, float* out) -> int {
        GemmP g;
        g.epi = EPI_CONV;
        g.A = A;
        gemm_set_weights(g, P, l.g[L], AK_GN[L], AK_GK[L], split);
        if (cin > 0)
            gemm_set_conv(g, 3, 1, 1, Hp >> sh, Wp >> sh, Hp >> sh, Wp >> sh, cin);
        else
            g.lda = AK_GK[L];
        g.M = (int)(B * px(sh));
        g.C = out;
        g.ldc = AK_GN[L];
        return gemm_launch(h, g, stream);
    };
    auto selu = [&](float* x, long n) { hipLaunchKernelGGL(ak_selu_kernel, dim3(grid_stride_blocks(n / 4)), dim3(256), 0, stream, x, n / 4); };
    auto pw = [&](int L, const float* in, int ldi, const float* add, float* out, long npix, int act) {
        const long n = npix * AK_PCOUT[L];
        hipLaunchKernelGGL(ak_pw_kernel, dim3(grid_stride_blocks(n)), dim3(256), 0, stream, in, ldi, AK_PCIN[L], P + l.pw[L], add, AK_PCOUT[L], out, AK_PCOUT[L],
                           AK_PCOUT[L], act, n);
    };
    auto pool = [&](const float* src, int C, float* dst, int ldd, int k, int sh_out) {
        const long n4 = (long)B * px(sh_out) * ldd / 4;
        hipLaunchKernelGGL(ak_pool_kernel<false>, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, src, C, C, dst, ldd, k, Hp >> sh_out, Wp >> sh_out, n4);
    };
    // deformable 3x3 (+ folded BatchNorm bias) of x [B, hl, wl, cin]: offsets (VALU layer V), gather, GEMM layer L -> out [.., N]
    auto deform = [&](int V, int L, const float* x, int cin, int sh, float* offb, float* A, float* out) -> int {
        const int hl = Hp >> sh, wl = Wp >> sh;
        AkConvP c{x, 0, 0, 0, 0, 0, cin, cin, P + l.vw[V], P + l.vb[V], offb, 18, hl, wl, hl, wl, 0, 0};
        ak_conv3<18, 16, 0>(c, B, stream);
        const long n4 = (long)B * px(sh) * 9 * cin / 4;
        hipLaunchKernelGGL(ak_deform_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, x, offb, A, hl, wl, cin, (float)max(hl, wl) / 4.0f, n4);
        IMCUI_CHECK_LAUNCH(h);
        return gemm(L, A, sh, 0, out);
    };
    // ---- block 1 (full resolution, VALU)
    {
        AkConvP c{image, 1, H, W, pt, pl, 0, 3, P + l.vw[0], P + l.vb[0], s.a16, 16, Hp, Wp, Hp, Wp, 0, 0};
        ak_conv3<16, 3, 1>(c, B, stream);
        AkConvP d{s.a16, 0, 0, 0, 0, 0, 16, 16, P + l.vw[1], P + l.vb[1], s.x1, 16, Hp, Wp, Hp, Wp, 0, 0};
        ak_conv3<16, 16, 1>(d, B, stream);
        IMCUI_CHECK_LAUNCH(h);
    }
    // ---- block 2 (1/2): x2 = SELU(bn2(conv2(SELU(bn1(conv1(p1))))) + downsample(p1))
    pool(s.x1, 16, s.p1, 32, 2, 1);
    IMCUI_RUN(gemm(0, s.p1, 1, 32, s.t2));
    selu(s.t2, B * px(1) * 32);
    IMCUI_RUN(gemm(1, s.t2, 1, 32, s.x2));
    pw(0, s.p1, 32, s.x2, s.x2, B * px(1), 1);
    // ---- block 3 (1/8, deformable)
    pool(s.x2, 32, s.p2, 32, 4, 3);
    IMCUI_RUN(deform(2, 2, s.p2, 32, 3, s.off3, s.A3, s.t3));
    selu(s.t3, B * px(3) * 64);
    IMCUI_RUN(deform(3, 3, s.t3, 64, 3, s.off3, s.A3, s.x3));
    pw(1, s.p2, 32, s.x3, s.x3, B * px(3), 1);
    // ---- block 4 (1/32, deformable)
    pool(s.x3, 64, s.p3, 64, 4, 5);
    IMCUI_RUN(deform(4, 4, s.p3, 64, 5, s.off4, s.A4, s.t4));
    selu(s.t4, B * px(5) * 128);
    IMCUI_RUN(deform(5, 5, s.t4, 128, 5, s.off4, s.A4, s.x4));
    pw(2, s.p3, 64, s.x4, s.x4, B * px(5), 1);
    IMCUI_CHECK_LAUNCH(h);
    if (dbg_x3) hipMemcpyAsync(dbg_x3, s.x3, (size_t)B * px(3) * 64 * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (dbg_x4) hipMemcpyAsync(dbg_x4, s.x4, (size_t)B * px(5) * 128 * sizeof(float), hipMemcpyDeviceToDevice, stream);
    // ---- f_i = SELU(conv_i(x_i)) at the branch's resolution (f1 only ever in registers), g_i = the score head's slice of it
    pw(4, s.x2, 32, nullptr, s.f2, B * px(1), 1);
    pw(5, s.x3, 64, nullptr, s.f3, B * px(3), 1);
    pw(6, s.x4, 128, nullptr, s.f4, B * px(5), 1);
    pw(8, s.f2, 32, nullptr, s.g2, B * px(1), 0);
    pw(9, s.f3, 32, nullptr, s.g3, B * px(3), 0);
    pw(10, s.f4, 32, nullptr, s.g4, B * px(5), 0);
    // ---- score head: 8 channels at full resolution, then 3x3 8 -> 4 -> 4 -> 1, sigmoid, cropped to H x W
    float* s8 = s.a16;
    float* s4a = s.a16 + (size_t)B * px(0) * 8;
    float* s4b = s.a16 + (size_t)B * px(0) * 12;
    float* smap = score_map ? score_map : s.score;
    {
        const long np = B * px(0);
        hipLaunchKernelGGL(ak_score8_kernel, dim3(blocks_256(np)), dim3(256), 0, stream, s.x1, P + l.pw[3], P + l.pw[7], s.g2, s.g3, s.g4,
                           s8, Hp, Wp, np);
        AkConvP c{s8, 0, 0, 0, 0, 0, 8, 8, P + l.vw[6], P + l.vb[6], s4a, 4, Hp, Wp, Hp, Wp, 0, 0};
        ak_conv3<4, 8, 1>(c, B, stream);
        AkConvP d{s4a, 0, 0, 0, 0, 0, 4, 4, P + l.vw[7], P + l.vb[7], s4b, 4, Hp, Wp, Hp, Wp, 0, 0};
        ak_conv3<4, 4, 1>(d, B, stream);
        AkConvP e{s4b, 0, 0, 0, 0, 0, 4, 4, P + l.vw[8], P + l.vb[8], smap, 1, Hp, Wp, H, W, pt, pl};
        ak_conv3<1, 4, 2>(e, B, stream);
        IMCUI_CHECK_LAUNCH(h);
    }
    // ---- DKD
    const int r = nms_radius;
    IMCUI_RUN(imcui_hip_simple_nms(h, smap, s.nms, B, H, W, r, stream));
    int* st = status ? status : s.status;
    const bool topk = !(threshold > 0.0f) && max_keypoints > 0;
    const int limit = max_keypoints > 0 ? max_keypoints : AK_NLIMIT;
    const int ccap = H * W;
    IMCUI_RUN(ak_dkd_candidates(h, smap, s.nms, H, W, B, r, r, threshold, topk, s.dkd, st, stream));
    float* kn = keypoints_norm ? keypoints_norm : s.knorm;
    hipLaunchKernelGGL(ak_select_kernel, dim3(B), dim3(1024), 0, stream, s.dkd.cand.cscore, s.dkd.cand.cidx, ccap, s.dkd.scan.total, limit, kcap, smap, H, W, r, keypoints, kn, scores,
                       num_keypoints, st);
    IMCUI_CHECK_LAUNCH(h);
    // ---- SDDH: two launches per batch, whatever kcap is
    const AkMaps m{s.x1, s.f2, s.f3, s.f4, P + l.pw[3], Hp, Wp, H, W, pt, pl};
    const float clampv = (float)max(H, W) / 4.0f;
    hipLaunchKernelGGL(ak_sddh_offsets_kernel, dim3(min(cdiv(kcap, AK_KB0), 1024), B), dim3(256), 0, stream, m, kn, num_keypoints, kcap, P + l.dh0t,
                       P + l.dh0b, P + l.pw[11], P + l.pb, clampv, descriptors);
    hipLaunchKernelGGL(ak_sddh_desc_kernel, dim3(min(cdiv(kcap, AK_KB1), 1024), B), dim3(256), 0, stream, m, kn, num_keypoints, kcap, P + l.sft,
                       P + l.agg, descriptors);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
