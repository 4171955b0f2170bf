// ALIKE forward on MI355X (alike-t / alike-s / alike-n): the four-block encoder (3x3 convolutions with folded BatchNorm and ReLU,
// max-pooling), the linear head evaluated sparsely, DKD with ALIKE's selection rule and the descriptors at the key-points.  Replaces
// `self.net(image, sub_pixel)` of imcui/hloc/extractors/alike.py:47-61 (Shiaoming/ALIKE: alnet.py, soft_detect.py, alike.py).
//
// Data flow (NHWC maps; Hp x Wp = the image zero-padded at the bottom and right to multiples of 32; c2..c4 are STORED padded to
// multiples of 32 -- P2, P3, P4 -- with zero weights and biases in the padding, so padded channels are exactly 0 after every ReLU):
//   block1 3 -> c1 -> c1 at 1/1            fp32 FMA on the VALU, LDS tiles (ak_shared.h); the input is read as (x * 255) / 255
//   max-pool 2 / 4 / 4                      ak_pool_kernel<true> (ak_shared.h)
//   block2..4 at 1/2, 1/8, 1/32             implicit-GEMM 3x3 (gemm.hip, both arithmetic modes), ReLU in its epilogue; the 1x1 shortcut
//                                           (with bias) is written first and enters conv2's epilogue as the residual
//   f_i = ReLU(conv_i x_i), dim/4 channels, and g_i = w_score[slice i] . f_i, ONE float per branch pixel, at 1/2, 1/8, 1/32
//   score = sigmoid(w_score[slice 1] . ReLU(conv1 x1) + up2(g2) + up8(g3) + up32(g4)), cropped: one float per pixel.  convhead2 is
//           linear behind the branch activations, so its score row commutes with the bilinear up-sampling.
//   The (dim + 1)-channel full-resolution map is never written: the descriptor rows of convhead2 are applied to x1234 gathered at
//   the pixels the key-points read (one for the default, four for sub_pixel), 32 key-points per MFMA tile.
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

#define AL_R 2      // DKD radius of every variant
#define AL_KB 32    // key-points per workgroup step of al_desc_kernel (one 32-row MFMA tile)
#define AL_NVAR 3

// ------------------------------------------------------------------ variants and the tensor table
struct AlVar {
    const char* name;
    int c[5];  // 3, c1, c2, c3, c4
    int dim;
};
static const AlVar AL_VARS[AL_NVAR] = {{"alike-t", {3, 8, 16, 32, 64}, 64}, {"alike-s", {3, 8, 16, 48, 96}, 96}, {"alike-n", {3, 16, 32, 64, 128}, 128}};
static const AlVar* al_var(int v) { return (v < 0 || v >= AL_NVAR) ? nullptr : &AL_VARS[v]; }
static int al_pad(int c) { return (c + 31) / 32 * 32; }

static const TensorTable& al_tensors(int variant) {
    static TensorTable built[AL_NVAR];
    static bool done = [] {
        for (int v = 0; v < AL_NVAR; ++v) {
            const AlVar& a = AL_VARS[v];
            TensorTable& t = built[v];
            for (int b = 1; b <= 4; ++b) {
                const int cin = a.c[b - 1], cout = a.c[b];
                const std::string p = "block" + std::to_string(b);
                for (int j = 1; j <= 2; ++j) {
                    t.add(p + ".conv" + std::to_string(j) + ".weight", (size_t)cout * (j == 1 ? cin : cout) * 9);
                    for (const char* s : {"weight", "bias", "running_mean", "running_var"}) t.add(p + ".bn" + std::to_string(j) + "." + s, (size_t)cout);
                }
                if (b >= 2) {
                    t.add(p + ".downsample.weight", (size_t)cout * cin);
                    t.add(p + ".downsample.bias", (size_t)cout);
                }
            }
            for (int i = 1; i <= 4; ++i) t.add("conv" + std::to_string(i) + ".weight", (size_t)(a.dim / 4) * a.c[i]);
            t.add("convhead2.weight", (size_t)(a.dim + 1) * a.dim);
        }
        return true;
    }();
    (void)done;
    return built[variant];
}
extern "C" int imcui_hip_alike_num_tensors(int variant) { return al_var(variant) ? al_tensors(variant).size() : 0; }
extern "C" const char* imcui_hip_alike_tensor_name(int variant, int i) { return al_var(variant) ? al_tensors(variant).name(i) : nullptr; }

// ------------------------------------------------------------------ packed weight layout
// vw / vb: block 1's two layers, [tap][cin][c1] + [c1].  GEMM layers [N][9 cin_stored]: block2.conv1 / conv2, block3.conv1 / conv2,
// block4.conv1 / conv2 (f32, bias, the two f16 planes and their scale).  dw / db: the shortcuts of blocks 2..4, [cin_stored][cout_stored]
// + bias.  cw: conv1..4 transposed [cin_stored][dim / 4].  sw: the score row of convhead2 [dim].  wdt: its descriptor rows, K-major
// [dim k][dim n].
#define AL_NG 6
struct AlDims {
    int c1, P[5];  // P[1] = 32 (block 1's pooled output is stored as 32 channels), P[2..4] = c2..c4 padded
    int dq, dim;
    int gcin[AL_NG], gn[AL_NG], acin[AL_NG], acout[AL_NG];
};
static AlDims al_dims(const AlVar& a) {
    AlDims d;
    d.c1 = a.c[1];
    d.P[0] = 0;
    d.P[1] = 32;
    for (int i = 2; i <= 4; ++i) d.P[i] = al_pad(a.c[i]);
    d.dim = a.dim;
    d.dq = a.dim / 4;
    for (int g = 0; g < AL_NG; ++g) {
        const int b = 2 + g / 2, j = g & 1;
        d.gcin[g] = j == 0 ? d.P[b - 1] : d.P[b];
        d.gn[g] = d.P[b];
        d.acin[g] = j == 0 ? a.c[b - 1] : a.c[b];
        d.acout[g] = a.c[b];
    }
    return d;
}
struct AlLayout {
    size_t vw[2], vb[2];
    GemmLayerOff g[AL_NG];
    size_t dw[3], db[3];
    size_t cw[4], sw, wdt;
    size_t total;
};
static AlLayout al_layout(const AlDims& d) {
    AlLayout l;
    PackCursor c;
    l.vw[0] = c.get((size_t)9 * 3 * d.c1);  // (block1.conv1 first: offset 0 of the packed buffer, see imcui_hip.h)
    l.vb[0] = c.get(d.c1);
    l.vw[1] = c.get((size_t)9 * d.c1 * d.c1);
    l.vb[1] = c.get(d.c1);
    for (int g = 0; g < AL_NG; ++g) l.g[g].place(c, d.gn[g], 9 * d.gcin[g]);
    for (int i = 0; i < 3; ++i) {
        l.dw[i] = c.get((size_t)d.P[i + 1] * d.P[i + 2]);
        l.db[i] = c.get(d.P[i + 2]);
    }
    l.cw[0] = c.get((size_t)d.c1 * d.dq);
    for (int i = 1; i < 4; ++i) l.cw[i] = c.get((size_t)d.P[i + 1] * d.dq);
    l.sw = c.get(d.dim);
    l.wdt = c.get((size_t)d.dim * d.dim);
    l.total = c.off;
    return l;
}
extern "C" size_t imcui_hip_alike_packed_floats(int variant) {
    const AlVar* a = al_var(variant);
    return a ? al_layout(al_dims(*a)).total : 0;
}

// t: host pointers of the tensors in imcui_hip_alike_tensor_name order (shapes checked by the caller).  BatchNorm2d (eval, eps 1e-5)
// is folded into the convolution before it: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)
extern "C" int imcui_hip_alike_pack_weights(int variant, const float* const* t, float* packed) {
    const AlVar* a = al_var(variant);
    if (!a || !t || !packed) return IMCUI_ERR_ARG;
    const int nt = imcui_hip_alike_num_tensors(variant);
    for (int i = 0; i < nt; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const AlDims d = al_dims(*a);
    const AlLayout l = al_layout(d);
    memset(packed, 0, l.total * sizeof(float));
    const TensorTable& names = al_tensors(variant);
    auto T = [&](const std::string& name) { return t[names.find(name)]; };
    std::vector<float> sc, sh, tmp;
    // (the four tensors of a BatchNorm follow each other in the table)
    auto fold = [&](const std::string& bn, int cout) { bn_fold_f32(t + names.find(bn + ".weight"), cout, sc, sh); };
    for (int v = 0; v < 2; ++v) {  // block 1: OIHW -> [tap][cin][cout]
        const int cin = v == 0 ? 3 : d.c1, cout = d.c1;
        const float* w = T("block1.conv" + std::to_string(v + 1) + ".weight");
        fold("block1.bn" + std::to_string(v + 1), cout);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int k = 0; k < 9; ++k) packed[l.vw[v] + ((size_t)k * cin + ci) * cout + co] = w[((size_t)co * cin + ci) * 9 + k] * sc[co];
        memcpy(packed + l.vb[v], sh.data(), cout * sizeof(float));
    }
    for (int g = 0; g < AL_NG; ++g) {  // blocks 2..4: a GEMM layer [N stored][tap][cin stored], rows and columns of the padding zero
        const int b = 2 + g / 2, j = 1 + (g & 1);
        const int K = 9 * d.gcin[g], N = d.gn[g], cout = d.acout[g];
        const std::string p = "block" + std::to_string(b);
        fold(p + ".bn" + std::to_string(j), cout);
        tmp.assign((size_t)N * K, 0.0f);
        pack_conv_gemm(T(p + ".conv" + std::to_string(j) + ".weight"), cout, d.acin[g], 3, d.gcin[g], tmp.data());
        for (int co = 0; co < cout; ++co)
            for (int k = 0; k < K; ++k) tmp[(size_t)co * K + k] *= sc[co];
        memcpy(packed + l.g[g].w, tmp.data(), (size_t)N * K * sizeof(float));
        memcpy(packed + l.g[g].b, sh.data(), cout * sizeof(float));
        l.g[g].split_planes(packed, N, K);
    }
    for (int i = 0; i < 3; ++i) {  // shortcuts [cout][cin] -> [cin stored][cout stored]
        const int cin = a->c[i + 1], cout = a->c[i + 2], ldo = d.P[i + 2];
        const std::string p = "block" + std::to_string(i + 2) + ".downsample";
        const float* w = T(p + ".weight");
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) packed[l.dw[i] + (size_t)ci * ldo + co] = w[(size_t)co * cin + ci];
        memcpy(packed + l.db[i], T(p + ".bias"), cout * sizeof(float));
    }
    for (int i = 0; i < 4; ++i) {  // conv1..4 [dq][c_i] -> [c_i stored][dq]
        const int cin = a->c[i + 1];
        const float* w = T("conv" + std::to_string(i + 1) + ".weight");
        for (int co = 0; co < d.dq; ++co)
            for (int ci = 0; ci < cin; ++ci) packed[l.cw[i] + (size_t)ci * d.dq + co] = w[(size_t)co * cin + ci];
    }
    const float* hw = T("convhead2.weight");  // [dim + 1][dim]: rows 0..dim-1 the descriptor, row dim the score
    memcpy(packed + l.sw, hw + (size_t)d.dim * d.dim, d.dim * sizeof(float));
    for (int n = 0; n < d.dim; ++n)
        for (int k = 0; k < d.dim; ++k) packed[l.wdt + (size_t)k * d.dim + n] = hw[(size_t)n * d.dim + k];
    return IMCUI_OK;
}

namespace {

// 1x1 convolution with bias on the VALU (the shortcut of a ResBlock): out[p][co] = bias[co] + sum_ci in[p][ci] wt[ci][co], one thread
// per (pixel, stored output channel), channels summed in ascending order
__global__ __launch_bounds__(256) void al_pw_kernel(const float* __restrict__ in, int ldi, int cin, const float* __restrict__ wt,
                                                    const float* __restrict__ bias, float* __restrict__ out, int cout, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int co = (int)(i % cout);
        const long p = i / cout;
        const float* x = in + p * ldi;
        float acc = bias[co];
        for (int ci = 0; ci < cin; ++ci) acc = fmaf(x[ci], wt[ci * cout + co], acc);
        out[i] = acc;
    }
}

// f = ReLU(conv_i x) (DQ channels) and g = w_score-slice . f at the branch's own resolution; one thread per pixel, the weights are
// wave-uniform reads.  Channels ascending in both sums.
template <int DQ>
__global__ __launch_bounds__(256) void al_head_kernel(const float* __restrict__ x, int ldi, int cin, const float* __restrict__ wt,
                                                      const float* __restrict__ ws, float* __restrict__ f, float* __restrict__ g, long npix) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    float acc[DQ];
#pragma unroll
    for (int c = 0; c < DQ; ++c) acc[c] = 0.0f;
    const float* xi = x + p * ldi;
    for (int ci = 0; ci < cin; ci += 4) {
        const float4 v = *reinterpret_cast<const float4*>(xi + ci);
        const float u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < DQ; ++c) acc[c] = fmaf(u[q], wt[(ci + q) * DQ + c], acc[c]);
    }
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < DQ; ++c) {
        acc[c] = fmaxf(acc[c], 0.0f);
        s = fmaf(acc[c], ws[c], s);
    }
#pragma unroll
    for (int c = 0; c < DQ; c += 4) *reinterpret_cast<float4*>(f + p * DQ + c) = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
    g[p] = s;
}

// bilinear up-sampling (align_corners=True) of a one-channel map g [hl, wl] at pixel (y, x) of the Hp x Wp map
__device__ __forceinline__ float al_up1(const float* __restrict__ g, int hl, int wl, int y, int x, int Hp, int Wp) {
    const AkTap ty = ak_tap(y, hl, Hp), tx = ak_tap(x, wl, Wp);
    const float v00 = g[(long)ty.i0 * wl + tx.i0], v01 = g[(long)ty.i0 * wl + tx.i1];
    const float v10 = g[(long)ty.i1 * wl + tx.i0], v11 = g[(long)ty.i1 * wl + tx.i1];
    return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

// score[b][y][x] = sigmoid(ws1 . ReLU(W_1 x1) + up2(g2) + up8(g3) + up32(g4)) on the cropped H x W grid: one thread per pixel
template <int C1, int DQ>
__global__ __launch_bounds__(256) void al_score_kernel(const float* __restrict__ x1, const float* __restrict__ c1t, const float* __restrict__ ws1,
                                                       const float* __restrict__ g2, const float* __restrict__ g3, const float* __restrict__ g4,
                                                       float* __restrict__ score, int H, int W, int Hp, int Wp, long npix) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % W);
    const long q = p / W;
    const int y = (int)(q % H);
    const long b = q / H;
    float xi[C1];
    const float* src = x1 + ((b * Hp + y) * (long)Wp + x) * C1;
#pragma unroll
    for (int c = 0; c < C1; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(src + c);
        xi[c] = v.x, xi[c + 1] = v.y, xi[c + 2] = v.z, xi[c + 3] = v.w;
    }
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < DQ; ++c) {
        float f = 0.0f;
#pragma unroll
        for (int ci = 0; ci < C1; ++ci) f = fmaf(xi[ci], c1t[ci * DQ + c], f);
        s = fmaf(fmaxf(f, 0.0f), ws1[c], s);
    }
    s += al_up1(g2 + b * (long)(Hp >> 1) * (Wp >> 1), Hp >> 1, Wp >> 1, y, x, Hp, Wp);
    s += al_up1(g3 + b * (long)(Hp >> 3) * (Wp >> 3), Hp >> 3, Wp >> 3, y, x, Hp, Wp);
    s += al_up1(g4 + b * (long)(Hp >> 5) * (Wp >> 5), Hp >> 5, Wp >> 5, y, x, Hp, Wp);
    score[p] = sigmoidf_(s);
}

// ------------------------------------------------------------------ x1234 where it is read
struct AlMaps {
    const float *x1, *f2, *f3, *f4, *c1t;
    int Hp, Wp, h, w, c1, dq, dim;
};
// channel c of x1234 = cat(f1, up2(f2), up8(f3), up32(f4)) at pixel (y, x) of the (cropped = top-left of the padded) map
__device__ __forceinline__ float al_feat(const AlMaps& m, long b, int y, int x, int c) {
    const int br = c / m.dq, cc = c - br * m.dq;
    if (br == 0) {
        const float* xi = m.x1 + ((b * m.Hp + y) * (long)m.Wp + x) * m.c1;
        float a = 0.0f;
        for (int ci = 0; ci < m.c1; ++ci) a = fmaf(xi[ci], m.c1t[ci * m.dq + cc], a);
        return fmaxf(a, 0.0f);
    }
    const int sh = br == 1 ? 1 : (br == 2 ? 3 : 5);
    const float* f = br == 1 ? m.f2 : (br == 2 ? m.f3 : m.f4);
    const int hl = m.Hp >> sh, wl = m.Wp >> sh;
    const AkTap ty = ak_tap(y, hl, m.Hp), tx = ak_tap(x, wl, m.Wp);
    f += b * (long)hl * wl * m.dq + cc;
    const float v00 = f[((long)ty.i0 * wl + tx.i0) * m.dq], v01 = f[((long)ty.i0 * wl + tx.i1) * m.dq];
    const float v10 = f[((long)ty.i1 * wl + tx.i0) * m.dq], v11 = f[((long)ty.i1 * wl + tx.i1) * m.dq];
    return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

// ------------------------------------------------------------------ float32 position arithmetic of upstream, one rounding per operation
// The restatement rounds after every operation, and so does upstream's torch code.  hipcc contracts a * b + c into a fused multiply-add
// by default and its __fmul_rn / __fadd_rn are plain operators, so every helper below switches contraction off for its own body.
__device__ __forceinline__ float al_norm_pos(float v, float m1) {  // v / (size - 1) * 2 - 1
#pragma clang fp contract(off)
    return __fsub_rn(__fmul_rn(__fdiv_rn(v, m1), 2.0f), 1.0f);
}
__device__ __forceinline__ float al_pix_pos(float n, float m1) {  // (n + 1) / 2 * (size - 1)
#pragma clang fp contract(off)
    return __fmul_rn(__fdiv_rn(__fadd_rn(n, 1.0f), 2.0f), m1);
}

// the four corners (nw, ne, sw, se) and weights of grid_sample(bilinear, align_corners=True, zeros) at pixel position (fx, fy)
struct AlBil {
    int x0, y0;
    float w[4];
};
__device__ __forceinline__ AlBil al_bil(float fx, float fy) {
#pragma clang fp contract(off)
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float x1f = __fadd_rn(x0f, 1.0f), y1f = __fadd_rn(y0f, 1.0f);
    const float wx0 = __fsub_rn(x1f, fx), wx1 = __fsub_rn(fx, x0f), wy0 = __fsub_rn(y1f, fy), wy1 = __fsub_rn(fy, y0f);
    AlBil r;
    r.x0 = (int)x0f;
    r.y0 = (int)y0f;
    r.w[0] = __fmul_rn(wx0, wy0);
    r.w[1] = __fmul_rn(wx1, wy0);
    r.w[2] = __fmul_rn(wx0, wy1);
    r.w[3] = __fmul_rn(wx1, wy1);
    return r;
}
__device__ __forceinline__ float al_sample_score(const float* __restrict__ sm, int h, int w, float fx, float fy) {
#pragma clang fp contract(off)
    const AlBil t = al_bil(fx, fy);
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = t.y0 + (j >> 1), xx = t.x0 + (j & 1);
        const float s = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? sm[(long)yy * w + xx] : 0.0f;
        const float pr = __fmul_rn(s, t.w[j]);
        v = j == 0 ? pr : __fadd_rn(v, pr);
    }
    return v;
}

// ------------------------------------------------------------------ DKD: the cut
// One workgroup per image.  More than `limit` candidates: the `limit` highest scores stay (radix select of the limit-th largest key;
// among candidates equal to it the lowest flat indices).  The kept candidates leave in row-major order into kscore / kidx; sorted[b]
// says whether al_emit_kernel has to order them by descending score (a cut was taken, or the top_k route).
__global__ __launch_bounds__(1024) void al_cut_kernel(const float* __restrict__ cscore, const int* __restrict__ cidx, int ccap,
                                                      const int* __restrict__ ncand, int limit_, int always_sorted, float* __restrict__ kscore,
                                                      int* __restrict__ kidx, int* __restrict__ nkept, int* __restrict__ sorted) {
    __shared__ int wcnt[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* cs = cscore + (long)b * ccap;
    const int* ci = cidx + (long)b * ccap;
    float* ks = kscore + (long)b * ccap;
    int* ki = kidx + (long)b * ccap;
    const int n = min(ncand[b], ccap);
    bool filter = false;
    unsigned kth = 0;
    int need_eq = 0;
    int limit = n;
    if (n > limit_) {  // (1 <= limit_ < n)
        filter = true;
        limit = limit_;
        kth = radix_select_kth<1024, unsigned>([&](int i) { return order_key(cs[i]); }, n, limit_, &need_eq);
    }
    int run = 0, eqrun = 0;
    for (int base = 0; base < n; base += 1024) {
        if (run >= limit) break;
        const int i = base + tid;
        bool gt = !filter && i < n, eq = false;
        if (i < n && filter) {
            const unsigned key = order_key(cs[i]);
            gt = key > kth;
            eq = key == kth;
        }
        int etot = 0, tot, eqpos = 0;
        if (filter) eqpos = eqrun + block_ordered_rank<16>(eq, wcnt, &etot);  // (uniform)
        const bool keep = gt || (eq && eqpos < need_eq);
        const int pos = run + block_ordered_rank<16>(keep, wcnt, &tot);
        if (keep && pos < limit) {
            ks[pos] = cs[i];
            ki[pos] = ci[i];
        }
        run += tot;
        eqrun += etot;
    }
    if (tid == 0) {
        nkept[b] = min(run, limit);
        sorted[b] = (filter || always_sorted) ? 1 : 0;
    }
}

// One thread per kept candidate: its output row (its row-major position, or its rank in (score descending, flat index ascending) order:
// the list is in row-major order, so among equal scores the earlier entry goes first), then the key-point itself.
//   default:   n = idx / (w - 1, h - 1) * 2 - 1;  score = bilinear sample of the score map at n;  key-point = (n + 1) / 2 * (w - 1, h - 1)
//   sub_pixel: n from the soft-argmax (temperature 0.1) over the (2r+1)^2 patch of the raw score map, the rest alike
// in upstream's float32 operation order.  knorm keeps n for the descriptor kernel.
__global__ __launch_bounds__(256) void al_emit_kernel(const float* __restrict__ kscore, const int* __restrict__ kidx, int ccap,
                                                      const int* __restrict__ nkept, const int* __restrict__ sorted, int kcap,
                                                      const float* __restrict__ score, int h, int w, int sub_pixel, float* __restrict__ kpts,
                                                      float* __restrict__ knorm, float* __restrict__ scores, int* __restrict__ nkpts,
                                                      int* __restrict__ status) {
    __shared__ float tile[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* ks = kscore + (long)b * ccap;
    const int* ki = kidx + (long)b * ccap;
    const float* sm = score + (long)b * h * w;
    const int n = nkept[b];
    const int cnt = min(n, kcap);
    float* kp = kpts + (long)b * kcap * 2;
    float* kn = knorm + (long)b * kcap * 2;
    float* sc = scores + (long)b * kcap;
    if (blockIdx.x == 0 && tid == 0) {
        nkpts[b] = cnt;
        if (n > kcap) atomicOr(status, 2);  // output capacity too small
    }
    for (int i = blockIdx.x * 256 + tid; i < kcap; i += gridDim.x * 256)  // entries past the count are zero
        if (i >= cnt) {
            kp[2 * i] = kp[2 * i + 1] = 0.0f;
            kn[2 * i] = kn[2 * i + 1] = 0.0f;
            sc[i] = 0.0f;
        }
    const int i0 = blockIdx.x * 256;
    if (i0 >= n) return;  // (uniform)
    const int i = i0 + tid;
    const float mine = i < n ? ks[i] : 0.0f;
    int rank = i;
    if (sorted[b]) {
        rank = 0;
        for (int base = 0; base < n; base += 256) {
            __syncthreads();
            tile[tid] = base + tid < n ? ks[base + tid] : -INFINITY;
            __syncthreads();
            const int m = min(256, n - base);
            for (int j = 0; j < m; ++j) {
                const float o = tile[j];
                rank += (o > mine || (o == mine && base + j < i)) ? 1 : 0;
            }
        }
    }
    if (i >= n || rank >= kcap) return;
    const int idx = ki[i];
    const int x = idx % w, y = idx / w;  // (inside the band: the patch is inside the map)
    const float wm = (float)(w - 1), hm = (float)(h - 1);
    float px = (float)x, py = (float)y;
    if (sub_pixel) {
        float mx = -INFINITY;
        for (int dy = -AL_R; dy <= AL_R; ++dy)
            for (int dx = -AL_R; dx <= AL_R; ++dx) mx = fmaxf(mx, sm[(long)(y + dy) * w + x + dx]);
        float se = 0.0f, sx = 0.0f, sy = 0.0f;
        for (int dy = -AL_R; dy <= AL_R; ++dy)
            for (int dx = -AL_R; dx <= AL_R; ++dx) {
                const float e = expf((sm[(long)(y + dy) * w + x + dx] - mx) / 0.1f);
                se += e;
                sx = fmaf(e, (float)dx, sx);
                sy = fmaf(e, (float)dy, sy);
            }
        px = __fadd_rn(px, sx / se);
        py = __fadd_rn(py, sy / se);
    }
    const float nx = al_norm_pos(px, wm), ny = al_norm_pos(py, hm);
    const float fx = al_pix_pos(nx, wm), fy = al_pix_pos(ny, hm);
    kn[2 * rank] = nx;
    kn[2 * rank + 1] = ny;
    kp[2 * rank] = fx;
    kp[2 * rank + 1] = fy;
    sc[rank] = al_sample_score(sm, h, w, fx, fy);
}

// ------------------------------------------------------------------ descriptors at the key-points
// AL_KB = 32 key-points per workgroup step (grid-stride over the capacity: steps past the count only write the zero rows).  Per corner
// (one for the default, four for sub_pixel): the 32 gathered dim-vectors x1234 go to LDS (one wave per key-point, lane l holds
// channels l and l + 64), Y = X Wd^T runs on v_mfma_f32_32x32x2_f32 with wave w owning output columns 32 w .. 32 w + 31 (dim / 32
// waves work; the f32 matrix pipe serves BOTH arithmetic modes, as in ALIKED's descriptor head), every row is normalised
// (descriptor_map = F.normalize(y)) and summed with its bilinear weight; the sum is normalised once more.
//   mode 0: the pixel trunc((n + 1) / 2 * (w - 1, h - 1)) of key-point n (knorm), weight 1
//   mode 1: the four corners of grid_sample(descriptor_map, n) (align_corners=True, zeros outside)
//   mode 2: the probe: integer pixels (x, y) given in pix, `nprobe` of them
__global__ __launch_bounds__(256) void al_desc_kernel(AlMaps m, const float* __restrict__ wdt, int mode, const float* __restrict__ knorm,
                                                      const int* __restrict__ pix, const int* __restrict__ nkpts, int nprobe, int kcap,
                                                      float* __restrict__ desc) {
    constexpr int LD = 129;  // odd row stride: the 32 rows of an A fragment hit distinct banks
    __shared__ float S[AL_KB * LD];
    __shared__ float G[AL_KB * LD];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int dim = m.dim;
    const int nk = nkpts ? min(nkpts[b], kcap) : min(nprobe, kcap);
    const int ncorner = mode == 1 ? 4 : 1;
    const float wm = (float)(m.w - 1), hm = (float)(m.h - 1);
    for (int k0 = blockIdx.x * AL_KB; k0 < kcap; k0 += gridDim.x * AL_KB) {
        float* out = desc + ((long)b * kcap + k0) * dim;
        if (k0 >= nk) {  // rows past the count are zero
            for (int e = tid; e < AL_KB * dim; e += 256)
                if (k0 + e / dim < kcap) out[e] = 0.0f;
            continue;
        }
        float acc[AL_KB / 4][2];
#pragma unroll
        for (int q = 0; q < AL_KB / 4; ++q) acc[q][0] = acc[q][1] = 0.0f;
        for (int j = 0; j < ncorner; ++j) {
            float cw[AL_KB / 4];
            __syncthreads();  // (every wave is done with S and G of the corner before)
#pragma unroll
            for (int q = 0; q < AL_KB / 4; ++q) {
                const int kp = wv + 4 * q, i = k0 + kp;
                int px = -1, py = -1;
                float wgt = 0.0f;
                if (i < nk) {  // (wave-uniform)
                    if (mode == 2) {
                        px = pix[2 * i];
                        py = pix[2 * i + 1];
                        wgt = 1.0f;
                    } else {
                        const float* kn = knorm + ((long)b * kcap + i) * 2;
                        const float fx = al_pix_pos(kn[0], wm), fy = al_pix_pos(kn[1], hm);
                        if (mode == 0) {
                            px = (int)fx;
                            py = (int)fy;
                            wgt = 1.0f;
                        } else {
                            const AlBil t = al_bil(fx, fy);
                            px = t.x0 + (j & 1);
                            py = t.y0 + (j >> 1);
                            wgt = t.w[j];
                        }
                    }
                }
                const bool inside = px >= 0 && px < m.w && py >= 0 && py < m.h;
                cw[q] = inside ? wgt : 0.0f;
                S[kp * LD + lane] = (inside && lane < dim) ? al_feat(m, b, py, px, lane) : 0.0f;
                S[kp * LD + lane + 64] = (inside && lane + 64 < dim) ? al_feat(m, b, py, px, lane + 64) : 0.0f;
            }
            __syncthreads();
            if (32 * wv < dim) {  // (wave-uniform)
                f32x16 g;
#pragma unroll
                for (int r = 0; r < 16; ++r) g[r] = 0.0f;
                for (int k = 0; k < dim; k += 2) g = mfma32(S[lo * LD + k + hi], wdt[(k + hi) * dim + 32 * wv + lo], g);
#pragma unroll
                for (int r = 0; r < 16; ++r) G[frag_row(r, hi) * LD + 32 * wv + lo] = g[r];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < AL_KB / 4; ++q) {  // descriptor_map = F.normalize(y, dim=1) at this corner, times its weight
                const int kp = wv + 4 * q;
                const float v0 = lane < dim ? G[kp * LD + lane] : 0.0f, v1 = lane + 64 < dim ? G[kp * LD + lane + 64] : 0.0f;
                const float d = fmaxf(sqrtf(wave_sum(v0 * v0 + v1 * v1)), 1e-12f);
                acc[q][0] = fmaf(v0 / d, cw[q], acc[q][0]);
                acc[q][1] = fmaf(v1 / d, cw[q], acc[q][1]);
            }
        }
#pragma unroll
        for (int q = 0; q < AL_KB / 4; ++q) {  // the second F.normalize; one wave per row
            const int kp = wv + 4 * q;
            if (k0 + kp >= kcap) continue;
            float v0 = acc[q][0], v1 = acc[q][1];
            if (k0 + kp < nk) {
                const float d = fmaxf(sqrtf(wave_sum(v0 * v0 + v1 * v1)), 1e-12f);
                v0 /= d;
                v1 /= d;
            } else {
                v0 = v1 = 0.0f;
            }
            if (lane < dim) out[(long)kp * dim + lane] = v0;
            if (lane + 64 < dim) out[(long)kp * dim + lane + 64] = v1;
        }
    }
}

}  // namespace

// ------------------------------------------------------------------ workspace
struct AlWs {
    float *a1, *x1, *p1, *t2, *x2, *f2, *g2, *p2, *t3, *x3, *f3, *g3, *p3, *t4, *x4, *f4, *g4;
    float *score, *nms, *kscore, *knorm;
    AkDkdWs dkd;
    int *kidx, *nkept, *sorted, *status;
    size_t total;
    bool ok;
};
static AlWs al_carve(void* ws, size_t bytes, const AlDims& d, int B, int h, int w, int kcap) {
    WsAlloc a(ws, bytes);
    AlWs s;
    const size_t P0 = (size_t)ak_pad32(h) * ak_pad32(w), P1 = P0 / 4, P3 = P0 / 64, P5 = P0 / 1024;
    s.a1 = a.get<float>(B * P0 * d.c1);
    s.x1 = a.get<float>(B * P0 * d.c1);
    s.p1 = a.get<float>(B * P1 * d.P[1]);
    s.t2 = a.get<float>(B * P1 * d.P[2]);
    s.x2 = a.get<float>(B * P1 * d.P[2]);
    s.f2 = a.get<float>(B * P1 * d.dq);
    s.g2 = a.get<float>(B * P1);
    s.p2 = a.get<float>(B * P3 * d.P[2]);
    s.t3 = a.get<float>(B * P3 * d.P[3]);
    s.x3 = a.get<float>(B * P3 * d.P[3]);
    s.f3 = a.get<float>(B * P3 * d.dq);
    s.g3 = a.get<float>(B * P3);
    s.p3 = a.get<float>(B * P5 * d.P[3]);
    s.t4 = a.get<float>(B * P5 * d.P[4]);
    s.x4 = a.get<float>(B * P5 * d.P[4]);
    s.f4 = a.get<float>(B * P5 * d.dq);
    s.g4 = a.get<float>(B * P5);
    s.score = a.get<float>((size_t)B * h * w);
    s.nms = a.get<float>((size_t)B * h * w);
    s.dkd.carve(a, B, h, w);
    s.kscore = a.get<float>((size_t)B * h * w);
    s.kidx = a.get<int>((size_t)B * h * w);
    s.nkept = a.get<int>(B);
    s.sorted = a.get<int>(B);
    s.knorm = a.get<float>((size_t)B * kcap * 2);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

// survivors of simple_nms (radius 2) are more than 2 apart (Chebyshev) unless scores tie exactly
extern "C" int imcui_hip_alike_max_keypoints_bound(int H, int W) { return cdiv(H, AL_R + 1) * cdiv(W, AL_R + 1); }
// (sized for kcap up to every pixel: the key-point list in the workspace is 2 floats per entry)
extern "C" size_t imcui_hip_alike_workspace_bytes(int variant, int B, int H, int W) {
    const AlVar* a = al_var(variant);
    if (!a || B <= 0 || H <= 0 || W <= 0) return 0;
    return al_carve(nullptr, 0, al_dims(*a), B, H, W, H * W).total;
}

// ------------------------------------------------------------------ the dense part: encoder, branch maps, score map
static int al_dense(imcui_hip_t* h, const AlDims& d, const AlLayout& l, const float* P, const float* image, int B, int H, int W, const AlWs& s,
                    float* smap, hipStream_t stream) {
    const int Hp = ak_pad32(H), Wp = ak_pad32(W);
    const bool split = h->precision == 1;
    int rc;
    auto px = [&](int sh) { return (long)(Hp >> sh) * (Wp >> sh); };
    // implicit-GEMM 3x3 convolution (pad 1) of the NHWC map `in` + folded-BatchNorm bias (+ resid), ReLU
    auto conv_gemm = [&](int L, const float* in, int sh, float* out, const float* resid) -> int {
        GemmP g;
        g.epi = EPI_CONV;
        g.A = in;
        gemm_set_weights(g, P, l.g[L], d.gn[L], 9 * d.gcin[L], split);
        gemm_set_conv(g, 3, 1, 1, Hp >> sh, Wp >> sh, Hp >> sh, Wp >> sh, d.gcin[L]);
        g.M = (int)(B * px(sh));
        g.C = out;
        g.ldc = d.gn[L];
        g.resid = resid;
        g.ldr = d.gn[L];
        g.act = 1;
        return gemm_launch(h, g, stream);
    };
    auto pool = [&](const float* src, int lds, int C, float* dst, int ldd, int k, int sh_out) {
        const long n4 = (long)B * px(sh_out) * ldd / 4;
        hipLaunchKernelGGL(ak_pool_kernel<true>, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, src, lds, C, dst, ldd, k, Hp >> sh_out, Wp >> sh_out, n4);
    };
    // a ResBlock at 1 / 2^sh: t = ReLU(bn1(conv1 x)); out = downsample(x) + bias; out = ReLU(bn2(conv2 t) + out)
    auto resblock = [&](int blk, const float* x, int sh, float* t, float* out) -> int {
        const int L = 2 * (blk - 2), cin = d.P[blk - 1], cout = d.P[blk];
        IMCUI_RUN(conv_gemm(L, x, sh, t, nullptr));
        const long n = B * px(sh) * cout;
        hipLaunchKernelGGL(al_pw_kernel, dim3(grid_stride_blocks(n)), dim3(256), 0, stream, x, cin, cin, P + l.dw[blk - 2], P + l.db[blk - 2], out, cout, n);
        return conv_gemm(L + 1, t, sh, out, out);
    };
    auto head = [&](int i, const float* x, int sh, float* f, float* g) {
        const long np = B * px(sh);
        const dim3 grid(blocks_256(np));
        const float *wt = P + l.cw[i], *ws = P + l.sw + (size_t)i * d.dq;
        if (d.dq == 16)
            hipLaunchKernelGGL(al_head_kernel<16>, grid, dim3(256), 0, stream, x, d.P[i + 1], d.P[i + 1], wt, ws, f, g, np);
        else if (d.dq == 24)
            hipLaunchKernelGGL(al_head_kernel<24>, grid, dim3(256), 0, stream, x, d.P[i + 1], d.P[i + 1], wt, ws, f, g, np);
        else
            hipLaunchKernelGGL(al_head_kernel<32>, grid, dim3(256), 0, stream, x, d.P[i + 1], d.P[i + 1], wt, ws, f, g, np);
    };
    // ---- block 1 (full resolution, VALU)
    {
        AkConvP c{image, 2, H, W, 0, 0, 0, 3, P + l.vw[0], P + l.vb[0], s.a1, d.c1, Hp, Wp, Hp, Wp, 0, 0};
        AkConvP e{s.a1, 0, 0, 0, 0, 0, d.c1, d.c1, P + l.vw[1], P + l.vb[1], s.x1, d.c1, Hp, Wp, Hp, Wp, 0, 0};
        if (d.c1 == 8) {
            ak_conv3<8, 3, 3>(c, B, stream);
            ak_conv3<8, 8, 3>(e, B, stream);
        } else {
            ak_conv3<16, 3, 3>(c, B, stream);
            ak_conv3<16, 16, 3>(e, B, stream);
        }
        IMCUI_CHECK_LAUNCH(h);
    }
    // ---- blocks 2..4
    pool(s.x1, d.c1, d.c1, s.p1, d.P[1], 2, 1);
    IMCUI_RUN(resblock(2, s.p1, 1, s.t2, s.x2));
    pool(s.x2, d.P[2], d.P[2], s.p2, d.P[2], 4, 3);
    IMCUI_RUN(resblock(3, s.p2, 3, s.t3, s.x3));
    pool(s.x3, d.P[3], d.P[3], s.p3, d.P[3], 4, 5);
    IMCUI_RUN(resblock(4, s.p3, 5, s.t4, s.x4));
    // ---- f_i and the score slices at the branch's resolution (f1 only ever in registers)
    head(1, s.x2, 1, s.f2, s.g2);
    head(2, s.x3, 3, s.f3, s.g3);
    head(3, s.x4, 5, s.f4, s.g4);
    // ---- the score map, cropped to H x W
    {
        const long np = (long)B * H * W;
        const dim3 grid(blocks_256(np));
        const float *c1t = P + l.cw[0], *ws1 = P + l.sw;
        if (d.c1 == 8 && d.dq == 16)
            hipLaunchKernelGGL((al_score_kernel<8, 16>), grid, dim3(256), 0, stream, s.x1, c1t, ws1, s.g2, s.g3, s.g4, smap, H, W, Hp, Wp, np);
        else if (d.c1 == 8 && d.dq == 24)
            hipLaunchKernelGGL((al_score_kernel<8, 24>), grid, dim3(256), 0, stream, s.x1, c1t, ws1, s.g2, s.g3, s.g4, smap, H, W, Hp, Wp, np);
        else
            hipLaunchKernelGGL((al_score_kernel<16, 32>), grid, dim3(256), 0, stream, s.x1, c1t, ws1, s.g2, s.g3, s.g4, smap, H, W, Hp, Wp, np);
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

static int al_check(imcui_hip_t* h, const AlVar* a, int variant, int B, int H, int W) {
    if (!a)
        return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "alike: variant %d is not served (0 alike-t, 1 alike-s, 2 alike-n; alike-l has a second head layer)", variant);
    if (B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "alike: B=%d above 1024", B);
    if (H < 32 || W < 32) return imcui_set_err(h, IMCUI_ERR_ARG, "alike: H=%d W=%d must be at least 32", H, W);
    if ((long)B * ak_pad32(H) * ak_pad32(W) > 0x7fffffffL) return imcui_set_err(h, IMCUI_ERR_ARG, "alike: B=%d images of %dx%d exceed 2^31 pixels per call", B, H, W);
    return IMCUI_OK;
}

extern "C" int imcui_hip_alike_forward(imcui_hip_t* h, int variant, const float* packed, const float* image, int B, int H, int W, float threshold,
                                       int top_k, int n_limit, int sub_pixel, int kcap, float* keypoints, float* scores, float* descriptors,
                                       int* num_keypoints, int* status, float* score_map, float* dbg_x4, float* dbg_f2, float* dbg_f3, float* dbg_f4,
                                       void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    const AlVar* a = al_var(variant);
    const int rc0 = al_check(h, a, variant, B, H, W);
    if (rc0 != IMCUI_OK) return rc0;
    if (kcap <= 0 || !packed || !image || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "alike: null argument or kcap<=0");
    if ((long)kcap > (long)H * W) return imcui_set_err(h, IMCUI_ERR_ARG, "alike: kcap=%d above H*W", kcap);
    const AlDims d = al_dims(*a);
    const AlLayout l = al_layout(d);
    AlWs s = al_carve(ws, ws_bytes, d, B, H, W, kcap);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "alike: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const int Hp = ak_pad32(H), Wp = ak_pad32(W);
    const float* P = packed;
    float* smap = score_map ? score_map : s.score;
    const int rc = al_dense(h, d, l, P, image, B, H, W, s, smap, stream);
    if (rc != IMCUI_OK) return rc;
    auto px = [&](int sh) { return (size_t)(Hp >> sh) * (Wp >> sh); };
    if (dbg_x4) hipMemcpyAsync(dbg_x4, s.x4, B * px(5) * d.P[4] * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (dbg_f2) hipMemcpyAsync(dbg_f2, s.f2, B * px(1) * d.dq * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (dbg_f3) hipMemcpyAsync(dbg_f3, s.f3, B * px(3) * d.dq * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (dbg_f4) hipMemcpyAsync(dbg_f4, s.f4, B * px(5) * d.dq * sizeof(float), hipMemcpyDeviceToDevice, stream);
    // ---- DKD
    const int rc1 = imcui_hip_simple_nms(h, smap, s.nms, B, H, W, AL_R, stream);
    if (rc1 != IMCUI_OK) return rc1;
    int* st = status ? status : s.status;
    const bool topk = top_k > 0;
    const int ccap = H * W;
    // the cut: top_k first, then n_limit (the smaller one decides; both keep the highest scores); 0 or less = no cut
    int limit = ccap;
    if (topk) limit = min(limit, top_k);
    if (n_limit > 0) limit = min(limit, n_limit);
    // (the band: rows / columns [0, r] and [h - r, h) are zeroed)
    const int rc2 = ak_dkd_candidates(h, smap, s.nms, H, W, B, AL_R + 1, AL_R, threshold, topk, s.dkd, st, stream);
    if (rc2 != IMCUI_OK) return rc2;
    hipLaunchKernelGGL(al_cut_kernel, dim3(B), dim3(1024), 0, stream, s.dkd.cand.cscore, s.dkd.cand.cidx, ccap, s.dkd.scan.total, limit, topk ? 1 : 0, s.kscore, s.kidx, s.nkept, s.sorted);
    hipLaunchKernelGGL(al_emit_kernel, dim3(cdiv(limit, 256), B), dim3(256), 0, stream, s.kscore, s.kidx, ccap, s.nkept, s.sorted, kcap, smap, H, W,
                       sub_pixel ? 1 : 0, keypoints, s.knorm, scores, num_keypoints, st);
    IMCUI_CHECK_LAUNCH(h);
    // ---- descriptors
    const AlMaps m{s.x1, s.f2, s.f3, s.f4, P + l.cw[0], Hp, Wp, H, W, d.c1, d.dq, d.dim};
    hipLaunchKernelGGL(al_desc_kernel, dim3(min(cdiv(kcap, AL_KB), 1024), B), dim3(256), 0, stream, m, P + l.wdt, sub_pixel ? 1 : 0, s.knorm, (const int*)nullptr,
                       num_keypoints, 0, kcap, descriptors);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// test entry: the sparse descriptor head at n caller-given integer pixels of ONE image
extern "C" int imcui_hip_alike_desc_probe(imcui_hip_t* h, int variant, const float* packed, const float* image, int H, int W, const int* xy, int n,
                                          float* descriptors, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    const AlVar* a = al_var(variant);
    const int rc0 = al_check(h, a, variant, 1, H, W);
    if (rc0 != IMCUI_OK) return rc0;
    if (n <= 0 || n > H * W || !packed || !image || !xy || !descriptors) return imcui_set_err(h, IMCUI_ERR_ARG, "alike probe: null argument or n outside 1..H*W");
    const AlDims d = al_dims(*a);
    const AlLayout l = al_layout(d);
    AlWs s = al_carve(ws, ws_bytes, d, 1, H, W, 1);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "alike probe: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const int rc = al_dense(h, d, l, packed, image, 1, H, W, s, s.score, stream);
    if (rc != IMCUI_OK) return rc;
    const AlMaps m{s.x1, s.f2, s.f3, s.f4, packed + l.cw[0], ak_pad32(H), ak_pad32(W), H, W, d.c1, d.dq, d.dim};
    hipLaunchKernelGGL(al_desc_kernel, dim3(min(cdiv(n, AL_KB), 1024), 1), dim3(256), 0, stream, m, packed + l.wdt, 2, (const float*)nullptr, xy,
                       (const int*)nullptr, n, n, descriptors);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
