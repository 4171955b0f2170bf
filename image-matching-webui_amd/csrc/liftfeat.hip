// LiftFeat sparse extraction on MI355X: the call behind imcui/hloc/extractors/liftfeat.py:34-53 (`self.net.extract(image)` and the
// wrapper's own cut).  The network is restated in tests/liftfeat_reference.py (the reference's third_party directory is empty); what
// that restatement rests on is listed in INTEGRATION.md, "LiftFeat: what is pinned".
//
// Data flow (NHWC maps; Hp x Wp = the image zero-padded at the bottom and right to multiples of 32, N = (Hp/8)(Wp/8) tokens per image):
//   gray    = channel mean of (x * 255) / 255, zero in the pad                                          [B, Hp, Wp]   lf_gray_pad_kernel
//   stats   = InstanceNorm2d(1) over the PADDED image (xf_shared.h: the pad zeros add nothing to the sums, the count is Hp Wp)
//   trunk   = XFeat's block1 .. block_fusion and keypoint head (xf_shared.h, the same kernels and layer table as xfeat.hip)
//             -> feats M1 [B, N, 64], logits K1 [B, N, 65], heat = softmax(K1)[:64] on the pixel grid [B, Hp, Wp]
//   normals = three lf_upconv_kernel launches, 64 -> 32 -> 16 -> 8 channels from 1/8 to full resolution: the LDS tile is filled with the
//             bilinear x2 of the low-resolution map (nothing up-sampled is stored), 3x3 + folded BatchNorm + LeakyReLU from LDS; the last
//             launch adds the 1x1 8 -> 3 and the L2 norm and stores the unfolded layout [B, N, 192] (channel c * 64 + dy * 8 + dx):
//             neither the full-resolution 8-channel map nor D1 exists in memory
//   booster = lf_token_kernel, one wave per tile of 32 tokens, every Linear on v_mfma_f32_32x32x2_f32 (both arithmetic modes) with the
//             activations in LDS: launch 0 = the three encoders + q / k / v of layer 0 + the tile's soft-max partials; launch i = proj,
//             residual, LayerNorm, FFN, LayerNorm of layer i - 1 + q / k / v and partials of layer i; the last launch ends with final_proj
//             and the L2 norm.  Between two launches lf_fold_kernel (one wave per image) folds the partials in tile order into kv [64].
//             No float atomics: an image's bits do not depend on the batch.
//   select  = 5x5 NMS over the PADDED heat map (XfKeep's rule) AND inside H x W -> candidate list (select.h) -> score = nearest sample
//             with XFeat's float32 grid arithmetic -> lf_cut_kernel: the wrapper's rule on the device from the image's own count
//             (count <= max_keypoints: row-major; else ascending stable argsort, the last max_keypoints, 0 keeps all, -k drops the k
//             lowest) -> ranked_rows_kernel with LfRow: key-point, score, bicubic descriptor of the boosted map, L2 norm
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "xf_shared.h"

// ------------------------------------------------------------------ configuration (read from the checkpoint's shapes by the caller)
// cfg [8] = {kenc present, FFN hidden width, denc hidden, nenc hidden 1, nenc hidden 2, kenc hidden 1, kenc hidden 2, AFT layers}
#define LF_NCFG 8
#define LF_MAX_LAYERS 8
struct LfCfg {
    int kenc, ffn, dh, nh1, nh2, kh1, kh2, nlayer;
    bool ok;
};
static LfCfg lf_cfg(const int* c) {
    LfCfg g{};
    if (!c) return g;
    g = LfCfg{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], false};
    auto wide = [](int v) { return v >= 32 && v <= 128 && v % 32 == 0; };  // the first hidden map of an MLP, the FFN: LDS [32][128]
    auto narrow = [](int v) { return v == 32 || v == 64; };                // the second hidden map: LDS [32][64]
    g.ok = (g.kenc == 0 || g.kenc == 1) && wide(g.ffn) && wide(g.dh) && wide(g.nh1) && narrow(g.nh2) && (!g.kenc || (wide(g.kh1) && narrow(g.kh2))) &&
           g.nlayer >= 1 && g.nlayer <= LF_MAX_LAYERS;
    return g;
}

// a Linear in the packed buffer: Wt [Kp][N] (transposed, Kp = K rounded up to even, the extra row zero), bias [N]
struct LfLin {
    size_t w, b;
    int K, N;
    void place(PackCursor& c, int K_, int N_) {
        K = K_;
        N = N_;
        w = c.get((size_t)((K + 1) & ~1) * N);
        b = c.get(N);
    }
};
struct LfLayout {
    size_t xf;  // XFeat's layout (xf_layout; heatmap_head unused and zero)
    LfLin denc[2], nenc[3], kenc[3];
    struct {
        LfLin q, k, v, proj, f0, f1;
        size_t ln1, ln2;  // gamma [64], beta [64]
    } aft[LF_MAX_LAYERS];
    LfLin fin;
    struct {
        size_t w, b;  // [tap][cin][cout] and [cout], BatchNorm folded
    } up[3];
    size_t w1, b1;  // 1x1 8 -> 3: [8][3], [3]
    size_t total;
};
static const int LF_UP_CIN[3] = {64, 32, 16};

static LfLayout lf_layout(const LfCfg& g) {
    LfLayout l;
    PackCursor c;
    l.xf = c.get(xf_layout().total);
    l.denc[0].place(c, 64, g.dh);
    l.denc[1].place(c, g.dh, 64);
    l.nenc[0].place(c, 192, g.nh1);
    l.nenc[1].place(c, g.nh1, g.nh2);
    l.nenc[2].place(c, g.nh2, 64);
    if (g.kenc) {
        l.kenc[0].place(c, 65, g.kh1);
        l.kenc[1].place(c, g.kh1, g.kh2);
        l.kenc[2].place(c, g.kh2, 64);
    }
    for (int i = 0; i < g.nlayer; ++i) {
        l.aft[i].q.place(c, 64, 64);
        l.aft[i].k.place(c, 64, 64);
        l.aft[i].v.place(c, 64, 64);
        l.aft[i].proj.place(c, 64, 64);
        l.aft[i].ln1 = c.get(128);
        l.aft[i].f0.place(c, 64, g.ffn);
        l.aft[i].f1.place(c, g.ffn, 64);
        l.aft[i].ln2 = c.get(128);
    }
    l.fin.place(c, 64, 64);
    for (int s = 0; s < 3; ++s) {
        l.up[s].w = c.get((size_t)9 * LF_UP_CIN[s] * (LF_UP_CIN[s] / 2));
        l.up[s].b = c.get(LF_UP_CIN[s] / 2);
    }
    l.w1 = c.get(24);
    l.b1 = c.get(3);
    l.total = c.off;
    return l;
}

// tensors in packing order: XFeat's trunk without heatmap_head.*, the normal head, the booster
static TensorTable lf_tensors(const LfCfg& g) {
    TensorTable t;
    for (int i = 0; i < imcui_hip_xfeat_num_tensors(); ++i) {
        const std::string n = imcui_hip_xfeat_tensor_name(i);
        if (n.rfind("heatmap_head.", 0) != 0) t.add(n, 0);
    }
    for (int s = 0; s < 3; ++s) {
        const std::string p = "normal_head." + std::to_string(s);
        const int ci = LF_UP_CIN[s], co = ci / 2;
        t.add(p + ".conv.weight", (size_t)co * ci * 9);
        t.add(p + ".conv.bias", co);
        t.add(p + ".bn.weight", co);
        t.add(p + ".bn.bias", co);
        t.add(p + ".bn.running_mean", co);
        t.add(p + ".bn.running_var", co);
    }
    t.add("normal_head.3.weight", 24);
    t.add("normal_head.3.bias", 3);
    auto lin = [&](const std::string& p, int K, int N) {
        t.add(p + ".weight", (size_t)K * N);
        t.add(p + ".bias", N);
    };
    const std::string fb = "feature_boost.";
    lin(fb + "denc.0", 64, g.dh);
    lin(fb + "denc.2", g.dh, 64);
    lin(fb + "nenc.0", 192, g.nh1);
    lin(fb + "nenc.2", g.nh1, g.nh2);
    lin(fb + "nenc.4", g.nh2, 64);
    if (g.kenc) {
        lin(fb + "kenc.0", 65, g.kh1);
        lin(fb + "kenc.2", g.kh1, g.kh2);
        lin(fb + "kenc.4", g.kh2, 64);
    }
    for (int i = 0; i < g.nlayer; ++i) {
        const std::string p = fb + "layers." + std::to_string(i);
        lin(p + ".attn.q", 64, 64);
        lin(p + ".attn.k", 64, 64);
        lin(p + ".attn.v", 64, 64);
        lin(p + ".attn.proj", 64, 64);
        t.add(p + ".norm1.weight", 64);
        t.add(p + ".norm1.bias", 64);
        lin(p + ".ffn.0", 64, g.ffn);
        lin(p + ".ffn.2", g.ffn, 64);
        t.add(p + ".norm2.weight", 64);
        t.add(p + ".norm2.bias", 64);
    }
    lin(fb + "final_proj", 64, 64);
    return t;
}

extern "C" size_t imcui_hip_liftfeat_packed_floats(const int* cfg) {
    const LfCfg g = lf_cfg(cfg);
    return g.ok ? lf_layout(g).total : 0;
}
extern "C" int imcui_hip_liftfeat_num_tensors(const int* cfg) {
    const LfCfg g = lf_cfg(cfg);
    return g.ok ? lf_tensors(g).size() : 0;
}
extern "C" const char* imcui_hip_liftfeat_tensor_name(const int* cfg, int i) {
    static thread_local std::string buf;
    const LfCfg g = lf_cfg(cfg);
    if (!g.ok) return nullptr;
    const TensorTable t = lf_tensors(g);
    if (i < 0 || i >= t.size()) return nullptr;
    buf = t.name(i);
    return buf.c_str();
}

static void lf_pack_linear(const float* w, const float* b, const LfLin& L, float* packed) {  // w [N][K] (torch Linear)
    for (int n = 0; n < L.N; ++n)
        for (int k = 0; k < L.K; ++k) packed[L.w + (size_t)k * L.N + n] = w[(size_t)n * L.K + k];
    memcpy(packed + L.b, b, L.N * sizeof(float));
}

// t: host pointers in imcui_hip_liftfeat_tensor_name order (shapes checked by the caller).  BatchNorm (eval, eps 1e-5, affine) of the
// normal head is folded in float32 into the convolution before it: w' = w * scale, b' = bias * scale + shift.
extern "C" int imcui_hip_liftfeat_pack_weights(const int* cfg, const float* const* t, float* packed) {
    const LfCfg g = lf_cfg(cfg);
    if (!g.ok || !t || !packed) return IMCUI_ERR_ARG;
    const TensorTable tt = lf_tensors(g);
    for (int i = 0; i < tt.size(); ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const LfLayout l = lf_layout(g);
    memset(packed, 0, l.total * sizeof(float));
    // the trunk through XFeat's packer: heatmap_head.* (absent here) gets zero weights and an identity BatchNorm
    std::vector<float> zeros(64 * 64, 0.0f), ones(64, 1.0f);
    std::vector<const float*> xt(imcui_hip_xfeat_num_tensors());
    int own = 0;
    for (size_t i = 0; i < xt.size(); ++i) {
        const std::string n = imcui_hip_xfeat_tensor_name((int)i);
        if (n.rfind("heatmap_head.", 0) == 0)
            xt[i] = n.find("running_var") != std::string::npos ? ones.data() : zeros.data();
        else
            xt[i] = t[own++];
    }
    const int rc = imcui_hip_xfeat_pack_weights(xt.data(), packed + l.xf);
    if (rc != IMCUI_OK) return rc;
    auto at = [&](const std::string& n) { return t[tt.find(n)]; };
    for (int s = 0; s < 3; ++s) {
        const std::string p = "normal_head." + std::to_string(s);
        const int ci = LF_UP_CIN[s], co = ci / 2;
        const float* bn[4] = {at(p + ".bn.weight"), at(p + ".bn.bias"), at(p + ".bn.running_mean"), at(p + ".bn.running_var")};
        std::vector<float> scale, shift;
        bn_fold_f32(bn, co, scale, shift);
        const float *w = at(p + ".conv.weight"), *b = at(p + ".conv.bias");  // OIHW
        for (int o = 0; o < co; ++o) {
            for (int i = 0; i < ci; ++i)
                for (int tap = 0; tap < 9; ++tap) packed[l.up[s].w + ((size_t)tap * ci + i) * co + o] = w[((size_t)o * ci + i) * 9 + tap] * scale[o];
            packed[l.up[s].b + o] = b[o] * scale[o] + shift[o];
        }
    }
    {
        const float *w = at("normal_head.3.weight"), *b = at("normal_head.3.bias");  // [3][8]
        for (int j = 0; j < 3; ++j) {
            for (int c = 0; c < 8; ++c) packed[l.w1 + c * 3 + j] = w[j * 8 + c];
            packed[l.b1 + j] = b[j];
        }
    }
    auto lin = [&](const std::string& p, const LfLin& L) { lf_pack_linear(at(p + ".weight"), at(p + ".bias"), L, packed); };
    const std::string fb = "feature_boost.";
    lin(fb + "denc.0", l.denc[0]);
    lin(fb + "denc.2", l.denc[1]);
    lin(fb + "nenc.0", l.nenc[0]);
    lin(fb + "nenc.2", l.nenc[1]);
    lin(fb + "nenc.4", l.nenc[2]);
    if (g.kenc) {
        lin(fb + "kenc.0", l.kenc[0]);
        lin(fb + "kenc.2", l.kenc[1]);
        lin(fb + "kenc.4", l.kenc[2]);
    }
    for (int i = 0; i < g.nlayer; ++i) {
        const std::string p = fb + "layers." + std::to_string(i);
        lin(p + ".attn.q", l.aft[i].q);
        lin(p + ".attn.k", l.aft[i].k);
        lin(p + ".attn.v", l.aft[i].v);
        lin(p + ".attn.proj", l.aft[i].proj);
        lin(p + ".ffn.0", l.aft[i].f0);
        lin(p + ".ffn.2", l.aft[i].f1);
        memcpy(packed + l.aft[i].ln1, at(p + ".norm1.weight"), 64 * sizeof(float));
        memcpy(packed + l.aft[i].ln1 + 64, at(p + ".norm1.bias"), 64 * sizeof(float));
        memcpy(packed + l.aft[i].ln2, at(p + ".norm2.weight"), 64 * sizeof(float));
        memcpy(packed + l.aft[i].ln2 + 64, at(p + ".norm2.bias"), 64 * sizeof(float));
    }
    lin(fb + "final_proj", l.fin);
    return IMCUI_OK;
}

namespace {

// ------------------------------------------------------------------ input stage
// image [B, 3, H, W] in [0, 1] -> gray [B, Hp, Wp]: the wrapper's `* 255` and extract's `/ 255` (float32, one rounding each), the channel
// mean (summed in double: three equal channels give the channel itself), zero in the pad
__global__ __launch_bounds__(256) void lf_gray_pad_kernel(const float* __restrict__ img, float* __restrict__ gray, int H, int W, int Hp, int Wp, long npix) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % Wp);
    const long q = p / Wp;
    const int y = (int)(q % Hp);
    const long b = q / Hp;
    float v = 0.0f;
    if (x < W && y < H) {
        double acc = 0.0;
        for (int c = 0; c < 3; ++c) acc += (double)__fdiv_rn(__fmul_rn(img[((b * 3 + c) * H + y) * (long)W + x], 255.0f), 255.0f);
        v = (float)(acc / 3.0);
    }
    gray[p] = v;
}

// ------------------------------------------------------------------ bilinear x2 + 3x3 convolution + folded BatchNorm + LeakyReLU
// in [B, h, w, CIN] -> [B, 2h, 2w, COUT].  One workgroup = TS x TS output pixels x NG = 256 / TS^2 groups of COUT / NG output channels (a
// group is one wave or more, so its weight reads are uniform).  The (TS + 2)^2 window of the UP-SAMPLED map is computed into LDS with
// ATen's float32 index arithmetic (align: scale = (in - 1) / (out - 1), src = scale * dst; else src = 0.5 (dst + 0.5) - 0.5 clamped at 0;
// rows mixed first), zero outside the up-sampled map (the convolution's padding).  One fmaf chain per output, (tap, channel) ascending.
// LAST: the 1x1 8 -> 3 (one chain each, channel ascending) and x / max(|x|, 1e-12), stored to the unfolded layout
// out [B, 2h/8, 2w/8, 192], channel c * 64 + dy * 8 + dx (2h and 2w multiples of 8).
struct LfUpP {
    const float* in;
    int h, w;
    const float *wt, *bias;
    float* out;
    int align;
    float slope, sh, sw;
    const float *w1, *b1;
};
template <int CIN, int COUT, int TS, bool LAST>
__global__ __launch_bounds__(256) void lf_upconv_kernel(LfUpP p) {
    constexpr int TW = TS + 2, CS = CIN + 1, NG = 256 / (TS * TS), CPT = COUT / NG;
    static_assert(NG * TS * TS == 256 && CPT * NG == COUT && (!LAST || NG == 1), "tile shape");
    __shared__ float S[TW * TW * CS];
    const int H = 2 * p.h, W = 2 * p.w, b = blockIdx.z;
    const int oy0 = blockIdx.y * TS - 1, ox0 = blockIdx.x * TS - 1;
    const float* src = p.in + (long)b * p.h * p.w * CIN;
    for (int e = threadIdx.x; e < TW * TW * CIN; e += 256) {
        const int c = e % CIN, pix = e / CIN;
        const int ty = pix / TW, tx = pix - ty * TW;
        const int oy = oy0 + ty, ox = ox0 + tx;
        float v = 0.0f;
        if (oy >= 0 && oy < H && ox >= 0 && ox < W) {
            int y0, y1, x0, x1;
            float hy0, hy1, wx0, wx1;
            if (p.align) {
                bilinear_src_align_corners(oy, p.sh, p.h, &y0, &y1, &hy0, &hy1);
                bilinear_src_align_corners(ox, p.sw, p.w, &x0, &x1, &wx0, &wx1);
            } else {
                bilinear_src_half_pixel(oy, 0.5f, p.h, &y0, &y1, &hy0, &hy1);
                bilinear_src_half_pixel(ox, 0.5f, p.w, &x0, &x1, &wx0, &wx1);
            }
            const float v00 = src[((long)y0 * p.w + x0) * CIN + c], v01 = src[((long)y0 * p.w + x1) * CIN + c];
            const float v10 = src[((long)y1 * p.w + x0) * CIN + c], v11 = src[((long)y1 * p.w + x1) * CIN + c];
            const float top = __fadd_rn(__fmul_rn(wx0, v00), __fmul_rn(wx1, v01)), bot = __fadd_rn(__fmul_rn(wx0, v10), __fmul_rn(wx1, v11));
            v = __fadd_rn(__fmul_rn(hy0, top), __fmul_rn(hy1, bot));
        }
        S[pix * CS + c] = v;
    }
    __syncthreads();
    const int pi = threadIdx.x % (TS * TS), g = __builtin_amdgcn_readfirstlane(threadIdx.x / (TS * TS));
    const int py = pi / TS, px = pi - py * TS;
    const float* wg = p.wt + g * CPT;
    float acc[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) acc[c] = p.bias[g * CPT + c];
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const float* s = S + ((py + tap / 3) * TW + px + tap % 3) * CS;
        const float* k = wg + (long)tap * CIN * COUT;
#pragma unroll 4
        for (int ci = 0; ci < CIN; ++ci) {
            const float v = s[ci];
#pragma unroll
            for (int c = 0; c < CPT; ++c) acc[c] = fmaf(v, k[ci * COUT + c], acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < CPT; ++c) acc[c] = acc[c] > 0.0f ? acc[c] : acc[c] * p.slope;
    const int oy = oy0 + 1 + py, ox = ox0 + 1 + px;
    if (oy >= H || ox >= W) return;
    if (!LAST) {
        float* o = p.out + (((long)b * H + oy) * W + ox) * COUT + g * CPT;
#pragma unroll
        for (int c = 0; c < CPT; ++c) o[c] = acc[c];
    } else {
        float n[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float a = p.b1[j];
#pragma unroll
            for (int c = 0; c < CPT; ++c) a = fmaf(acc[c], p.w1[c * 3 + j], a);
            n[j] = a;
        }
        const float nrm = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12f);
        float* o = p.out + (((long)b * (H / 8) + oy / 8) * (W / 8) + ox / 8) * 192 + (oy & 7) * 8 + (ox & 7);
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j * 64] = n[j] / nrm;
    }
}

// ------------------------------------------------------------------ the token network
#define LF_TILE 32  // tokens per workgroup = the FIXED soft-max chunk
struct LfLinD {
    const float *w, *b;  // Wt [Kp][N], bias [N]
    int K, N;
};
struct LfTokP {
    int N, ntile;
    int enc, finish, qkv, fin;  // what this launch does (uniform)
    const float *in_d, *in_k, *in_n;  // enc: [B, N, 64], [B, N, 65], [B, N, 192]
    LfLinD denc[2], nenc[3], kenc[3];
    int has_kenc;
    const float *q_prev, *kv_prev;  // finish: sigmoid(q) [.] kv of the layer being finished: [B, N, 64], [B, 64]
    LfLinD proj, f0, f1;
    const float *ln1, *ln2;
    float* x;  // [B, N, 64]: read unless enc, written unless fin
    LfLinD lq, lk, lv;
    float *q_out, *part;  // qkv: q [B, N, 64] (may be q_prev: a tile reads its rows before it writes them), part [B][ntile][3][64]
    LfLinD lfin;
    float* out;  // fin: [B, N, 64], unit rows
};

// Y [32][L.N] (LDS, row stride yst) = act(X [32][L.K] (LDS, row stride xst, column K zero when K is odd) Wt + bias), or Y += ... (ACC).
// One wave; 32-column blocks in turn, K ascending in steps of 2 on v_mfma_f32_32x32x2_f32.  ACT: 0 none, 1 ReLU, 2 GELU (erf).
template <int ACT, bool ACC>
__device__ __forceinline__ void lf_linear(const float* xs, int xst, const LfLinD& L, float* ys, int yst) {
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    const int Kp = (L.K + 1) & ~1;
    const float* xrow = xs + lo * xst + hi;
    for (int nb = 0; nb < L.N; nb += 32) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float* wcol = L.w + (long)hi * L.N + nb + lo;
        for (int k0 = 0; k0 < Kp; k0 += 2) acc = mfma32(xrow[k0], wcol[(long)k0 * L.N], acc);
        const float bv = L.b[nb + lo];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r] + bv;
            if (ACT == 1) v = fmaxf(v, 0.0f);
            if (ACT == 2) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
            float* y = ys + frag_row(r, hi) * yst + nb + lo;
            *y = ACC ? *y + v : v;
        }
    }
    __syncthreads();
}

// rows t0 .. t0 + nv - 1 of src [N][C] -> dst [32][stride], columns C .. CP - 1 and rows nv .. 31 zero
template <int C, int CP>
__device__ __forceinline__ void lf_load_rows(float* dst, int stride, const float* src, int nv) {
    for (int e = threadIdx.x; e < LF_TILE * CP; e += 64) {
        const int r = e / CP, c = e - r * CP;
        dst[r * stride + c] = (r < nv && c < C) ? src[(long)r * C + c] : 0.0f;
    }
    __syncthreads();
}
__device__ __forceinline__ void lf_store_rows(const float* s, int stride, float* dst, int nv) {
    for (int e = threadIdx.x; e < LF_TILE * 64; e += 64) {
        const int r = e >> 6, c = e & 63;
        if (r < nv) dst[(long)r * 64 + c] = s[r * stride + c];
    }
}
// LayerNorm(64, eps 1e-6) of the 32 rows of x (LDS, stride xst) in place: lane (row = l & 31, half = l >> 5) walks 32 channels, the two
// halves meet through one shuffle; mean, then the centred variance (biased)
__device__ __forceinline__ void lf_layernorm(float* x, int xst, const float* gb) {
    const int r = threadIdx.x & 31, hf = threadIdx.x >> 5;
    float* row = x + r * xst + hf * 32;
    float s = 0.0f;
    for (int j = 0; j < 32; ++j) s += row[j];
    s += __shfl_xor(s, 32, 64);
    const float mean = s * (1.0f / 64.0f);
    float v = 0.0f;
    for (int j = 0; j < 32; ++j) {
        const float d = row[j] - mean;
        v = fmaf(d, d, v);
    }
    v += __shfl_xor(v, 32, 64);
    const float inv = 1.0f / sqrtf(v * (1.0f / 64.0f) + 1e-6f);
    for (int j = 0; j < 32; ++j) row[j] = (row[j] - mean) * inv * gb[hf * 32 + j] + gb[64 + hf * 32 + j];
    __syncthreads();
}

#define LF_ST_IN 194  // strides = width + 2: rows two banks apart, the two k of an MFMA step on even / odd banks
#define LF_ST_H1 130
#define LF_ST_64 66
__global__ __launch_bounds__(64) void lf_token_kernel(LfTokP p) {
    __shared__ float S_in[LF_TILE * LF_ST_IN], S_h1[LF_TILE * LF_ST_H1], S_h2[LF_TILE * LF_ST_64], S_x[LF_TILE * LF_ST_64];
    const int b = blockIdx.y, tile = blockIdx.x, t0 = tile * LF_TILE, lane = threadIdx.x;
    const int nv = min(LF_TILE, p.N - t0);
    const long row0 = (long)b * p.N + t0;
    if (p.enc) {
        lf_load_rows<64, 64>(S_x, LF_ST_64, p.in_d + row0 * 64, nv);  // x = d
        lf_linear<1, false>(S_x, LF_ST_64, p.denc[0], S_h1, LF_ST_H1);
        lf_linear<0, true>(S_h1, LF_ST_H1, p.denc[1], S_x, LF_ST_64);  // x += MLP(d)
        lf_load_rows<192, 192>(S_in, LF_ST_IN, p.in_n + row0 * 192, nv);
        lf_linear<1, false>(S_in, LF_ST_IN, p.nenc[0], S_h1, LF_ST_H1);
        lf_linear<1, false>(S_h1, LF_ST_H1, p.nenc[1], S_h2, LF_ST_64);
        lf_linear<0, true>(S_h2, LF_ST_64, p.nenc[2], S_x, LF_ST_64);  // x += MLP(n)
        if (p.has_kenc) {
            lf_load_rows<65, 66>(S_in, LF_ST_IN, p.in_k + row0 * 65, nv);
            lf_linear<1, false>(S_in, LF_ST_IN, p.kenc[0], S_h1, LF_ST_H1);
            lf_linear<1, false>(S_h1, LF_ST_H1, p.kenc[1], S_h2, LF_ST_64);
            lf_linear<0, true>(S_h2, LF_ST_64, p.kenc[2], S_x, LF_ST_64);  // x += MLP(k)
        }
    } else {
        lf_load_rows<64, 64>(S_x, LF_ST_64, p.x + row0 * 64, nv);
    }
    if (p.finish) {
        const float kvc = p.kv_prev[b * 64 + lane];
        for (int r = 0; r < LF_TILE; ++r) S_in[r * LF_ST_64 + lane] = r < nv ? sigmoidf_(p.q_prev[(row0 + r) * 64 + lane]) * kvc : 0.0f;
        __syncthreads();
        lf_linear<0, true>(S_in, LF_ST_64, p.proj, S_x, LF_ST_64);
        lf_layernorm(S_x, LF_ST_64, p.ln1);
        lf_linear<2, false>(S_x, LF_ST_64, p.f0, S_h1, LF_ST_H1);
        lf_linear<0, true>(S_h1, LF_ST_H1, p.f1, S_x, LF_ST_64);
        lf_layernorm(S_x, LF_ST_64, p.ln2);
    }
    if (!p.fin) lf_store_rows(S_x, LF_ST_64, p.x + row0 * 64, nv);
    if (p.qkv) {
        lf_linear<0, false>(S_x, LF_ST_64, p.lq, S_in, LF_ST_64);
        lf_linear<0, false>(S_x, LF_ST_64, p.lk, S_h2, LF_ST_64);
        lf_linear<0, false>(S_x, LF_ST_64, p.lv, S_h1, LF_ST_H1);
        lf_store_rows(S_in, LF_ST_64, p.q_out + row0 * 64, nv);
        // the tile's soft-max partials of channel `lane`, tokens ascending
        float m = -INFINITY;
        for (int r = 0; r < nv; ++r) m = fmaxf(m, S_h2[r * LF_ST_64 + lane]);
        float s = 0.0f, a = 0.0f;
        for (int r = 0; r < nv; ++r) {
            const float e = expf(S_h2[r * LF_ST_64 + lane] - m);
            s += e;
            a = fmaf(e, S_h1[r * LF_ST_H1 + lane], a);
        }
        float* pt = p.part + ((long)b * p.ntile + tile) * 192;
        pt[lane] = m;
        pt[64 + lane] = s;
        pt[128 + lane] = a;
    }
    if (p.fin) {
        lf_linear<0, false>(S_x, LF_ST_64, p.lfin, S_in, LF_ST_64);
        const int r = lane & 31, hf = lane >> 5;
        float* row = S_in + r * LF_ST_64 + hf * 32;
        float q = 0.0f;
        for (int j = 0; j < 32; ++j) q = fmaf(row[j], row[j], q);
        q += __shfl_xor(q, 32, 64);
        const float nrm = fmaxf(sqrtf(q), 1e-12f);
        for (int j = 0; j < 32; ++j) row[j] = row[j] / nrm;
        __syncthreads();
        lf_store_rows(S_in, LF_ST_64, p.out + row0 * 64, nv);
    }
}

// kv [b][c] = sum_t softmax_t(k)[t, c] v[t, c] from the tile partials, folded in tile order: one wave per image, lane = channel
__global__ __launch_bounds__(64) void lf_fold_kernel(const float* __restrict__ part, int ntile, float* __restrict__ kv) {
    const int b = blockIdx.x, c = threadIdx.x;
    const float* pt = part + (long)b * ntile * 192;
    float M = -INFINITY;
    for (int t = 0; t < ntile; ++t) M = fmaxf(M, pt[(long)t * 192 + c]);
    float S = 0.0f, A = 0.0f;
    for (int t = 0; t < ntile; ++t) {
        const float f = expf(pt[(long)t * 192 + c] - M);
        S = fmaf(pt[(long)t * 192 + 64 + c], f, S);
        A = fmaf(pt[(long)t * 192 + 128 + c], f, A);
    }
    kv[b * 64 + c] = A / S;
}

// ------------------------------------------------------------------ selection
// XfKeep's 5x5 NMS over the padded Hp x Wp map, and inside the H x W image: a pad pixel can suppress a real one and is not itself kept
struct LfKeep {
    XfKeep nms;
    int H, W;
    __device__ void bind(int) {}
    __device__ bool operator()(const float* hm, int idx) const {
        const int y = idx / nms.w, x = idx - y * nms.w;
        return x < W && y < H && nms(hm, idx);
    }
};

// score of candidate i = InterpolateSparse2d("nearest") of the heat map at its own pixel (XFeat's grid arithmetic against (Wp, Hp): the
// last column / row of the padded map samples outside and gives 0).  Grid (cdiv(ccap, 256), B).
__global__ __launch_bounds__(256) void lf_score_kernel(const float* __restrict__ k1h, const int* __restrict__ cidx, const int* __restrict__ ncand, int ccap,
                                                       int Hp, int Wp, float* __restrict__ cscore) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(ncand[b], ccap)) return;
    const int idx = cidx[(long)b * ccap + i];
    const int y = idx / Wp, x = idx - y * Wp;
    cscore[(long)b * ccap + i] = xf_sample_nearest(k1h + (long)b * Hp * Wp, Hp, Wp, xf_coord(x, Wp, Wp), xf_coord(y, Hp, Hp));
}

// The wrapper's cut (liftfeat.py:42-46) from the image's own count n.  max_keypoints >= n: every candidate, row-major (asc [b] = 0).
// Otherwise ascending stable argsort and its last max_keypoints entries: k > 0 the k largest (score, list index) keys, 0 all of them,
// k < 0 all but the -k lowest.  The kept slots leave in list order; LfRow ranks them.  status bit 1: more rows than the outputs hold.
__global__ __launch_bounds__(1024) void lf_cut_kernel(const float* __restrict__ cscore, const int* __restrict__ ntotal, int ccap, int max_kp, int kout,
                                                      int* __restrict__ kslot, int* __restrict__ nkept, int* __restrict__ asc, int* __restrict__ status) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* cs = cscore + (long)b * ccap;
    const int n = min(ntotal[b], ccap);
    const auto key_at = [&](int i) { return score_index_key(cs[i], i); };
    const bool ascending = max_kp < n;
    const int keep = !ascending ? n : (max_kp > 0 ? max_kp : max(n + max_kp, 0));
    bool filter = false;
    unsigned long long kth = 0;
    if (keep > 0 && keep < n) {  // (uniform)
        filter = true;
        kth = radix_select_kth<1024, unsigned long long>(key_at, n, keep);
    }
    const int run = keep_kth_in_order(key_at, keep > 0 ? n : 0, filter, kth, keep, kslot + (long)b * ccap);
    if (tid == 0) {
        nkept[b] = min(run, keep);
        asc[b] = ascending ? 1 : 0;
        if (ntotal[b] > ccap || keep > kout) atomicOr(status, 2);
    }
}

// the rows of ranked_rows_kernel: key-point (x, y), score, descriptor = bicubic sample of the boosted map [h8, w8, 64], L2 norm
struct LfRow {
    const int *cidx, *asc;
    const float* boost;
    int ccap, kout, Hp, Wp;
    float *kpts, *scores, *desc;
    __device__ void clear(int b, int lo, int hi) const {
        for (int i = lo + (threadIdx.x >> 6); i < hi; i += 4) {
            const int lane = threadIdx.x & 63;
            desc[((long)b * kout + i) * 64 + lane] = 0.0f;
            if (lane < 2) kpts[((long)b * kout + i) * 2 + lane] = 0.0f;
            if (lane == 2) scores[(long)b * kout + i] = 0.0f;
        }
    }
    __device__ void emit(int b, int i0, int m, const int* ks, const int* rank, const float* cs) const {
        const int lane = threadIdx.x & 63, h8 = Hp / 8, w8 = Wp / 8;
        const bool ascending = asc[b] != 0;
        for (int j = threadIdx.x >> 6; j < m; j += 4) {
            const int slot = ks[i0 + j], r = ascending ? rank[j] : i0 + j;
            const int idx = cidx[(long)b * ccap + slot];
            const int y = idx / Wp, x = idx - y * Wp;
            const float v = xf_sample_bicubic(boost + (long)b * h8 * w8 * 64, h8, w8, xf_coord(x, Wp, w8), xf_coord(y, Hp, h8), lane);
            const float nrm = sqrtf(wave_sum(v * v));
            desc[((long)b * kout + r) * 64 + lane] = v / fmaxf(nrm, 1e-12f);
            if (lane == 0) {
                kpts[((long)b * kout + r) * 2 + 0] = (float)x;
                kpts[((long)b * kout + r) * 2 + 1] = (float)y;
                scores[(long)b * kout + r] = cs[slot];
            }
        }
    }
};

// ------------------------------------------------------------------ launches
static inline float lf_align_scale(int in) { return in > 1 ? (float)(in - 1) / (float)(2 * in - 1) : 0.0f; }

// up-conv stage s (0, 1; 2 plain or fused) of in [B, h, w, cin] -> out
int lf_upconv(imcui_hip_t* h, const float* PK, const LfLayout& l, int s, bool fused, const float* in, int B, int hh, int ww, float* out, int align,
              float slope, hipStream_t stream) {
    LfUpP p{in, hh, ww, PK + l.up[s].w, PK + l.up[s].b, out, align, slope, lf_align_scale(hh), lf_align_scale(ww), PK + l.w1, PK + l.b1};
    const int H = 2 * hh, W = 2 * ww;
    if (s == 0)
        hipLaunchKernelGGL((lf_upconv_kernel<64, 32, 8, false>), dim3(cdiv(W, 8), cdiv(H, 8), B), dim3(256), 0, stream, p);
    else if (s == 1)
        hipLaunchKernelGGL((lf_upconv_kernel<32, 16, 8, false>), dim3(cdiv(W, 8), cdiv(H, 8), B), dim3(256), 0, stream, p);
    else if (!fused)
        hipLaunchKernelGGL((lf_upconv_kernel<16, 8, 16, false>), dim3(cdiv(W, 16), cdiv(H, 16), B), dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL((lf_upconv_kernel<16, 8, 16, true>), dim3(cdiv(W, 16), cdiv(H, 16), B), dim3(256), 0, stream, p);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

LfLinD lf_lin(const float* PK, const LfLin& L) { return LfLinD{PK + L.w, PK + L.b, L.K, L.N}; }

// scratch of the token network for B images of N tokens
struct LfTokBufs {
    float *x, *q, *part, *kv;
    void carve(WsAlloc& a, int B, int N) {
        x = a.get<float>((size_t)B * N * 64);
        q = a.get<float>((size_t)B * N * 64);
        part = a.get<float>((size_t)B * cdiv(N, LF_TILE) * 192);
        kv = a.get<float>((size_t)B * 64);
    }
};
void lf_set_layer(LfTokP& p, const float* PK, const LfLayout& l, int i) {
    p.lq = lf_lin(PK, l.aft[i].q);
    p.lk = lf_lin(PK, l.aft[i].k);
    p.lv = lf_lin(PK, l.aft[i].v);
}
void lf_set_finish(LfTokP& p, const float* PK, const LfLayout& l, int i) {
    p.proj = lf_lin(PK, l.aft[i].proj);
    p.f0 = lf_lin(PK, l.aft[i].f0);
    p.f1 = lf_lin(PK, l.aft[i].f1);
    p.ln1 = PK + l.aft[i].ln1;
    p.ln2 = PK + l.aft[i].ln2;
}
LfTokP lf_tok_base(const LfTokBufs& t, int N) {
    LfTokP p{};
    p.N = N;
    p.ntile = cdiv(N, LF_TILE);
    p.x = t.x;
    p.q_prev = t.q;
    p.q_out = t.q;
    p.kv_prev = t.kv;
    p.part = t.part;
    return p;
}
void lf_set_enc(LfTokP& p, const float* PK, const LfLayout& l, const LfCfg& g, const float* d, const float* k, const float* n) {
    p.enc = 1;
    p.in_d = d;
    p.in_k = k;
    p.in_n = n;
    p.has_kenc = g.kenc;
    for (int i = 0; i < 2; ++i) p.denc[i] = lf_lin(PK, l.denc[i]);
    for (int i = 0; i < 3; ++i) p.nenc[i] = lf_lin(PK, l.nenc[i]);
    if (g.kenc)
        for (int i = 0; i < 3; ++i) p.kenc[i] = lf_lin(PK, l.kenc[i]);
}
void lf_tok_launch(const LfTokP& p, int B, hipStream_t stream) { hipLaunchKernelGGL(lf_token_kernel, dim3(p.ntile, B), dim3(64), 0, stream, p); }
void lf_fold_launch(const LfTokBufs& t, int N, int B, hipStream_t stream) {
    hipLaunchKernelGGL(lf_fold_kernel, dim3(B), dim3(64), 0, stream, t.part, cdiv(N, LF_TILE), t.kv);
}

// FeatureBooster on d [B, N, 64], k [B, N, 65], n [B, N, 192] -> out [B, N, 64] (unit rows): nlayer + 1 token launches, nlayer folds
int lf_booster(imcui_hip_t* h, const float* PK, const LfLayout& l, const LfCfg& g, const LfTokBufs& t, const float* d, const float* k, const float* n, int B,
               int N, float* out, hipStream_t stream) {
    for (int i = 0; i <= g.nlayer; ++i) {
        LfTokP p = lf_tok_base(t, N);
        if (i == 0) lf_set_enc(p, PK, l, g, d, k, n);
        if (i > 0) {
            p.finish = 1;
            lf_set_finish(p, PK, l, i - 1);
        }
        if (i < g.nlayer) {
            p.qkv = 1;
            lf_set_layer(p, PK, l, i);
        } else {
            p.fin = 1;
            p.lfin = lf_lin(PK, l.fin);
            p.out = out;
        }
        lf_tok_launch(p, B, stream);
        if (i < g.nlayer) lf_fold_launch(t, N, B, stream);
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// scratch of the selection for B maps of Hp x Wp
struct LfSelBufs {
    CandScan scan;
    ScoreIndexList cand;
    CutList cut;
    int *asc, *status;
    void carve(WsAlloc& a, int B, int Hp, int Wp) {
        scan.carve(a, B, (size_t)Hp * Wp);
        cand.carve(a, B, Hp * Wp);  // a constant map is one plateau: every pixel can be a candidate
        cut.carve(a, B, Hp * Wp);
        asc = a.get<int>(B);
        status = a.get<int>(1);
    }
};
int lf_select(imcui_hip_t* h, const LfSelBufs& s, const float* k1h, const float* boost, int B, int H, int W, int Hp, int Wp, float threshold, int max_kp,
              int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, hipStream_t stream) {
    int* st = status ? status : s.status;
    hipMemsetAsync(st, 0, sizeof(int), stream);
    const int ccap = s.cand.cap;
    cand_list(stream, k1h, Hp * Wp, B, LfKeep{XfKeep{Hp, Wp, threshold}, H, W}, s.scan, ccap, s.cand.emit());
    hipLaunchKernelGGL(lf_score_kernel, dim3(cdiv(ccap, 256), B), dim3(256), 0, stream, k1h, s.cand.cidx, s.scan.total, ccap, Hp, Wp, s.cand.cscore);
    hipLaunchKernelGGL(lf_cut_kernel, dim3(B), dim3(1024), 0, stream, s.cand.cscore, s.scan.total, ccap, max_kp, kcap, s.cut.kslot, s.cut.nkept, s.asc, st);
    ranked_rows(stream, s.cand.cscore, ccap, s.cut, kcap, num_keypoints, LfRow{s.cand.cidx, s.asc, boost, ccap, kcap, Hp, Wp, keypoints, scores, descriptors}, B);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

struct LfWs {
    XfTrunkBufs t;
    float *k1h, *u1, *u2, *nrm, *boost;
    LfTokBufs tok;
    LfSelBufs sel;
    size_t total;
    bool ok;
};
LfWs lf_carve(void* ws, size_t bytes, int B, int Hp, int Wp) {
    WsAlloc a(ws, bytes);
    LfWs s;
    const size_t P = (size_t)B * Hp * Wp;
    s.t.carve(a, B, Hp, Wp);
    s.k1h = a.get<float>(P);
    s.u1 = a.get<float>(P / 16 * 32);
    s.u2 = a.get<float>(P / 4 * 16);
    s.nrm = a.get<float>(P / 64 * 192);
    s.boost = a.get<float>(P / 64 * 64);
    s.tok.carve(a, B, Hp / 8 * (Wp / 8));
    s.sel.carve(a, B, Hp, Wp);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

inline int lf_pad32(int v) { return (v + 31) / 32 * 32; }

}  // namespace

extern "C" size_t imcui_hip_liftfeat_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H < 1 || W < 1) return 0;
    return lf_carve(nullptr, 0, B, lf_pad32(H), lf_pad32(W)).total;
}

// NMS survivors whose scores do not tie exactly are more than 2 apart (Chebyshev), over the padded map
extern "C" int imcui_hip_liftfeat_max_keypoints_bound(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return cdiv(lf_pad32(H), 3) * cdiv(lf_pad32(W), 3);
}

extern "C" int imcui_hip_liftfeat_forward(imcui_hip_t* h, const int* cfg, const float* packed, const float* image, int B, int C, int H, int W, float threshold,
                                          int max_keypoints, int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status,
                                          float* kpt_heat, float* normals, float* boosted, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    const LfCfg g = lf_cfg(cfg);
    if (!g.ok) return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat: configuration not supported (hidden widths: multiples of 32 up to 128, second hidden 32 or 64)");
    if (C != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat: C=%d must be 3 (the wrapper's squeeze().transpose(1, 2, 0) needs three channels)", C);
    if (H < 1 || W < 1 || (long)lf_pad32(H) * lf_pad32(W) > (1l << 30)) return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat: H=%d W=%d out of range", H, W);
    if (kcap <= 0 || !packed || !image || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat: null argument or kcap<=0");
    const int Hp = lf_pad32(H), Wp = lf_pad32(W), h8 = Hp / 8, w8 = Wp / 8, N = h8 * w8;
    LfWs s = lf_carve(ws, ws_bytes, B, Hp, Wp);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "liftfeat: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const LfLayout l = lf_layout(g);
    const XfLayout xl = xf_layout();
    const float* XP = packed + l.xf;
    int rc;
    // ---- input stage, trunk, key-point head
    const long np0 = (long)B * Hp * Wp;
    hipLaunchKernelGGL(lf_gray_pad_kernel, dim3(blocks_256(np0)), dim3(256), 0, stream, image, s.t.gray, H, W, Hp, Wp, np0);
    xf_stats(stream, s.t.gray, (long)Hp * Wp, B, s.t.part, s.t.norm);
    IMCUI_CHECK_LAUNCH(h);
    IMCUI_RUN(xf_trunk_feats(h, XP, xl, s.t, B, Hp, Wp, stream));
    float* k1h = kpt_heat ? kpt_heat : s.k1h;
    IMCUI_RUN(xf_trunk_kpts(h, XP, xl, s.t, B, Hp, Wp, k1h, stream));
    // ---- normal head: 1/8 -> 1/4 -> 1/2 -> full resolution, unfolded
    float* nrm = normals ? normals : s.nrm;
    IMCUI_RUN(lf_upconv(h, packed, l, 0, false, s.t.e3, B, h8, w8, s.u1, 1, 0.1f, stream));
    IMCUI_RUN(lf_upconv(h, packed, l, 1, false, s.u1, B, 2 * h8, 2 * w8, s.u2, 1, 0.1f, stream));
    IMCUI_RUN(lf_upconv(h, packed, l, 2, true, s.u2, B, 4 * h8, 4 * w8, nrm, 1, 0.1f, stream));
    // ---- lifting: d = feats, k = the key-point logits, n = the unfolded normals
    float* boost = boosted ? boosted : s.boost;
    IMCUI_RUN(lf_booster(h, packed, l, g, s.tok, s.t.e3, s.t.logits, nrm, B, N, boost, stream));
    // ---- selection
    return lf_select(h, s.sel, k1h, boost, B, H, W, Hp, Wp, threshold, max_keypoints, kcap, keypoints, scores, descriptors, num_keypoints, status, stream);
}

// ------------------------------------------------------------------ test entries (device pointers)
// the input stage: image [B, 3, H, W] -> gray [B, Hp, Wp] and norm [B][2] = (invstd, -mean * invstd); ws: B * cdiv(Hp Wp, 4096) * 16 bytes
extern "C" int imcui_hip_liftfeat_input_probe(imcui_hip_t* h, const float* image, int B, int H, int W, float* gray, float* norm, void* ws, size_t ws_bytes,
                                              void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0 || H < 1 || W < 1 || !image || !gray || !norm) return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat input probe: bad argument");
    const int Hp = lf_pad32(H), Wp = lf_pad32(W);
    if (!ws || ws_bytes < (size_t)B * cdiv(Hp * Wp, XF_STAT_CHUNK) * 16) return imcui_set_err(h, IMCUI_ERR_WS, "liftfeat input probe: workspace too small");
    const long np0 = (long)B * Hp * Wp;
    hipLaunchKernelGGL(lf_gray_pad_kernel, dim3(blocks_256(np0)), dim3(256), 0, stream, image, gray, H, W, Hp, Wp, np0);
    xf_stats(stream, gray, (long)Hp * Wp, B, (double*)ws, norm);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// one up-conv stage (stage 0, 1, 2) on x [B, hh, ww, cin]: fused == 0 -> out [B, 2hh, 2ww, cin / 2]; stage 2 with fused == 1 -> the
// unfolded unit normals [B, 2hh/8, 2ww/8, 192] (2hh, 2ww multiples of 8)
extern "C" int imcui_hip_liftfeat_upconv_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* x, int stage, int fused, int B, int hh, int ww,
                                               int align_corners, float slope, float* out, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    const LfCfg g = lf_cfg(cfg);
    if (!g.ok || stage < 0 || stage > 2 || (fused && stage != 2) || B <= 0 || hh < 1 || ww < 1 || !packed || !x || !out)
        return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat upconv probe: bad argument");
    if (fused && ((2 * hh) % 8 || (2 * ww) % 8)) return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat upconv probe: the fused stage needs 2h, 2w multiples of 8");
    return lf_upconv(h, packed, lf_layout(g), stage, fused != 0, x, B, hh, ww, out, align_corners, slope, (hipStream_t)stream_);
}

extern "C" size_t imcui_hip_liftfeat_tokens_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    WsAlloc a(nullptr, 0);
    LfTokBufs t;
    t.carve(a, B, N);
    return a.off;
}
// the booster on d [B, N, 64], k [B, N, 65], n [B, N, 192] -> out [B, N, 64] (unit rows); x_enc (optional) [B, N, 64] = the sum of the
// encoders (the state ahead of the first AFT layer)
extern "C" int imcui_hip_liftfeat_booster_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* d, const float* k, const float* n, int B, int N,
                                                float* out, float* x_enc, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    const LfCfg g = lf_cfg(cfg);
    if (!g.ok || B <= 0 || N <= 0 || !packed || !d || !k || !n || !out) return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat booster probe: bad argument");
    WsAlloc a(ws, ws_bytes);
    LfTokBufs t;
    t.carve(a, B, N);
    if (!ws || !a.ok) return imcui_set_err(h, IMCUI_ERR_WS, "liftfeat booster probe: workspace too small");
    const LfLayout l = lf_layout(g);
    if (x_enc) {  // the encoders alone: x is stored, no q / k / v
        LfTokP p = lf_tok_base(t, N);
        lf_set_enc(p, packed, l, g, d, k, n);
        p.x = x_enc;
        lf_tok_launch(p, B, stream);
    }
    return lf_booster(h, packed, l, g, t, d, k, n, B, N, out, stream);
}
// AFT layer `layer` on x [B, N, 64] -> out [B, N, 64]; kv (optional) [B, 64]
extern "C" int imcui_hip_liftfeat_aft_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* x, int layer, int B, int N, float* out, float* kv,
                                            void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    const LfCfg g = lf_cfg(cfg);
    if (!g.ok || layer < 0 || layer >= g.nlayer || B <= 0 || N <= 0 || !packed || !x || !out) return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat aft probe: bad argument");
    WsAlloc a(ws, ws_bytes);
    LfTokBufs t;
    t.carve(a, B, N);
    if (!ws || !a.ok) return imcui_set_err(h, IMCUI_ERR_WS, "liftfeat aft probe: workspace too small");
    const LfLayout l = lf_layout(g);
    hipMemcpyAsync(out, x, (size_t)B * N * 64 * sizeof(float), hipMemcpyDeviceToDevice, stream);
    LfTokP p = lf_tok_base(t, N);
    p.x = out;
    p.qkv = 1;
    lf_set_layer(p, packed, l, layer);
    lf_tok_launch(p, B, stream);
    lf_fold_launch(t, N, B, stream);
    copy_if(kv, t.kv, (size_t)B * 64 * sizeof(float), stream);
    LfTokP f = lf_tok_base(t, N);
    f.x = out;
    f.finish = 1;
    lf_set_finish(f, packed, l, layer);
    lf_tok_launch(f, B, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_liftfeat_select_workspace_bytes(int B, int Hp, int Wp) {
    if (B <= 0 || Hp < 8 || Wp < 8) return 0;
    WsAlloc a(nullptr, 0);
    LfSelBufs s;
    s.carve(a, B, Hp, Wp);
    return a.off;
}
// the selection on a given heat map [B, Hp, Wp] (Hp, Wp multiples of 8 >= H, W) and boosted map [B, Hp/8, Wp/8, 64]
extern "C" int imcui_hip_liftfeat_select_probe(imcui_hip_t* h, const float* heat, const float* boosted, int B, int H, int W, int Hp, int Wp, float threshold,
                                               int max_keypoints, int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status,
                                               void* ws, size_t ws_bytes, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0 || Hp < 8 || Wp < 8 || Hp % 8 || Wp % 8 || H < 1 || W < 1 || H > Hp || W > Wp || kcap <= 0 || !heat || !boosted || !keypoints || !scores ||
        !descriptors || !num_keypoints || (long)Hp * Wp > (1l << 30))
        return imcui_set_err(h, IMCUI_ERR_ARG, "liftfeat select probe: bad argument");
    WsAlloc a(ws, ws_bytes);
    LfSelBufs s;
    s.carve(a, B, Hp, Wp);
    if (!ws || !a.ok) return imcui_set_err(h, IMCUI_ERR_WS, "liftfeat select probe: workspace too small");
    return lf_select(h, s, heat, boosted, B, H, W, Hp, Wp, threshold, max_keypoints, kcap, keypoints, scores, descriptors, num_keypoints, status,
                     (hipStream_t)stream_);
}
