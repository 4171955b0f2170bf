// LANet forward on MI355X (zoo entry lanet + NN-mutual; extractor conf lanet): imcui/hloc/extractors/lanet.py:39-63 around
// lanet.network_v0.model.PointModel(is_test=True) as one batched call.  The network is NOT in the reference checkout: it is restated in
// tests/lanet_reference.py, and that file is the definition this one is tested against ("LANet: what is pinned").
//
//   image       [B, 3, H, W] RGB in [0, 1]; tvf.Normalize(mean, std) is applied where the image is READ (two float32 roundings), so the
//               zero padding of layer 0 is zero in normalised units; mean and std live in the packed buffer's header
//   conv1a      3 -> c1 on the VALU (stem3x3_kernel, ReLU, c1 = 32 / 64); any other width or LeakyReLU: the normalised image is written
//               as a 32-channel NHWC map (la_pad_kernel) and the layer runs on the implicit GEMM like the rest
//   conv1b .. conv4b, convDa, convPa   implicit-GEMM 3x3 (gemm.hip, both arithmetic modes), folded BatchNorm and the activation in its
//               epilogue; the flooring 2x2 max-pools are pool2x2_kernel<0>.  x2 (1/2), x3 (1/4), x4 (1/8) are kept.
//   tail        one wave per cell: the 256 -> 4 and 256 -> 2 3x3 layers on the two hidden maps, soft-max of channels 0..2 (aware),
//               sigmoid of channel 3 with the border cells multiplied by 0 (score), tanh and the cell-relative position (coord).  The
//               6-channel maps are not written.
//   selection   score > threshold in row-major cell order (select.h cand_list), the cut and the ascending stable rank
//               R2D2 and D2-Net use (cand_cut, ranked_rows_kernel with LaRow); the list holds every cell, so it cannot overflow
//   descriptor  only at the kept key-points.  des_conv2(x2) and des_conv3(x3) are never written: convolution, folded BatchNorm and
//               bilinear sampling are linear, so the k x k x C neighbourhoods of the up to four corners grid_sample touches are blended
//               into one patch per key-point and level and that patch is multiplied by the level's [k k C][256] weights on
//               v_mfma_f32_32x32x2_f32, 32 key-points per tile (the f32 matrix pipe serves both arithmetic modes, as in ALIKE's head);
//               + (sum of the in-map corner weights) bias; level 4 is a 4-corner gather of x4; aware-weighted sum; d / |d|.
// Explicit float32 order in the decode (no fused multiply-add: build.py compiles this file with -ffp-contract=off), fixed summation
// orders, no float atomics, grids sized by shapes or capacities: a row's bits do not depend on its batch or on replay; no host
// synchronisation.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "imcui_hip.h"
#include "net_kernels.h"
#include "netpack.h"
#include "select.h"

#define LA_DIM 256   // descriptor width = hidden width of the two heads = c4
#define LA_KB 32     // key-points per workgroup step of la_desc_kernel (one 32-row MFMA tile)
#define LA_NCFG 12
#define LA_MAGIC 19521.0f  // "LA"

// ------------------------------------------------------------------ configuration (imcui_hip.h: the 12 ints of `cfg`)
struct LaCfg {
    int c[5];  // 3, c1..c4
    int k[2], bias[2], bn[2];  // des_conv2 / des_conv3
    int act;                   // 1 ReLU, 2 LeakyReLU(0.01)
    int conv_bias;             // the convolutions in front of a BatchNorm carry a bias
};
static bool la_cfg(const int* v, LaCfg* c) {
    if (!v) return false;
    c->c[0] = 3;
    for (int i = 0; i < 4; ++i) c->c[i + 1] = v[i];
    c->k[0] = v[4], c->k[1] = v[5], c->bias[0] = v[6], c->bias[1] = v[7], c->bn[0] = v[8], c->bn[1] = v[9], c->act = v[10], c->conv_bias = v[11];
    for (int i = 1; i <= 4; ++i)
        if (c->c[i] < 32 || c->c[i] % 32 || c->c[i] > 512) return false;
    if (c->c[4] != LA_DIM) return false;  // level 4 IS x4: its width is the descriptor's
    for (int i = 0; i < 2; ++i)
        if ((c->k[i] != 1 && c->k[i] != 3) || (c->bias[i] & ~1) || (c->bn[i] & ~1)) return false;
    return (c->act == 1 || c->act == 2) && !(c->conv_bias & ~1);
}
static bool la_stem_valu(const LaCfg& c) { return c.act == 1 && (c.c[1] == 32 || c.c[1] == 64); }

// the BatchNorm'd 3x3 layers in launch order: the trunk, then the hidden layers of the score and the location head
#define LA_NL 10
static const char* const LA_CONV[LA_NL] = {"conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convDa", "convPa"};
static const char* const LA_BN[LA_NL] = {"bn1a", "bn1b", "bn2a", "bn2b", "bn3a", "bn3b", "bn4a", "bn4b", "bnDa", "bnPa"};
static int la_cin(const LaCfg& c, int i) { return i >= 8 ? c.c[4] : (i & 1) ? c.c[i / 2 + 1] : c.c[i / 2]; }
static int la_cout(const LaCfg& c, int i) { return i >= 8 ? LA_DIM : c.c[i / 2 + 1]; }

static const TensorTable& la_tensors(const LaCfg& c) {
    static std::map<std::string, TensorTable> built;
    static std::mutex mu;
    char key[128];
    snprintf(key, sizeof key, "%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d", c.c[1], c.c[2], c.c[3], c.c[4], c.k[0], c.k[1], c.bias[0], c.bias[1], c.bn[0], c.bn[1],
             c.conv_bias);
    std::lock_guard<std::mutex> g(mu);
    auto it = built.find(key);
    if (it != built.end()) return it->second;
    TensorTable& t = built[key];
    for (int i = 0; i < LA_NL; ++i) {
        const int co = la_cout(c, i);
        t.add(std::string(LA_CONV[i]) + ".weight", (size_t)co * la_cin(c, i) * 9);
        if (c.conv_bias) t.add(std::string(LA_CONV[i]) + ".bias", co);
        for (const char* s : {"weight", "bias", "running_mean", "running_var"}) t.add(std::string(LA_BN[i]) + "." + s, co);
    }
    t.add("convDb.weight", (size_t)4 * LA_DIM * 9);
    t.add("convDb.bias", 4);
    t.add("convPb.weight", (size_t)2 * LA_DIM * 9);
    t.add("convPb.bias", 2);
    for (int l = 0; l < 2; ++l) {
        const std::string n = l == 0 ? "des_conv2" : "des_conv3", b = l == 0 ? "des_bn2" : "des_bn3";
        t.add(n + ".weight", (size_t)LA_DIM * c.c[2 + l] * c.k[l] * c.k[l]);
        if (c.bias[l]) t.add(n + ".bias", LA_DIM);
        if (c.bn[l])
            for (const char* s : {"weight", "bias", "running_mean", "running_var"}) t.add(b + "." + s, LA_DIM);
    }
    return t;
}
extern "C" int imcui_hip_lanet_num_tensors(const int* cfg) {
    LaCfg c;
    return la_cfg(cfg, &c) ? la_tensors(c).size() : 0;
}
extern "C" const char* imcui_hip_lanet_tensor_name(const int* cfg, int i) {
    LaCfg c;
    return la_cfg(cfg, &c) ? la_tensors(c).name(i) : nullptr;
}

// ------------------------------------------------------------------ packed layout
// hdr [64]: magic, the 12 cfg values, mean, std.  w0 / b0: conv1a for the VALU kernel [tap][cin 3][c1] + [c1].  g[0]: conv1a as a GEMM
// layer on the 32-channel padded image (K = 288, channels 3.. zero), g[1..9]: the other BatchNorm'd layers [cout][tap][cin].  tws / twp:
// the tails [tap][256][4] and [tap][256][2], tb [6].  Per level: dw the sparse head's K-major weights [k k C][256], db its bias [256]
// (convolution bias through the BatchNorm), dg the same layer for the dense form.
struct LaLayout {
    size_t hdr, w0, b0;
    GemmLayerOff g[LA_NL];
    size_t tws, twp, tb;
    size_t dw[2], db[2];
    GemmLayerOff dg[2];
    size_t total;
};
static int la_gcin(const LaCfg& c, int i) { return i == 0 ? 32 : la_cin(c, i); }
static LaLayout la_layout(const LaCfg& c) {
    LaLayout l;
    PackCursor p;
    l.hdr = p.get(64);
    l.w0 = p.get((size_t)27 * c.c[1]);
    l.b0 = p.get(c.c[1]);
    for (int i = 0; i < LA_NL; ++i) l.g[i].place(p, la_cout(c, i), 9 * la_gcin(c, i));
    l.tws = p.get((size_t)9 * LA_DIM * 4);
    l.twp = p.get((size_t)9 * LA_DIM * 2);
    l.tb = p.get(6);
    for (int v = 0; v < 2; ++v) {
        const int K = c.k[v] * c.k[v] * c.c[2 + v];
        l.dw[v] = p.get((size_t)K * LA_DIM);
        l.db[v] = p.get(LA_DIM);
        l.dg[v].place(p, LA_DIM, K);
    }
    l.total = p.off;
    return l;
}
extern "C" size_t imcui_hip_lanet_packed_floats(const int* cfg) {
    LaCfg c;
    return la_cfg(cfg, &c) ? la_layout(c).total : 0;
}

// t: host pointers of the tensors in imcui_hip_lanet_tensor_name order (shapes checked by the caller)
extern "C" int imcui_hip_lanet_pack_weights(const int* cfg, const float* const* t, float* packed) {
    LaCfg c;
    if (!la_cfg(cfg, &c) || !t || !packed) return IMCUI_ERR_ARG;
    const TensorTable& names = la_tensors(c);
    for (int i = 0; i < names.size(); ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const LaLayout l = la_layout(c);
    memset(packed, 0, l.total * sizeof(float));
    auto T = [&](const std::string& name) { return t[names.find(name)]; };
    packed[l.hdr] = LA_MAGIC;
    for (int i = 0; i < LA_NCFG; ++i) packed[l.hdr + 1 + i] = (float)cfg[i];
    packed[l.hdr + 13] = 0.5f;    // tvf.Normalize(mean=0.5, std=0.225), every channel
    packed[l.hdr + 14] = 0.225f;
    std::vector<float> sc, sh, tmp;
    for (int i = 0; i < LA_NL; ++i) {
        const int cin = la_cin(c, i), cout = la_cout(c, i), gcin = la_gcin(c, i), K = 9 * gcin;
        const float* w = T(std::string(LA_CONV[i]) + ".weight");
        bn_fold_f32(t + names.find(std::string(LA_BN[i]) + ".weight"), cout, sc, sh);  // (the four tensors follow each other)
        if (c.conv_bias) {
            const float* b = T(std::string(LA_CONV[i]) + ".bias");
            for (int co = 0; co < cout; ++co) sh[co] = b[co] * sc[co] + sh[co];
        }
        if (i == 0) {
            for (int co = 0; co < cout; ++co)
                for (int ci = 0; ci < 3; ++ci)
                    for (int k = 0; k < 9; ++k) packed[l.w0 + ((size_t)k * 3 + ci) * cout + co] = w[((size_t)co * 3 + ci) * 9 + k] * sc[co];
            memcpy(packed + l.b0, sh.data(), cout * sizeof(float));
        }
        tmp.assign((size_t)cout * K, 0.0f);
        pack_conv_gemm(w, cout, cin, 3, gcin, tmp.data());
        for (int co = 0; co < cout; ++co)
            for (int k = 0; k < K; ++k) tmp[(size_t)co * K + k] *= sc[co];
        memcpy(packed + l.g[i].w, tmp.data(), (size_t)cout * K * sizeof(float));
        memcpy(packed + l.g[i].b, sh.data(), cout * sizeof(float));
        l.g[i].split_planes(packed, cout, K);
    }
    const float *ws = T("convDb.weight"), *wp = T("convPb.weight");
    for (int k = 0; k < 9; ++k)
        for (int ci = 0; ci < LA_DIM; ++ci) {
            for (int co = 0; co < 4; ++co) packed[l.tws + ((size_t)k * LA_DIM + ci) * 4 + co] = ws[((size_t)co * LA_DIM + ci) * 9 + k];
            for (int co = 0; co < 2; ++co) packed[l.twp + ((size_t)k * LA_DIM + ci) * 2 + co] = wp[((size_t)co * LA_DIM + ci) * 9 + k];
        }
    memcpy(packed + l.tb, T("convDb.bias"), 4 * sizeof(float));
    memcpy(packed + l.tb + 4, T("convPb.bias"), 2 * sizeof(float));
    for (int v = 0; v < 2; ++v) {
        const std::string n = v == 0 ? "des_conv2" : "des_conv3", b = v == 0 ? "des_bn2" : "des_bn3";
        const int C = c.c[2 + v], k = c.k[v], K = k * k * C;
        sc.assign(LA_DIM, 1.0f);
        sh.assign(LA_DIM, 0.0f);
        if (c.bn[v]) bn_fold_f32(t + names.find(b + ".weight"), LA_DIM, sc, sh);
        if (c.bias[v]) {
            const float* bb = T(n + ".bias");
            for (int co = 0; co < LA_DIM; ++co) sh[co] = bb[co] * sc[co] + sh[co];
        }
        tmp.assign((size_t)LA_DIM * K, 0.0f);
        pack_conv_gemm(T(n + ".weight"), LA_DIM, C, k, C, tmp.data());
        for (int co = 0; co < LA_DIM; ++co)
            for (int q = 0; q < K; ++q) {
                tmp[(size_t)co * K + q] *= sc[co];
                packed[l.dw[v] + (size_t)q * LA_DIM + co] = tmp[(size_t)co * K + q];
            }
        memcpy(packed + l.dg[v].w, tmp.data(), (size_t)LA_DIM * K * sizeof(float));
        memcpy(packed + l.db[v], sh.data(), LA_DIM * sizeof(float));
        memcpy(packed + l.dg[v].b, sh.data(), LA_DIM * sizeof(float));
        l.dg[v].split_planes(packed, LA_DIM, K);
    }
    return IMCUI_OK;
}

namespace {

// tvf.Normalize: (x - mean) / std, one rounding each; ms = {mean, std} in the packed header
__device__ __forceinline__ float la_norm(float x, const float* __restrict__ ms) { return __fdiv_rn(__fsub_rn(x, ms[0]), ms[1]); }

struct LaStemLoad {
    const float* ms;
    __device__ float operator()(const float* __restrict__ img, long b, int c, int h, int w, int yy, int xx) const {
        return la_norm(img[((b * 3 + c) * h + yy) * (long)w + xx], ms);
    }
};

// planar image [B, 3, H, W] -> the normalised NHWC map [B, H, W, 32], channels 3.. zero (layer 0 on the implicit GEMM); one thread
// per float4
__global__ __launch_bounds__(256) void la_pad_kernel(const float* __restrict__ img, const float* __restrict__ ms, float* __restrict__ out, int h, int w, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int q = (int)(i & 7);
        const long p = i >> 3;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q == 0) {
            const long hw = (long)h * w, b = p / hw, r = p - b * hw;
            const float* s = img + b * 3 * hw + r;
            o.x = la_norm(s[0], ms);
            o.y = la_norm(s[hw], ms);
            o.z = la_norm(s[2 * hw], ms);
        }
        *reinterpret_cast<float4*>(out + i * 4) = o;
    }
}

// ------------------------------------------------------------------ decode of one cell
// v = the six head outputs (score head 0..3, location head 4..5) of cell (cx, cy).  aware = soft-max(v0, v1, v2); score = sigmoid(v3),
// times 0 on the first / last row and column; t = tanh(v4, v5); coord = (c * 8 + 3.5) + t * 7.0 in ONE float32 order (a product, a
// sum: this file is compiled without contraction), clamped to the image.
__device__ __forceinline__ void la_decode(const float* v, int cx, int cy, int Wc, int Hc, int W, int H, float* score, float* coord, float* tanhv, float* aware) {
    const float m = fmaxf(fmaxf(v[0], v[1]), v[2]);
    const float e0 = expf(v[0] - m), e1 = expf(v[1] - m), e2 = expf(v[2] - m);
    const float s = (e0 + e1) + e2;
    aware[0] = e0 / s;
    aware[1] = e1 / s;
    aware[2] = e2 / s;
    const bool border = cx == 0 || cy == 0 || cx == Wc - 1 || cy == Hc - 1;
    *score = __fmul_rn(sigmoidf_(v[3]), border ? 0.0f : 1.0f);
    const float tx = tanhf(v[4]), ty = tanhf(v[5]);
    tanhv[0] = tx;
    tanhv[1] = ty;
    const float bx = __fadd_rn(__fmul_rn((float)cx, 8.0f), 3.5f), by = __fadd_rn(__fmul_rn((float)cy, 8.0f), 3.5f);
    coord[0] = fminf(fmaxf(__fadd_rn(bx, __fmul_rn(tx, 7.0f)), 0.0f), (float)(W - 1));
    coord[1] = fminf(fmaxf(__fadd_rn(by, __fmul_rn(ty, 7.0f)), 0.0f), (float)(H - 1));
}

// One wave per cell: the 3x3 tails 256 -> 4 (on s1) and 256 -> 2 (on p1), zero padding.  Lane l owns channels 4 l .. 4 l + 3 and sums
// them over the taps in ascending (tap, channel) order; the 64 partial sums meet in wave_sum's fixed butterfly; + bias; la_decode.
__global__ __launch_bounds__(256) void la_tail_kernel(const float* __restrict__ s1, const float* __restrict__ p1, const float* __restrict__ tws,
                                                      const float* __restrict__ twp, const float* __restrict__ tb, int Hc, int Wc, int H, int W,
                                                      float* __restrict__ score, float* __restrict__ coord, float* __restrict__ tanhv,
                                                      float* __restrict__ aware, long total) {
    const int lane = threadIdx.x & 63;
    const long gp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gp >= total) return;  // (wave-uniform)
    const int np = Hc * Wc;
    const long b = gp / np;
    const int cell = (int)(gp - b * np), cy = cell / Wc, cx = cell - cy * Wc;
    float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = cy + ky - 1, xx = cx + kx - 1;
            if (yy < 0 || yy >= Hc || xx < 0 || xx >= Wc) continue;  // (uniform)
            const long o = ((b * Hc + yy) * (long)Wc + xx) * LA_DIM + 4 * lane;
            const float4 u = *reinterpret_cast<const float4*>(s1 + o), q = *reinterpret_cast<const float4*>(p1 + o);
            const float us[4] = {u.x, u.y, u.z, u.w}, qs[4] = {q.x, q.y, q.z, q.w};
            const int t = ky * 3 + kx;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 w4 = *reinterpret_cast<const float4*>(tws + ((long)t * LA_DIM + 4 * lane + j) * 4);
                const float2 w2 = *reinterpret_cast<const float2*>(twp + ((long)t * LA_DIM + 4 * lane + j) * 2);
                a[0] = fmaf(us[j], w4.x, a[0]);
                a[1] = fmaf(us[j], w4.y, a[1]);
                a[2] = fmaf(us[j], w4.z, a[2]);
                a[3] = fmaf(us[j], w4.w, a[3]);
                a[4] = fmaf(qs[j], w2.x, a[4]);
                a[5] = fmaf(qs[j], w2.y, a[5]);
            }
        }
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = wave_sum(a[j]) + tb[j];
    if (lane == 0) la_decode(a, cx, cy, Wc, Hc, W, H, score + gp, coord + 2 * gp, tanhv + 2 * gp, aware + 3 * gp);
}

// the decode alone on given head outputs raw [B, Hc Wc, 6]: one thread per cell (imcui_hip_lanet_select_probe)
__global__ __launch_bounds__(256) void la_decode_kernel(const float* __restrict__ raw, int Hc, int Wc, int H, int W, float* __restrict__ score,
                                                        float* __restrict__ coord, float* __restrict__ tanhv, float* __restrict__ aware, long total) {
    const long gp = (long)blockIdx.x * 256 + threadIdx.x;
    if (gp >= total) return;
    const int np = Hc * Wc, cell = (int)(gp % np), cy = cell / Wc, cx = cell - cy * Wc;
    float v[6];
    for (int j = 0; j < 6; ++j) v[j] = raw[gp * 6 + j];
    la_decode(v, cx, cy, Wc, Hc, W, H, score + gp, coord + 2 * gp, tanhv + 2 * gp, aware + 3 * gp);
}

// lanet.py:49-50: `score > keypoint_threshold`, strict
struct LaPred {
    float thr;
    __device__ void bind(int) {}
    __device__ bool operator()(const float* img, int idx) const { return img[idx] > thr; }
};

// The rows of ranked_rows_kernel (ascending (score, cell) order: lanet.py:54 with equal scores in cell order), one thread each:
// key-point, score and the cell's level weights (kaw, for the descriptor kernel).  Rows past the count are zero.
struct LaRow {
    const int* cidx;
    const float *coord, *aware;
    int np, kout;
    float *kpts, *scores, *kaw;
    __device__ void clear(int b, int lo, int hi) const {
        const int i = lo + threadIdx.x;
        if (i >= hi) return;
        float* kp = kpts + (long)b * kout * 2;
        float* ka = kaw + (long)b * kout * 3;
        kp[2 * i] = kp[2 * i + 1] = scores[(long)b * kout + i] = 0.0f;
        ka[3 * i] = ka[3 * i + 1] = ka[3 * i + 2] = 0.0f;
    }
    __device__ void emit(int b, int i0, int m, const int* ks, const int* rank, const float* cs) const {
        const int j = threadIdx.x;
        if (j >= m) return;
        const int slot = ks[i0 + j], r = rank[j];
        const long cell = (long)b * np + cidx[(long)b * np + slot];
        float* kp = kpts + (long)b * kout * 2;
        float* ka = kaw + (long)b * kout * 3;
        kp[2 * r] = coord[2 * cell];
        kp[2 * r + 1] = coord[2 * cell + 1];
        scores[(long)b * kout + r] = cs[slot];
        ka[3 * r] = aware[3 * cell];
        ka[3 * r + 1] = aware[3 * cell + 1];
        ka[3 * r + 2] = aware[3 * cell + 2];
    }
};

// ------------------------------------------------------------------ the sparse level-aware descriptor head
// F.grid_sample(map [h, w], g) at its defaults (bilinear, zeros, align_corners=False) for the key-point at pixel position c of the
// H x W image: g = c / float32((size - 1) / 2) - 1, ATen's un-normalisation ((g + 1) * size - 1) / 2, corners nw, ne, sw, se with the
// weights (x1 - x)(y1 - y) ...; a corner outside the map gets weight 0.  wsum = the in-map weights summed in corner order.
struct LaCorners {
    int x0, y0;
    float w[4], wsum;
};
__device__ __forceinline__ LaCorners la_corners(float cx, float cy, int W, int H, int w, int h) {
    const float gx = __fsub_rn(__fdiv_rn(cx, __fmul_rn((float)(W - 1), 0.5f)), 1.0f), gy = __fsub_rn(__fdiv_rn(cy, __fmul_rn((float)(H - 1), 0.5f)), 1.0f);
    const float fx = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.0f), (float)w), 1.0f), 2.0f);
    const float fy = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.0f), (float)h), 1.0f), 2.0f);
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float wx1 = __fsub_rn(fx, x0f), wy1 = __fsub_rn(fy, y0f), wx0 = __fsub_rn(__fadd_rn(x0f, 1.0f), fx), wy0 = __fsub_rn(__fadd_rn(y0f, 1.0f), fy);
    LaCorners r;
    // (positions are clamped to the image, so the float -> int conversions are in range)
    r.x0 = (int)x0f;
    r.y0 = (int)y0f;
    const float ws[4] = {__fmul_rn(wx0, wy0), __fmul_rn(wx1, wy0), __fmul_rn(wx0, wy1), __fmul_rn(wx1, wy1)};
    r.wsum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xx = r.x0 + (j & 1), yy = r.y0 + (j >> 1);
        const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h;
        r.w[j] = in ? ws[j] : 0.0f;
        r.wsum = __fadd_rn(r.wsum, r.w[j]);
    }
    return r;
}

struct LaLevel {
    const float* x;   // [B, h, w, C]
    const float* wt;  // [k k C][256]
    const float* bias;
    int h, w, C, k;
};

// LA_KB = 32 key-points per workgroup step (grid-stride over the capacity: steps past the count only write the zero rows), 256 threads.
// Per level 2 / 3 and per (tap, 64- or 32-channel chunk): the blended inputs of the 32 key-points go to LDS (one wave per key-point,
// a lane per channel; corners in the order nw, ne, sw, se; a tap outside the map is the convolution's zero padding), then
// Y += S Wt[chunk] on v_mfma_f32_32x32x2_f32, wave w owning output columns 64 w .. 64 w + 63: one chain per chunk, channels ascending,
// the chunks added in ascending (tap, chunk) order.  + wsum bias, times the key-point's level weight; level 4 is gathered per output element; the sum goes through LDS
// to one wave per row, which divides by the norm (plain IEEE quotient, no epsilon).
//   coords [B, kcap, 2] pixels, aw [B, kcap, 3]; the count is nkpts[b] (or nprobe when nkpts is null)
__global__ __launch_bounds__(256) void la_desc_kernel(LaLevel L2, LaLevel L3, const float* __restrict__ x4, int h4, int w4, const float* __restrict__ coords,
                                                      const float* __restrict__ aw, const int* __restrict__ nkpts, int nprobe, int kcap, int H, int W,
                                                      float* __restrict__ desc) {
    constexpr int LDS_ = 65, LDG = LA_DIM + 1;
    __shared__ float S[LA_KB * LDS_];
    __shared__ float G[LA_KB * LDG];
    __shared__ int kx0[LA_KB], ky0[LA_KB];
    __shared__ float kw[LA_KB][4], kws[LA_KB], ka[LA_KB][3];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int nk = min(nkpts ? nkpts[b] : nprobe, kcap);
    for (int k0 = blockIdx.x * LA_KB; k0 < kcap; k0 += gridDim.x * LA_KB) {
        float* out = desc + ((long)b * kcap + k0) * LA_DIM;
        if (k0 >= nk) {  // rows past the count are zero (uniform)
            for (int e = tid; e < LA_KB * LA_DIM; e += 256)
                if (k0 + e / LA_DIM < kcap) out[e] = 0.0f;
            continue;
        }
        f32x16 fin[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) fin[0][r] = fin[1][r] = 0.0f;
        for (int lev = 0; lev < 3; ++lev) {
            const LaLevel L = lev == 0 ? L2 : L3;
            const int lh = lev == 2 ? h4 : L.h, lw = lev == 2 ? w4 : L.w;
            __syncthreads();  // (every wave is done with the level before)
            if (tid < LA_KB) {
                const int i = k0 + tid;
                LaCorners c;
                c.x0 = c.y0 = 0;
                c.w[0] = c.w[1] = c.w[2] = c.w[3] = c.wsum = 0.0f;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
                if (i < nk) {
                    const float* p = coords + ((long)b * kcap + i) * 2;
                    c = la_corners(p[0], p[1], W, H, lw, lh);
                    const float* q = aw + ((long)b * kcap + i) * 3;
                    a0 = q[0], a1 = q[1], a2 = q[2];
                }
                kx0[tid] = c.x0;
                ky0[tid] = c.y0;
                for (int j = 0; j < 4; ++j) kw[tid][j] = c.w[j];
                kws[tid] = c.wsum;
                ka[tid][0] = a0, ka[tid][1] = a1, ka[tid][2] = a2;
            }
            __syncthreads();
            if (lev == 2) {  // x4 itself: every lane gathers its 2 x 16 output elements
                const float* xb = x4 + (long)b * h4 * w4 * LA_DIM;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = frag_row(r, hi), col = 64 * wv + 32 * ct + lo;
                        float v = 0.0f;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float wj = kw[row][j];
                            if (wj != 0.0f) v = v + wj * xb[((long)(ky0[row] + (j >> 1)) * w4 + kx0[row] + (j & 1)) * LA_DIM + col];
                        }
                        fin[ct][r] = fin[ct][r] + ka[row][2] * v;
                    }
                continue;
            }
            const int C = L.C, k = L.k, pad = k >> 1, CH = (C & 63) ? 32 : 64;
            const float* xb = L.x + (long)b * L.h * L.w * C;
            f32x16 g[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) g[0][r] = g[1][r] = 0.0f;
            for (int tap = 0; tap < k * k; ++tap) {
                const int dy = tap / k - pad, dx = tap % k - pad;
                for (int c0 = 0; c0 < C; c0 += CH) {
                    __syncthreads();  // (every wave is done with S of the chunk before)
                    if (lane < CH)
#pragma unroll
                        for (int q = 0; q < LA_KB / 4; ++q) {
                            const int kp = wv + 4 * q;
                            float v = 0.0f;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const float wj = kw[kp][j];
                                const int yy = ky0[kp] + (j >> 1) + dy, xx = kx0[kp] + (j & 1) + dx;
                                if (wj != 0.0f && yy >= 0 && yy < L.h && xx >= 0 && xx < L.w) v = v + wj * xb[((long)yy * L.w + xx) * C + c0 + lane];
                            }
                            S[kp * LDS_ + lane] = v;
                        }
                    __syncthreads();
                    const float* wrow = L.wt + ((long)tap * C + c0) * LA_DIM + 64 * wv + lo;
                    f32x16 gc[2];  // the chunk's own chain; the chunks are added in ascending order (two levels: K up to 4608 at float32 grade)
#pragma unroll
                    for (int r = 0; r < 16; ++r) gc[0][r] = gc[1][r] = 0.0f;
                    for (int kk = 0; kk < CH; kk += 2) {
                        const float a = S[lo * LDS_ + kk + hi];
                        gc[0] = mfma32(a, wrow[(long)(kk + hi) * LA_DIM], gc[0]);
                        gc[1] = mfma32(a, wrow[(long)(kk + hi) * LA_DIM + 32], gc[1]);
                    }
                    g[0] += gc[0];
                    g[1] += gc[1];
                }
            }
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const float bs = L.bias[64 * wv + 32 * ct + lo];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = frag_row(r, hi);
                    fin[ct][r] = fin[ct][r] + ka[row][lev] * (g[ct][r] + kws[row] * bs);
                }
            }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) G[frag_row(r, hi) * LDG + 64 * wv + 32 * ct + lo] = fin[ct][r];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < LA_KB / 4; ++q) {  // d / |d|: one wave per row, the squares summed per lane in channel order, then the butterfly
            const int kp = wv + 4 * q;
            if (k0 + kp >= kcap) continue;
            float v[4], ss = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = G[kp * LDG + lane + 64 * j];
                ss = ss + v[j] * v[j];
            }
            const float nrm = sqrtf(wave_sum(ss));
#pragma unroll
            for (int j = 0; j < 4; ++j) out[(long)kp * LA_DIM + lane + 64 * j] = k0 + kp < nk ? __fdiv_rn(v[j], nrm) : 0.0f;
        }
    }
}

}  // namespace

// ------------------------------------------------------------------ host: launches
static void la_pool(const float* src, float* dst, int B, int hi, int wi, int C, hipStream_t stream) {
    const long n4 = (long)B * (hi / 2) * (wi / 2) * (C / 4);
    hipLaunchKernelGGL(pool2x2_kernel<0>, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, src, dst, hi, wi, hi / 2, wi / 2, C, n4);
}
// a k x k convolution (pad k / 2) of the NHWC map `in` [B, hh, ww, cin] as an implicit GEMM: folded bias, activation `act`
static int la_conv(imcui_hip_t* h, const float* P, const GemmLayerOff& o, const float* in, float* out, int B, int hh, int ww, int cin, int cout, int k, int act,
                   hipStream_t stream) {
    GemmP g;
    g.epi = EPI_CONV;
    g.A = in;
    gemm_set_weights(g, P, o, cout, k * k * cin, h->precision == 1);
    gemm_set_conv(g, k, 1, k / 2, hh, ww, hh, ww, cin);
    g.M = B * hh * ww;
    g.C = out;
    g.ldc = cout;
    g.act = act;
    return gemm_launch(h, g, stream);
}
// layer 0 on the planar image -> out [B, H, W, c1]; scratch [B, H, W, 32] is used by the GEMM route only
static int la_stem(imcui_hip_t* h, const LaCfg& c, const LaLayout& l, const float* P, const float* img, int B, int H, int W, float* out, float* scratch,
                   hipStream_t stream) {
    const long npix = (long)B * H * W;
    const float* ms = P + l.hdr + 13;
    if (la_stem_valu(c)) {
        if (c.c[1] == 32)
            hipLaunchKernelGGL((stem3x3_kernel<32, LaStemLoad>), dim3(blocks_256(npix)), dim3(256), 0, stream, img, P + l.w0, P + l.b0, out, H, W, LaStemLoad{ms}, npix);
        else
            hipLaunchKernelGGL((stem3x3_kernel<64, LaStemLoad>), dim3(blocks_256(npix)), dim3(256), 0, stream, img, P + l.w0, P + l.b0, out, H, W, LaStemLoad{ms}, npix);
        IMCUI_CHECK_LAUNCH(h);
        return IMCUI_OK;
    }
    hipLaunchKernelGGL(la_pad_kernel, dim3(grid_stride_blocks(npix * 8)), dim3(256), 0, stream, img, ms, scratch, H, W, npix * 8);
    IMCUI_CHECK_LAUNCH(h);
    return la_conv(h, P, l.g[0], scratch, out, B, H, W, 32, c.c[1], 3, c.act, stream);
}

struct LaWs {
    float *fa, *fb, *x2, *x3, *x4, *s1, *p1, *score, *coord, *tanhv, *aware, *kaw;
    CandScan scan;
    ScoreIndexList cand;  // (holds every cell)
    CutList cut;
    int* status;
    size_t total;
    bool ok;
};
// trunk: the maps are carved (the forward); otherwise only the cell arrays and the lists (the select probe)
static LaWs la_carve(void* ws, size_t bytes, const LaCfg* c, int B, int H, int W, int Hc, int Wc, int kout) {
    WsAlloc a(ws, bytes);
    LaWs s;
    memset(&s, 0, sizeof s);
    const size_t np = (size_t)Hc * Wc;
    if (c) {
        const size_t p1 = (size_t)H * W, p2 = (size_t)(H / 2) * (W / 2), p3 = (size_t)(H / 4) * (W / 4);
        size_t m = p1 * c->c[1];
        m = std::max(m, p2 * c->c[2]);
        m = std::max(m, p3 * c->c[3]);
        m = std::max(m, np * c->c[4]);
        s.fa = a.get<float>(B * m);
        s.fb = a.get<float>(B * m);
        s.x2 = a.get<float>(B * p2 * c->c[2]);
        s.x3 = a.get<float>(B * p3 * c->c[3]);
        s.x4 = a.get<float>(B * np * c->c[4]);
        s.s1 = a.get<float>(B * np * LA_DIM);
        s.p1 = a.get<float>(B * np * LA_DIM);
    }
    s.score = a.get<float>(B * np);
    s.coord = a.get<float>(B * np * 2);
    s.tanhv = a.get<float>(B * np * 2);
    s.aware = a.get<float>(B * np * 3);
    s.scan.carve(a, B, np);
    s.cand.carve(a, B, (int)np);
    s.cut.carve(a, B, (int)np);
    s.kaw = a.get<float>((size_t)B * kout * 3);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

static int la_check(imcui_hip_t* h, const LaCfg& c, int B, int H, int W) {
    if (B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet: B=%d above 1024", B);
    if (H < 8 || W < 8) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet: H=%d W=%d: every side needs at least 8 pixels (one cell)", H, W);
    // int indices: the floats of the largest map of the batch (the 32-channel padded image of the GEMM route included)
    long m = (long)H * W * std::max(c.c[1], 32);
    m = std::max(m, (long)(H / 2) * (W / 2) * c.c[2]);
    m = std::max(m, (long)(H / 4) * (W / 4) * c.c[3]);
    m = std::max(m, (long)(H / 8) * (W / 8) * LA_DIM);
    if (m > 0x7fffffffL / B) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet: B=%d images of %dx%d exceed the 2^31 index range of one call", B, H, W);
    return IMCUI_OK;
}
// kout rows per image: every key-point the cut can leave must fit
static int la_check_k(imcui_hip_t* h, int np, int max_keypoints, int kout) {
    if (max_keypoints < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet: max_keypoints=%d is negative (0 keeps every key-point)", max_keypoints);
    const int need = max_keypoints > 0 ? std::min(max_keypoints, np) : np;
    if (kout < need || kout < 1) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet: kout=%d below min(max_keypoints or all, %d cells) = %d", kout, np, need);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_lanet_workspace_bytes(const int* cfg, int B, int H, int W, int kout) {
    LaCfg c;
    if (!la_cfg(cfg, &c) || B <= 0 || H < 8 || W < 8 || kout <= 0) return 0;
    return la_carve(nullptr, 0, &c, B, H, W, H / 8, W / 8, kout).total;
}
extern "C" size_t imcui_hip_lanet_select_workspace_bytes(int B, int Hc, int Wc, int kout) {
    if (B <= 0 || Hc <= 0 || Wc <= 0 || kout <= 0) return 0;
    return la_carve(nullptr, 0, nullptr, B, 0, 0, Hc, Wc, kout).total;
}

// threshold compaction in cell order, the cut, the ranked rows
static int la_select(imcui_hip_t* h, const LaWs& s, int B, int np, float threshold, int max_keypoints, int kout, float* keypoints, float* scores,
                     int* num_keypoints, int* st, hipStream_t stream) {
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, st, 1);
    cand_list(stream, s.score, np, B, LaPred{threshold}, s.scan, np, s.cand.emit());
    cand_cut(stream, s.cand.cscore, s.scan.total, np, max_keypoints, s.cut, st, B);
    ranked_rows(stream, s.cand.cscore, np, s.cut, kout, num_keypoints, LaRow{s.cand.cidx, s.coord, s.aware, np, kout, keypoints, scores, s.kaw}, B);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

static void la_desc(const LaCfg& c, const LaLayout& l, const float* P, const float* x2, int h2, int w2, const float* x3, int h3, int w3, const float* x4, int h4,
                    int w4, const float* coords, const float* aw, const int* nkpts, int nprobe, int kcap, int B, int H, int W, float* desc, hipStream_t stream) {
    const LaLevel L2{x2, P + l.dw[0], P + l.db[0], h2, w2, c.c[2], c.k[0]}, L3{x3, P + l.dw[1], P + l.db[1], h3, w3, c.c[3], c.k[1]};
    hipLaunchKernelGGL(la_desc_kernel, dim3(std::min(cdiv(kcap, LA_KB), 1024), B), dim3(256), 0, stream, L2, L3, x4, h4, w4, coords, aw, nkpts, nprobe, kcap, H, W,
                       desc);
}

extern "C" int imcui_hip_lanet_forward(imcui_hip_t* h, const int* cfg, const float* packed, const float* image, int B, int H, int W, float threshold,
                                       int max_keypoints, int kout, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status,
                                       float* dbg_x2, float* dbg_x3, float* dbg_x4, float* dbg_score, float* dbg_coord, float* dbg_aware, float* dbg_tanh, void* ws,
                                       size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    LaCfg c;
    if (!la_cfg(cfg, &c))
        return imcui_set_err(h, IMCUI_ERR_ARG, "lanet: configuration refused (widths multiples of 32 with c4 = 256, k of the level convolutions 1 or 3, activation 1 or 2)");
    int rc;
    IMCUI_RUN(la_check(h, c, B, H, W));
    const int Hc = H / 8, Wc = W / 8, np = Hc * Wc;
    IMCUI_RUN(la_check_k(h, np, max_keypoints, kout));
    if (!packed || !image || !keypoints || !scores || !descriptors || !num_keypoints) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet: null argument");
    const LaLayout l = la_layout(c);
    LaWs s = la_carve(ws, ws_bytes, &c, B, H, W, Hc, Wc, kout);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "lanet: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const float* P = packed;
    // ---- trunk
    IMCUI_RUN(la_stem(h, c, l, P, image, B, H, W, s.fa, s.fb, stream));
    float *cur = s.fa, *oth = s.fb;
    float* keep[5] = {nullptr, nullptr, s.x2, s.x3, s.x4};
    int hh = H, ww = W;
    for (int i = 1; i < 8; ++i) {
        const int blk = i / 2 + 1;  // conv{blk}a / conv{blk}b
        float* dst = ((i & 1) && keep[blk]) ? keep[blk] : oth;
        IMCUI_RUN(la_conv(h, P, l.g[i], cur, dst, B, hh, ww, la_cin(c, i), la_cout(c, i), 3, c.act, stream));
        if (dst == oth) std::swap(cur, oth);
        if ((i & 1) && blk < 4) {  // the flooring 2x2 max-pool behind conv1b, conv2b, conv3b
            la_pool(dst, dst == cur ? oth : cur, B, hh, ww, la_cout(c, i), stream);
            IMCUI_CHECK_LAUNCH(h);
            if (dst == cur) std::swap(cur, oth);
            hh /= 2;
            ww /= 2;
        }
    }
    // ---- the heads' hidden layers, the tails and the decode
    IMCUI_RUN(la_conv(h, P, l.g[8], s.x4, s.s1, B, Hc, Wc, LA_DIM, LA_DIM, 3, c.act, stream));
    IMCUI_RUN(la_conv(h, P, l.g[9], s.x4, s.p1, B, Hc, Wc, LA_DIM, LA_DIM, 3, c.act, stream));
    const long ncell = (long)B * np;
    hipLaunchKernelGGL(la_tail_kernel, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, stream, s.s1, s.p1, P + l.tws, P + l.twp, P + l.tb, Hc, Wc, H, W, s.score,
                       s.coord, s.tanhv, s.aware, ncell);
    IMCUI_CHECK_LAUNCH(h);
    copy_if(dbg_x2, s.x2, (size_t)B * (H / 2) * (W / 2) * c.c[2] * sizeof(float), stream);
    copy_if(dbg_x3, s.x3, (size_t)B * (H / 4) * (W / 4) * c.c[3] * sizeof(float), stream);
    copy_if(dbg_x4, s.x4, (size_t)ncell * LA_DIM * sizeof(float), stream);
    copy_if(dbg_score, s.score, ncell * sizeof(float), stream);
    copy_if(dbg_coord, s.coord, ncell * 2 * sizeof(float), stream);
    copy_if(dbg_aware, s.aware, ncell * 3 * sizeof(float), stream);
    copy_if(dbg_tanh, s.tanhv, ncell * 2 * sizeof(float), stream);
    // ---- selection and descriptors
    IMCUI_RUN(la_select(h, s, B, np, threshold, max_keypoints, kout, keypoints, scores, num_keypoints, status ? status : s.status, stream));
    la_desc(c, l, P, s.x2, H / 2, W / 2, s.x3, H / 4, W / 4, s.x4, Hc, Wc, keypoints, s.kaw, num_keypoints, 0, kout, B, H, W, descriptors, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ test entries
// layer 0 alone: image [B, 3, H, W] -> out [B, H, W, c1]; scratch [B, H, W, 32] floats (read by the GEMM route only, may be null on the
// VALU route)
extern "C" int imcui_hip_lanet_stem_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* image, int B, int H, int W, float* out, float* scratch,
                                          void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    LaCfg c;
    if (!la_cfg(cfg, &c)) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet stem probe: configuration refused");
    if (B < 1 || H < 1 || W < 1 || (long)B * H * W > 0x7fffffffL / 512 || !packed || !image || !out || (!la_stem_valu(c) && !scratch))
        return imcui_set_err(h, IMCUI_ERR_ARG, "lanet stem probe: shape or null argument");
    return la_stem(h, c, la_layout(c), packed, image, B, H, W, out, scratch, (hipStream_t)stream_);
}

// the tails and the decode on given hidden maps s1 / p1 [B, Hc, Wc, 256] of an H x W image -> score [B, Hc Wc], coord and tanh
// [B, Hc Wc, 2], aware [B, Hc Wc, 3]
extern "C" int imcui_hip_lanet_tail_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* s1, const float* p1, int B, int Hc, int Wc, int H, int W,
                                          float* score, float* coord, float* tanhv, float* aware, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    LaCfg c;
    if (!la_cfg(cfg, &c)) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet tail probe: configuration refused");
    if (B < 1 || Hc < 1 || Wc < 1 || H / 8 != Hc || W / 8 != Wc || (long)B * Hc * Wc > 0x7fffffffL / 512 || !packed || !s1 || !p1 || !score || !coord || !tanhv || !aware)
        return imcui_set_err(h, IMCUI_ERR_ARG, "lanet tail probe: shape (Hc = H / 8, Wc = W / 8) or null argument");
    const LaLayout l = la_layout(c);
    const long ncell = (long)B * Hc * Wc;
    hipLaunchKernelGGL(la_tail_kernel, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, s1, p1, packed + l.tws, packed + l.twp, packed + l.tb,
                       Hc, Wc, H, W, score, coord, tanhv, aware, ncell);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// decode and selection from crafted head outputs raw [B, Hc Wc, 6] (score head 0..3, location head 4..5) of an H x W image
extern "C" int imcui_hip_lanet_select_probe(imcui_hip_t* h, const float* raw, int B, int Hc, int Wc, int H, int W, float threshold, int max_keypoints, int kout,
                                            float* keypoints, float* scores, int* num_keypoints, int* status, float* dbg_score, float* dbg_coord, float* dbg_aware,
                                            float* dbg_tanh, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (B > 1024 || Hc < 1 || Wc < 1 || H / 8 != Hc || W / 8 != Wc || (long)B * Hc * Wc > 0x7fffffffL / 8 || !raw || !keypoints || !scores || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "lanet select probe: shape (Hc = H / 8, Wc = W / 8) or null argument");
    const int np = Hc * Wc;
    int rc;
    IMCUI_RUN(la_check_k(h, np, max_keypoints, kout));
    LaWs s = la_carve(ws, ws_bytes, nullptr, B, 0, 0, Hc, Wc, kout);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "lanet select probe: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const long ncell = (long)B * np;
    hipLaunchKernelGGL(la_decode_kernel, dim3(blocks_256(ncell)), dim3(256), 0, stream, raw, Hc, Wc, H, W, s.score, s.coord, s.tanhv, s.aware, ncell);
    IMCUI_CHECK_LAUNCH(h);
    copy_if(dbg_score, s.score, ncell * sizeof(float), stream);
    copy_if(dbg_coord, s.coord, ncell * 2 * sizeof(float), stream);
    copy_if(dbg_aware, s.aware, ncell * 3 * sizeof(float), stream);
    copy_if(dbg_tanh, s.tanhv, ncell * 2 * sizeof(float), stream);
    return la_select(h, s, B, np, threshold, max_keypoints, kout, keypoints, scores, num_keypoints, status ? status : s.status, stream);
}

static int la_levels_check(imcui_hip_t* h, const char* who, const LaCfg& c, int h2, int w2, int h3, int w3) {
    if (h2 < 1 || w2 < 1 || h3 < 1 || w3 < 1 || (long)h2 * w2 * c.c[2] > 0x7fffffffL / 4 || (long)h3 * w3 * c.c[3] > 0x7fffffffL / 4)
        return imcui_set_err(h, IMCUI_ERR_ARG, "%s: map shapes %dx%d, %dx%d", who, h2, w2, h3, w3);
    return IMCUI_OK;
}

// the sparse head at n given positions coords [n, 2] (pixels of the H x W image) with the level weights aw [n, 3] of ONE image, from
// given maps x2 [h2, w2, c2], x3 [h3, w3, c3], x4 [h4, w4, 256] -> descriptors [n, 256]
extern "C" int imcui_hip_lanet_desc_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* x2, int h2, int w2, const float* x3, int h3, int w3,
                                          const float* x4, int h4, int w4, int H, int W, const float* coords, const float* aw, int n, float* descriptors,
                                          void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    LaCfg c;
    if (!la_cfg(cfg, &c)) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet desc probe: configuration refused");
    int rc;
    IMCUI_RUN(la_levels_check(h, "lanet desc probe", c, h2, w2, h3, w3));
    if (h4 < 1 || w4 < 1 || H < 2 || W < 2 || n < 1 || !packed || !x2 || !x3 || !x4 || !coords || !aw || !descriptors)
        return imcui_set_err(h, IMCUI_ERR_ARG, "lanet desc probe: shape, n < 1 or null argument");
    la_desc(c, la_layout(c), packed, x2, h2, w2, x3, h3, w3, x4, h4, w4, coords, aw, nullptr, n, n, 1, H, W, descriptors, (hipStream_t)stream_);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// the dense form the forward never runs: d2 = des_conv2(x2) [B, h2, w2, 256], d3 = des_conv3(x3) [B, h3, w3, 256] on the shared GEMM
extern "C" int imcui_hip_lanet_dense_levels(imcui_hip_t* h, const int* cfg, const float* packed, const float* x2, int B, int h2, int w2, const float* x3, int h3,
                                            int w3, float* d2, float* d3, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    LaCfg c;
    if (!la_cfg(cfg, &c)) return imcui_set_err(h, IMCUI_ERR_ARG, "lanet dense levels: configuration refused");
    int rc;
    IMCUI_RUN(la_levels_check(h, "lanet dense levels", c, h2, w2, h3, w3));
    if (B < 1 || B > 1024 || (long)B * h2 * w2 > 0x7fffffffL / 512 || (long)B * h3 * w3 > 0x7fffffffL / 512 || !packed || !x2 || !x3 || !d2 || !d3)
        return imcui_set_err(h, IMCUI_ERR_ARG, "lanet dense levels: B or null argument");
    const LaLayout l = la_layout(c);
    IMCUI_RUN(la_conv(h, packed, l.dg[0], x2, d2, B, h2, w2, c.c[2], LA_DIM, c.k[0], 0, (hipStream_t)stream_));
    return la_conv(h, packed, l.dg[1], x3, d3, B, h3, w3, c.c[3], LA_DIM, c.k[1], 0, (hipStream_t)stream_);
}
