// What SuperGlue (superglue.hip) and IMP (imp.hip) share: the attentional-GNN trunk of upstream SuperGlue -- packed-weight layout,
// state-dict tensor table, host packer, trunk workspace, the launches from the key-point encoder to the similarity matrix -- and the
// arg-max / mutual-check stage after either network's Sinkhorn.  IMP adds input_proj (128 -> 256) and reads one of nine final
// projections; everything else about the trunk is the same network.
// Device code, host packing and launch helpers; included by both files, each translation unit compiles its own copy with its own
// flags (imp.hip: -ffp-contract=off, so glue_kenc0 rounds after every operation there and contracts in superglue.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "attention.h"
#include "ffn.h"
#include "gemm.h"
#include "imcui_hip.h"

namespace {  // internal linkage: two translation units include this code

#define GLUE_LAYERS 18
#define GLUE_HEADS 4
#define GLUE_DESC_IN 128  // input_proj input width
#define GLUE_BN_EPS 1e-5  // nn.BatchNorm1d default

// ------------------------------------------------------------------ packed weights
struct GlueSplit {
    size_t h, l, s;  // f16 hi / lo planes (float offsets) and the 2^-e scale
};
struct GlueLayerOff {
    size_t wqkv, bqkv, w1, b1, w2, b2;
    GlueSplit sqkv, s1, s2, s2p;  // s2p: mlp.3 planes in the fused FFN kernel's K order
};
struct GlueLayout {
    bool input_proj;
    size_t k0;            // [32][4]: wx, wy, wscore, bias of the first key-point encoder layer (BN folded)
    size_t kw[4], kb[4];  // encoder layers 1..4: 32->64, 64->128, 128->256 (BN folded), 256->256
    GlueSplit ks[4];
    size_t win, bin_;  // input_proj (taken only when the network has one)
    GlueSplit sin_;
    GlueLayerOff L[GLUE_LAYERS];
    size_t wfinal, bfinal, bin;
    GlueSplit sfinal;
    size_t total;
};
const int GLUE_KENC[6] = {3, 32, 64, 128, 256, 256};

GlueLayout glue_layout(bool input_proj) {
    GlueLayout l;
    l.input_proj = input_proj;
    size_t off = 0;
    auto take = [&](size_t n) {
        size_t r = off;
        off += align_up(n, 64);
        return r;
    };
    auto take_split = [&](size_t n) {
        GlueSplit sp;
        sp.h = take(n / 2);
        sp.l = take(n / 2);
        sp.s = take(64);
        return sp;
    };
    l.k0 = take(32 * 4);
    for (int i = 0; i < 4; ++i) {
        l.kw[i] = take((size_t)GLUE_KENC[i + 2] * GLUE_KENC[i + 1]);
        l.kb[i] = take(GLUE_KENC[i + 2]);
    }
    l.win = input_proj ? take(256 * GLUE_DESC_IN) : 0;
    l.bin_ = input_proj ? take(256) : 0;
    for (int i = 0; i < GLUE_LAYERS; ++i) {
        GlueLayerOff& o = l.L[i];
        o.wqkv = take(768 * 256);
        o.bqkv = take(768);
        o.w1 = take(512 * 512);
        o.b1 = take(512);
        o.w2 = take(256 * 512);
        o.b2 = take(256);
    }
    l.wfinal = take(256 * 256);
    l.bfinal = take(256);
    l.bin = take(64);
    for (int i = 0; i < 4; ++i) l.ks[i] = take_split((size_t)GLUE_KENC[i + 2] * GLUE_KENC[i + 1]);
    l.sin_ = input_proj ? take_split(256 * GLUE_DESC_IN) : GlueSplit{0, 0, 0};
    for (int i = 0; i < GLUE_LAYERS; ++i) {
        GlueLayerOff& o = l.L[i];
        o.sqkv = take_split(768 * 256);
        o.s1 = take_split(512 * 512);
        o.s2 = take_split(256 * 512);
        o.s2p = take_split(256 * 512);
    }
    l.sfinal = take_split(256 * 256);
    l.total = off;
    return l;
}

// ------------------------------------------------------------------ the tensor table (names and shapes of the state dict)
// Order of the host-side packer = upstream state-dict keys:
//   kenc.encoder.{0,3,6,9,12}.{weight,bias}, kenc.encoder.{1,4,7,10}.{weight,bias,running_mean,running_var},
//   [input_proj.{weight,bias}], gnn.layers.i.<GLUE_LAYER_KEYS[j]>, the final projection(s), bin_score
struct GlueTensor {
    char name[64];
    int nd, d[3];
};
enum { GLUE_T_CONV = 0, GLUE_T_BN = 10, GLUE_T_INPROJ = 26, GLUE_T_PER_LAYER = 16 };
const struct {
    const char* key;
    int nd, d0, d1;
} GLUE_LAYER_KEYS[GLUE_T_PER_LAYER] = {
    {"attn.proj.0.weight", 3, 256, 256}, {"attn.proj.0.bias", 1, 256, 0},  {"attn.proj.1.weight", 3, 256, 256}, {"attn.proj.1.bias", 1, 256, 0},
    {"attn.proj.2.weight", 3, 256, 256}, {"attn.proj.2.bias", 1, 256, 0},  {"attn.merge.weight", 3, 256, 256},  {"attn.merge.bias", 1, 256, 0},
    {"mlp.0.weight", 3, 512, 512},       {"mlp.0.bias", 1, 512, 0},        {"mlp.1.weight", 1, 512, 0},         {"mlp.1.bias", 1, 512, 0},
    {"mlp.1.running_mean", 1, 512, 0},   {"mlp.1.running_var", 1, 512, 0}, {"mlp.3.weight", 3, 256, 512},       {"mlp.3.bias", 1, 256, 0},
};
const char* const GLUE_BN_FIELDS[4] = {"weight", "bias", "running_mean", "running_var"};
// table index of the first layer tensor, of the first final projection and of bin_score (the last entry)
constexpr int glue_t_layer0(bool input_proj) { return GLUE_T_INPROJ + (input_proj ? 2 : 0); }
constexpr int glue_t_final(bool input_proj) { return glue_t_layer0(input_proj) + GLUE_T_PER_LAYER * GLUE_LAYERS; }
constexpr int glue_t_bin(bool input_proj, int nfinal) { return glue_t_final(input_proj) + 2 * nfinal; }

// nfinal == 1: the one projection is `final_proj`; otherwise `final_proj.0` .. `final_proj.<nfinal - 1>`
std::vector<GlueTensor> glue_table(bool input_proj, int nfinal) {
    std::vector<GlueTensor> t;
#define add(nd_, d0_, d1_, ...)                                                              \
    do {                                                                                     \
        GlueTensor e;                                                                        \
        snprintf(e.name, sizeof e.name, __VA_ARGS__);                                        \
        e.nd = (nd_), e.d[0] = (d0_), e.d[1] = (d1_), e.d[2] = 1; /* Conv1d: [out, in, 1] */ \
        t.push_back(e);                                                                      \
    } while (0)
    for (int i = 0; i < 5; ++i) {  // convolutions of the key-point encoder
        add(3, GLUE_KENC[i + 1], GLUE_KENC[i], "kenc.encoder.%d.weight", 3 * i);
        add(1, GLUE_KENC[i + 1], 0, "kenc.encoder.%d.bias", 3 * i);
    }
    for (int i = 0; i < 4; ++i)  // its BatchNorms
        for (int f = 0; f < 4; ++f) add(1, GLUE_KENC[i + 1], 0, "kenc.encoder.%d.%s", 3 * i + 1, GLUE_BN_FIELDS[f]);
    if (input_proj) {
        add(3, 256, GLUE_DESC_IN, "input_proj.weight");
        add(1, 256, 0, "input_proj.bias");
    }
    for (int i = 0; i < GLUE_LAYERS; ++i)
        for (int j = 0; j < GLUE_T_PER_LAYER; ++j)
            add(GLUE_LAYER_KEYS[j].nd, GLUE_LAYER_KEYS[j].d0, GLUE_LAYER_KEYS[j].d1, "gnn.layers.%d.%s", i, GLUE_LAYER_KEYS[j].key);
    for (int k = 0; k < nfinal; ++k) {
        char idx[16] = "";
        if (nfinal > 1) snprintf(idx, sizeof idx, ".%d", k);
        add(3, 256, 256, "final_proj%s.weight", idx);
        add(1, 256, 0, "final_proj%s.bias", idx);
    }
    add(0, 1, 0, "bin_score");  // a scalar parameter
#undef add
    return t;
}

// ------------------------------------------------------------------ host-side packing
// Everything that is affine at inference time is folded in double here:
//   BatchNorm (eval):  y = (x - mean) * gamma / sqrt(var + eps) + beta  ->  scale and shift of the preceding conv
//   attn.merge:        mlp.0(cat[x, Wm ctx + bm]) = cat[x, ctx] [W0a | W0b Wm]^T + (b0 + W0b bm)
// Heads: upstream views the 256 projection channels as (64, 4): channel = d * 4 + head.  The packed q / k / v rows and
// the merge input columns are re-ordered to head * 64 + d, the head-major layout of the attention kernel.
// kenc_conv: the 10 encoder conv tensors, kenc_bn: its 16 BatchNorm tensors, inproj: {weight, bias} or null,
// layer0: the 16 * GLUE_LAYERS layer tensors, final_wb: {weight, bias} of the projection that inference reads.
void glue_pack(const GlueLayout& l, const float* const* kenc_conv, const float* const* kenc_bn, const float* const* inproj,
               const float* const* layer0, const float* const* final_wb, const float* bin, float* packed) {
    memset(packed, 0, l.total * sizeof(float));
    // ---- key-point encoder
    for (int i = 0; i < 5; ++i) {
        const int cin = GLUE_KENC[i], cout = GLUE_KENC[i + 1];
        const float* w = kenc_conv[2 * i];
        const float* b = kenc_conv[2 * i + 1];
        for (int o = 0; o < cout; ++o) {
            double sc = 1.0, sh = 0.0;
            if (i < 4) {
                const float* const* bn = kenc_bn + 4 * i;
                sc = (double)bn[0][o] / sqrt((double)bn[3][o] + GLUE_BN_EPS);
                sh = (double)bn[1][o] - (double)bn[2][o] * sc;
            }
            float* dw = (i == 0) ? packed + l.k0 + (size_t)o * 4 : packed + l.kw[i - 1] + (size_t)o * cin;
            for (int k = 0; k < cin; ++k) dw[k] = (float)((double)w[(size_t)o * cin + k] * sc);
            const float bias = (float)((double)b[o] * sc + sh);
            if (i == 0)
                dw[3] = bias;
            else
                packed[l.kb[i - 1] + o] = bias;
        }
    }
    if (inproj) {
        memcpy(packed + l.win, inproj[0], (size_t)256 * GLUE_DESC_IN * sizeof(float));
        memcpy(packed + l.bin_, inproj[1], 256 * sizeof(float));
    }
    // ---- attentional propagation layers
    std::vector<double> row(256);
    for (int i = 0; i < GLUE_LAYERS; ++i) {
        const float* const* s = layer0 + GLUE_T_PER_LAYER * i;
        const GlueLayerOff& o = l.L[i];
        for (int tt = 0; tt < 3; ++tt)
            for (int hh = 0; hh < 4; ++hh)
                for (int d = 0; d < 64; ++d) {
                    const int src = d * 4 + hh, dst = tt * 256 + hh * 64 + d;
                    memcpy(packed + o.wqkv + (size_t)dst * 256, s[2 * tt] + (size_t)src * 256, 256 * sizeof(float));
                    packed[o.bqkv + dst] = s[2 * tt + 1][src];
                }
        const float *wm = s[6], *bm = s[7], *w0 = s[8], *b0 = s[9];
        for (int n = 0; n < 512; ++n) {
            const double sc = (double)s[10][n] / sqrt((double)s[13][n] + GLUE_BN_EPS);
            const double sh = (double)s[11][n] - (double)s[12][n] * sc;
            const float* w0r = w0 + (size_t)n * 512;
            float* dst = packed + o.w1 + (size_t)n * 512;
            for (int k = 0; k < 256; ++k) dst[k] = (float)((double)w0r[k] * sc);
            double bacc = b0[n];
            for (int k = 0; k < 256; ++k) row[k] = 0.0;
            for (int j = 0; j < 256; ++j) {
                const double c = w0r[256 + j];
                const float* wmr = wm + (size_t)j * 256;
                for (int k = 0; k < 256; ++k) row[k] += c * (double)wmr[k];
                bacc += c * (double)bm[j];
            }
            // context channel head*64 + d  <-  upstream merge input channel d*4 + head
            for (int hh = 0; hh < 4; ++hh)
                for (int d = 0; d < 64; ++d) dst[256 + hh * 64 + d] = (float)(row[d * 4 + hh] * sc);
            packed[o.b1 + n] = (float)(bacc * sc + sh);
        }
        memcpy(packed + o.w2, s[14], (size_t)256 * 512 * sizeof(float));
        memcpy(packed + o.b2, s[15], 256 * sizeof(float));
    }
    memcpy(packed + l.wfinal, final_wb[0], (size_t)256 * 256 * sizeof(float));
    memcpy(packed + l.bfinal, final_wb[1], 256 * sizeof(float));
    packed[l.bin] = bin[0];
    // split-precision copies of every GEMM weight (taken from the packed f32 layout)
    auto sp = [&](const GlueSplit& d, const float* src, int N, int K) {
        packed[d.s] = split_weights_frag_host(src, N, K, reinterpret_cast<unsigned short*>(packed + d.h),
                                              reinterpret_cast<unsigned short*>(packed + d.l));
    };
    for (int i = 0; i < 4; ++i) sp(l.ks[i], packed + l.kw[i], GLUE_KENC[i + 2], GLUE_KENC[i + 1]);
    if (inproj) sp(l.sin_, packed + l.win, 256, GLUE_DESC_IN);
    std::vector<float> perm((size_t)256 * 512);
    for (int i = 0; i < GLUE_LAYERS; ++i) {
        const GlueLayerOff& o = l.L[i];
        sp(o.sqkv, packed + o.wqkv, 768, 256);
        sp(o.s1, packed + o.w1, 512, 512);
        sp(o.s2, packed + o.w2, 256, 512);
        ffn_permute_k(packed + o.w2, 256, 512, perm.data());
        sp(o.s2p, perm.data(), 256, 512);
    }
    sp(l.sfinal, packed + l.wfinal, 256, 256);
}

// ------------------------------------------------------------------ workspace
// The trunk's buffers.  A network's own carve function decides the offsets: glue_carve_tokens first, its Sinkhorn scratch between
// the two calls, glue_carve_pairs last.
struct GlueTrunkWs {
    float *x, *ctx, *hbuf, *q, *k, *v, *one, *zero, *md, *d128, *sim;
    int *cnt, *active, *m0, *m1;
};
void glue_carve_tokens(WsAlloc& a, GlueTrunkWs& w, int B, int R, bool input_proj) {
    const size_t rows = (size_t)2 * B * R;
    w.x = a.get<float>(rows * 256);
    w.ctx = a.get<float>(rows * 256);
    w.hbuf = a.get<float>(rows * 512);
    w.q = a.get<float>(rows * 256);
    w.k = a.get<float>(rows * 256);
    w.v = a.get<float>(rows * 256);
    w.one = a.get<float>(rows * 32);  // identity rotation for the shared QKV epilogue (cos = 1, sin = 0)
    w.zero = a.get<float>(rows * 32);
    w.md = a.get<float>(rows * 256);
    w.d128 = input_proj ? a.get<float>(rows * GLUE_DESC_IN) : nullptr;
    w.sim = a.get<float>((size_t)B * R * R);
}
void glue_carve_pairs(WsAlloc& a, GlueTrunkWs& w, int B, int R) {
    w.cnt = a.get<int>(2 * B);
    w.active = a.get<int>(B);
    w.m0 = a.get<int>((size_t)B * R);
    w.m1 = a.get<int>((size_t)B * R);
}

// ------------------------------------------------------------------ kernels
__global__ void glue_pairs_kernel(const int* __restrict__ n0, const int* __restrict__ n1, int B, int* __restrict__ cnt,
                                  int* __restrict__ active) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int a = n0[b], c = n1[b];
    const int act = (a > 0 && c > 0) ? 1 : 0;  // upstream returns all -1 / 0 when either image has no key-points
    active[b] = act;
    cnt[2 * b] = act ? a : 0;
    cnt[2 * b + 1] = act ? c : 0;
}

// normalize_keypoints, (k - size / 2) / (max(size) * 0.7), and one channel of the first encoder layer:
// relu(W0' [kx, ky, score] + b0'), w4 = (wx, wy, wscore, bias)
__device__ __forceinline__ float glue_kenc0(const float* __restrict__ kp, float s, float W, float H, float4 w4) {
    const float scaling = fmaxf(W, H) * 0.7f;
    const float kx = (kp[0] - W / 2.0f) / scaling, ky = (kp[1] - H / 2.0f) / scaling;
    return fmaxf(((kx * w4.x + ky * w4.y) + s * w4.z) + w4.w, 0.0f);
}

// The value whose arg-maxima are the matches, as each reference associates it.  Built per pair from (n0, n1).
// SuperGlue: the final log assignment ((Z + u_i) + v_j) - norm
struct SgScore {
    float norm;
    __device__ SgScore(int n0, int n1) : norm(-logf((float)n0 + (float)n1)) {}
    __device__ float operator()(float z, float ui, float vj) const { return ((z + ui) + vj) - norm; }
};
// IMP: P_ij = (p_ij u_i) v_j
struct ImpScore {
    __device__ ImpScore(int, int) {}
    __device__ float operator()(float p, float ui, float vj) const { return (p * ui) * vj; }
};

// one wave per row; equal maxima go to the lowest index
template <class Score>
__global__ __launch_bounds__(256) void glue_rowarg_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
                                                          const int* __restrict__ active, int R, const float* __restrict__ u,
                                                          const float* __restrict__ v, float* __restrict__ max0, int* __restrict__ m0) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    if (i >= n0) return;
    const float* row = sim + ((size_t)b * R + i) * R;
    const float* vb = v + (size_t)b * (R + 64);
    const float ui = u[(size_t)b * (R + 64) + i];
    const Score score(n0, n1);
    float best = -INFINITY;
    int bj = 0x7fffffff;
    for (int j = lane; j < n1; j += 64) {
        const float val = score(row[j], ui, vb[j]);
        if (val > best) {
            best = val;
            bj = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ov > best || (ov == best && oj < bj)) {
            best = ov;
            bj = oj;
        }
    }
    if (lane == 0) {
        max0[(size_t)b * R + i] = best;
        m0[(size_t)b * R + i] = bj;
    }
}

// block = 64 columns x 4 interleaved row groups, 8 rows in flight per thread
template <class Score>
__global__ __launch_bounds__(256) void glue_colarg_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
                                                          const int* __restrict__ active, int R, const float* __restrict__ u,
                                                          const float* __restrict__ v, int* __restrict__ m1) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    if ((int)blockIdx.x * 64 >= n1) return;
    const float* base = sim + (size_t)b * R * R;
    const float* ub = u + (size_t)b * (R + 64);
    const Score score(n0, n1);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if (j < n1) {
        const float vj = v[(size_t)b * (R + 64) + j];
        for (int i0 = g; i0 < n0; i0 += 32) {
            float z[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) z[t] = (i0 + 4 * t < n0) ? base[(size_t)(i0 + 4 * t) * R + j] : 0.0f;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int i = i0 + 4 * t;
                if (i < n0) {
                    const float val = score(z[t], ub[i], vj);
                    if (val > best) {  // rows ascend within a thread: the first of equal maxima stays
                        best = val;
                        bi = i;
                    }
                }
            }
        }
    }
    sv[g][c] = best;
    si[g][c] = bi;
    __syncthreads();
    if (g == 0 && j < n1) {
        for (int gg = 1; gg < 4; ++gg) {
            const float ov = sv[gg][c];
            const int oi = si[gg][c];
            if (ov > best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        m1[(size_t)b * R + j] = bi;
    }
}

// mutual check + strict threshold, one block per pair.  EXP: max0 holds log scores (SuperGlue), else the probabilities themselves.
template <bool EXP>
__global__ __launch_bounds__(256) void glue_filter_kernel(const int* __restrict__ cnt, const int* __restrict__ active, int R, int ncap,
                                                          const int* __restrict__ m0, const int* __restrict__ m1,
                                                          const float* __restrict__ max0, float thr, int* __restrict__ matches0,
                                                          int* __restrict__ matches1, float* __restrict__ mscores0,
                                                          float* __restrict__ mscores1) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!active[b]) return;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    const size_t pb = (size_t)b * R, ob = (size_t)b * ncap;
    for (int i = tid; i < n0; i += 256) {
        const int j = m0[pb + i];  // (stays out of range when every entry of the row is NaN)
        const bool mutual = (unsigned)j < (unsigned)n1 && (m1[pb + j] == i);
        const float ms = mutual ? (EXP ? expf(max0[pb + i]) : max0[pb + i]) : 0.0f;
        matches0[ob + i] = (mutual && ms > thr) ? j : -1;
        mscores0[ob + i] = ms;
    }
    for (int j = tid; j < n1; j += 256) {
        const int i = m1[pb + j];
        const bool mutual = (unsigned)i < (unsigned)n0 && (m0[pb + i] == j);
        const float ms = mutual ? (EXP ? expf(max0[pb + i]) : max0[pb + i]) : 0.0f;  // = mscores0[i] (i is mutual with j)
        matches1[ob + j] = (mutual && ms > thr) ? i : -1;
        mscores1[ob + j] = ms;
    }
}

// arg-maxima of Score over w.sim with the scalings / potentials u, v, then the filter
template <class Score, bool EXP>
void glue_match(const GlueTrunkWs& w, const float* u, const float* v, float* max0, int B, int ncap, int R, float thr, int* matches0,
                int* matches1, float* mscores0, float* mscores1, hipStream_t stream) {
    const dim3 blk(256);
    hipLaunchKernelGGL(glue_rowarg_kernel<Score>, dim3(R / 4, B), blk, 0, stream, w.sim, w.cnt, w.active, R, u, v, max0, w.m0);
    hipLaunchKernelGGL(glue_colarg_kernel<Score>, dim3(R / 64, B), blk, 0, stream, w.sim, w.cnt, w.active, R, u, v, w.m1);
    hipLaunchKernelGGL(glue_filter_kernel<EXP>, dim3(B), blk, 0, stream, w.cnt, w.active, R, ncap, w.m0, w.m1, max0, thr, matches0,
                       matches1, mscores0, mscores1);
}

// ------------------------------------------------------------------ the trunk
// From e32 (first encoder layer, in w.ctx) and the descriptors (SuperGlue: already in w.x; IMP: in w.d128) to the similarity
// matrices w.sim [B,R,R].  Every layer is
//   QKV GEMM (three 256->256 projections as one N=768 launch, heads de-interleaved at pack time)
//   -> flash attention (self: own keys; cross: keys/values of the partner sequence)
//   -> x += mlp.3(relu(bn(mlp.0(cat[x, merge(ctx)])))), merge and bn folded into mlp.0: one fused kernel in split precision
//      (ffn.hip), else GEMM 512->512 + ReLU and GEMM 512->256 with the residual add.
int glue_trunk(imcui_hip_t* h, const float* P, const GlueLayout& l, const GlueTrunkWs& w, int B, int R, int heads, bool ffn_unfused,
               hipStream_t stream) {
    const int S = 2 * B;
    const bool split = h->precision == 1;
    int rc;
    auto base = [&](GemmP& g) {
        g.M = S * R;
        g.cnt = w.cnt;
        g.active = w.active;
        g.rows_per_seq = R;
    };
    auto wts = [&](GemmP& g, size_t wf32, const GlueSplit& sp) {
        g.W = P + wf32;
        if (split) {
            g.Wh = reinterpret_cast<const unsigned short*>(P + sp.h);
            g.Wl = reinterpret_cast<const unsigned short*>(P + sp.l);
            g.wscale = P + sp.s;
        }
    };
    // C[:, :N] = epi(A[:, :K] W^T + bias) over all token rows
    auto linear = [&](int epi, const float* A, int K, int N, size_t wf32, const GlueSplit& sp, size_t bias, float* Cout, float alpha = 1.0f) {
        GemmP g;
        base(g);
        g.epi = epi;
        g.A = A;
        g.lda = K;
        g.K = K;
        g.N = N;
        wts(g, wf32, sp);
        g.ldw = K;
        g.bias = P + bias;
        g.alpha = alpha;
        g.C = Cout;
        g.ldc = N;
        return gemm_launch(h, g, stream);
    };
    // ---- key-point encoder layers 1..4: e32 -> e64 -> e128 -> e256 -> x += e; with input_proj x = e, then x += input_proj(desc)
    {
        const float* src = w.ctx;
        float* bufs[2] = {w.hbuf, w.ctx};
        for (int i = 0; i < 3; ++i) {
            IMCUI_RUN(linear(EPI_RELU, src, GLUE_KENC[i + 1], GLUE_KENC[i + 2], l.kw[i], l.ks[i], l.kb[i], bufs[i & 1]));
            src = bufs[i & 1];
        }
        IMCUI_RUN(linear(l.input_proj ? EPI_BIAS : EPI_RESID, src, 256, 256, l.kw[3], l.ks[3], l.kb[3], w.x));
        if (l.input_proj) IMCUI_RUN(linear(EPI_RESID, w.d128, GLUE_DESC_IN, 256, l.win, l.sin_, l.bin_, w.x));
    }
    // ---- attentional GNN: ['self', 'cross'] * 9
    for (int layer = 0; layer < GLUE_LAYERS; ++layer) {
        const GlueLayerOff& o = l.L[layer];
        GemmP g;
        base(g);
        g.epi = EPI_QKV;
        g.A = w.x;
        g.lda = 256;
        g.K = 256;
        g.N = 768;
        wts(g, o.wqkv, o.sqkv);
        g.ldw = 256;
        g.bias = P + o.bqkv;
        g.v_transposed = split ? 1 : 0;
        g.split_out = split ? 1 : 0;
        g.plane_halves = (size_t)S * R * 256;
        g.Q = w.q;
        g.Kt = w.k;
        g.V = w.v;
        g.rope_cos = w.one;  // no rotary encoding in SuperGlue: q * 1 + rotate_half(q) * 0
        g.rope_sin = w.zero;
        g.alpha = 0.125f * 1.44269504088896340736f;  // scores / 64 ** .5 and log2(e) folded into q: the attention kernels work in base 2
        g.heads = heads;
        IMCUI_RUN(gemm_launch(h, g, stream));
        AttnP a;
        a.Q = w.q;
        a.K = w.k;
        a.V = w.v;
        a.O = w.ctx;
        a.cnt = w.cnt;
        a.active = w.active;
        a.nseq = S;
        a.heads = heads;
        a.rows_per_seq = R;
        a.cross = layer & 1;
        a.log2_domain = 1;
        IMCUI_RUN(attention_launch(h, a, stream));
        if (split && !ffn_unfused) {
            FfnP f;
            f.act = 1;
            f.x = w.x;
            f.ctx = w.ctx;
            f.out = w.x;
            f.w1h = reinterpret_cast<const unsigned short*>(P + o.s1.h);
            f.w1l = reinterpret_cast<const unsigned short*>(P + o.s1.l);
            f.s1 = P + o.s1.s;
            f.b1 = P + o.b1;
            f.w2h = reinterpret_cast<const unsigned short*>(P + o.s2p.h);
            f.w2l = reinterpret_cast<const unsigned short*>(P + o.s2p.l);
            f.s2 = P + o.s2p.s;
            f.b2 = P + o.b2;
            f.M = S * R;
            f.cnt = w.cnt;
            f.active = w.active;
            f.rows_per_seq = R;
            IMCUI_RUN(ffn_launch(h, f, stream));
            continue;
        }
        GemmP f1;  // hbuf = relu(mlp.0'(cat[x, ctx]))
        base(f1);
        f1.epi = EPI_RELU;
        f1.A = w.x;
        f1.lda = 256;
        f1.A2 = w.ctx;
        f1.lda2 = 256;
        f1.K1 = 256;
        f1.K = 512;
        f1.N = 512;
        wts(f1, o.w1, o.s1);
        f1.ldw = 512;
        f1.bias = P + o.b1;
        f1.C = w.hbuf;
        f1.ldc = 512;
        IMCUI_RUN(gemm_launch(h, f1, stream));
        IMCUI_RUN(linear(EPI_RESID, w.hbuf, 512, 256, o.w2, o.s2, o.b2, w.x));  // x += mlp.3(h)
    }
    // md = final_proj(x) / 256^(1/4): md0 . md1 = scores / 256 ** .5 (exact power of two)
    IMCUI_RUN(linear(EPI_BIAS, w.x, 256, 256, l.wfinal, l.sfinal, l.bfinal, w.md, 0.25f));
    GemmP g;  // sim[b] = md0[b] . md1[b]^T
    g.epi = EPI_BIAS;
    g.batch = B;
    g.A = w.md;
    g.lda = 256;
    g.a_bs = (long)2 * R * 256;
    g.W = w.md + (size_t)R * 256;
    g.ldw = 256;
    g.w_bs = (long)2 * R * 256;
    g.C = w.sim;
    g.ldc = R;
    g.c_bs = (long)R * R;
    g.M = R;
    g.N = R;
    g.K = 256;
    g.mcnt = w.cnt;
    g.ncnt = w.cnt + 1;
    g.cnt_stride = 2;
    return gemm_launch(h, g, stream);
}

}  // namespace
