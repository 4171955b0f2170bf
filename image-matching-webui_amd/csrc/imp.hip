// IMP (`sfd2+imp` of the zoo): what imcui/hloc/matchers/imp.py:51 `self.net.produce_matches(data, p=0.2)` computes
// (pram.nets.gml.GML, restated in tests/imp_reference.py: the submodule is absent, see INTEGRATION.md "IMP: what is pinned"),
// for B pairs at once.
//
// Trunk = SuperGlue's, on the shared kernels and in superglue.hip's data layout: 2B sequences of R = roundup(ncap,128) token
// rows, x [2B*R,256] token-major, attention operands head-major, per-sequence counts on the device.  What differs: the
// descriptors are 128 wide and enter through input_proj (128 -> 256, the key-point encoding joins in the residual epilogue),
// and one of nine final projections (final_proj.8) feeds the similarity.
//
// Assignment = probability-domain Sinkhorn on the materialised matrix [B,R,R], hand-written here (imp_* kernels):
//   imp_softmax_kernel   M -> p in place (row soft-max over the n1 columns and the dust-bin column, which goes to a vector;
//                        the dust-bin row is the constant 1 / (n1 + 1) and is never stored)
//   imp_round_kernel     one round reads the matrix ONCE: a workgroup owns IMP_BAND rows, computes their u from the staged v
//                        and at once the band's contribution to the column sums with the new u
//   imp_merge_kernel     folds the band partials in band order, adds the dust-bin row's term, writes v
//   imp_rowarg / colarg / filter   arg-maxima of p_ij u_i v_j, mutual check, strict threshold; P is never written
// Every sum has one fixed order (no float atomics), and the file is compiled with -ffp-contract=off: every operation rounds
// once, so tests/imp_reference.py `sinkhorn_explicit` states the same float32 order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "attention.h"
#include "ffn.h"
#include "gemm.h"
#include "imcui_hip.h"

#define IMP_LAYERS 18
#define IMP_HEADS 4
#define IMP_DESC 128     // input_proj input width (anything else is refused by the binding)
#define IMP_FINAL 9      // final_proj.{0..8}: training supervises every layer pair, inference reads the last
#define IMP_BN_EPS 1e-5  // nn.BatchNorm1d default
#define IMP_EPS 1e-8f    // epsilon of the Sinkhorn divisions
#define IMP_BAND 16      // rows per workgroup of a round (8 waves x 2 rows)
#define IMP_NK 16        // float4 per lane and row: 16 x 256 = 4096 columns stay in registers
#define IMP_COLS (IMP_NK * 256)
#define IMP_HALF 2048    // columns per cross-wave fold through LDS
#define IMP_MG 16        // groups of the merge kernel = bands per group (16 x 16 = 4096 / IMP_BAND bands)
// marginals of the dust-bins: r = [1] * n0 + [n1], c = [1] * n1 + [n0]
#define IMP_ROW_BIN_MASS(n0, n1) ((float)(n1))
#define IMP_COL_BIN_MASS(n0, n1) ((float)(n0))

// ------------------------------------------------------------------ the tensor table (names and shapes of the state dict)
static const int IMP_KENC[6] = {3, 32, 64, 128, 256, 256};
static const char* const IMP_BN_FIELDS[4] = {"weight", "bias", "running_mean", "running_var"};
struct ImpTensor {
    char name[64];
    int nd, d[3];
};
// first table index of each group
enum { IMP_T_CONV = 0, IMP_T_BN = 10, IMP_T_INPROJ = 26, IMP_T_LAYER0 = 28, IMP_T_PER_LAYER = 16 };
enum { IMP_T_FINAL = IMP_T_LAYER0 + IMP_T_PER_LAYER * IMP_LAYERS, IMP_T_BIN = IMP_T_FINAL + 2 * IMP_FINAL, IMP_NUM_TENSORS = IMP_T_BIN + 1 };
// per layer, in this order (j = index inside the layer)
static const struct {
    const char* key;
    int nd, d0, d1;
} IMP_LAYER_KEYS[IMP_T_PER_LAYER] = {
    {"attn.proj.0.weight", 3, 256, 256}, {"attn.proj.0.bias", 1, 256, 0},  {"attn.proj.1.weight", 3, 256, 256}, {"attn.proj.1.bias", 1, 256, 0},
    {"attn.proj.2.weight", 3, 256, 256}, {"attn.proj.2.bias", 1, 256, 0},  {"attn.merge.weight", 3, 256, 256},  {"attn.merge.bias", 1, 256, 0},
    {"mlp.0.weight", 3, 512, 512},       {"mlp.0.bias", 1, 512, 0},        {"mlp.1.weight", 1, 512, 0},         {"mlp.1.bias", 1, 512, 0},
    {"mlp.1.running_mean", 1, 512, 0},   {"mlp.1.running_var", 1, 512, 0}, {"mlp.3.weight", 3, 256, 512},       {"mlp.3.bias", 1, 256, 0},
};
static const std::vector<ImpTensor>& imp_table() {
    static const std::vector<ImpTensor> table = [] {
        std::vector<ImpTensor> t;
        auto push = [&](const ImpTensor& e) { t.push_back(e); };
#define add(nd_, d0_, d1_, ...)                                                              \
    do {                                                                                     \
        ImpTensor e;                                                                         \
        snprintf(e.name, sizeof e.name, __VA_ARGS__);                                        \
        e.nd = (nd_), e.d[0] = (d0_), e.d[1] = (d1_), e.d[2] = 1; /* Conv1d: [out, in, 1] */ \
        push(e);                                                                             \
    } while (0)
        for (int i = 0; i < 5; ++i) {  // 0..9: convolutions of the key-point encoder
            add(3, IMP_KENC[i + 1], IMP_KENC[i], "kenc.encoder.%d.weight", 3 * i);
            add(1, IMP_KENC[i + 1], 0, "kenc.encoder.%d.bias", 3 * i);
        }
        for (int i = 0; i < 4; ++i)  // 10..25: its BatchNorms
            for (int f = 0; f < 4; ++f) add(1, IMP_KENC[i + 1], 0, "kenc.encoder.%d.%s", 3 * i + 1, IMP_BN_FIELDS[f]);
        add(3, 256, IMP_DESC, "input_proj.weight");  // 26, 27
        add(1, 256, 0, "input_proj.bias");
        for (int i = 0; i < IMP_LAYERS; ++i)  // 28 + 16 i + j
            for (int j = 0; j < IMP_T_PER_LAYER; ++j)
                add(IMP_LAYER_KEYS[j].nd, IMP_LAYER_KEYS[j].d0, IMP_LAYER_KEYS[j].d1, "gnn.layers.%d.%s", i, IMP_LAYER_KEYS[j].key);
        for (int k = 0; k < IMP_FINAL; ++k) {  // IMP_T_FINAL + 2 k
            add(3, 256, 256, "final_proj.%d.weight", k);
            add(1, 256, 0, "final_proj.%d.bias", k);
        }
        add(0, 1, 0, "bin_score");  // a scalar parameter
#undef add
        return t;
    }();
    return table;
}

extern "C" int imcui_hip_imp_num_tensors(void) { return IMP_NUM_TENSORS; }
extern "C" const char* imcui_hip_imp_tensor_name(int i) { return (i < 0 || i >= IMP_NUM_TENSORS) ? nullptr : imp_table()[i].name; }
extern "C" int imcui_hip_imp_tensor_shape(int i, int* dims) {
    if (i < 0 || i >= IMP_NUM_TENSORS || !dims) return -1;
    const ImpTensor& e = imp_table()[i];
    for (int k = 0; k < e.nd; ++k) dims[k] = e.d[k];
    return e.nd;
}

// ------------------------------------------------------------------ packed weights (superglue.hip's format plus input_proj)
struct ImpSplit {
    size_t h, l, s;  // f16 hi / lo planes (float offsets) and the 2^-e scale
};
struct ImpLayerOff {
    size_t wqkv, bqkv, w1, b1, w2, b2;
    ImpSplit sqkv, s1, s2, s2p;  // s2p: mlp.3 planes in the fused FFN kernel's K order
};
struct ImpLayout {
    size_t k0;            // [32][4]: wx, wy, wscore, bias of the first key-point encoder layer (BN folded)
    size_t kw[4], kb[4];  // encoder layers 1..4
    ImpSplit ks[4];
    size_t win, bin_;  // input_proj
    ImpSplit sin_;
    ImpLayerOff L[IMP_LAYERS];
    size_t wfinal, bfinal, bin;
    ImpSplit sfinal;
    size_t total;
};

static ImpLayout imp_layout() {
    ImpLayout l;
    size_t off = 0;
    auto take = [&](size_t n) {
        size_t r = off;
        off += align_up(n, 64);
        return r;
    };
    auto take_split = [&](size_t n) {
        ImpSplit sp;
        sp.h = take(n / 2);
        sp.l = take(n / 2);
        sp.s = take(64);
        return sp;
    };
    l.k0 = take(32 * 4);
    for (int i = 0; i < 4; ++i) {
        l.kw[i] = take((size_t)IMP_KENC[i + 2] * IMP_KENC[i + 1]);
        l.kb[i] = take(IMP_KENC[i + 2]);
    }
    l.win = take(256 * IMP_DESC);
    l.bin_ = take(256);
    for (int i = 0; i < IMP_LAYERS; ++i) {
        ImpLayerOff& o = l.L[i];
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
    for (int i = 0; i < 4; ++i) l.ks[i] = take_split((size_t)IMP_KENC[i + 2] * IMP_KENC[i + 1]);
    l.sin_ = take_split(256 * IMP_DESC);
    for (int i = 0; i < IMP_LAYERS; ++i) {
        ImpLayerOff& o = l.L[i];
        o.sqkv = take_split(768 * 256);
        o.s1 = take_split(512 * 512);
        o.s2 = take_split(256 * 512);
        o.s2p = take_split(256 * 512);
    }
    l.sfinal = take_split(256 * 256);
    l.total = off;
    return l;
}

extern "C" size_t imcui_hip_imp_packed_floats(void) { return imp_layout().total; }

// Host-side packing: eval-mode BatchNorm into the preceding convolution, attn.merge into mlp.0, heads de-interleaved
// (upstream channel d * 4 + head -> head * 64 + d), all in double -- the folds of imcui_hip_superglue_pack_weights.
extern "C" int imcui_hip_imp_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    for (int i = 0; i < IMP_NUM_TENSORS; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const ImpLayout l = imp_layout();
    memset(packed, 0, l.total * sizeof(float));
    for (int i = 0; i < 5; ++i) {
        const int cin = IMP_KENC[i], cout = IMP_KENC[i + 1];
        const float* w = t[IMP_T_CONV + 2 * i];
        const float* b = t[IMP_T_CONV + 2 * i + 1];
        for (int o = 0; o < cout; ++o) {
            double sc = 1.0, sh = 0.0;
            if (i < 4) {
                const float* const* bn = t + IMP_T_BN + 4 * i;
                sc = (double)bn[0][o] / sqrt((double)bn[3][o] + IMP_BN_EPS);
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
    memcpy(packed + l.win, t[IMP_T_INPROJ], (size_t)256 * IMP_DESC * sizeof(float));
    memcpy(packed + l.bin_, t[IMP_T_INPROJ + 1], 256 * sizeof(float));
    std::vector<double> row(256);
    for (int i = 0; i < IMP_LAYERS; ++i) {
        const float* const* s = t + IMP_T_LAYER0 + IMP_T_PER_LAYER * i;
        const ImpLayerOff& o = l.L[i];
        for (int tt = 0; tt < 3; ++tt)
            for (int hh = 0; hh < 4; ++hh)
                for (int d = 0; d < 64; ++d) {
                    const int src = d * 4 + hh, dst = tt * 256 + hh * 64 + d;
                    memcpy(packed + o.wqkv + (size_t)dst * 256, s[2 * tt] + (size_t)src * 256, 256 * sizeof(float));
                    packed[o.bqkv + dst] = s[2 * tt + 1][src];
                }
        const float *wm = s[6], *bm = s[7], *w0 = s[8], *b0 = s[9];
        for (int n = 0; n < 512; ++n) {
            const double sc = (double)s[10][n] / sqrt((double)s[13][n] + IMP_BN_EPS);
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
            for (int hh = 0; hh < 4; ++hh)
                for (int d = 0; d < 64; ++d) dst[256 + hh * 64 + d] = (float)(row[d * 4 + hh] * sc);
            packed[o.b1 + n] = (float)(bacc * sc + sh);
        }
        memcpy(packed + o.w2, s[14], (size_t)256 * 512 * sizeof(float));
        memcpy(packed + o.b2, s[15], 256 * sizeof(float));
    }
    const float* const* f = t + IMP_T_FINAL + 2 * (IMP_FINAL - 1);  // inference reads final_proj.8 only
    memcpy(packed + l.wfinal, f[0], (size_t)256 * 256 * sizeof(float));
    memcpy(packed + l.bfinal, f[1], 256 * sizeof(float));
    packed[l.bin] = t[IMP_T_BIN][0];
    auto sp = [&](const ImpSplit& d, size_t src, int N, int K) {
        packed[d.s] = split_weights_frag_host(packed + src, N, K, reinterpret_cast<unsigned short*>(packed + d.h),
                                              reinterpret_cast<unsigned short*>(packed + d.l));
    };
    for (int i = 0; i < 4; ++i) sp(l.ks[i], l.kw[i], IMP_KENC[i + 2], IMP_KENC[i + 1]);
    sp(l.sin_, l.win, 256, IMP_DESC);
    for (int i = 0; i < IMP_LAYERS; ++i) {
        const ImpLayerOff& o = l.L[i];
        sp(o.sqkv, o.wqkv, 768, 256);
        sp(o.s1, o.w1, 512, 512);
        sp(o.s2, o.w2, 256, 512);
        std::vector<float> perm((size_t)256 * 512);
        ffn_permute_k(packed + o.w2, 256, 512, perm.data());
        packed[o.s2p.s] = split_weights_frag_host(perm.data(), 256, 512, reinterpret_cast<unsigned short*>(packed + o.s2p.h),
                                                  reinterpret_cast<unsigned short*>(packed + o.s2p.l));
    }
    sp(l.sfinal, l.wfinal, 256, 256);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ workspace
struct ImpWs {
    float *x, *ctx, *hbuf, *q, *k, *v, *one, *zero, *md, *d128, *sim, *u, *vv, *binc, *max0, *part;
    int *cnt, *active, *m0, *m1;
    size_t total;
    bool ok;
};

static ImpWs imp_carve(void* ws, size_t bytes, int B, int R) {
    WsAlloc a(ws, bytes);
    ImpWs w;
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
    w.d128 = a.get<float>(rows * IMP_DESC);
    w.sim = a.get<float>((size_t)B * R * R);
    w.u = a.get<float>((size_t)B * (R + 64));
    w.vv = a.get<float>((size_t)B * (R + 64));
    w.binc = a.get<float>((size_t)B * R);  // dust-bin column of p
    w.max0 = a.get<float>((size_t)B * R);
    w.part = a.get<float>((size_t)B * (R / IMP_BAND) * R);  // column sums per row band
    w.cnt = a.get<int>(2 * B);
    w.active = a.get<int>(B);
    w.m0 = a.get<int>((size_t)B * R);
    w.m1 = a.get<int>((size_t)B * R);
    w.total = a.off;
    w.ok = a.ok;
    return w;
}

extern "C" size_t imcui_hip_imp_workspace_bytes(int B, int ncap) {
    const int R = (int)align_up((size_t)(ncap > 0 ? ncap : 1), 128);
    return imp_carve(nullptr, 0, B, R).total;
}

// ------------------------------------------------------------------ kernels
__global__ void imp_pairs_kernel(const int* __restrict__ n0, const int* __restrict__ n1, int B, int* __restrict__ cnt,
                                 int* __restrict__ active) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int a = n0[b], c = n1[b];
    const int act = (a > 0 && c > 0) ? 1 : 0;  // a pair with an empty side returns all -1 / 0
    active[b] = act;
    cnt[2 * b] = act ? a : 0;
    cnt[2 * b + 1] = act ? c : 0;
}

// outputs preset to -1 / 0, scalings u = v = 1 (R + 1 entries: index n is the dust-bin)
__global__ __launch_bounds__(256) void imp_reset_kernel(int ncap, int R, float* __restrict__ u, float* __restrict__ v,
                                                        int* __restrict__ matches0, int* __restrict__ matches1,
                                                        float* __restrict__ ms0, float* __restrict__ ms1) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > R) return;
    u[(size_t)b * (R + 64) + i] = 1.0f;
    v[(size_t)b * (R + 64) + i] = 1.0f;
    if (i < ncap) {
        const size_t o = (size_t)b * ncap + i;
        matches0[o] = -1, matches1[o] = -1;
        ms0[o] = 0.0f, ms1[o] = 0.0f;
    }
}

// one wave per token row: descriptor -> d128 (padded rows cleared), key-point normalisation and the first encoder layer
// relu(W0' [kx, ky, score] + b0') -> e32, identity rotation tables for the shared QKV epilogue
__global__ __launch_bounds__(256) void imp_init_kernel(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                       const float* __restrict__ sc0, const float* __restrict__ sc1,
                                                       const float* __restrict__ d0, const float* __restrict__ d1,
                                                       const int* __restrict__ cnt, int ncap, int R, float w0, float h0, float w1,
                                                       float h1, const float* __restrict__ k0w, float* __restrict__ d128,
                                                       float* __restrict__ e32, float* __restrict__ one, float* __restrict__ zero) {
    const int lane = threadIdx.x & 63;
    const int seq = blockIdx.y, b = seq >> 1, img = seq & 1;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= R) return;
    const int n = cnt[seq];
    const size_t row = (size_t)seq * R + i;
    if (lane >= 32) {
        one[row * 32 + lane - 32] = 1.0f;
        zero[row * 32 + lane - 32] = 0.0f;
        return;
    }
    if (i >= n) {
        *reinterpret_cast<float4*>(d128 + row * IMP_DESC + lane * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        e32[row * 32 + lane] = 0.0f;
        return;
    }
    const float* d = (img ? d1 : d0) + ((size_t)b * ncap + i) * IMP_DESC;
    *reinterpret_cast<float4*>(d128 + row * IMP_DESC + lane * 4) = *reinterpret_cast<const float4*>(d + lane * 4);
    const float* kp = (img ? kp1 : kp0) + ((size_t)b * ncap + i) * 2;
    const float W = img ? w1 : w0, H = img ? h1 : h0;
    const float scaling = fmaxf(W, H) * 0.7f;  // (k - size / 2) / (0.7 * max(size))
    const float kx = (kp[0] - W / 2.0f) / scaling, ky = (kp[1] - H / 2.0f) / scaling;
    const float s = (img ? sc1 : sc0)[(size_t)b * ncap + i];
    const float4 w4 = *reinterpret_cast<const float4*>(k0w + lane * 4);
    e32[row * 32 + lane] = fmaxf(((kx * w4.x + ky * w4.y) + s * w4.z) + w4.w, 0.0f);
}

// probe only: scores [B, ncap, ncap] -> the R-strided matrix
__global__ __launch_bounds__(256) void imp_stage_kernel(const float* __restrict__ src, const int* __restrict__ cnt, int ncap, int R,
                                                        float* __restrict__ sim) {
    const int b = blockIdx.z, i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt[2 * b] || j >= cnt[2 * b + 1]) return;
    sim[((size_t)b * R + i) * R + j] = src[((size_t)b * ncap + i) * ncap + j];
}

__global__ __launch_bounds__(256) void imp_copy_kernel(const float* __restrict__ src, int sstride, int n, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[(size_t)blockIdx.y * n + i] = src[(size_t)blockIdx.y * sstride + i];
}

// the 64 lane values folded as a tree, every lane ends with the same bits: t = s[l] + s[l ^ 32], then ^ 16, ... ^ 1
__device__ __forceinline__ float imp_wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
    return s;
}

// a row of the matrix in registers: lane holds columns k * 256 + lane * 4 .. + 3, k < IMP_NK; entries outside the n1 real
// columns (and rows that do not exist) are 0.  Padding of the matrix is never read as a value: it may hold anything.
__device__ __forceinline__ void imp_load_row(float4 (&z)[IMP_NK], const float* __restrict__ row, bool ok, int lane, int n1) {
    const int nch = (n1 + 255) >> 8;
#pragma unroll
    for (int k = 0; k < IMP_NK; ++k) {
        const int j = k * 256 + lane * 4;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && k < nch && j < n1) t = *reinterpret_cast<const float4*>(row + j);
        if (j + 1 >= n1) t.y = 0.0f;
        if (j + 2 >= n1) t.z = 0.0f;
        if (j + 3 >= n1) t.w = 0.0f;
        z[k] = t;
    }
}

// Row soft-max with the dust-bin column, one wave per row: p_ij = exp(M_ij - max) / sum over the n1 columns and the
// dust-bin entry bin_score; replaces M by p, the dust-bin entry p[i][n1] goes to binc.
// Sum order: per lane k-major then x, y, z, w; lanes as a tree (imp_wave_sum); the dust-bin term last.
__global__ __launch_bounds__(256) void imp_softmax_kernel(float* __restrict__ sim, const int* __restrict__ cnt,
                                                          const int* __restrict__ active, int R, const float* __restrict__ binp,
                                                          float binv, float* __restrict__ binc) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    if (i >= n0) return;
    const float alpha = binp ? binp[0] : binv;
    float* row = sim + ((size_t)b * R + i) * R;
    float4 z[IMP_NK];
    imp_load_row(z, row, true, lane, n1);
    float mx = alpha;
#pragma unroll
    for (int k = 0; k < IMP_NK; ++k) {
        const int j = k * 256 + lane * 4;
        if (j < n1) mx = fmaxf(mx, z[k].x);
        if (j + 1 < n1) mx = fmaxf(mx, z[k].y);
        if (j + 2 < n1) mx = fmaxf(mx, z[k].z);
        if (j + 3 < n1) mx = fmaxf(mx, z[k].w);
    }
    mx = wave_max(mx);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < IMP_NK; ++k) {
        const int j = k * 256 + lane * 4;
        z[k].x = (j < n1) ? expf(z[k].x - mx) : 0.0f;
        z[k].y = (j + 1 < n1) ? expf(z[k].y - mx) : 0.0f;
        z[k].z = (j + 2 < n1) ? expf(z[k].z - mx) : 0.0f;
        z[k].w = (j + 3 < n1) ? expf(z[k].w - mx) : 0.0f;
        s = s + z[k].x;
        s = s + z[k].y;
        s = s + z[k].z;
        s = s + z[k].w;
    }
    const float eb = expf(alpha - mx);
    const float tot = imp_wave_sum(s) + eb;
#pragma unroll
    for (int k = 0; k < IMP_NK; ++k) {
        const int j = k * 256 + lane * 4;
        if (j < n1) *reinterpret_cast<float4*>(row + j) = make_float4(z[k].x / tot, z[k].y / tot, z[k].z / tot, z[k].w / tot);
    }
    if (lane == 0) binc[(size_t)b * R + i] = eb / tot;
}

// One Sinkhorn round, first half: workgroup = IMP_BAND rows of one pair (wave w: rows 2w, 2w + 1 of the band), a row lives
// in registers (IMP_NK float4 per lane = 4096 columns, so one regime serves every ncap the call accepts).
//   u_i = 1 / ((sum_j p_ij v_j + p_i,bin v_bin) + eps)          sum order as in the soft-max, v staged in LDS
//   part[band][j] = fold over waves 0..7 of (p_ij u_i + p_i'j u_i')   with the NEW u: the matrix is read once per round
// Block index == number of bands: the dust-bin row, u_bin = n1 / (sum_{j <= n1} v_j / (n1 + 1) + eps).
__global__ __launch_bounds__(512) void imp_round_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
                                                        const int* __restrict__ active, int R, const float* __restrict__ binc,
                                                        const float* __restrict__ v, float* __restrict__ u, float* __restrict__ part) {
    __shared__ float4 lds4[(8 * IMP_HALF + IMP_COLS + 64) / 4];
    float* lm = reinterpret_cast<float*>(lds4);  // [8 waves][2048]: a wave's column sums, one half of the columns at a time
    float* lv = lm + 8 * IMP_HALF;               // [4096 + 64]: staged v, 0 beyond the dust-bin entry
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    const int nbands = (n0 + IMP_BAND - 1) / IMP_BAND;
    const int band = blockIdx.x;
    if (band > nbands) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* vb = v + (size_t)b * (R + 64);
    float* ub = u + (size_t)b * (R + 64);
    for (int j = tid; j < IMP_COLS + 64; j += 512) lv[j] = (j <= n1) ? vb[j] : 0.0f;
    __syncthreads();
    if (band == nbands) {
        const float dbrow = 1.0f / (float)(n1 + 1);
        float s = 0.0f;
        for (int j = tid; j <= n1; j += 512) s = s + dbrow * lv[j];
        s = imp_wave_sum(s);
        if (lane == 0) lm[w] = s;
        __syncthreads();
        if (tid == 0) {
            float S = lm[0];
            for (int k = 1; k < 8; ++k) S = S + lm[k];
            ub[n0] = IMP_ROW_BIN_MASS(n0, n1) / (S + IMP_EPS);
        }
        return;
    }
    const float* simb = sim + (size_t)b * R * R;
    const float* bincb = binc + (size_t)b * R;
    const float vbin = lv[n1];
    float4 acc[IMP_NK];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int i = band * IMP_BAND + 2 * w + rr;
        const bool ok = i < n0;  // wave-uniform
        float4 z[IMP_NK];
        imp_load_row(z, simb + (size_t)i * R, ok, lane, n1);
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < IMP_NK; ++k) {
            const float4 vj = *reinterpret_cast<const float4*>(lv + k * 256 + lane * 4);
            s = s + z[k].x * vj.x;
            s = s + z[k].y * vj.y;
            s = s + z[k].z * vj.z;
            s = s + z[k].w * vj.w;
        }
        s = imp_wave_sum(s);
        float ui = 0.0f;
        if (ok) {
            ui = 1.0f / ((s + bincb[i] * vbin) + IMP_EPS);
            if (lane == 0) ub[i] = ui;
        }
#pragma unroll
        for (int k = 0; k < IMP_NK; ++k) {
            if (rr == 0)
                acc[k] = make_float4(z[k].x * ui, z[k].y * ui, z[k].z * ui, z[k].w * ui);
            else
                acc[k] = make_float4(acc[k].x + z[k].x * ui, acc[k].y + z[k].y * ui, acc[k].z + z[k].z * ui, acc[k].w + z[k].w * ui);
        }
    }
    const int nch = (n1 + 255) >> 8;
    float* pb = part + ((size_t)b * (R / IMP_BAND) + band) * R;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half * 8 >= nch) break;  // block-uniform
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(lm + w * IMP_HALF + k * 256 + lane * 4) = acc[half * 8 + k];
        __syncthreads();
        float4 S = *reinterpret_cast<const float4*>(lm + 4 * tid);
#pragma unroll
        for (int ww = 1; ww < 8; ++ww) {
            const float4 t = *reinterpret_cast<const float4*>(lm + ww * IMP_HALF + 4 * tid);
            S = make_float4(S.x + t.x, S.y + t.y, S.z + t.z, S.w + t.w);
        }
        const int col = half * IMP_HALF + 4 * tid;
        if (col < R) *reinterpret_cast<float4*>(pb + col) = S;
        __syncthreads();
    }
}

// Second half of the round: v_j = 1 / ((sum over bands + u_bin / (n1 + 1)) + eps).  Block = 256 columns x IMP_MG groups; group g
// folds bands 16 g .. 16 g + 15 in order, then the groups are folded in order.  The last block is the dust-bin column:
// v_bin = n0 / ((sum_i p_i,bin u_i + u_bin / (n1 + 1)) + eps), thread-strided partial sums, wave tree, waves in order.
__global__ __launch_bounds__(64 * IMP_MG) void imp_merge_kernel(const int* __restrict__ cnt, const int* __restrict__ active, int R,
                                                                const float* __restrict__ binc, const float* __restrict__ u,
                                                                const float* __restrict__ part, float* __restrict__ v) {
    __shared__ float sm[IMP_MG][256];
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const float* ub = u + (size_t)b * (R + 64);
    const float dbrow = 1.0f / (float)(n1 + 1);
    const float rowterm = dbrow * ub[n0];
    if (blockIdx.x == gridDim.x - 1) {
        const float* bincb = binc + (size_t)b * R;
        float s = 0.0f;
        for (int i = threadIdx.x; i < n0; i += 64 * IMP_MG) s = s + bincb[i] * ub[i];
        s = imp_wave_sum(s);
        if (c == 0) sm[g][0] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            float S = sm[0][0];
            for (int gg = 1; gg < IMP_MG; ++gg) S = S + sm[gg][0];
            v[(size_t)b * (R + 64) + n1] = IMP_COL_BIN_MASS(n0, n1) / ((S + rowterm) + IMP_EPS);
        }
        return;
    }
    if ((int)blockIdx.x * 256 >= n1) return;
    const int nbands = (n0 + IMP_BAND - 1) / IMP_BAND;
    const int j = blockIdx.x * 256 + c * 4;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < n1) {
        const int k1 = min(nbands, (g + 1) * IMP_MG);
        const float* p = part + (size_t)b * (R / IMP_BAND) * R + j;
#pragma unroll 4
        for (int k = g * IMP_MG; k < k1; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(p + (size_t)k * R);
            t = make_float4(t.x + a.x, t.y + a.y, t.z + a.z, t.w + a.w);
        }
    }
    *reinterpret_cast<float4*>(&sm[g][c * 4]) = t;
    __syncthreads();
    const int jj = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < 256 && jj < n1) {
        float r = sm[0][threadIdx.x];
        for (int gg = 1; gg * IMP_MG < nbands; ++gg) r = r + sm[gg][threadIdx.x];
        v[(size_t)b * (R + 64) + jj] = 1.0f / ((r + rowterm) + IMP_EPS);
    }
}

// P_ij = (p_ij u_i) v_j in the reference's association; only its arg-maxima leave the chip
__device__ __forceinline__ float imp_score(float p, float ui, float vj) { return (p * ui) * vj; }

__global__ __launch_bounds__(256) void imp_rowarg_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
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
    float best = -INFINITY;
    int bj = 0x7fffffff;
    for (int j = lane; j < n1; j += 64) {
        const float val = imp_score(row[j], ui, vb[j]);
        if (val > best) {
            best = val;
            bj = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // equal maxima go to the lowest index
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

__global__ __launch_bounds__(256) void imp_colarg_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
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
                    const float val = imp_score(z[t], ub[i], vj);
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

// mutual check + strict threshold on the probabilities themselves (no exp), one block per pair
__global__ __launch_bounds__(256) void imp_filter_kernel(const int* __restrict__ cnt, const int* __restrict__ active, int R, int ncap,
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
        const float ms = mutual ? max0[pb + i] : 0.0f;
        matches0[ob + i] = (mutual && ms > thr) ? j : -1;
        mscores0[ob + i] = ms;
    }
    for (int j = tid; j < n1; j += 256) {
        const int i = m1[pb + j];
        const bool mutual = (unsigned)i < (unsigned)n0 && (m0[pb + i] == j);
        const float ms = mutual ? max0[pb + i] : 0.0f;  // = mscores0[i] (i is mutual with j)
        matches1[ob + j] = (mutual && ms > thr) ? i : -1;
        mscores1[ob + j] = ms;
    }
}

// the assignment stage on w.sim: soft-max, `iterations` rounds, arg-maxima, filter
static int imp_assign(imcui_hip_t* h, const ImpWs& w, int B, int ncap, int R, const float* binp, float binv, int iterations, float thr,
                      int* matches0, int* matches1, float* mscores0, float* mscores1, hipStream_t stream) {
    const dim3 blk(256);
    hipLaunchKernelGGL(imp_softmax_kernel, dim3(R / 4, B), blk, 0, stream, w.sim, w.cnt, w.active, R, binp, binv, w.binc);
    const dim3 rg(R / IMP_BAND + 1, B), mg(cdiv(R, 256) + 1, B);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(imp_round_kernel, rg, dim3(512), 0, stream, w.sim, w.cnt, w.active, R, w.binc, w.vv, w.u, w.part);
        hipLaunchKernelGGL(imp_merge_kernel, mg, dim3(64 * IMP_MG), 0, stream, w.cnt, w.active, R, w.binc, w.u, w.part, w.vv);
    }
    hipLaunchKernelGGL(imp_rowarg_kernel, dim3(R / 4, B), blk, 0, stream, w.sim, w.cnt, w.active, R, w.u, w.vv, w.max0, w.m0);
    hipLaunchKernelGGL(imp_colarg_kernel, dim3(R / 64, B), blk, 0, stream, w.sim, w.cnt, w.active, R, w.u, w.vv, w.m1);
    hipLaunchKernelGGL(imp_filter_kernel, dim3(B), blk, 0, stream, w.cnt, w.active, R, ncap, w.m0, w.m1, w.max0, thr, matches0, matches1,
                       mscores0, mscores1);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ probe: the assignment stage alone
extern "C" int imcui_hip_imp_ot_probe(imcui_hip_t* h, const float* scores, int B, int ncap, const int* n0, const int* n1, float bin_score,
                                      int iterations, double p, int* matches0, int* matches1, float* mscores0, float* mscores1,
                                      float* u_out, float* v_out, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (ncap <= 0 || ncap > IMP_COLS) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: ncap=%d outside 1..%d", ncap, IMP_COLS);
    if (iterations < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: iterations=%d", iterations);
    if (!scores || !n0 || !n1 || !matches0 || !matches1 || !mscores0 || !mscores1) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: null argument");
    const int R = (int)align_up((size_t)ncap, 128);
    ImpWs w = imp_carve(ws, ws_bytes, B, R);
    if (!ws || !w.ok) return imcui_set_err(h, IMCUI_ERR_WS, "imp: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipLaunchKernelGGL(imp_pairs_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, n0, n1, B, w.cnt, w.active);
    hipLaunchKernelGGL(imp_reset_kernel, dim3(cdiv(R + 1, 256), B), dim3(256), 0, stream, ncap, R, w.u, w.vv, matches0, matches1, mscores0,
                       mscores1);
    hipLaunchKernelGGL(imp_stage_kernel, dim3(cdiv(ncap, 256), ncap, B), dim3(256), 0, stream, scores, w.cnt, ncap, R, w.sim);
    int rc;
    IMCUI_RUN(imp_assign(h, w, B, ncap, R, nullptr, bin_score, iterations, (float)p, matches0, matches1, mscores0, mscores1, stream));
    // u, v [B, ncap + 1]: entry n0 / n1 of a pair is its dust-bin (entries beyond it are 1)
    if (u_out) hipLaunchKernelGGL(imp_copy_kernel, dim3(cdiv(ncap + 1, 256), B), dim3(256), 0, stream, w.u, R + 64, ncap + 1, u_out);
    if (v_out) hipLaunchKernelGGL(imp_copy_kernel, dim3(cdiv(ncap + 1, 256), B), dim3(256), 0, stream, w.vv, R + 64, ncap + 1, v_out);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ forward
extern "C" int imcui_hip_imp_forward(imcui_hip_t* h, const float* packed, int B, int ncap, const float* keypoints0, const float* keypoints1,
                                     const float* scores0, const float* scores1, const float* descriptors0, const float* descriptors1,
                                     const int* n0, const int* n1, float w0, float h0, float w1, float h1, int sinkhorn_iterations,
                                     double match_threshold, int* matches0, int* matches1, float* mscores0, float* mscores1, void* ws,
                                     size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (ncap <= 0 || ncap > IMP_COLS) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: ncap=%d outside 1..%d", ncap, IMP_COLS);
    if (sinkhorn_iterations < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: sinkhorn_iterations=%d", sinkhorn_iterations);
    if (!packed || !keypoints0 || !keypoints1 || !scores0 || !scores1 || !descriptors0 || !descriptors1 || !n0 || !n1 || !matches0 ||
        !matches1 || !mscores0 || !mscores1)
        return imcui_set_err(h, IMCUI_ERR_ARG, "imp: null argument");
    const int R = (int)align_up((size_t)ncap, 128);
    ImpWs w = imp_carve(ws, ws_bytes, B, R);
    if (!ws || !w.ok) return imcui_set_err(h, IMCUI_ERR_WS, "imp: workspace too small (%zu < %zu)", ws_bytes, w.total);
    const ImpLayout l = imp_layout();
    const float* P = packed;
    const int S = 2 * B;
    int rc;

    hipLaunchKernelGGL(imp_pairs_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, n0, n1, B, w.cnt, w.active);
    hipLaunchKernelGGL(imp_reset_kernel, dim3(cdiv(R + 1, 256), B), dim3(256), 0, stream, ncap, R, w.u, w.vv, matches0, matches1, mscores0,
                       mscores1);
    hipLaunchKernelGGL(imp_init_kernel, dim3(R / 4, S), dim3(256), 0, stream, keypoints0, keypoints1, scores0, scores1, descriptors0,
                       descriptors1, w.cnt, ncap, R, w0, h0, w1, h1, P + l.k0, w.d128, w.ctx, w.one, w.zero);
    IMCUI_CHECK_LAUNCH(h);

    const bool split = h->precision == 1;
    auto base = [&](GemmP& g) {
        g.M = S * R;
        g.cnt = w.cnt;
        g.active = w.active;
        g.rows_per_seq = R;
    };
    auto wts = [&](GemmP& g, size_t wf32, const ImpSplit& sp) {
        g.W = P + wf32;
        if (split) {
            g.Wh = reinterpret_cast<const unsigned short*>(P + sp.h);
            g.Wl = reinterpret_cast<const unsigned short*>(P + sp.l);
            g.wscale = P + sp.s;
        }
    };
    // ---- key-point encoder layers 1..4 (layer 0 ran in imp_init_kernel): e32 -> e64 -> e128 -> e256 -> x
    {
        const float* src = w.ctx;
        float* bufs[2] = {w.hbuf, w.ctx};
        for (int i = 0; i < 4; ++i) {
            const int K = IMP_KENC[i + 1], N = IMP_KENC[i + 2];
            GemmP g;
            base(g);
            g.epi = (i < 3) ? EPI_RELU : EPI_BIAS;
            g.A = src;
            g.lda = K;
            g.K = K;
            g.N = N;
            wts(g, l.kw[i], l.ks[i]);
            g.ldw = K;
            g.bias = P + l.kb[i];
            g.C = (i < 3) ? bufs[i & 1] : w.x;
            g.ldc = (i < 3) ? N : 256;
            IMCUI_RUN(gemm_launch(h, g, stream));
            src = bufs[i & 1];
        }
    }
    {
        GemmP g;  // x += input_proj(desc): desc = input_proj(desc) + kenc(kpts, scores)
        base(g);
        g.epi = EPI_RESID;
        g.A = w.d128;
        g.lda = IMP_DESC;
        g.K = IMP_DESC;
        g.N = 256;
        wts(g, l.win, l.sin_);
        g.ldw = IMP_DESC;
        g.bias = P + l.bin_;
        g.C = w.x;
        g.ldc = 256;
        IMCUI_RUN(gemm_launch(h, g, stream));
    }
    // ---- attentional GNN: ['self', 'cross'] * 9, launch for launch as in superglue.hip
    for (int layer = 0; layer < IMP_LAYERS; ++layer) {
        const ImpLayerOff& o = l.L[layer];
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
        g.rope_cos = w.one;  // no rotary encoding: q * 1 + rotate_half(q) * 0
        g.rope_sin = w.zero;
        g.alpha = 0.125f * 1.44269504088896340736f;  // scores / 64 ** .5 and log2(e) folded into q
        g.heads = IMP_HEADS;
        IMCUI_RUN(gemm_launch(h, g, stream));
        AttnP a;
        a.Q = w.q;
        a.K = w.k;
        a.V = w.v;
        a.O = w.ctx;
        a.cnt = w.cnt;
        a.active = w.active;
        a.nseq = S;
        a.heads = IMP_HEADS;
        a.rows_per_seq = R;
        a.cross = layer & 1;
        a.log2_domain = 1;
        IMCUI_RUN(attention_launch(h, a, stream));
        if (split) {
            FfnP f;  // x += mlp.3(relu(bn(mlp.0(cat[x, merge(ctx)])))) as one kernel (merge and bn folded into mlp.0)
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
        GemmP f1;
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
        GemmP f2;
        base(f2);
        f2.epi = EPI_RESID;
        f2.A = w.hbuf;
        f2.lda = 512;
        f2.K = 512;
        f2.N = 256;
        wts(f2, o.w2, o.s2);
        f2.ldw = 512;
        f2.bias = P + o.b2;
        f2.C = w.x;
        f2.ldc = 256;
        IMCUI_RUN(gemm_launch(h, f2, stream));
    }
    {
        GemmP g;  // md = final_proj.8(x) / 256^(1/4): md0 . md1 = scores / 256 ** .5 (exact power of two)
        base(g);
        g.epi = EPI_BIAS;
        g.A = w.x;
        g.lda = 256;
        g.K = 256;
        g.N = 256;
        wts(g, l.wfinal, l.sfinal);
        g.ldw = 256;
        g.bias = P + l.bfinal;
        g.alpha = 0.25f;
        g.C = w.md;
        g.ldc = 256;
        IMCUI_RUN(gemm_launch(h, g, stream));
    }
    {
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
        IMCUI_RUN(gemm_launch(h, g, stream));
    }
    return imp_assign(h, w, B, ncap, R, P + l.bin, 0.0f, sinkhorn_iterations, (float)match_threshold, matches0, matches1, mscores0,
                      mscores1, stream);
}
