// SFD2 forward on MI355X (zoo entry sfd2 + NN-mutual; extractor conf sfd2): imcui/hloc/extractors/sfd2.py:35-44 around
// pram.nets.sfd2.load_sfd2(...).extract_local_global(...) as one batched call.  The network is NOT in the reference checkout
// (third_party is empty): it is restated in tests/sfd2_reference.py, and that file is the definition this one is tested against
// ("SFD2: what is pinned").
//
//   image       [B, 3, H, W] RGB in [0, 1]; tvf.Normalize(mean, std) per channel (sfd2.py:24-26) is applied where layer 0 READS the image
//               (two float32 roundings), so its zero padding is zero in normalised units; mean and std live in the packed header
//   conv1a      3 -> 64 on the VALU (stem3x3_kernel<64> with Sfd2StemLoad), folded BatchNorm, ReLU
//   trunk       SFD2_LAYERS: 3x3 layers on the shared implicit GEMM (stride 1 / 2), the 1x1 layers of the bottlenecks as plain GEMMs on
//               the NHWC map, folded BatchNorm, ReLU and the bottleneck's `+ identity` in the EPI_CONV epilogue (both arithmetic modes)
//   grouped 3x3 sfd2_gconv_kernel<CG>: fp32 on the VALU in both modes (18 FLOP per byte moved: a memory-bound pass)
//   heads       convPa and convDa read the same map: ONE launch with N = 2 x hidden (rows concatenated at pack time); convPb / convDb read
//               their half of that map (1x1: a plain GEMM with lda = 2 x hidden; 3x3: the implicit GEMM over all 2 x hidden channels with
//               zero weights on the other head's half)
//   score       sfd2_score_kernel: sigmoid and the 4x4 depth-to-space (channel c = 4 dy + dx) -> one float per pixel of the (4 Hc, 4 Wc) map
//   selection   imcui_hip_simple_nms radius 4; Sfd2Pred (score > threshold, border band against the IMAGE's H, W) counted once with conf_th;
//               sfd2_thr_kernel: an image with fewer than min_keypoints candidates gets threshold 0 (every NMS survivor inside the band);
//               select.h cand_list with the per-image threshold into a list that holds every score-map pixel, written in DESCENDING pixel
//               order so that cand_cut's (score, list index) key prefers the lower pixel among equal scores; ranked_rows with Sfd2Row:
//               descending score, equal scores by ascending pixel index
//   describe    the convDb map is L2-normalised over channels (sfd2_dnorm_kernel), then one wave per key-point: SuperPoint's
//               sample_descriptors with s = 4 (align_corners=True grid_sample, zero padding), d / max(|d|, 1e-12)
// Explicit float32 order in the decode and the sampler (build.py compiles this file with -ffp-contract=off), fixed summation orders, no
// float atomics, grids sized by shapes or capacities: a row's bits do not depend on its batch or on replay; no host synchronisation.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "imcui_hip.h"
#include "net_kernels.h"
#include "netpack.h"
#include "select.h"

#define SF_DIM 128          // descriptor width
#define SF_NSCORE 16        // score channels: a 4 x 4 depth-to-space
#define SF_MAGIC 21318.0f   // "SF"
#define SF_NCFG 12
#define SF_MIN_SIDE 16
#define SF_NMS_RADIUS 4
#define SF_MAX_BLOCKS 8

// ------------------------------------------------------------------ configuration (imcui_hip.h: the 12 ints of `cfg`)
struct SfCfg {
    int c1, c2, c3;  // trunk widths
    int nb, cg;      // bottlenecks of conv4, channels per group of their 3x3
    int ch;          // hidden width of either head
    int kpb, kdb;    // kernel size of convPb / convDb
    int bn, bias, blk_bias;  // BatchNorm behind the convolutions; bias on the trunk / head convolutions; bias on the bottleneck convolutions
};
static bool sf_cfg(const int* v, SfCfg* c) {
    if (!v) return false;
    c->c1 = v[0], c->c2 = v[1], c->c3 = v[2], c->nb = v[3], c->cg = v[4], c->ch = v[5], c->kpb = v[6], c->kdb = v[7], c->bn = v[8], c->bias = v[9], c->blk_bias = v[10];
    if (c->c1 != 64) return false;  // (layer 0 is stem3x3_kernel<64>)
    for (int w : {c->c2, c->c3, c->ch})
        if (w < 32 || w % 32 || w > 512) return false;
    if (c->nb < 0 || c->nb > SF_MAX_BLOCKS) return false;
    if (c->cg != 4 && c->cg != 8 && c->cg != 16) return false;
    if (c->c3 % (2 * c->cg)) return false;  // (a workgroup of the grouped kernel owns two groups)
    if ((c->kpb != 1 && c->kpb != 3) || (c->kdb != 1 && c->kdb != 3)) return false;
    return !(c->bn & ~1) && !(c->bias & ~1) && !(c->blk_bias & ~1) && v[11] == 0;
}

// ------------------------------------------------------------------ the layer table (the ONE place that states the backbone)
// kind: 0 layer 0 on the VALU, 1 3x3 on the implicit GEMM, 2 1x1 as a plain GEMM, 3 grouped 3x3, 4 the two heads' hidden 3x3 layers as one
// launch.  cin / cout name a width slot (0: the image's 3 channels, 1..3: c1..c3, 4: 2 x ch).  block: 0 trunk; 1 / 2 / 3 = first / middle /
// last launch of a bottleneck (the rows with block > 0 repeat nb times as conv4.{i}; the last adds the first's input before its ReLU).
enum { SF_STEM = 0, SF_CONV3 = 1, SF_PW = 2, SF_GROUP = 3, SF_HEADS = 4 };
struct SfRow {
    const char *conv, *bn;
    int kind, cin, cout, stride, block;
};
static const SfRow SFD2_LAYERS[] = {
    {"conv1a.0", "conv1a.1", SF_STEM, 0, 1, 1, 0},  {"conv1b.0", "conv1b.1", SF_CONV3, 1, 1, 2, 0}, {"conv2a.0", "conv2a.1", SF_CONV3, 1, 2, 1, 0},
    {"conv2b.0", "conv2b.1", SF_CONV3, 2, 2, 2, 0}, {"conv3a.0", "conv3a.1", SF_CONV3, 2, 3, 1, 0}, {"conv3b.0", "conv3b.1", SF_CONV3, 3, 3, 1, 0},
    {"conv1", "bn1", SF_PW, 3, 3, 1, 1},            {"conv2", "bn2", SF_GROUP, 3, 3, 1, 2},         {"conv3", "bn3", SF_PW, 3, 3, 1, 3},
    {"convPa.0+convDa.0", "", SF_HEADS, 3, 4, 1, 0},
};
struct SfLayer {
    std::string name, conv, bn;  // launch name; state-dict prefix of the convolution and of its BatchNorm
    int kind, cin, cout, stride, block;
};
static std::vector<SfLayer> sf_layers(const SfCfg& c) {
    const int width[5] = {3, c.c1, c.c2, c.c3, 2 * c.ch};
    constexpr size_t NROWS = sizeof(SFD2_LAYERS) / sizeof(SFD2_LAYERS[0]);
    std::vector<SfLayer> out;
    const auto push = [&](const SfRow& q, const std::string& pre) {
        out.push_back({pre + q.conv, pre + q.conv, pre + q.bn, q.kind, width[q.cin], width[q.cout], q.stride, q.block});
    };
    for (size_t r = 0; r < NROWS;) {
        if (!SFD2_LAYERS[r].block) {
            push(SFD2_LAYERS[r++], "");
            continue;
        }
        size_t e = r;  // the rows of a bottleneck leave together, nb times
        while (e < NROWS && SFD2_LAYERS[e].block) ++e;
        for (int i = 0; i < c.nb; ++i)
            for (size_t q = r; q < e; ++q) push(SFD2_LAYERS[q], "conv4." + std::to_string(i) + ".");
        r = e;
    }
    return out;
}

extern "C" int imcui_hip_sfd2_num_layers(const int* cfg) {
    SfCfg c;
    return sf_cfg(cfg, &c) ? (int)sf_layers(c).size() : 0;
}
// out5 = kind, cin, cout, stride, block; the name lives until the next call of this thread
extern "C" const char* imcui_hip_sfd2_layer(const int* cfg, int i, int* out5) {
    static thread_local std::string name;
    SfCfg c;
    if (!sf_cfg(cfg, &c)) return nullptr;
    const std::vector<SfLayer> L = sf_layers(c);
    if (i < 0 || i >= (int)L.size()) return nullptr;
    if (out5) out5[0] = L[i].kind, out5[1] = L[i].cin, out5[2] = L[i].cout, out5[3] = L[i].stride, out5[4] = L[i].block;
    name = L[i].name;
    return name.c_str();
}

static const char* const SF_BN_KEYS[4] = {"weight", "bias", "running_mean", "running_var"};
// the tensors of one convolution (+ BatchNorm): weight, bias when it has one, the four BatchNorm tensors (following each other)
static void sf_add_conv(TensorTable& t, const std::string& conv, const std::string& bn, size_t wn, int cout, bool bias, bool has_bn) {
    t.add(conv + ".weight", wn);
    if (bias) t.add(conv + ".bias", cout);
    if (has_bn)
        for (const char* s : SF_BN_KEYS) t.add(bn + "." + s, cout);
}
static TensorTable sf_tensors(const SfCfg& c) {
    TensorTable t;
    for (const SfLayer& L : sf_layers(c)) {
        if (L.kind == SF_HEADS) {
            sf_add_conv(t, "convPa.0", "convPa.1", (size_t)c.ch * c.c3 * 9, c.ch, c.bias, c.bn);
            sf_add_conv(t, "convDa.0", "convDa.1", (size_t)c.ch * c.c3 * 9, c.ch, c.bias, c.bn);
            continue;
        }
        const size_t wn = L.kind == SF_PW ? (size_t)L.cout * L.cin : L.kind == SF_GROUP ? (size_t)L.cout * c.cg * 9 : (size_t)L.cout * L.cin * 9;
        sf_add_conv(t, L.conv, L.bn, wn, L.cout, L.block ? c.blk_bias : c.bias, c.bn);
    }
    t.add("convPb.weight", (size_t)SF_NSCORE * c.ch * c.kpb * c.kpb);
    t.add("convPb.bias", SF_NSCORE);  // (zeros when the checkpoint has none: backend.pack_sfd2)
    t.add("convDb.weight", (size_t)SF_DIM * c.ch * c.kdb * c.kdb);
    t.add("convDb.bias", SF_DIM);
    return t;
}
extern "C" int imcui_hip_sfd2_num_tensors(const int* cfg) {
    SfCfg c;
    return sf_cfg(cfg, &c) ? sf_tensors(c).size() : 0;
}
extern "C" const char* imcui_hip_sfd2_tensor_name(const int* cfg, int i) {
    static thread_local std::string name;
    SfCfg c;
    if (!sf_cfg(cfg, &c)) return nullptr;
    const TensorTable t = sf_tensors(c);
    if (i < 0 || i >= t.size()) return nullptr;
    name = t.t[i].name;
    return name.c_str();
}

// ------------------------------------------------------------------ packed layout
// hdr [64]: magic, the 12 cfg values, mean [3] at 16, std [3] at 19.  w0 / b0: layer 0 for the VALU kernel [tap][cin 3][64] + [64].  Per
// layer of the table: a GEMM layer [cout][tap][cin] (3x3, heads), [cout][cin] (1x1), or the grouped layer gw [group][tap][ci][co] + gb
// [C].  pb / db: the heads' second layers (see the top of the file).  BatchNorm is folded everywhere.
struct SfLayout {
    size_t hdr, w0, b0;
    std::vector<GemmLayerOff> g;   // (GEMM layers; unused entries stay zero)
    std::vector<size_t> gw, gb;    // (grouped layers)
    GemmLayerOff pb, db;
    size_t total;
};
static int sf_head_k(const SfCfg& c, int k) { return k == 1 ? c.ch : 9 * 2 * c.ch; }
static SfLayout sf_layout(const SfCfg& c) {
    SfLayout l;
    PackCursor p;
    const std::vector<SfLayer> L = sf_layers(c);
    l.g.resize(L.size());
    l.gw.assign(L.size(), 0);
    l.gb.assign(L.size(), 0);
    l.hdr = p.get(64);
    l.w0 = p.get((size_t)27 * c.c1);
    l.b0 = p.get(c.c1);
    for (size_t i = 1; i < L.size(); ++i) {
        if (L[i].kind == SF_GROUP) {
            l.gw[i] = p.get((size_t)L[i].cout * c.cg * 9);
            l.gb[i] = p.get(L[i].cout);
        } else {
            l.g[i].place(p, L[i].cout, (L[i].kind == SF_PW ? 1 : 9) * L[i].cin);
        }
    }
    l.pb.place(p, SF_NSCORE, sf_head_k(c, c.kpb));
    l.db.place(p, SF_DIM, sf_head_k(c, c.kdb));
    l.total = p.off;
    return l;
}
extern "C" size_t imcui_hip_sfd2_packed_floats(const int* cfg) {
    SfCfg c;
    return sf_cfg(cfg, &c) ? sf_layout(c).total : 0;
}

// scale / shift of the (optional) BatchNorm behind convolution `conv`, with the (optional) convolution bias carried through it
static void sf_fold(const TensorTable& names, const float* const* t, const std::string& conv, const std::string& bn, int cout, bool bias, bool has_bn,
                    std::vector<float>& sc, std::vector<float>& sh) {
    sc.assign(cout, 1.0f);
    sh.assign(cout, 0.0f);
    if (has_bn) bn_fold_f32(t + names.find(bn + ".weight"), cout, sc, sh);
    if (bias) {
        const float* b = t[names.find(conv + ".bias")];
        for (int co = 0; co < cout; ++co) sh[co] = b[co] * sc[co] + sh[co];
    }
}

// t: host pointers of the tensors in imcui_hip_sfd2_tensor_name order (shapes checked by the caller)
extern "C" int imcui_hip_sfd2_pack_weights(const int* cfg, const float* const* t, float* packed) {
    SfCfg c;
    if (!sf_cfg(cfg, &c) || !t || !packed) return IMCUI_ERR_ARG;
    const TensorTable names = sf_tensors(c);
    for (int i = 0; i < names.size(); ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const SfLayout l = sf_layout(c);
    const std::vector<SfLayer> L = sf_layers(c);
    memset(packed, 0, l.total * sizeof(float));
    auto T = [&](const std::string& name) { return t[names.find(name)]; };
    packed[l.hdr] = SF_MAGIC;
    for (int i = 0; i < SF_NCFG; ++i) packed[l.hdr + 1 + i] = (float)cfg[i];
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};  // sfd2.py:24-26
    for (int i = 0; i < 3; ++i) packed[l.hdr + 16 + i] = mean[i], packed[l.hdr + 19 + i] = sd[i];
    std::vector<float> sc, sh, tmp;
    // a GEMM layer from OIHW weights: rows scaled by the fold, K order (tap, channel); row0 = first row of the layer it is written to
    auto put_gemm = [&](const GemmLayerOff& o, const float* w, int cout, int cin, int k, int K, int row0) {
        tmp.assign((size_t)cout * k * k * cin, 0.0f);
        pack_conv_gemm(w, cout, cin, k, cin, tmp.data());
        for (int co = 0; co < cout; ++co) {
            for (int q = 0; q < k * k * cin; ++q) packed[o.w + (size_t)(row0 + co) * K + q] = tmp[(size_t)co * k * k * cin + q] * sc[co];
            packed[o.b + row0 + co] = sh[co];
        }
    };
    for (size_t i = 0; i < L.size(); ++i) {
        const SfLayer& Y = L[i];
        if (Y.kind == SF_HEADS) {
            const char* heads[2][2] = {{"convPa.0", "convPa.1"}, {"convDa.0", "convDa.1"}};
            for (int v = 0; v < 2; ++v) {
                sf_fold(names, t, heads[v][0], heads[v][1], c.ch, c.bias, c.bn, sc, sh);
                put_gemm(l.g[i], T(std::string(heads[v][0]) + ".weight"), c.ch, c.c3, 3, 9 * c.c3, v * c.ch);
            }
            l.g[i].split_planes(packed, 2 * c.ch, 9 * c.c3);
            continue;
        }
        sf_fold(names, t, Y.conv, Y.bn, Y.cout, Y.block ? c.blk_bias : c.bias, c.bn, sc, sh);
        const float* w = T(Y.conv + ".weight");
        if (Y.kind == SF_STEM) {
            for (int co = 0; co < Y.cout; ++co)
                for (int ci = 0; ci < 3; ++ci)
                    for (int k = 0; k < 9; ++k) packed[l.w0 + ((size_t)k * 3 + ci) * Y.cout + co] = w[((size_t)co * 3 + ci) * 9 + k] * sc[co];
            memcpy(packed + l.b0, sh.data(), Y.cout * sizeof(float));
        } else if (Y.kind == SF_GROUP) {  // [C][CG][3][3] -> [group][tap][ci][co]
            const int CG = c.cg;
            for (int co = 0; co < Y.cout; ++co)
                for (int ci = 0; ci < CG; ++ci)
                    for (int k = 0; k < 9; ++k)
                        packed[l.gw[i] + (((size_t)(co / CG) * 9 + k) * CG + ci) * CG + co % CG] = w[((size_t)co * CG + ci) * 9 + k] * sc[co];
            memcpy(packed + l.gb[i], sh.data(), Y.cout * sizeof(float));
        } else {
            const int k = Y.kind == SF_PW ? 1 : 3;
            put_gemm(l.g[i], w, Y.cout, Y.cin, k, k * k * Y.cin, 0);
            l.g[i].split_planes(packed, Y.cout, k * k * Y.cin);
        }
    }
    // convPb / convDb: no BatchNorm; 1x1 reads its half through lda, 3x3 carries zeros on the other head's channels
    for (int v = 0; v < 2; ++v) {
        const int k = v ? c.kdb : c.kpb, n = v ? SF_DIM : SF_NSCORE, K = sf_head_k(c, k);
        const GemmLayerOff& o = v ? l.db : l.pb;
        const float *w = T(v ? "convDb.weight" : "convPb.weight"), *b = T(v ? "convDb.bias" : "convPb.bias");
        for (int co = 0; co < n; ++co) {
            for (int ci = 0; ci < c.ch; ++ci)
                for (int q = 0; q < k * k; ++q)
                    packed[o.w + (size_t)co * K + (k == 1 ? ci : q * 2 * c.ch + v * c.ch + ci)] = w[((size_t)co * c.ch + ci) * k * k + q];
            packed[o.b + co] = b[co];
        }
        o.split_planes(packed, n, K);
    }
    return IMCUI_OK;
}

namespace {

// tvf.Normalize per channel: (x - mean[c]) / std[c], one rounding each; ms = mean [3], std [3] in the packed header
struct Sfd2StemLoad {
    const float* ms;
    __device__ float operator()(const float* __restrict__ img, long b, int c, int h, int w, int yy, int xx) const {
        return __fdiv_rn(__fsub_rn(img[((b * 3 + c) * h + yy) * (long)w + xx], ms[c]), ms[3 + c]);
    }
};

// ------------------------------------------------------------------ grouped 3x3 convolution
// x [B, h, w, C] NHWC -> out [B, h, w, C]: 3x3, pad 1, groups of CG channels (CG in, CG out), folded BatchNorm, optional ReLU.
// Grid (cdiv(w, 16) * cdiv(h, 16), C / (2 CG), B), 256 threads: a workgroup owns a 16 x 16 pixel tile of two groups.  The 18 x 18 pixel
// tile of their 2 CG input channels is staged in LDS with 16-byte accesses, channels innermost, the pixel stride padded by one float4
// (an odd number of float4s for CG = 4, 8, 16: the per-pixel float4 reads of a wave fall on distinct bank groups).  A thread owns one
// pixel and walks the two groups; the group's weights [tap][ci][co] are wave-uniform and come through the scalar cache.  Per output one
// fmaf chain starting at the folded shift, in ascending (tap, input channel) order.  A map smaller than the tile runs the same code
// (pixels outside are staged as zero -- the padding -- and not written).
template <int CG>
__global__ __launch_bounds__(256) void sfd2_gconv_kernel(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ shift,
                                                         float* __restrict__ out, int h, int w, int C, int tiles_x, int relu) {
    constexpr int CS = 2 * CG, PS = CS + 4, TW = 18, Q = CS / 4;
    __shared__ __attribute__((aligned(16))) float tile[TW * TW * PS];
    const int b = blockIdx.z, slice = blockIdx.y, ty0 = (blockIdx.x / tiles_x) * 16, tx0 = (blockIdx.x % tiles_x) * 16, tid = threadIdx.x;
    const float* xb = x + (long)b * h * w * C + slice * CS;
    for (int e = tid; e < TW * TW * Q; e += 256) {
        const int pp = e / Q, q = e - pp * Q, py = pp / TW, px = pp - py * TW;
        const int gy = ty0 + py - 1, gx = tx0 + px - 1;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = *reinterpret_cast<const float4*>(xb + ((long)gy * w + gx) * C + 4 * q);
        *reinterpret_cast<float4*>(tile + pp * PS + 4 * q) = v;
    }
    __syncthreads();
    const int ly = tid >> 4, lx = tid & 15, y = ty0 + ly, xx = tx0 + lx;
    if (y >= h || xx >= w) return;
    float* o = out + (((long)b * h + y) * w + xx) * C + slice * CS;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const float* wg = wt + (long)(slice * 2 + g) * 9 * CG * CG;
        float acc[CG];
#pragma unroll
        for (int co = 0; co < CG; ++co) acc[co] = shift[slice * CS + g * CG + co];
#pragma unroll(CG <= 8 ? 9 : 1)  // (16 channels per group: 2304 weights per tap walk would fill the register file)
        for (int t = 0; t < 9; ++t) {
            const float* p = tile + ((ly + t / 3) * TW + lx + t % 3) * PS + g * CG;
            float in[CG];
#pragma unroll
            for (int q = 0; q < CG / 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(p + 4 * q);
                in[4 * q] = v.x, in[4 * q + 1] = v.y, in[4 * q + 2] = v.z, in[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int ci = 0; ci < CG; ++ci)
#pragma unroll
                for (int co = 0; co < CG; ++co) acc[co] = fmaf(in[ci], wg[(t * CG + ci) * CG + co], acc[co]);
        }
#pragma unroll
        for (int q = 0; q < CG / 4; ++q) {
            float4 v = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
            if (relu) v = max4(v, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            *reinterpret_cast<float4*>(o + g * CG + 4 * q) = v;
        }
    }
}

// ------------------------------------------------------------------ score decode
// logits [B, Hc, Wc, 16] -> score [B, 4 Hc, 4 Wc]: pixel (4 cy + dy, 4 cx + dx) = sigmoid(logit 4 dy + dx of cell (cy, cx)) with
// sigmoid(v) = 1 / (1 + exp(-v)): a negation, expf, a sum, a quotient, each rounded once.  One thread per pixel.
__global__ __launch_bounds__(256) void sfd2_score_kernel(const float* __restrict__ logits, int Hc, int Wc, float* __restrict__ score, long npix) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int Ws = 4 * Wc, Hs = 4 * Hc;
    const int x = (int)(p % Ws);
    const long q = p / Ws;
    const int y = (int)(q % Hs);
    const long b = q / Hs;
    const float v = logits[((b * Hc + (y >> 2)) * Wc + (x >> 2)) * SF_NSCORE + 4 * (y & 3) + (x & 3)];
    score[p] = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-v)));
}

// ------------------------------------------------------------------ selection
// nms score > the image's threshold, inside the border band of the IMAGE (H x W; the map is Hs x Ws >= it): strict, as upstream's
struct Sfd2Pred {
    int Ws, H, W, border;
    float thr;
    const float* eff;  // per-image threshold, or null: thr for every image
    __device__ void bind(int b) {
        if (eff) thr = eff[b];
    }
    __device__ bool operator()(const float* img, int idx) const {
        const int y = idx / Ws, x = idx - y * Ws;
        return img[idx] > thr && y >= border && y < H - border && x >= border && x < W - border;
    }
};
// the min_keypoints fallback: an image with fewer than min_keypoints candidates at conf_th is selected again with threshold 0
__global__ void sfd2_thr_kernel(const int* __restrict__ total, int B, int min_keypoints, float conf_th, float* __restrict__ eff) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) eff[b] = total[b] < min_keypoints ? 0.0f : conf_th;
}
// the candidate list in DESCENDING pixel order (candidate number pos of n goes to slot n - 1 - pos): cand_cut's key (score, slot) then
// keeps, among equal scores, the LOWER pixel indices.  The list holds every pixel, so no slot is out of range.
struct Sfd2Emit {
    float* cscore;
    int* cidx;
    int ccap;
    const int* total;
    __device__ void operator()(int b, int pos, int idx, float v) const {
        const int slot = total[b] - 1 - pos;
        cscore[(long)b * ccap + slot] = v;
        cidx[(long)b * ccap + slot] = idx;
    }
};
// The rows of ranked_rows_kernel turned round: ascending rank r of n -> output row n - 1 - r, i.e. descending score and, among equal
// scores, descending slot = ascending pixel.  (x, y) of the pixel on the Ws-wide map and its score.  Rows past the count are zero.
struct Sfd2Row {
    const int *cidx, *nkept;
    int np, Ws, kout;
    float *kpts, *scores;
    __device__ void clear(int b, int lo, int hi) const {
        const int i = lo + threadIdx.x;
        if (i >= hi) return;
        float* kp = kpts + (long)b * kout * 2;
        kp[2 * i] = kp[2 * i + 1] = scores[(long)b * kout + i] = 0.0f;
    }
    __device__ void emit(int b, int i0, int m, const int* ks, const int* rank, const float* cs) const {
        const int j = threadIdx.x;
        if (j >= m) return;
        const int n = min(nkept[b], kout);
        const int slot = ks[i0 + j], r = n - 1 - rank[j], pix = cidx[(long)b * np + slot];
        float* kp = kpts + (long)b * kout * 2;
        kp[2 * r] = (float)(pix % Ws);
        kp[2 * r + 1] = (float)(pix / Ws);
        scores[(long)b * kout + r] = cs[slot];
    }
};

// ------------------------------------------------------------------ descriptors
// F.normalize over the 128 channels of every pixel of dmap [npix, 128], in place: one wave per pixel, lane l owns channels 2 l, 2 l + 1
__global__ __launch_bounds__(256) void sfd2_dnorm_kernel(float* __restrict__ dmap, long npix) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix) return;  // (wave-uniform)
    float2* q = reinterpret_cast<float2*>(dmap + p * SF_DIM + 2 * lane);
    const float2 v = *q;
    const float nrm = fmaxf(sqrtf(wave_sum(v.x * v.x + v.y * v.y)), 1e-12f);
    *q = make_float2(__fdiv_rn(v.x, nrm), __fdiv_rn(v.y, nrm));
}

// One wave per key-point row (grid (cdiv(kcap, 4), B)): SuperPoint's sample_descriptors with s = 4 on the normalised map dmap [B, h, w, 128]:
//   g = ((k - 2) + 0.5) / (size * 4 - 2 - 0.5) * 2 - 1;  i = ((g + 1) / 2) * (size - 1)  (ATen, align_corners=True)
//   corners floor(i), floor(i) + 1 with ATen's weights (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0), (ix - x0)(iy - y0); a corner outside
//   the map contributes zero; ((nw w_nw + ne w_ne) + sw w_sw) + se w_se, every product and sum rounded once; d / max(|d|, 1e-12).
// Lane l owns channels 2 l, 2 l + 1.  Rows past the count (nkpts[b]) are zero.
__global__ __launch_bounds__(256) void sfd2_describe_kernel(const float* __restrict__ dmap, int h, int w, const float* __restrict__ kpts,
                                                            const int* __restrict__ nkpts, int kcap, float* __restrict__ desc) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= kcap) return;  // (wave-uniform)
    float* o = desc + ((long)b * kcap + i) * SF_DIM + 2 * lane;
    if (i >= min(nkpts[b], kcap)) {
        *reinterpret_cast<float2*>(o) = make_float2(0.0f, 0.0f);
        return;
    }
    const float* kp = kpts + ((long)b * kcap + i) * 2;
    const float dx = __fsub_rn(__fsub_rn(__fmul_rn((float)w, 4.0f), 2.0f), 0.5f), dy = __fsub_rn(__fsub_rn(__fmul_rn((float)h, 4.0f), 2.0f), 0.5f);
    const float gx = __fsub_rn(__fmul_rn(__fdiv_rn(__fadd_rn(__fsub_rn(kp[0], 2.0f), 0.5f), dx), 2.0f), 1.0f);
    const float gy = __fsub_rn(__fmul_rn(__fdiv_rn(__fadd_rn(__fsub_rn(kp[1], 2.0f), 0.5f), dy), 2.0f), 1.0f);
    const float ix = __fmul_rn(__fdiv_rn(__fadd_rn(gx, 1.0f), 2.0f), (float)(w - 1)), iy = __fmul_rn(__fdiv_rn(__fadd_rn(gy, 1.0f), 2.0f), (float)(h - 1));
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float ax = __fsub_rn(__fadd_rn(fx, 1.0f), ix), bx = __fsub_rn(ix, fx), ay = __fsub_rn(__fadd_rn(fy, 1.0f), iy), by = __fsub_rn(iy, fy);
    const float wnw = __fmul_rn(ax, ay), wne = __fmul_rn(bx, ay), wsw = __fmul_rn(ax, by), wse = __fmul_rn(bx, by);
    const float* mb = dmap + (long)b * h * w * SF_DIM + 2 * lane;
    const auto at = [&](int yy, int xx) {
        return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? *reinterpret_cast<const float2*>(mb + ((long)yy * w + xx) * SF_DIM) : make_float2(0.0f, 0.0f);
    };
    const float2 nw = at(y0, x0), ne = at(y0, x1), sw = at(y1, x0), se = at(y1, x1);
    const float d0 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(nw.x, wnw), __fmul_rn(ne.x, wne)), __fmul_rn(sw.x, wsw)), __fmul_rn(se.x, wse));
    const float d1 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(nw.y, wnw), __fmul_rn(ne.y, wne)), __fmul_rn(sw.y, wsw)), __fmul_rn(se.y, wse));
    const float nrm = fmaxf(sqrtf(wave_sum(d0 * d0 + d1 * d1)), 1e-12f);
    *reinterpret_cast<float2*>(o) = make_float2(__fdiv_rn(d0, nrm), __fdiv_rn(d1, nrm));
}

}  // namespace

// ------------------------------------------------------------------ host: launches
static int sf_down(int n) { return (n - 1) / 2 + 1; }  // rows / columns behind a stride-2 layer (3x3, pad 1)

// a k x k convolution (pad k / 2; k = 1: a plain GEMM on the NHWC map with row stride lda) + folded bias (+ resid) (+ ReLU)
static int sf_gemm(imcui_hip_t* h, const float* P, const GemmLayerOff& o, const float* in, long lda, float* out, int B, int hin, int win, int cin, int cout,
                   int k, int stride, const float* resid, int act, hipStream_t stream) {
    const int ho = stride == 2 ? sf_down(hin) : hin, wo = stride == 2 ? sf_down(win) : win;
    GemmP g;
    g.epi = EPI_CONV;
    g.A = in;
    g.lda = lda;
    gemm_set_weights(g, P, o, cout, k * k * cin, h->precision == 1);
    if (k == 3) gemm_set_conv(g, 3, stride, 1, hin, win, ho, wo, cin);
    g.M = B * ho * wo;
    g.C = out;
    g.ldc = cout;
    g.resid = resid;
    g.ldr = cout;
    g.act = act;
    return gemm_launch(h, g, stream);
}

static int sf_gconv(imcui_hip_t* h, const float* x, const float* wt, const float* shift, float* out, int B, int hh, int ww, int C, int cg, int relu,
                    hipStream_t stream) {
    const int tx = cdiv(ww, 16), ty = cdiv(hh, 16);
    if (C % (2 * cg) || C / (2 * cg) > 65535 || B > 65535) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: grouped convolution with C=%d, %d channels per group, B=%d", C, cg, B);
    const dim3 grid(tx * ty, C / (2 * cg), B);
    if (cg == 8)
        hipLaunchKernelGGL(sfd2_gconv_kernel<8>, grid, dim3(256), 0, stream, x, wt, shift, out, hh, ww, C, tx, relu);
    else if (cg == 4)
        hipLaunchKernelGGL(sfd2_gconv_kernel<4>, grid, dim3(256), 0, stream, x, wt, shift, out, hh, ww, C, tx, relu);
    else if (cg == 16)
        hipLaunchKernelGGL(sfd2_gconv_kernel<16>, grid, dim3(256), 0, stream, x, wt, shift, out, hh, ww, C, tx, relu);
    else
        return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: the grouped convolution is built for 4 / 8 / 16 channels per group, not %d", cg);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// the floats of the largest map the entries [first, last] of the launch list write for B maps of hin x win at entry `first`
static size_t sf_run_floats(const std::vector<SfLayer>& L, int first, int last, int B, int hin, int win) {
    size_t m = 0;
    int hh = hin, ww = win;
    for (int i = first; i <= last; ++i) {
        if (L[i].stride == 2) hh = sf_down(hh), ww = sf_down(ww);
        m = std::max(m, (size_t)B * hh * ww * L[i].cout);
    }
    return m;
}

// Entries [first, last] of the launch list on `in` (the planar image when first == 0, else the NHWC map [B, hh, ww, cin of `first`]);
// every entry writes the one of buf[0..2] that is neither its input nor the pending residual.  -> the last entry's output, *hh / *ww its size
static int sf_run(imcui_hip_t* h, const SfCfg& c, const SfLayout& l, const std::vector<SfLayer>& L, const float* P, int first, int last, const float* in, int B,
                  int* hh, int* ww, float* const buf[3], int dbg_layer, float* dbg_map, const float** result, hipStream_t stream) {
    const float *cur = in, *blockin = nullptr;
    int rc;
    for (int i = first; i <= last; ++i) {
        const SfLayer& Y = L[i];
        if (Y.block == 1) blockin = cur;
        const float* resid = Y.block == 3 ? blockin : nullptr;
        if (Y.block == 3 && !resid) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: entry %d closes a bottleneck whose first entry is not part of the run", i);
        float* dst = nullptr;
        for (int k = 0; k < 3 && !dst; ++k)
            if (buf[k] != cur && buf[k] != blockin) dst = buf[k];
        if (Y.kind == SF_STEM) {
            const long npix = (long)B * *hh * *ww;
            hipLaunchKernelGGL((stem3x3_kernel<64, Sfd2StemLoad>), dim3(blocks_256(npix)), dim3(256), 0, stream, cur, P + l.w0, P + l.b0, dst, *hh, *ww,
                               Sfd2StemLoad{P + l.hdr + 16}, npix);
            IMCUI_CHECK_LAUNCH(h);
        } else if (Y.kind == SF_GROUP) {
            IMCUI_RUN(sf_gconv(h, cur, P + l.gw[i], P + l.gb[i], dst, B, *hh, *ww, Y.cout, c.cg, 1, stream));
        } else {
            const int k = Y.kind == SF_PW ? 1 : 3;
            IMCUI_RUN(sf_gemm(h, P, l.g[i], cur, Y.cin, dst, B, *hh, *ww, Y.cin, Y.cout, k, Y.stride, resid, 1, stream));
        }
        if (Y.stride == 2) *hh = sf_down(*hh), *ww = sf_down(*ww);
        if (Y.block == 3) blockin = nullptr;
        cur = dst;
        if (i == dbg_layer) copy_if(dbg_map, cur, (size_t)B * *hh * *ww * Y.cout * sizeof(float), stream);
    }
    *result = cur;
    return IMCUI_OK;
}

struct SfSel {
    float *nms, *eff;
    CandScan scan;
    ScoreIndexList cand;  // (holds every score-map pixel)
    CutList cut;
};
static void sf_carve_sel(WsAlloc& a, SfSel& s, int B, int np) {
    s.nms = a.get<float>((size_t)B * np);
    s.eff = a.get<float>(B);
    s.scan.carve(a, B, (size_t)np);
    s.cand.carve(a, B, np);
    s.cut.carve(a, B, np);
}
struct SfSelConf {
    float conf_th;
    int remove_borders, min_keypoints, max_keypoints;
};
static int sf_sel_check(imcui_hip_t* h, const SfSelConf& s, int np, int kout) {
    if (s.max_keypoints < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: max_keypoints=%d is negative (0 keeps every key-point)", s.max_keypoints);
    if (s.remove_borders < 0 || s.min_keypoints < 0)
        return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: remove_borders=%d, min_keypoints=%d (both >= 0)", s.remove_borders, s.min_keypoints);
    if (!(s.conf_th >= 0.0f)) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: conf_th=%g (>= 0: the fallback selects with threshold 0)", (double)s.conf_th);
    const int need = s.max_keypoints > 0 ? std::min(s.max_keypoints, np) : np;
    if (kout < need || kout < 1) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: kout=%d below min(max_keypoints or all, %d pixels) = %d", kout, np, need);
    return IMCUI_OK;
}
// NMS, the first count, the per-image threshold, the list, the cut, the ranked rows: score [B, Hs, Ws] of H x W images
static int sf_select(imcui_hip_t* h, const SfSel& s, const float* score, int B, int Hs, int Ws, int H, int W, const SfSelConf& sc, int kout, float* keypoints,
                     float* scores, int* num_keypoints, int* status, hipStream_t stream) {
    const int np = Hs * Ws;
    int rc;
    IMCUI_RUN(imcui_hip_simple_nms(h, score, s.nms, B, Hs, Ws, SF_NMS_RADIUS, stream));
    cand_count_scan(stream, s.nms, np, B, Sfd2Pred{Ws, H, W, sc.remove_borders, sc.conf_th, nullptr}, s.scan);
    hipLaunchKernelGGL(sfd2_thr_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, s.scan.total, B, sc.min_keypoints, sc.conf_th, s.eff);
    cand_list(stream, s.nms, np, B, Sfd2Pred{Ws, H, W, sc.remove_borders, sc.conf_th, s.eff}, s.scan, np, Sfd2Emit{s.cand.cscore, s.cand.cidx, np, s.scan.total});
    cand_cut(stream, s.cand.cscore, s.scan.total, np, sc.max_keypoints, s.cut, status, B);
    ranked_rows(stream, s.cand.cscore, np, s.cut, kout, num_keypoints, Sfd2Row{s.cand.cidx, s.cut.nkept, np, Ws, kout, keypoints, scores}, B);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

static void sf_score(const float* logits, int B, int Hc, int Wc, float* score, hipStream_t stream) {
    const long npix = (long)B * 16 * Hc * Wc;
    hipLaunchKernelGGL(sfd2_score_kernel, dim3(blocks_256(npix)), dim3(256), 0, stream, logits, Hc, Wc, score, npix);
}
static void sf_describe(const float* dmap, int h4, int w4, const float* kpts, const int* nkpts, int kcap, int B, float* desc, hipStream_t stream) {
    hipLaunchKernelGGL(sfd2_describe_kernel, dim3(cdiv(kcap, 4), B), dim3(256), 0, stream, dmap, h4, w4, kpts, nkpts, kcap, desc);
}

struct SfWs {
    float *buf[3], *logits, *dmap, *score;
    SfSel sel;
    int* status;
    size_t total;
    bool ok;
};
// `run` floats per rotating buffer; Hc x Wc cells (0: no head maps, the layer probe)
static SfWs sf_carve(void* ws, size_t bytes, size_t run, int B, int Hc, int Wc, bool sel) {
    WsAlloc a(ws, bytes);
    SfWs s;
    memset(&s, 0, sizeof s);
    for (int k = 0; k < 3; ++k) s.buf[k] = a.get<float>(run);
    const size_t nc = (size_t)B * Hc * Wc;
    s.logits = a.get<float>(nc * SF_NSCORE);
    s.dmap = a.get<float>(nc * SF_DIM);
    s.score = a.get<float>(nc * 16);
    if (sel) sf_carve_sel(a, s.sel, B, 16 * Hc * Wc);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

static int sf_check(imcui_hip_t* h, int B, int H, int W) {
    if (B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: B=%d above 1024", B);
    if (H < SF_MIN_SIDE || W < SF_MIN_SIDE)
        return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: H=%d W=%d: every side needs at least %d pixels (the 1/4-resolution maps and the border band need them)", H, W,
                             SF_MIN_SIDE);
    // int indices: the 64-channel full-resolution map is the largest of the batch (512 channels at 1/16 of the pixels are half of it)
    if (((long)H + 3) * ((long)W + 3) * 64 > 0x7fffffffL / B) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: B=%d images of %dx%d exceed the 2^31 index range of one call", B, H, W);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_sfd2_workspace_bytes(const int* cfg, int B, int H, int W) {
    SfCfg c;
    if (!sf_cfg(cfg, &c) || B <= 0 || B > 1024 || H < SF_MIN_SIDE || W < SF_MIN_SIDE) return 0;
    const std::vector<SfLayer> L = sf_layers(c);
    return sf_carve(nullptr, 0, sf_run_floats(L, 0, (int)L.size() - 1, B, H, W), B, sf_down(sf_down(H)), sf_down(sf_down(W)), true).total;
}

// the heads behind the merged hidden map hid [B, Hc, Wc, 2 ch]: logits [.., 16], dmap [.., 128] (raw: normalised by the caller)
static int sf_heads(imcui_hip_t* h, const SfCfg& c, const SfLayout& l, const float* P, const float* hid, int B, int Hc, int Wc, float* logits, float* dmap,
                    hipStream_t stream) {
    int rc;
    if (c.kpb == 1)
        IMCUI_RUN(sf_gemm(h, P, l.pb, hid, 2 * c.ch, logits, B, Hc, Wc, c.ch, SF_NSCORE, 1, 1, nullptr, 0, stream));
    else
        IMCUI_RUN(sf_gemm(h, P, l.pb, hid, 2 * c.ch, logits, B, Hc, Wc, 2 * c.ch, SF_NSCORE, 3, 1, nullptr, 0, stream));
    if (c.kdb == 1) return sf_gemm(h, P, l.db, hid + c.ch, 2 * c.ch, dmap, B, Hc, Wc, c.ch, SF_DIM, 1, 1, nullptr, 0, stream);
    return sf_gemm(h, P, l.db, hid, 2 * c.ch, dmap, B, Hc, Wc, 2 * c.ch, SF_DIM, 3, 1, nullptr, 0, stream);
}

extern "C" int imcui_hip_sfd2_forward(imcui_hip_t* h, const int* cfg, const float* packed, const float* image, int B, int C, int H, int W, float conf_th,
                                      int remove_borders, int min_keypoints, int max_keypoints, int kout, float* keypoints, float* scores, float* descriptors,
                                      int* num_keypoints, int* status, float* dbg_score, float* dbg_desc, int dbg_layer, float* dbg_map, void* ws, size_t ws_bytes,
                                      void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    SfCfg c;
    if (!sf_cfg(cfg, &c))
        return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: configuration refused (c1 = 64, widths multiples of 32 up to 512, up to %d bottlenecks, 4 / 8 / 16 channels per group, convPb / convDb 1x1 or 3x3)", SF_MAX_BLOCKS);
    if (C != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: %d image channels; the network reads RGB (3)", C);
    int rc;
    IMCUI_RUN(sf_check(h, B, H, W));
    const int Hc = sf_down(sf_down(H)), Wc = sf_down(sf_down(W)), Hs = 4 * Hc, Ws = 4 * Wc;
    const SfSelConf sc{conf_th, remove_borders, min_keypoints, max_keypoints};
    IMCUI_RUN(sf_sel_check(h, sc, Hs * Ws, kout));
    if (!packed || !image || !keypoints || !scores || !descriptors || !num_keypoints) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2: null argument");
    const SfLayout l = sf_layout(c);
    const std::vector<SfLayer> L = sf_layers(c);
    const int nl = (int)L.size();
    SfWs s = sf_carve(ws, ws_bytes, sf_run_floats(L, 0, nl - 1, B, H, W), B, Hc, Wc, true);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "sfd2: workspace too small (%zu < %zu)", ws_bytes, s.total);
    int* st = status ? status : s.status;
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, st, 1);
    // ---- trunk, bottlenecks, the heads' hidden layers: the launch list
    int hh = H, ww = W;
    const float* hid = nullptr;
    IMCUI_RUN(sf_run(h, c, l, L, packed, 0, nl - 1, image, B, &hh, &ww, s.buf, dbg_layer, dbg_map, &hid, stream));
    // ---- heads, score, descriptors map
    IMCUI_RUN(sf_heads(h, c, l, packed, hid, B, Hc, Wc, s.logits, s.dmap, stream));
    sf_score(s.logits, B, Hc, Wc, s.score, stream);
    const long ncell = (long)B * Hc * Wc;
    hipLaunchKernelGGL(sfd2_dnorm_kernel, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, stream, s.dmap, ncell);
    IMCUI_CHECK_LAUNCH(h);
    copy_if(dbg_score, s.score, (size_t)B * Hs * Ws * sizeof(float), stream);
    copy_if(dbg_desc, s.dmap, (size_t)ncell * SF_DIM * sizeof(float), stream);
    // ---- selection and descriptors
    IMCUI_RUN(sf_select(h, s.sel, s.score, B, Hs, Ws, H, W, sc, kout, keypoints, scores, num_keypoints, st, stream));
    sf_describe(s.dmap, Hc, Wc, keypoints, num_keypoints, kout, B, descriptors, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ test entries
static bool sf_probe_shape(int B, int H, int W, int C) { return B >= 1 && B <= 1024 && H >= 1 && W >= 1 && C >= 1 && ((long)H + 3) * ((long)W + 3) * C <= 0x7fffffffL / B; }

// the grouped convolution alone: x [B, H, W, C] NHWC, w_packed [group][tap][ci][co] (the packed order; backend.sfd2_pack_group makes it
// from OIHW), shift [C] -> out [B, H, W, C]
extern "C" int imcui_hip_sfd2_gconv_probe(imcui_hip_t* h, const float* x, const float* w_packed, const float* shift, int B, int H, int W, int C, int cg, int relu,
                                          float* out, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    if (!sf_probe_shape(B, H, W, C) || !x || !w_packed || !shift || !out) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2 gconv probe: shape or null argument");
    return sf_gconv(h, x, w_packed, shift, out, B, H, W, C, cg, relu, (hipStream_t)stream_);
}

extern "C" size_t imcui_hip_sfd2_layers_workspace_bytes(const int* cfg, int first, int last, int B, int H, int W) {
    SfCfg c;
    if (!sf_cfg(cfg, &c) || B <= 0 || H < 1 || W < 1) return 0;
    const std::vector<SfLayer> L = sf_layers(c);
    if (first < 0 || last < first || last >= (int)L.size()) return 0;
    return sf_carve(nullptr, 0, sf_run_floats(L, first, last, B, H, W), B, 0, 0, false).total;
}
// entries [first, last] of the forward's own launch list on `in`: the planar image [B, 3, H, W] when first == 0, else the NHWC map
// [B, H, W, cin of entry first] -> out (the last entry's NHWC map)
extern "C" int imcui_hip_sfd2_layers_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* in, int first, int last, int B, int H, int W,
                                           float* out, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    SfCfg c;
    if (!sf_cfg(cfg, &c)) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2 layers probe: configuration refused");
    const std::vector<SfLayer> L = sf_layers(c);
    if (first < 0 || last < first || last >= (int)L.size() || !sf_probe_shape(B, H, W, 512) || !packed || !in || !out)
        return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2 layers probe: entries [%d, %d] of %d, shape or null argument", first, last, (int)L.size());
    SfWs s = sf_carve(ws, ws_bytes, sf_run_floats(L, first, last, B, H, W), B, 0, 0, false);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "sfd2 layers probe: workspace too small (%zu < %zu)", ws_bytes, s.total);
    int hh = H, ww = W, rc;
    const float* res = nullptr;
    IMCUI_RUN(sf_run(h, c, sf_layout(c), L, packed, first, last, in, B, &hh, &ww, s.buf, -1, nullptr, &res, stream));
    copy_if(out, res, (size_t)B * hh * ww * L[last].cout * sizeof(float), stream);
    return IMCUI_OK;
}

// the score decode alone: logits [B, Hc, Wc, 16] -> score [B, 4 Hc, 4 Wc]
extern "C" int imcui_hip_sfd2_score_probe(imcui_hip_t* h, const float* logits, int B, int Hc, int Wc, float* score, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    if (!sf_probe_shape(B, Hc, Wc, 16) || !logits || !score) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2 score probe: shape or null argument");
    sf_score(logits, B, Hc, Wc, score, (hipStream_t)stream_);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_sfd2_select_workspace_bytes(int B, int Hs, int Ws) {
    if (!sf_probe_shape(B, Hs, Ws, 1)) return 0;
    WsAlloc a(nullptr, 0);
    SfSel s;
    sf_carve_sel(a, s, B, Hs * Ws);
    return a.off;
}
// NMS, fallback, cut and ranked rows on a given score map [B, Hs, Ws] of H x W images (H <= Hs, W <= Ws); nms_map (optional) [B, Hs, Ws],
// num_candidates (optional) [B] = the candidates of the list that was cut, eff (optional) [B] = the per-image threshold
extern "C" int imcui_hip_sfd2_select_probe(imcui_hip_t* h, const float* score, int B, int Hs, int Ws, int H, int W, float conf_th, int remove_borders,
                                           int min_keypoints, int max_keypoints, int kout, float* keypoints, float* scores, int* num_keypoints, int* num_candidates,
                                           float* eff, int* status, float* nms_map, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (!sf_probe_shape(B, Hs, Ws, 1) || H < 1 || W < 1 || H > Hs || W > Ws) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2 select probe: map %dx%d of a %dx%d image, B=%d", Hs, Ws, H, W, B);
    const SfSelConf sc{conf_th, remove_borders, min_keypoints, max_keypoints};
    int rc;
    IMCUI_RUN(sf_sel_check(h, sc, Hs * Ws, kout));
    if (!score || !keypoints || !scores || !num_keypoints || !status) return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2 select probe: null argument");
    WsAlloc a(ws, ws_bytes);
    SfSel s;
    sf_carve_sel(a, s, B, Hs * Ws);
    if (!ws || !a.ok) return imcui_set_err(h, IMCUI_ERR_WS, "sfd2 select probe: workspace too small (%zu < %zu)", ws_bytes, a.off);
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, status, 1);
    IMCUI_RUN(sf_select(h, s, score, B, Hs, Ws, H, W, sc, kout, keypoints, scores, num_keypoints, status, stream));
    copy_if(nms_map, s.nms, (size_t)B * Hs * Ws * sizeof(float), stream);
    copy_if(num_candidates, s.scan.total, (size_t)B * sizeof(int), stream);
    copy_if(eff, s.eff, (size_t)B * sizeof(float), stream);
    return IMCUI_OK;
}

// describe on a given map dmap [B, h4, w4, 128] (normalised here when `normalise`, in a copy: dmap_out [B, h4, w4, 128]) at keypoints
// [B, K, 2] (x, y in image pixels), nkpts [B] -> [B, K, 128]
extern "C" int imcui_hip_sfd2_describe_probe(imcui_hip_t* h, const float* dmap, int B, int h4, int w4, int normalise, float* dmap_out, const float* keypoints,
                                             const int* nkpts, int K, float* descriptors, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (!sf_probe_shape(B, h4, w4, SF_DIM) || K < 1 || !dmap || !keypoints || !nkpts || !descriptors || (normalise && !dmap_out))
        return imcui_set_err(h, IMCUI_ERR_ARG, "sfd2 describe probe: shape, K < 1 or null argument");
    const float* m = dmap;
    if (normalise) {
        const long ncell = (long)B * h4 * w4;
        hipMemcpyAsync(dmap_out, dmap, (size_t)ncell * SF_DIM * sizeof(float), hipMemcpyDeviceToDevice, stream);
        hipLaunchKernelGGL(sfd2_dnorm_kernel, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, stream, dmap_out, ncell);
        m = dmap_out;
    }
    sf_describe(m, h4, w4, keypoints, nkpts, K, B, descriptors, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
