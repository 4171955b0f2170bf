// DeDoDe forward on MI355X (zoo entry dedode: `feature: dedode` + Dual-Softmax): the extraction of imcui/hloc/extractors/dedode.py:55-86
// -- transforms.Normalize, dedode_detector_L.detect(num_keypoints), dedode_descriptor_B.describe_keypoints, to_pixel_coords -- as one
// batched call.  Upstream's package (Parskatt/DeDoDe) is restated from its description (tests/dedode_reference.py), parity-unpinned.
//
// Both models: a VGG-BN encoder (detector vgg19_bn.features[:40], descriptor vgg11_bn.features[:22]; BatchNorm folded at pack time) whose
// maps in front of the four max-pools are the features at 1, 1/2, 1/4, 1/8, and a decoder of four ConvRefiners run 1/8 -> 1 whose widths
// and block counts come from the checkpoint (`dims`, read from the tensors by the binding).
//   layer 0     3 -> 64 on the VALU with Normalize applied as the raw image is read (zero padding stays zero in normalised units)
//   encoder     conv3x3_launch / conv3x3_split_launch.  Every layer in front of a pool IS a feature, so its un-pooled map has to
//               exist: those layers take the un-pooled launch and pool2x2_kernel<0> follows; the fused pool has no layer to serve here
//   refiner     block1.0 on the shared GEMM with feature and context as two K slabs (no concat buffer), ReLU in the epilogue; every
//               other 1x1 on the same GEMM; the depth-wise 5x5 + folded BN + ReLU is dd_dw5_kernel (LDS tile with a 2-pixel halo,
//               channels innermost); the x0 residual rides in the epilogue of the last hidden block's 1x1, `/ 1.4` is a pass of its own
//               (a true division behind the sum, upstream's order); out_conv's rows are packed [context | logits] so that both
//               column groups of its output start on 16 bytes (the last scale keeps [logits | context] and computes the logits only)
//   between scales   context: bilinear x2; accumulated logits: bicubic x2 (detector, 1 channel, A = -0.75, border clamp) or bilinear x2
//               (descriptor, 256 channels), `+ logits of the scale` in the same pass; ATen's float32 formulas, align_corners=False
//   detect      per-image soft-max statistics in a fixed chunk order (no float atomics), log p, p = exp(log p) with a written-out
//               float32 exp, the separable 51-tap density filter (rows, then columns, zero padding), score = p / sqrt(density + 1e-8),
//               all in ONE explicit float32 order that tests/dedode_reference.py carries too (this file is built with
//               -ffp-contract=off; fmaf is written where a fused product is wanted); the cut is a radix select of the k-th
//               (score, lower index first) key over every pixel, rows leave in descending score, ties by ascending index
//   describe    the descriptor's full-resolution 257-channel output is never written: its scale-1 hidden stack runs densely, and one
//               wave per key-point applies out_conv's 256 description rows to the hidden vectors at the (up to four) pixels that
//               grid_sample's coordinate round trip touches, adds the bilinear x2 of the 1/2-resolution accumulated grid there and
//               blends with grid_sample's weights
// Grids are sized by shapes, nothing synchronises with the host, every image of a batch is computed independently.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "conv.h"
#include "imcui_hip.h"
#include "net_kernels.h"
#include "netpack.h"
#include "select.h"

#define DD_MAXCONV 12
#define DD_MAXBLK 16
#define DD_TAPS 51
#define DD_DESC 256

// ------------------------------------------------------------------ the networks and their tensor table
struct DdEnc {
    int nconv;
    int cin[DD_MAXCONV], cout[DD_MAXCONV], op[DD_MAXCONV], feat[DD_MAXCONV];  // op: index in vgg.features; feat: a max-pool follows
};
static DdEnc dd_enc(int model) {
    static const int VGG19[] = {64, 64, -1, 128, 128, -1, 256, 256, 256, 256, -1, 512, 512, 512, 512, -1, 0};
    static const int VGG11[] = {64, -1, 128, -1, 256, 256, -1, 512, 512, -1, 0};
    const int* cfg = model == 0 ? VGG19 : VGG11;
    DdEnc e;
    e.nconv = 0;
    int op = 0, cin = 3;
    for (int i = 0; cfg[i] != 0; ++i) {
        if (cfg[i] < 0) {
            e.feat[e.nconv - 1] = 1;
            op += 1;
        } else {
            e.cin[e.nconv] = cin;
            e.cout[e.nconv] = cfg[i];
            e.op[e.nconv] = op;
            e.feat[e.nconv] = 0;
            cin = cfg[i];
            op += 3;  // conv, BatchNorm, ReLU
            ++e.nconv;
        }
    }
    return e;
}
static const int DD_FC[4] = {512, 256, 128, 64};  // feature channels of decoder step 0..3 (scales 8, 4, 2, 1)
static const int DD_SCALE[4] = {8, 4, 2, 1};
static int dd_P(int model) { return model == 0 ? 1 : DD_DESC; }

// ConvRefiner shapes as read from the checkpoint: dims [2 models][4 steps][in, hidden, out, hidden blocks]
struct DdRef {
    int in, hid, out, nblk;
};
struct DdDims {
    DdRef r[2][4];
    int ctx(int m, int s) const { return r[m][s].in - DD_FC[s]; }  // context channels read at step s
    int nout(int m, int s) const { return s == 3 ? dd_P(m) : r[m][s].out; }  // rows of out_conv that are computed
    int ldo(int m, int s) const { return (int)align_up((size_t)nout(m, s), 4); }
};
static bool dd_dims(const int* dims, DdDims* d, std::string* why) {
    if (!dims) {
        *why = "no dims";
        return false;
    }
    char buf[256];
    for (int m = 0; m < 2; ++m)
        for (int s = 0; s < 4; ++s) {
            DdRef& r = d->r[m][s];
            r.in = dims[(m * 4 + s) * 4];
            r.hid = dims[(m * 4 + s) * 4 + 1];
            r.out = dims[(m * 4 + s) * 4 + 2];
            r.nblk = dims[(m * 4 + s) * 4 + 3];
            const char* who = m == 0 ? "detector" : "descriptor";
            const int cc = r.in - DD_FC[s], P = dd_P(m);
            const int want = s == 0 ? 0 : d->r[m][s - 1].out - P;
            if (r.hid < 32 || r.hid > 512 || r.hid % 32 || r.nblk < 1 || r.nblk > DD_MAXBLK) {
                snprintf(buf, sizeof buf, "%s scale %d: hidden %d (a multiple of 32 in 32..512) with %d hidden blocks (1..%d)", who, DD_SCALE[s], r.hid, r.nblk, DD_MAXBLK);
                *why = buf;
                return false;
            }
            if (cc != want || cc < 0 || cc % 32 || cc > 512) {
                snprintf(buf, sizeof buf, "%s scale %d: block1 reads %d channels = %d feature + %d context, the coarser scale hands down %d (out - %d); context a multiple of 32", who,
                         DD_SCALE[s], r.in, DD_FC[s], cc, want, P);
                *why = buf;
                return false;
            }
            if (r.out < P + (s < 3 ? 32 : 0) || r.out > 1024) {
                snprintf(buf, sizeof buf, "%s scale %d: out_conv has %d rows, %d logits + context expected", who, DD_SCALE[s], r.out, P);
                *why = buf;
                return false;
            }
        }
    return true;
}

static const char* DD_MODEL[2] = {"detector.", "descriptor."};
static TensorTable dd_table(const DdDims& d) {
    TensorTable t;
    auto bn = [&](const std::string& p, int c) {
        t.add(p + ".weight", c);
        t.add(p + ".bias", c);
        t.add(p + ".running_mean", c);
        t.add(p + ".running_var", c);
    };
    auto block = [&](const std::string& p, int cin, int c, bool dw) {
        t.add(p + ".0.weight", dw ? (size_t)c * 25 : (size_t)c * cin);
        t.add(p + ".0.bias", c);
        bn(p + ".1", c);
        t.add(p + ".3.weight", (size_t)c * c);
        t.add(p + ".3.bias", c);
    };
    for (int m = 0; m < 2; ++m) {
        const DdEnc e = dd_enc(m);
        for (int i = 0; i < e.nconv; ++i) {
            const std::string p = std::string(DD_MODEL[m]) + "encoder.layers." + std::to_string(e.op[i]);
            t.add(p + ".weight", (size_t)e.cout[i] * e.cin[i] * 9);
            t.add(p + ".bias", e.cout[i]);
            bn(std::string(DD_MODEL[m]) + "encoder.layers." + std::to_string(e.op[i] + 1), e.cout[i]);
        }
        for (int s = 0; s < 4; ++s) {
            const DdRef& r = d.r[m][s];
            const std::string p = std::string(DD_MODEL[m]) + "decoder.layers." + std::to_string(DD_SCALE[s]);
            block(p + ".block1", r.in, r.hid, false);
            for (int i = 0; i < r.nblk; ++i) block(p + ".hidden_blocks." + std::to_string(i), r.hid, r.hid, true);
            t.add(p + ".out_conv.weight", (size_t)r.out * r.hid);
            t.add(p + ".out_conv.bias", r.out);
        }
    }
    t.add("density_taps", DD_TAPS);  // exp(-linspace(-2, 2, 51)^2) as the binding's float32 evaluates it
    return t;
}
extern "C" int imcui_hip_dedode_num_tensors(const int* dims) {
    DdDims d;
    std::string why;
    return dd_dims(dims, &d, &why) ? dd_table(d).size() : 0;
}
extern "C" const char* imcui_hip_dedode_tensor_name(const int* dims, int i) {
    static thread_local std::string name;
    DdDims d;
    std::string why;
    if (!dd_dims(dims, &d, &why)) return nullptr;
    const TensorTable t = dd_table(d);
    if (!t.name(i)) return nullptr;
    name = t.name(i);
    return name.c_str();
}
// why `dims` is refused (empty when it is served); the binding raises it
extern "C" const char* imcui_hip_dedode_dims_error(const int* dims) {
    static thread_local std::string why;
    DdDims d;
    why.clear();
    dd_dims(dims, &d, &why);
    return why.c_str();
}

// packed: per model layer 0 [tap][cin 3][64] + bias, the other encoder layers in both layouts of conv.h + bias, per refiner its 1x1
// layers as GEMM layers and its depth-wise layers [25 taps][C] + bias; the descriptor's last out_conv also transposed [hidden][256] for
// the sparse head; the 51 taps last
struct DdRefOff {
    GemmLayerOff b1a, b1b, pw[DD_MAXBLK], out;
    size_t dw[DD_MAXBLK], db[DD_MAXBLK];
};
struct DdModelOff {
    size_t w0, b0;
    size_t w[DD_MAXCONV], b[DD_MAXCONV], wh[DD_MAXCONV], wl[DD_MAXCONV], ws[DD_MAXCONV];
    DdRefOff r[4];
};
struct DdLayout {
    DdModelOff m[2];
    size_t wt, bt, taps, total;
};
static DdLayout dd_layout(const DdDims& d) {
    DdLayout l;
    PackCursor c;
    for (int m = 0; m < 2; ++m) {
        const DdEnc e = dd_enc(m);
        DdModelOff& o = l.m[m];
        o.w0 = c.get(27 * 64);
        o.b0 = c.get(64);
        for (int i = 1; i < e.nconv; ++i) {
            const size_t n = (size_t)e.cout[i] * e.cin[i] * 9;
            o.w[i] = c.get(n);
            o.b[i] = c.get(e.cout[i]);
            o.wh[i] = c.get(n / 2);
            o.wl[i] = c.get(n / 2);
            o.ws[i] = c.get(1);
        }
        for (int s = 0; s < 4; ++s) {
            const DdRef& r = d.r[m][s];
            o.r[s].b1a.place(c, r.hid, r.in);
            o.r[s].b1b.place(c, r.hid, r.hid);
            for (int i = 0; i < r.nblk; ++i) {
                o.r[s].dw[i] = c.get((size_t)25 * r.hid);
                o.r[s].db[i] = c.get(r.hid);
                o.r[s].pw[i].place(c, r.hid, r.hid);
            }
            o.r[s].out.place(c, r.out, r.hid);
        }
    }
    l.wt = c.get((size_t)d.r[1][3].hid * DD_DESC);
    l.bt = c.get(DD_DESC);
    l.taps = c.get(DD_TAPS);
    l.total = c.off;
    return l;
}
extern "C" size_t imcui_hip_dedode_packed_floats(const int* dims) {
    DdDims d;
    std::string why;
    return dd_dims(dims, &d, &why) ? dd_layout(d).total : 0;
}

extern "C" int imcui_hip_dedode_pack_weights(const int* dims, const float* const* t, float* packed) {
    DdDims d;
    std::string why;
    if (!t || !packed || !dd_dims(dims, &d, &why)) return IMCUI_ERR_ARG;
    const TensorTable tab = dd_table(d);
    for (int i = 0; i < tab.size(); ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const DdLayout l = dd_layout(d);
    memset(packed, 0, l.total * sizeof(float));
    int q = 0;  // cursor over the tensors, in table order
    std::vector<float> scale, shift, w, b;
    // convolution (weight [cout][per], bias) + the BatchNorm behind it -> w, b
    auto fold = [&](int cout, size_t per) {
        const float *cw = t[q], *cb = t[q + 1];
        bn_fold_f32(t + q + 2, cout, scale, shift);
        q += 6;
        w.resize((size_t)cout * per);
        b.resize(cout);
        for (int co = 0; co < cout; ++co) {
            for (size_t k = 0; k < per; ++k) w[(size_t)co * per + k] = cw[(size_t)co * per + k] * scale[co];
            b[co] = cb[co] * scale[co] + shift[co];
        }
    };
    auto gemm_layer = [&](const GemmLayerOff& g, const float* gw, const float* gb, int n, int k) {
        memcpy(packed + g.w, gw, (size_t)n * k * sizeof(float));
        memcpy(packed + g.b, gb, (size_t)n * sizeof(float));
        g.split_planes(packed, n, k);
    };
    for (int m = 0; m < 2; ++m) {
        const DdEnc e = dd_enc(m);
        const DdModelOff& o = l.m[m];
        for (int i = 0; i < e.nconv; ++i) {
            fold(e.cout[i], (size_t)e.cin[i] * 9);
            if (i == 0) {
                for (int co = 0; co < 64; ++co)
                    for (int ci = 0; ci < 3; ++ci)
                        for (int k = 0; k < 9; ++k) packed[o.w0 + ((size_t)k * 3 + ci) * 64 + co] = w[((size_t)co * 3 + ci) * 9 + k];
                memcpy(packed + o.b0, b.data(), 64 * sizeof(float));
            } else {
                pack_conv3x3(w.data(), e.cout[i], e.cin[i], packed + o.w[i]);
                memcpy(packed + o.b[i], b.data(), e.cout[i] * sizeof(float));
                packed[o.ws[i]] = pack_conv3x3_split(w.data(), e.cout[i], e.cin[i], reinterpret_cast<unsigned short*>(packed + o.wh[i]),
                                                     reinterpret_cast<unsigned short*>(packed + o.wl[i]));
            }
        }
        for (int s = 0; s < 4; ++s) {
            const DdRef& r = d.r[m][s];
            const DdRefOff& ro = o.r[s];
            fold(r.hid, r.in);
            gemm_layer(ro.b1a, w.data(), b.data(), r.hid, r.in);
            gemm_layer(ro.b1b, t[q], t[q + 1], r.hid, r.hid);
            q += 2;
            for (int i = 0; i < r.nblk; ++i) {
                fold(r.hid, 25);
                for (int c = 0; c < r.hid; ++c)
                    for (int k = 0; k < 25; ++k) packed[ro.dw[i] + (size_t)k * r.hid + c] = w[(size_t)c * 25 + k];
                memcpy(packed + ro.db[i], b.data(), r.hid * sizeof(float));
                gemm_layer(ro.pw[i], t[q], t[q + 1], r.hid, r.hid);
                q += 2;
            }
            // out_conv: rows [P, out) (context) ahead of rows [0, P) (logits), except at the last scale
            const float *ow = t[q], *ob = t[q + 1];
            q += 2;
            const int P = dd_P(m), first = s == 3 ? 0 : P;
            w.resize((size_t)r.out * r.hid);
            b.resize(r.out);
            for (int j = 0; j < r.out; ++j) {
                const int src = (j + first) % r.out;
                memcpy(w.data() + (size_t)j * r.hid, ow + (size_t)src * r.hid, r.hid * sizeof(float));
                b[j] = ob[src];
            }
            gemm_layer(ro.out, w.data(), b.data(), r.out, r.hid);
            if (m == 1 && s == 3) {
                for (int j = 0; j < DD_DESC; ++j) {
                    for (int k = 0; k < r.hid; ++k) packed[l.wt + (size_t)k * DD_DESC + j] = ow[(size_t)j * r.hid + k];
                    packed[l.bt + j] = ob[j];
                }
            }
        }
    }
    memcpy(packed + l.taps, t[q], DD_TAPS * sizeof(float));
    return IMCUI_OK;
}

namespace {

// exp in one written-out float32 order (Cephes expf: n = rint(x log2 e), r = x - n ln 2 in two parts, degree-5 polynomial, 2^n by
// ldexp), so that the restatement can carry the same bits; arguments below -80 are clamped (exp(-80) = 1.8e-35 is still normal)
__device__ __forceinline__ float dd_exp(float x) {
    x = fmaxf(x, -80.0f);
    const float n = rintf(__fmul_rn(x, 1.44269504088896341f));
    const float r = __fsub_rn(__fsub_rn(x, __fmul_rn(n, 0.693359375f)), __fmul_rn(n, -2.12194440e-4f));
    float p = 1.9875691500e-4f;
    p = __fadd_rn(__fmul_rn(p, r), 1.3981999507e-3f);
    p = __fadd_rn(__fmul_rn(p, r), 8.3334519073e-3f);
    p = __fadd_rn(__fmul_rn(p, r), 4.1665795894e-2f);
    p = __fadd_rn(__fmul_rn(p, r), 1.6666665459e-1f);
    p = __fadd_rn(__fmul_rn(p, r), 5.0000001201e-1f);
    const float y = __fadd_rn(__fadd_rn(__fmul_rn(p, __fmul_rn(r, r)), r), 1.0f);
    return ldexpf(y, (int)n);
}

// what layer 0 reads: transforms.Normalize of the raw image, (x - mean) / std with one rounding each
struct DdStemLoad {
    __device__ float operator()(const float* __restrict__ img, long b, int c, int h, int w, int yy, int xx) const {
        const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
        return __fdiv_rn(__fsub_rn(img[((b * 3 + c) * h + yy) * (long)w + xx], mean), sd);
    }
};

__device__ __forceinline__ float4 dd_fma4(float4 a, float4 b, float4 c) { return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w)); }

// Depth-wise 5x5 (pad 2) + folded BatchNorm + ReLU on an NHWC map [B, H, W, C], C % 32 == 0; w [25 taps][C], bias [C].
// One workgroup = 8 x 16 pixels x 32 channels: the 12 x 20 pixel window (2-pixel halo, zeros outside the map) is staged in LDS with the
// channels innermost (a pixel's 32 channels are one 128-byte line, in memory and in LDS), thread = (channel quad, column, 4 rows):
// 40 16-byte LDS reads feed 100 float4 FMAs.  A map smaller than the tile, or than the filter, is the same code: what is outside is zero
// in LDS and is not stored.
#define DW_TW 16
#define DW_TH 8
#define DW_PW (DW_TW + 4)
#define DW_PH (DW_TH + 4)
__global__ __launch_bounds__(256) void dd_dw5_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ out, int H, int W, int C, int tiles_x) {
    __shared__ float4 tile[DW_PH * DW_PW * 8];
    __shared__ float4 sw[25 * 8];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, tx0 = (blockIdx.x % tiles_x) * DW_TW, ty0 = (blockIdx.x / tiles_x) * DW_TH;
    const int tid = threadIdx.x, cg = tid & 7;
    const float* ib = in + (long)b * H * W * C + c0;
    for (int i = tid; i < DW_PH * DW_PW * 8; i += 256) {
        const int g = i & 7, pc = i >> 3, px = pc % DW_PW, py = pc / DW_PW;
        const int gy = ty0 + py - 2, gx = tx0 + px - 2;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const float4*>(ib + ((long)gy * W + gx) * C + g * 4);
        tile[i] = v;
    }
    if (tid < 200) sw[tid] = *reinterpret_cast<const float4*>(w + (long)(tid >> 3) * C + c0 + (tid & 7) * 4);
    __syncthreads();
    const int slot = tid >> 3, x = slot & 15, yb = (slot >> 4) * 4;
    const float4 b4 = *reinterpret_cast<const float4*>(bias + c0 + cg * 4);
    float4 acc[4] = {b4, b4, b4, b4};
#pragma unroll 1
    for (int dx = 0; dx < 5; ++dx) {  // (rolled: unrolled, the compiler hoists all 40 tile reads and the kernel needs 256 VGPRs)
        float4 wv[5];
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) wv[ky] = sw[(ky * 5 + dx) * 8 + cg];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float4 v = tile[((yb + r) * DW_PW + x + dx) * 8 + cg];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int ky = r - o;
                if (ky >= 0 && ky < 5) acc[o] = dd_fma4(v, wv[ky], acc[o]);
            }
        }
    }
    const int gx = tx0 + x;
    if (gx >= W) return;
    float* ob = out + (long)b * H * W * C + c0 + cg * 4;
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = ty0 + yb + o;
        if (gy < H) *reinterpret_cast<float4*>(ob + ((long)gy * W + gx) * C) = max4(acc[o], z);
    }
}

// x /= 1.4 (IEEE division), n4 float4s
__global__ __launch_bounds__(256) void dd_div14_kernel(float* __restrict__ x, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 v = *reinterpret_cast<float4*>(x + i * 4);
        v = make_float4(__fdiv_rn(v.x, 1.4f), __fdiv_rn(v.y, 1.4f), __fdiv_rn(v.z, 1.4f), __fdiv_rn(v.w, 1.4f));
        *reinterpret_cast<float4*>(x + i * 4) = v;
    }
}

// ATen's upsample_bilinear2d source index at scale 1 / 2, align_corners=False: max(0.5 (dst + 0.5) - 0.5, 0)
__device__ __forceinline__ void dd_lin_src(int o, int in, int* i0, int* i1, float* l0, float* l1) {
    const float s = fmaxf(__fsub_rn(__fmul_rn(0.5f, __fadd_rn((float)o, 0.5f)), 0.5f), 0.0f);
    const int a = min((int)s, in - 1);
    *i0 = a;
    *i1 = a + (a < in - 1 ? 1 : 0);
    *l1 = __fsub_rn(s, (float)a);
    *l0 = __fsub_rn(1.0f, *l1);
}
__device__ __forceinline__ float dd_lin_mix(float hy0, float hy1, float wx0, float wx1, float v00, float v01, float v10, float v11) {
    return __fadd_rn(__fmul_rn(hy0, __fadd_rn(__fmul_rn(wx0, v00), __fmul_rn(wx1, v01))), __fmul_rn(hy1, __fadd_rn(__fmul_rn(wx0, v10), __fmul_rn(wx1, v11))));
}
// channel c of the bilinear x2 of one image's map src [h, w, lds] at pixel (y, x) of the 2h x 2w map
__device__ __forceinline__ float dd_up2_at(const float* __restrict__ src, long lds, int h, int w, int y, int x, int c) {
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    dd_lin_src(y, h, &y0, &y1, &hy0, &hy1);
    dd_lin_src(x, w, &x0, &x1, &wx0, &wx1);
    return dd_lin_mix(hy0, hy1, wx0, wx1, src[((long)y0 * w + x0) * lds + c], src[((long)y0 * w + x1) * lds + c], src[((long)y1 * w + x0) * lds + c],
                      src[((long)y1 * w + x1) * lds + c]);
}

// dst [B, 2h, 2w, C] = bilinear x2 of src [B, h, w, (lds)] (+ add [B, 2h, 2w, (lda)], may alias dst); C % 4 == 0, pointers and strides
// on 16 bytes; n4 = float4s of dst
__global__ __launch_bounds__(256) void dd_up2_kernel(const float* __restrict__ src, long lds, int h, int w, int C, float* dst, const float* add, long lda,
                                                     long n4) {
    const int C4 = C >> 2, ho = 2 * h, wo = 2 * w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        long t = i / C4;
        const int x = (int)(t % wo);
        t /= wo;
        const int y = (int)(t % ho);
        const long b = t / ho;
        int y0, y1, x0, x1;
        float hy0, hy1, wx0, wx1;
        dd_lin_src(y, h, &y0, &y1, &hy0, &hy1);
        dd_lin_src(x, w, &x0, &x1, &wx0, &wx1);
        const float* pb = src + b * (long)h * w * lds + c;
        const float4 v00 = *reinterpret_cast<const float4*>(pb + ((long)y0 * w + x0) * lds), v01 = *reinterpret_cast<const float4*>(pb + ((long)y0 * w + x1) * lds),
                     v10 = *reinterpret_cast<const float4*>(pb + ((long)y1 * w + x0) * lds), v11 = *reinterpret_cast<const float4*>(pb + ((long)y1 * w + x1) * lds);
        float4 o = make_float4(dd_lin_mix(hy0, hy1, wx0, wx1, v00.x, v01.x, v10.x, v11.x), dd_lin_mix(hy0, hy1, wx0, wx1, v00.y, v01.y, v10.y, v11.y),
                               dd_lin_mix(hy0, hy1, wx0, wx1, v00.z, v01.z, v10.z, v11.z), dd_lin_mix(hy0, hy1, wx0, wx1, v00.w, v01.w, v10.w, v11.w));
        const long pix = (b * ho + y) * (long)wo + x;
        if (add) {
            const float4 a = *reinterpret_cast<const float4*>(add + pix * lda + c);
            o = make_float4(__fadd_rn(o.x, a.x), __fadd_rn(o.y, a.y), __fadd_rn(o.z, a.z), __fadd_rn(o.w, a.w));
        }
        *reinterpret_cast<float4*>(dst + pix * C + c) = o;
    }
}

// ATen's cubic convolution coefficients (A = -0.75) for the fraction t
__device__ __forceinline__ void dd_cubic(float t, float* c) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}
// dst [B, 2h, 2w] = bicubic x2 (align_corners=False, indices clamped to the border) of the plane src (element (b, y, x) at
// src[((b h + y) w + x) lds]) (+ add, element at add[pixel * lda]); n = B * 4 h w
__global__ __launch_bounds__(256) void dd_cub2_kernel(const float* __restrict__ src, long lds, int h, int w, float* __restrict__ dst, const float* __restrict__ add,
                                                      long lda, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int wo = 2 * w, ho = 2 * h;
    const int x = (int)(i % wo);
    const long t = i / wo;
    const int y = (int)(t % ho);
    const long b = t / ho;
    const float ry = 0.5f * ((float)y + 0.5f) - 0.5f, rx = 0.5f * ((float)x + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    float cy[4], cx[4];
    dd_cubic(ry - fy, cy);
    dd_cubic(rx - fx, cx);
    const float* pb = src + b * (long)h * w * lds;
    float o = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int yy = min(max((int)fy - 1 + a, 0), h - 1);
        float r = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xx = min(max((int)fx - 1 + k, 0), w - 1);
            r = fmaf(cx[k], pb[((long)yy * w + xx) * lds], r);
        }
        o = fmaf(cy[a], r, o);
    }
    if (add) o += add[i * lda];
    dst[i] = o;
}

// dst[i] = src[i * ld]
__global__ __launch_bounds__(256) void dd_col_kernel(const float* __restrict__ src, long ld, float* __restrict__ dst, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i * ld];
}

// ---- per-image soft-max statistics, batch-independent: chunk c of 4096 logits -> (max, sum exp(l - max)) in a fixed order, then one
// workgroup per image folds the chunks in a fixed order -> stat[b] = (max, log sum)
#define DD_CHUNK 4096
__device__ __forceinline__ float dd_block_max(float v, float* s4) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s4[0], s4[1]), fmaxf(s4[2], s4[3]));
}
__device__ __forceinline__ float dd_block_sum(float v, float* s4) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}
__global__ __launch_bounds__(256) void dd_smax_part_kernel(const float* __restrict__ l, int npix, float* __restrict__ part, int nchunk) {
    __shared__ float s4[4];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* lb = l + (long)b * npix;
    const int base = chunk * DD_CHUNK + threadIdx.x * 16;
    float v[16];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        v[j] = base + j < npix ? lb[base + j] : -INFINITY;
        m = fmaxf(m, v[j]);
    }
    m = dd_block_max(m, s4);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += base + j < npix ? expf(v[j] - m) : 0.0f;
    s = dd_block_sum(s, s4);
    if (threadIdx.x == 0) {
        part[((long)b * nchunk + chunk) * 2] = m;
        part[((long)b * nchunk + chunk) * 2 + 1] = s;
    }
}
__global__ __launch_bounds__(256) void dd_smax_fin_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ stat) {
    __shared__ float s4[4];
    const int b = blockIdx.x;
    const float* pb = part + (long)b * nchunk * 2;
    float m = -INFINITY;
    for (int c = threadIdx.x; c < nchunk; c += 256) m = fmaxf(m, pb[2 * c]);
    m = dd_block_max(m, s4);
    float s = 0.0f;
    for (int c = threadIdx.x; c < nchunk; c += 256) s += pb[2 * c + 1] * expf(pb[2 * c] - m);
    s = dd_block_sum(s, s4);
    if (threadIdx.x == 0) {
        stat[2 * b] = m;
        stat[2 * b + 1] = logf(s);
    }
}
// log p = (l - max) - log sum, p = exp(log p)
__global__ __launch_bounds__(256) void dd_logp_kernel(const float* __restrict__ l, const float* __restrict__ stat, int npix, float* __restrict__ logp,
                                                      float* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long b = i / npix;
    const float lp = __fsub_rn(__fsub_rn(l[i], stat[2 * b]), stat[2 * b + 1]);
    logp[i] = lp;
    p[i] = dd_exp(lp);
}

// the 51-tap filter along a row, zero padding, taps summed in ascending order with one rounding per product and per sum;
// q: the input is (v + 1e-6) * 10000 of the plane read
__global__ __launch_bounds__(256) void dd_rowf_kernel(const float* __restrict__ src, const float* __restrict__ taps, float* __restrict__ dst, int W, int q, long n) {
    __shared__ float tw[DD_TAPS];
    if (threadIdx.x < DD_TAPS) tw[threadIdx.x] = taps[threadIdx.x];
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W);
    const float* row = src + (i - x);
    float acc = 0.0f;
    for (int t = max(0, 25 - x); t < min(DD_TAPS, W + 25 - x); ++t) {
        float v = row[x + t - 25];
        if (q) v = __fmul_rn(__fadd_rn(v, 1e-6f), 10000.0f);
        acc = __fadd_rn(acc, __fmul_rn(tw[t], v));
    }
    dst[i] = acc;
}
// the same along a column -> density; p given: dst = p * (1 / sqrt(density + 1e-8)) (sample_keypoints' `p * (density + 1e-8) ** -0.5`
// with a correctly rounded square root and IEEE division), else dst = density
__global__ __launch_bounds__(256) void dd_colf_kernel(const float* __restrict__ src, const float* __restrict__ taps, const float* __restrict__ p,
                                                      float* __restrict__ dst, int H, int W, long n) {
    __shared__ float tw[DD_TAPS];
    if (threadIdx.x < DD_TAPS) tw[threadIdx.x] = taps[threadIdx.x];
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int y = (int)((i / W) % H);
    float acc = 0.0f;
    for (int t = max(0, 25 - y); t < min(DD_TAPS, H + 25 - y); ++t) acc = __fadd_rn(acc, __fmul_rn(tw[t], src[i + (long)(t - 25) * W]));
    // (the root through float64, rounded once: the correctly rounded float32 root whatever the build's float32 sqrt is; __fsqrt_rn is
    // the native approximation in this toolchain)
    dst[i] = p ? __fmul_rn(p[i], __fdiv_rn(1.0f, (float)sqrt((double)__fadd_rn(acc, 1e-8f)))) : acc;
}

// (score, pixel) as one ordered key: of equal scores the LOWER flat index is the larger key
__device__ __forceinline__ unsigned long long dd_key(float s, int i) { return ((unsigned long long)order_key(s) << 32) | (0xFFFFFFFFu - (unsigned)i); }

// The cut.  One workgroup per image, every pixel a candidate: the k largest keys stay and leave in pixel order (klist [B, k]).
__global__ __launch_bounds__(1024) void dd_cut_kernel(const float* __restrict__ score, int npix, int k, int* __restrict__ klist) {
    const int b = blockIdx.x;
    const float* sc = score + (long)b * npix;
    const auto key_at = [&](int i) { return dd_key(sc[i], i); };
    const unsigned long long kth = radix_select_kth<1024, unsigned long long>(key_at, npix, k);
    keep_kth_in_order(key_at, npix, true, kth, k, klist + (long)b * k);
}

// One workgroup = 256 kept pixels: the rank of each in descending key order, then row `rank` gets the key-point: grid coordinate
// x = (2 j + 1) / W - 1 (the pixel centre of get_grid), to_pixel_coords ((x + 1) / 2) W, the score; kidx [B, k] = the pixel of every
// row, for the description head.  Rows k .. kout are zero.
__global__ __launch_bounds__(256) void dd_emit_kernel(const float* __restrict__ score, const int* __restrict__ klist, int npix, int W, int H, int k, int kout,
                                                      float* __restrict__ kpts, float* __restrict__ scores, int* __restrict__ kidx, int* __restrict__ nkpts) {
    __shared__ float ts[256];
    __shared__ int ti[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* sc = score + (long)b * npix;
    const int* ks = klist + (long)b * k;
    if (blockIdx.x == 0 && tid == 0) nkpts[b] = k;
    float* kp = kpts + (long)b * kout * 2;
    float* so = scores + (long)b * kout;
    const int i = blockIdx.x * 256 + tid;
    if (i >= k && i < kout) kp[2 * i] = kp[2 * i + 1] = so[i] = 0.0f;
    if (blockIdx.x * 256 >= k) return;  // (uniform)
    const int mi = i < k ? ks[i] : 0;
    const float ms = i < k ? sc[mi] : 0.0f;
    int rank = 0;
    for (int base = 0; base < k; base += 256) {
        __syncthreads();
        if (base + tid < k) {
            ti[tid] = ks[base + tid];
            ts[tid] = sc[ti[tid]];
        }
        __syncthreads();
        const int m = min(256, k - base);
        for (int j = 0; j < m; ++j) {
            const float o = ts[j];
            rank += (o > ms || (o == ms && ti[j] < mi)) ? 1 : 0;
        }
    }
    if (i >= k) return;
    const int y = mi / W, x = mi - y * W;
    const float gx = __fsub_rn(__fdiv_rn((float)(2 * x + 1), (float)W), 1.0f), gy = __fsub_rn(__fdiv_rn((float)(2 * y + 1), (float)H), 1.0f);
    kp[2 * rank] = __fmul_rn(__fdiv_rn(__fadd_rn(gx, 1.0f), 2.0f), (float)W);
    kp[2 * rank + 1] = __fmul_rn(__fdiv_rn(__fadd_rn(gy, 1.0f), 2.0f), (float)H);
    so[rank] = ms;
    kidx[(long)b * k + rank] = mi;
}

// The sparse description head.  One wave per output row.  The key-point's grid coordinate goes through grid_sample's round trip
// ((x + 1) W - 1) / 2 in float32, and the four corners floor / floor + 1 get ATen's weights (nw, ne, sw, se, zeros outside the map).  At
// a corner pixel the description is out_conv(hidden) + bias + bilinear x2 of the 1/2-resolution accumulated grid: lane l owns channels
// l, l + 64, l + 128, l + 192; wt [hid][256], acc2 [B, H / 2, W / 2, 256], hidden [B, H, W, hid].
__global__ __launch_bounds__(256) void dd_describe_kernel(const int* __restrict__ kidx, const float* __restrict__ hidden, int hid, const float* __restrict__ wt,
                                                          const float* __restrict__ bt, const float* __restrict__ acc2, int H, int W, int k, int kout,
                                                          float* __restrict__ desc) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= kout) return;  // (wave-uniform)
    float* de = desc + ((long)b * kout + r) * DD_DESC;
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < k) {
        const int pix = kidx[(long)b * k + r];
        const int py = pix / W, px = pix - py * W;
        const float gx = __fsub_rn(__fdiv_rn((float)(2 * px + 1), (float)W), 1.0f), gy = __fsub_rn(__fdiv_rn((float)(2 * py + 1), (float)H), 1.0f);
        const float ix = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.0f), (float)W), 1.0f), 2.0f);
        const float iy = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.0f), (float)H), 1.0f), 2.0f);
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float wx1 = __fsub_rn(ix, fx), wx0 = __fsub_rn(__fadd_rn(fx, 1.0f), ix), wy1 = __fsub_rn(iy, fy), wy0 = __fsub_rn(__fadd_rn(fy, 1.0f), iy);
        const float cw[4] = {__fmul_rn(wx0, wy0), __fmul_rn(wx1, wy0), __fmul_rn(wx0, wy1), __fmul_rn(wx1, wy1)};
        const float* a2 = acc2 + (long)b * (H / 2) * (W / 2) * DD_DESC;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int xx = x0 + (c & 1), yy = y0 + (c >> 1);
            if (cw[c] == 0.0f || xx < 0 || xx >= W || yy < 0 || yy >= H) continue;  // (wave-uniform; a zero weight adds nothing)
            const float* hv = hidden + (((long)b * H + yy) * W + xx) * hid;
            float d[4] = {bt[lane], bt[lane + 64], bt[lane + 128], bt[lane + 192]};
            for (int j = 0; j < hid; ++j) {
                const float v = hv[j];
                const float* wr = wt + (long)j * DD_DESC + lane;
                d[0] = fmaf(v, wr[0], d[0]);
                d[1] = fmaf(v, wr[64], d[1]);
                d[2] = fmaf(v, wr[128], d[2]);
                d[3] = fmaf(v, wr[192], d[3]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = __fadd_rn(o[q], __fmul_rn(cw[c], __fadd_rn(d[q], dd_up2_at(a2, DD_DESC, H / 2, W / 2, yy, xx, lane + 64 * q))));
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) de[lane + 64 * q] = o[q];
}

}  // namespace

// ------------------------------------------------------------------ workspace
struct DdWs {
    float *enc[2], *feat[4], *hx0, *ha, *ht, *o[2], *ctx, *accd[2], *logits, *stat, *part, *logp, *p, *rowf, *score;
    int *klist, *kidx, *status;
    size_t total;
    bool ok;
};
static DdWs dd_carve(void* ws, size_t bytes, const DdDims& d, int B, int H, int W, int k) {
    WsAlloc a(ws, bytes);
    DdWs s;
    const size_t npix = (size_t)H * W, bp = (size_t)B * npix;
    s.enc[0] = a.get<float>(bp * 64);
    s.enc[1] = a.get<float>(bp * 64);
    for (int i = 0; i < 4; ++i) s.feat[i] = a.get<float>((bp >> (2 * (3 - i))) * DD_FC[i]);  // step i: scale DD_SCALE[i]
    size_t hmax = 0, omax = 0, cmax = 0;
    for (int m = 0; m < 2; ++m)
        for (int i = 0; i < 4; ++i) {
            const size_t M = bp >> (2 * (3 - i));
            hmax = std::max(hmax, M * d.r[m][i].hid);
            omax = std::max(omax, M * d.ldo(m, i));
            if (i > 0) cmax = std::max(cmax, M * d.ctx(m, i));
        }
    s.hx0 = a.get<float>(hmax);
    s.ha = a.get<float>(hmax);
    s.ht = a.get<float>(hmax);
    s.o[0] = a.get<float>(omax);
    s.o[1] = a.get<float>(omax);
    s.ctx = a.get<float>(cmax);
    s.accd[0] = a.get<float>((bp / 16) * DD_DESC);
    s.accd[1] = a.get<float>((bp / 4) * DD_DESC);
    s.logits = a.get<float>(bp + bp / 4 + bp / 16 + bp / 64);
    s.stat = a.get<float>((size_t)B * 2);
    s.part = a.get<float>((size_t)B * ((npix + DD_CHUNK - 1) / DD_CHUNK) * 2);
    s.logp = a.get<float>(bp);
    s.p = a.get<float>(bp);
    s.rowf = a.get<float>(bp);
    s.score = a.get<float>(bp);
    s.klist = a.get<int>((size_t)B * k);
    s.kidx = a.get<int>((size_t)B * k);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

static int dd_check(imcui_hip_t* h, const int* dims, DdDims* d, int B, int H, int W, int k) {
    std::string why;
    if (!dd_dims(dims, d, &why)) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode: %s", why.c_str());
    if (B < 1 || B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode: B=%d (1..1024)", B);
    if (H < 8 || W < 8 || H % 8 || W % 8) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode: H=%d W=%d must be multiples of 8 (the reference resizes with dfactor 8)", H, W);
    if ((long)B * H * W > 0x7fffffffL / 64) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode: B=%d images of %dx%d exceed the 2^31 index range of one call", B, H, W);
    if (k < 1 || (long)k > (long)H * W) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode: num_keypoints=%d outside 1..H*W=%ld (topk would raise)", k, (long)H * W);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_dedode_workspace_bytes(const int* dims, int B, int H, int W, int k) {
    DdDims d;
    std::string why;
    if (!dd_dims(dims, &d, &why) || B <= 0 || H <= 0 || W <= 0 || k <= 0) return 0;
    return dd_carve(nullptr, 0, d, B, H, W, k).total;
}

static int dd_dw5(imcui_hip_t* h, const float* in, const float* w, const float* b, float* out, int B, int H, int W, int C, hipStream_t stream) {
    const int tx = cdiv(W, DW_TW), ty = cdiv(H, DW_TH);
    hipLaunchKernelGGL(dd_dw5_kernel, dim3(tx * ty, C / 32, B), dim3(256), 0, stream, in, w, b, out, H, W, C, tx);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// layer 0 (weights w0, bias b0 of one model) on the raw planar image [B, 3, H, W] -> out [B, H, W, 64]
static void dd_stem(const float* image, const float* w0, const float* b0, float* out, int B, int H, int W, hipStream_t stream) {
    const long npix = (long)B * H * W;
    hipLaunchKernelGGL((stem3x3_kernel<64, DdStemLoad>), dim3(blocks_256(npix)), dim3(256), 0, stream, image, w0, b0, out, H, W, DdStemLoad{}, npix);
}

// the encoder of model m on the raw image: features of steps 0..3 (scales 8, 4, 2, 1) -> s.feat
static int dd_encoder(imcui_hip_t* h, int m, const DdLayout& l, const float* P, const float* image, int B, int H, int W, const DdWs& s, hipStream_t stream) {
    const bool split = h->precision == 1;
    const DdEnc e = dd_enc(m);
    const DdModelOff& o = l.m[m];
    int rc, hh = H, ww = W, step = 3;
    const float* cur = nullptr;
    int pp = 0;
    for (int i = 0; i < e.nconv; ++i) {
        float* dst = e.feat[i] ? s.feat[step] : s.enc[pp];
        if (i == 0) {
            dd_stem(image, P + o.w0, P + o.b0, dst, B, H, W, stream);
            IMCUI_CHECK_LAUNCH(h);
        } else if (split) {
            IMCUI_RUN(conv3x3_split_launch(h, cur, reinterpret_cast<const unsigned short*>(P + o.wh[i]), reinterpret_cast<const unsigned short*>(P + o.wl[i]),
                                           P + o.ws[i], P + o.b[i], dst, B, hh, ww, e.cin[i], e.cout[i], 1, 0, stream));
        } else {
            IMCUI_RUN(conv3x3_launch(h, cur, P + o.w[i], P + o.b[i], dst, B, hh, ww, e.cin[i], e.cout[i], 1, 0, stream));
        }
        cur = dst;
        if (!e.feat[i]) {
            pp ^= 1;
        } else if (step > 0) {  // (the fourth pool's output is discarded)
            const long n4 = (long)B * (hh / 2) * (ww / 2) * (e.cout[i] / 4);
            hipLaunchKernelGGL(pool2x2_kernel<0>, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, cur, s.enc[pp], hh, ww, hh / 2, ww / 2, e.cout[i], n4);
            IMCUI_CHECK_LAUNCH(h);
            cur = s.enc[pp];
            pp ^= 1;
            hh /= 2;
            ww /= 2;
            --step;
        }
    }
    return IMCUI_OK;
}

// ConvRefiner of model m, step st, up to `x = (hidden_blocks(x0) + x0) / 1.4` -> s.ha [M, hid]; feature [M, fc] and context [M, cc]
static int dd_refiner(imcui_hip_t* h, int m, int st, const DdDims& d, const DdLayout& l, const float* P, const float* ctx, int B, int hh, int ww, const DdWs& s,
                      hipStream_t stream) {
    const bool split = h->precision == 1;
    const DdRef& r = d.r[m][st];
    const DdRefOff& ro = l.m[m].r[st];
    const int M = B * hh * ww, cc = d.ctx(m, st);
    int rc;
    auto lin = [&](const GemmLayerOff& go, const float* A, int K, float* C, int act, const float* resid) -> int {
        GemmP g;
        g.epi = EPI_CONV;
        g.A = A;
        g.lda = K;
        gemm_set_weights(g, P, go, r.hid, K, split);
        g.M = M;
        g.C = C;
        g.ldc = r.hid;
        g.act = act;
        g.resid = resid;
        g.ldr = r.hid;
        return gemm_launch(h, g, stream);
    };
    {
        GemmP g;
        g.epi = EPI_CONV;
        g.A = s.feat[st];
        g.lda = DD_FC[st];
        if (cc > 0) {
            g.A2 = ctx;
            g.lda2 = cc;
            g.K1 = DD_FC[st];
        }
        gemm_set_weights(g, P, ro.b1a, r.hid, r.in, split);
        g.M = M;
        g.C = s.ht;
        g.ldc = r.hid;
        g.act = 1;
        IMCUI_RUN(gemm_launch(h, g, stream));
    }
    IMCUI_RUN(lin(ro.b1b, s.ht, r.hid, s.hx0, 0, nullptr));
    const float* x = s.hx0;
    for (int i = 0; i < r.nblk; ++i) {
        IMCUI_RUN(dd_dw5(h, x, P + ro.dw[i], P + ro.db[i], s.ht, B, hh, ww, r.hid, stream));
        IMCUI_RUN(lin(ro.pw[i], s.ht, r.hid, s.ha, 0, i == r.nblk - 1 ? s.hx0 : nullptr));
        x = s.ha;
    }
    const long n4 = (long)M * r.hid / 4;
    hipLaunchKernelGGL(dd_div14_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, s.ha, n4);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

extern "C" int imcui_hip_dedode_forward(imcui_hip_t* h, const float* packed, const int* dims, const float* image, int B, int H, int W, int k, int kout,
                                        float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, float* dbg_logits, float* dbg_logp,
                                        float* dbg_score, float* dbg_desc2, float* dbg_dense, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    DdDims d;
    int rc;
    IMCUI_RUN(dd_check(h, dims, &d, B, H, W, k));
    if (kout < k || !packed || !image || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "dedode: null argument or kout=%d below num_keypoints=%d", kout, k);
    if ((long)B * kout > 0x7fffffffL / DD_DESC) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode: B=%d rows of kout=%d exceed the 2^31 index range", B, kout);
    const DdLayout l = dd_layout(d);
    const DdWs s = dd_carve(ws, ws_bytes, d, B, H, W, k);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "dedode: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const bool split = h->precision == 1;
    const float* P = packed;
    const int npix = H * W;
    const long bp = (long)B * npix;
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, status ? status : s.status, 1);

    for (int m = 0; m < 2; ++m) {
        IMCUI_RUN(dd_encoder(h, m, l, P, image, B, H, W, s, stream));
        const int Pn = dd_P(m);
        const float* accp = nullptr;  // the accumulated logits of the previous step and the stride of a pixel there
        long acc_ld = 0;
        long loff = 0;  // detector: this step's plane in s.logits
        for (int st = 0; st < 4; ++st) {
            const int hh = H / DD_SCALE[st], ww = W / DD_SCALE[st], M = B * hh * ww;
            const DdRef& r = d.r[m][st];
            IMCUI_RUN(dd_refiner(h, m, st, d, l, P, s.ctx, B, hh, ww, s, stream));
            float* o = s.o[st & 1];
            const int N = d.nout(m, st), ldo = d.ldo(m, st), cc_next = st < 3 ? r.out - Pn : 0;
            const bool dense_out = !(m == 1 && st == 3);  // the descriptor's last out_conv runs at the key-points only
            if (dense_out || dbg_dense) {
                GemmP g;
                g.epi = EPI_CONV;
                g.A = s.ha;
                g.lda = r.hid;
                gemm_set_weights(g, P, l.m[m].r[st].out, N, r.hid, split);
                g.M = M;
                g.C = dense_out ? o : dbg_dense;
                g.ldc = dense_out ? ldo : DD_DESC;
                IMCUI_RUN(gemm_launch(h, g, stream));
            }
            const float* lg = o + cc_next;  // this step's logits, pixel stride ldo
            if (m == 0) {
                float* plane = s.logits + loff;
                if (st == 0)
                    hipLaunchKernelGGL(dd_col_kernel, dim3(blocks_256(M)), dim3(256), 0, stream, lg, (long)ldo, plane, (long)M);
                else
                    hipLaunchKernelGGL(dd_cub2_kernel, dim3(blocks_256(M)), dim3(256), 0, stream, accp, acc_ld, hh / 2, ww / 2, plane, lg, (long)ldo, (long)M);
                accp = plane;
                acc_ld = 1;
                loff += M;
            } else if (st == 0) {
                accp = lg;
                acc_ld = ldo;
            } else if (st < 3) {
                float* acc = s.accd[st - 1];
                const long n4 = (long)M * DD_DESC / 4;
                hipLaunchKernelGGL(dd_up2_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, accp, acc_ld, hh / 2, ww / 2, DD_DESC, acc, lg, (long)ldo, n4);
                accp = acc;
                acc_ld = DD_DESC;
            } else if (dbg_dense) {
                const long n4 = (long)M * DD_DESC / 4;
                hipLaunchKernelGGL(dd_up2_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, accp, acc_ld, hh / 2, ww / 2, DD_DESC, dbg_dense, dbg_dense, (long)DD_DESC, n4);
            }
            IMCUI_CHECK_LAUNCH(h);
            if (st < 3 && cc_next > 0) {
                const long n4 = (long)M * 4 * cc_next / 4;
                hipLaunchKernelGGL(dd_up2_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, o, (long)ldo, hh, ww, cc_next, s.ctx, (const float*)nullptr, 0L, n4);
                IMCUI_CHECK_LAUNCH(h);
            }
        }
        if (m == 0) {
            // ---- detect: soft-max over the image, density, score, the cut
            const float* L = s.logits + (loff - bp);
            const int nchunk = cdiv(npix, DD_CHUNK);
            const float* taps = P + l.taps;
            hipLaunchKernelGGL(dd_smax_part_kernel, dim3(nchunk, B), dim3(256), 0, stream, L, npix, s.part, nchunk);
            hipLaunchKernelGGL(dd_smax_fin_kernel, dim3(B), dim3(256), 0, stream, s.part, nchunk, s.stat);
            hipLaunchKernelGGL(dd_logp_kernel, dim3(blocks_256(bp)), dim3(256), 0, stream, L, s.stat, npix, s.logp, s.p, bp);
            hipLaunchKernelGGL(dd_rowf_kernel, dim3(blocks_256(bp)), dim3(256), 0, stream, s.p, taps, s.rowf, W, 1, bp);
            hipLaunchKernelGGL(dd_colf_kernel, dim3(blocks_256(bp)), dim3(256), 0, stream, s.rowf, taps, s.p, s.score, H, W, bp);
            hipLaunchKernelGGL(dd_cut_kernel, dim3(B), dim3(1024), 0, stream, s.score, npix, k, s.klist);
            hipLaunchKernelGGL(dd_emit_kernel, dim3(cdiv(kout, 256), B), dim3(256), 0, stream, s.score, s.klist, npix, W, H, k, kout, keypoints, scores, s.kidx,
                               num_keypoints);
            IMCUI_CHECK_LAUNCH(h);
            if (dbg_logits) hipMemcpyAsync(dbg_logits, s.logits, (size_t)loff * sizeof(float), hipMemcpyDeviceToDevice, stream);
            if (dbg_logp) hipMemcpyAsync(dbg_logp, s.logp, (size_t)bp * sizeof(float), hipMemcpyDeviceToDevice, stream);
            if (dbg_score) hipMemcpyAsync(dbg_score, s.score, (size_t)bp * sizeof(float), hipMemcpyDeviceToDevice, stream);
        } else {
            // ---- describe: s.ha = the scale-1 hidden map, accp = the 1/2-resolution accumulated grid
            hipLaunchKernelGGL(dd_describe_kernel, dim3(cdiv(kout, 4), B), dim3(256), 0, stream, s.kidx, s.ha, d.r[1][3].hid, P + l.wt, P + l.bt, accp, H, W, k, kout,
                               descriptors);
            IMCUI_CHECK_LAUNCH(h);
            if (dbg_desc2) hipMemcpyAsync(dbg_desc2, accp, (size_t)(bp / 4) * DD_DESC * sizeof(float), hipMemcpyDeviceToDevice, stream);
        }
    }
    return IMCUI_OK;
}

// test entry: one of the new kernels alone.  op 0: layer 0 of model `model` with Normalize, in = image [B, 3, H, W] -> out [B, H, W, 64]
// (needs packed + dims); op 1: the depth-wise 5x5 + bias + ReLU, in [B, H, W, C], wts = [25][C] weights then [C] bias; op 2: bilinear x2,
// in [B, H, W, C] -> [B, 2H, 2W, C]; op 3: bicubic x2 of the planes in [B, H, W]; op 4: soft-max statistics of in [B, H * W] -> out [B, 2]
// = (max, log sum exp(l - max)), scratch [B, chunks, 2] after them in `out`; op 5: the separable 51-tap filter (rows, then columns) of
// the planes in [B, H, W], wts = 51 taps, out [2, B, H, W]: the filtered planes, then the row pass
extern "C" int imcui_hip_dedode_layer_probe(imcui_hip_t* h, int op, const float* packed, const int* dims, int model, const float* wts, const float* in, int B,
                                            int H, int W, int C, float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B < 1 || H < 1 || W < 1 || !in || !out || (long)B * H * W > 0x7fffffffL / 512 / 4) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode layer probe: shape");
    const long bp = (long)B * H * W;
    if (op == 0) {
        DdDims d;
        std::string why;
        if (!packed || !dd_dims(dims, &d, &why) || model < 0 || model > 1) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode layer probe: layer 0 needs packed weights, dims and a model");
        const DdLayout l = dd_layout(d);
        dd_stem(in, packed + l.m[model].w0, packed + l.m[model].b0, out, B, H, W, stream);
    } else if (op == 1) {
        if (C < 32 || C % 32 || C > 512 || !wts) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode layer probe: C=%d (a multiple of 32 up to 512) and weights", C);
        return dd_dw5(h, in, wts, wts + (size_t)25 * C, out, B, H, W, C, stream);
    } else if (op == 2) {
        if (C < 4 || C % 4 || C > 512) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode layer probe: C=%d (a multiple of 4 up to 512)", C);
        const long n4 = bp * 4 * C / 4;
        hipLaunchKernelGGL(dd_up2_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, in, (long)C, H, W, C, out, (const float*)nullptr, 0L, n4);
    } else if (op == 3) {
        hipLaunchKernelGGL(dd_cub2_kernel, dim3(blocks_256(bp * 4)), dim3(256), 0, stream, in, 1L, H, W, out, (const float*)nullptr, 0L, bp * 4);
    } else if (op == 4) {
        const int npix = H * W, nchunk = cdiv(npix, DD_CHUNK);
        hipLaunchKernelGGL(dd_smax_part_kernel, dim3(nchunk, B), dim3(256), 0, stream, in, npix, out + 2 * B, nchunk);
        hipLaunchKernelGGL(dd_smax_fin_kernel, dim3(B), dim3(256), 0, stream, out + 2 * B, nchunk, out);
    } else if (op == 5) {
        if (!wts) return imcui_set_err(h, IMCUI_ERR_ARG, "dedode layer probe: the filter needs its 51 taps");
        hipLaunchKernelGGL(dd_rowf_kernel, dim3(blocks_256(bp)), dim3(256), 0, stream, in, wts, out + bp, W, 0, bp);
        hipLaunchKernelGGL(dd_colf_kernel, dim3(blocks_256(bp)), dim3(256), 0, stream, out + bp, wts, (const float*)nullptr, out, H, W, bp);
    } else {
        return imcui_set_err(h, IMCUI_ERR_ARG, "dedode layer probe: op %d", op);
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// test entry: the selection code without the networks.  mode 0: `map` is log p [B, H, W] (p = exp(log p) in this file's order, then
// filter, score, cut, rows); mode 1: `map` is the score map itself (cut and rows only: crafted equal scores).  score_out optional.
struct DdSelWs {
    float *stat, *p, *rowf, *score;
    int *klist, *kidx;
    size_t total;
    bool ok;
};
static DdSelWs dd_sel_carve(void* ws, size_t bytes, int B, int H, int W, int k) {
    WsAlloc a(ws, bytes);
    DdSelWs s;
    const size_t bp = (size_t)B * H * W;
    s.stat = a.get<float>((size_t)B * 2);
    s.p = a.get<float>(bp);
    s.rowf = a.get<float>(bp);
    s.score = a.get<float>(bp);
    s.klist = a.get<int>((size_t)B * k);
    s.kidx = a.get<int>((size_t)B * k);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}
extern "C" size_t imcui_hip_dedode_select_probe_workspace_bytes(int B, int H, int W, int k) {
    if (B <= 0 || H <= 0 || W <= 0 || k <= 0) return 0;
    return dd_sel_carve(nullptr, 0, B, H, W, k).total;
}
extern "C" int imcui_hip_dedode_select_probe(imcui_hip_t* h, int mode, const float* taps, const float* map, int B, int H, int W, int k, int kout,
                                             float* keypoints, float* scores, int* num_keypoints, float* score_out, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B < 1 || B > 1024 || H < 1 || W < 1 || (long)B * H * W > 0x7fffffffL / 4 || k < 1 || (long)k > (long)H * W || kout < k || (mode == 0 && !taps) || mode < 0 ||
        mode > 1 || !map || !keypoints || !scores || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "dedode select probe: shape, mode, k=%d outside 1..H*W or kout below k", k);
    const int npix = H * W;
    const long bp = (long)B * npix;
    const DdSelWs s = dd_sel_carve(ws, ws_bytes, B, H, W, k);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "dedode select probe: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const float* score = map;
    if (mode == 0) {
        // (log p is given: with zero statistics dd_logp_kernel leaves it as it is; its log p output lands in the row buffer)
        hipLaunchKernelGGL(zero_i32_kernel<>, dim3(cdiv(2 * B, 256)), dim3(256), 0, stream, reinterpret_cast<int*>(s.stat), 2 * B);
        hipLaunchKernelGGL(dd_logp_kernel, dim3(blocks_256(bp)), dim3(256), 0, stream, map, s.stat, npix, s.rowf, s.p, bp);
        hipLaunchKernelGGL(dd_rowf_kernel, dim3(blocks_256(bp)), dim3(256), 0, stream, s.p, taps, s.rowf, W, 1, bp);
        hipLaunchKernelGGL(dd_colf_kernel, dim3(blocks_256(bp)), dim3(256), 0, stream, s.rowf, taps, s.p, s.score, H, W, bp);
        score = s.score;
    }
    hipLaunchKernelGGL(dd_cut_kernel, dim3(B), dim3(1024), 0, stream, score, npix, k, s.klist);
    hipLaunchKernelGGL(dd_emit_kernel, dim3(cdiv(kout, 256), B), dim3(256), 0, stream, score, s.klist, npix, W, H, k, kout, keypoints, scores, s.kidx, num_keypoints);
    if (score_out) hipMemcpyAsync(score_out, score, (size_t)bp * sizeof(float), hipMemcpyDeviceToDevice, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
