// CosPlace / EigenPlaces global descriptors on MI355X (retrieval_zoo entry cosplace; extractor confs `cosplace` / `eigenplaces`):
// imcui/hloc/extractors/cosplace.py:40-45 and eigenplaces.py:53-58 `_forward` -- tvf.Normalize, a torchvision ResNet-18 / 50 / 101 / 152
// without its pool and classifier, L2Norm over channels, GeM, one linear layer, L2Norm -- as one batched call.  The network itself is NOT
// in the reference checkout (the wrappers fetch it through torch.hub): it is restated from torchvision's ResNet and gmberton/CosPlace's
// cosplace_model/network.py (tests/places_reference.py), so this stage is parity-unpinned.
//
//   stem + pool  pl_stem_kernel: (x - mean) / std as the raw image window is staged in LDS (the zero padding is zero in normalised
//                units), conv1 7x7 / 2 with bn1 folded in float32 at pack time, ReLU, and the 3x3 / 2 max-pool over the conv positions
//                that exist -> NHWC [B, Hp, Wp, 64].  The un-pooled half-resolution map is never written.  fp32 FMA on the VALU.
//   trunk        a launch list over the shared GEMM (gemm.hip / gemm_wreg.hip), BatchNorm folded: every 1x1 a plain GEMM on the NHWC map
//                (a stride-2 shortcut: implicit GEMM conv_k = 1, conv_stride = 2), every 3x3 the implicit GEMM (stride 1 or 2, pad 1);
//                residual and ReLU in the EPI_CONV epilogue; a block's `downsample` is launched first and is the residual
//   GeM          pl_norm_kernel (one wave per pixel: max(|x|, 1e-12)), pl_gem_part_kernel (clamp(x / |x|, 1e-6) ** p summed over chunks of
//                PL_CHUNK = 64 pixels: one [F] partial per chunk), pl_gem_fold_kernel (the partials in chunk order, / (H W), ** (1 / p));
//                p is read from the packed buffer; library powf
//   head         pl_head_kernel: y = W g + b, one wave per output feature, a row's sum one chain per lane in ascending f and the wave
//                butterfly; pl_l2_kernel: y / max(|y|, 1e-12)
// GeM and the head are the same fp32 VALU code in both arithmetic modes.  No float atomics; chunks have a fixed size and are folded in a
// fixed order; every image (row) is computed independently of the batch it rides in.  Nothing synchronises with the host.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "imcui_hip.h"
#include "netpack.h"

#define PL_TPH 4                 // stem: pooled rows ...
#define PL_TPW 8                 // ... and columns of a workgroup's tile
#define PL_CH (2 * PL_TPH + 1)   // conv rows the tile's pool windows cover (9)
#define PL_CW (2 * PL_TPW + 1)   // ... and columns (17)
#define PL_IH (2 * PL_CH + 5)    // image rows those conv positions read (23)
#define PL_IW (2 * PL_CW + 5)    // ... and columns (39)
#define PL_IWP 40                // row pitch of the staged window
#define PL_CS 68                 // floats between two conv positions in LDS (64 channels + 4: 16-byte rows that do not share banks)
#define PL_NPOS (PL_CH * PL_CW)  // 153
#define PL_CHUNK 64              // GeM: pixels per partial

// ------------------------------------------------------------------ the network and its tensor table
struct PlConv {
    int cin, cout, k, stride;
    int layer, blk, role;  // role 0 .. 2: conv1 .. conv3 of block `blk` of layer 1 .. 4; 3: its downsample
    GemmLayerOff g;
};
struct PlBlock {
    int layer, idx, cin, mid, cout, stride;
    int nc, c[3], ds;  // indices into PlNet::convs; ds = -1: the identity shortcut
};
struct PlNet {
    int backbone = 0, F = 0, D = 0;
    bool bott = false;
    std::vector<PlConv> convs;
    std::vector<PlBlock> blocks;
    size_t w0 = 0, b0 = 0, p = 0, hw = 0, hb = 0, total = 0;
};
// torchvision.models.resnet{18,50,101,152} without avgpool / fc; the stride of a bottleneck sits on its 3x3 (v1.5)
static bool pl_net(int backbone, int D, PlNet& n) {
    int depth[4];
    const int d18[4] = {2, 2, 2, 2}, d50[4] = {3, 4, 6, 3}, d101[4] = {3, 4, 23, 3}, d152[4] = {3, 8, 36, 3};
    const int* d = backbone == 18 ? d18 : backbone == 50 ? d50 : backbone == 101 ? d101 : backbone == 152 ? d152 : nullptr;
    if (!d || D < 1 || D > 65536) return false;
    memcpy(depth, d, sizeof(depth));
    n.backbone = backbone;
    n.D = D;
    n.bott = backbone != 18;
    PackCursor c;
    n.w0 = c.get(147 * 64);
    n.b0 = c.get(64);
    auto add = [&](int ci, int co, int k, int s, int layer, int blk, int role) {
        PlConv v{ci, co, k, s, layer, blk, role, {}};
        v.g.place(c, co, k * k * ci);
        n.convs.push_back(v);
        return (int)n.convs.size() - 1;
    };
    int cin = 64;
    for (int L = 0; L < 4; ++L) {
        const int width = 64 << L, cout = n.bott ? 4 * width : width;
        for (int i = 0; i < depth[L]; ++i) {
            PlBlock b{L + 1, i, cin, width, cout, (i == 0 && L > 0) ? 2 : 1, 0, {-1, -1, -1}, -1};
            if (n.bott) {
                b.c[0] = add(cin, width, 1, 1, L + 1, i, 0);
                b.c[1] = add(width, width, 3, b.stride, L + 1, i, 1);
                b.c[2] = add(width, cout, 1, 1, L + 1, i, 2);
                b.nc = 3;
            } else {
                b.c[0] = add(cin, width, 3, b.stride, L + 1, i, 0);
                b.c[1] = add(width, width, 3, 1, L + 1, i, 1);
                b.nc = 2;
            }
            if (b.stride != 1 || cin != cout) b.ds = add(cin, cout, 1, b.stride, L + 1, i, 3);
            n.blocks.push_back(b);
            cin = cout;
        }
    }
    n.F = cin;
    n.p = c.get(1);
    n.hw = c.get((size_t)D * n.F);
    n.hb = c.get(D);
    n.total = c.off;
    return true;
}
// state-dict order of nn.Sequential(conv1, bn1, relu, maxpool, layer1 .. layer4) + the aggregation: a convolution, then the four
// tensors of its BatchNorm
static TensorTable pl_table(const PlNet& n) {
    static const char* BN[4] = {"weight", "bias", "running_mean", "running_var"};
    TensorTable t;
    t.add("backbone.0.weight", 64 * 3 * 49);
    for (int j = 0; j < 4; ++j) t.add(std::string("backbone.1.") + BN[j], 64);
    for (const PlConv& v : n.convs) {
        const std::string blk = "backbone." + std::to_string(3 + v.layer) + "." + std::to_string(v.blk) + ".";
        const std::string cv = v.role == 3 ? blk + "downsample.0" : blk + "conv" + std::to_string(v.role + 1);
        const std::string bn = v.role == 3 ? blk + "downsample.1" : blk + "bn" + std::to_string(v.role + 1);
        t.add(cv + ".weight", (size_t)v.cout * v.cin * v.k * v.k);
        for (int j = 0; j < 4; ++j) t.add(bn + "." + BN[j], v.cout);
    }
    t.add("aggregation.1.p", 1);
    t.add("aggregation.3.weight", (size_t)n.D * n.F);
    t.add("aggregation.3.bias", n.D);
    return t;
}

extern "C" size_t imcui_hip_places_packed_floats(int backbone, int fc_output_dim) {
    PlNet n;
    return pl_net(backbone, fc_output_dim, n) ? n.total : 0;
}
extern "C" int imcui_hip_places_num_tensors(int backbone, int fc_output_dim) {
    PlNet n;
    return pl_net(backbone, fc_output_dim, n) ? 5 + 5 * (int)n.convs.size() + 3 : 0;
}
extern "C" const char* imcui_hip_places_tensor_name(int backbone, int fc_output_dim, int i) {
    static thread_local std::string name;
    PlNet n;
    if (!pl_net(backbone, fc_output_dim, n)) return nullptr;
    const TensorTable t = pl_table(n);
    if (!t.name(i)) return nullptr;
    name = t.name(i);
    return name.c_str();
}

// packed: the stem [tap (ky, kx)][cin 3 (RGB)][64] with bn1's scale folded + its shift; every trunk convolution as a GEMM layer
// [cout][tap][cin] (scale folded, bias = shift, both f16 planes); p; the head's W [D][F] and bias, float32 only
extern "C" int imcui_hip_places_pack_weights(int backbone, int fc_output_dim, const float* const* t, float* packed) {
    PlNet n;
    if (!t || !packed || !pl_net(backbone, fc_output_dim, n)) return IMCUI_ERR_ARG;
    const int nt = 5 + 5 * (int)n.convs.size() + 3;
    for (int i = 0; i < nt; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    memset(packed, 0, n.total * sizeof(float));
    std::vector<float> sc, sh, tmp;
    bn_fold_f32(t + 1, 64, sc, sh);
    for (int co = 0; co < 64; ++co)
        for (int ci = 0; ci < 3; ++ci)
            for (int k = 0; k < 49; ++k) packed[n.w0 + ((size_t)k * 3 + ci) * 64 + co] = t[0][((size_t)co * 3 + ci) * 49 + k] * sc[co];
    memcpy(packed + n.b0, sh.data(), 64 * sizeof(float));
    for (size_t j = 0; j < n.convs.size(); ++j) {
        const PlConv& v = n.convs[j];
        const float* const* tt = t + 5 + 5 * j;
        const int K = v.k * v.k * v.cin;
        bn_fold_f32(tt + 1, v.cout, sc, sh);
        tmp.assign((size_t)v.cout * K, 0.0f);
        pack_conv_gemm(tt[0], v.cout, v.cin, v.k, v.cin, tmp.data());
        float* w = packed + v.g.w;
        for (int co = 0; co < v.cout; ++co)
            for (int k = 0; k < K; ++k) w[(size_t)co * K + k] = tmp[(size_t)co * K + k] * sc[co];
        memcpy(packed + v.g.b, sh.data(), v.cout * sizeof(float));
        v.g.split_planes(packed, v.cout, K);
    }
    const float* const* ta = t + 5 + 5 * n.convs.size();
    packed[n.p] = ta[0][0];
    memcpy(packed + n.hw, ta[1], (size_t)n.D * n.F * sizeof(float));
    memcpy(packed + n.hb, ta[2], n.D * sizeof(float));
    return IMCUI_OK;
}

namespace {

// cosplace.py:41 norm_rgb + backbone.0 (7x7, stride 2, pad 3) + bn1 + ReLU + MaxPool2d(3, 2, 1).  Workgroup (tile x, tile y, image): the
// PL_TPH x PL_TPW pooled pixels from (py0, px0) need the conv positions from (2 py0 - 1, 2 px0 - 1), PL_CH x PL_CW of them, and those the
// image window from (4 py0 - 5, 4 px0 - 5), PL_IH x PL_IW pixels: staged normalised, zeros outside the image.  Wave w owns output channels
// 16 w .. 16 w + 15 (its weights are wave-uniform: scalar loads), a lane one conv position per pass; taps in (ky, kx, channel) order, one
// chain per output, then the shift and the ReLU -> LDS.  The pool then reads 16 bytes per lane, 16 lanes sharing a pixel's 64 channels,
// over the conv positions inside [0, Hc) x [0, Wc) only (the centre always is), and stores NHWC.
__global__ __launch_bounds__(256) void pl_stem_kernel(const float* __restrict__ img, const float* __restrict__ w, const float* __restrict__ shift,
                                                      float* __restrict__ out, int H, int W, int Hc, int Wc, int Hp, int Wp) {
    __shared__ float simg[3 * PL_IH * PL_IWP];
    __shared__ __attribute__((aligned(16))) float sconv[PL_NPOS * PL_CS];
    const int b = blockIdx.z, py0 = blockIdx.y * PL_TPH, px0 = blockIdx.x * PL_TPW;
    const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1, iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;
    for (int i = threadIdx.x; i < 3 * PL_IH * PL_IW; i += 256) {
        const int x = i % PL_IW, t = i / PL_IW, y = t % PL_IH, c = t / PL_IH;
        const int yy = iy0 + y, xx = ix0 + x;
        float v = 0.0f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f, sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
            v = (img[(((long)b * 3 + c) * H + yy) * W + xx] - mean) / sd;
        }
        simg[(c * PL_IH + y) * PL_IWP + x] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* wq = w + wv * 16;
#pragma unroll 1
    for (int it = 0; it < (PL_NPOS + 63) / 64; ++it) {
        const int pos = it * 64 + lane, q = min(pos, PL_NPOS - 1);
        const int ly = q / PL_CW, lx = q - ly * PL_CW;
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {
            const float* wr = wq + ky * 21 * 64;
            const float* ir = simg + (2 * ly + ky) * PL_IWP + 2 * lx;
#pragma unroll
            for (int kx = 0; kx < 7; ++kx)
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const float v = ir[ci * PL_IH * PL_IWP + kx];
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[j] = fmaf(v, wr[(kx * 3 + ci) * 64 + j], acc[j]);
                }
        }
        if (pos < PL_NPOS) {
            float* o = sconv + pos * PL_CS + wv * 16;
#pragma unroll
            for (int j = 0; j < 16; j += 4)
                *reinterpret_cast<float4*>(o + j) =
                    make_float4(fmaxf(acc[j] + shift[wv * 16 + j], 0.0f), fmaxf(acc[j + 1] + shift[wv * 16 + j + 1], 0.0f),
                                fmaxf(acc[j + 2] + shift[wv * 16 + j + 2], 0.0f), fmaxf(acc[j + 3] + shift[wv * 16 + j + 3], 0.0f));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PL_TPH * PL_TPW * 16; i += 256) {
        const int c4 = i & 15, pp = i >> 4, ty = pp / PL_TPW, tx = pp - ty * PL_TPW;
        const int py = py0 + ty, px = px0 + tx;
        if (py >= Hp || px >= Wp) continue;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ly = 2 * ty + dy, lx = 2 * tx + dx, cy = cy0 + ly, cx = cx0 + lx;
                if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) m = max4(m, *reinterpret_cast<const float4*>(sconv + (ly * PL_CW + lx) * PL_CS + c4 * 4));
            }
        *reinterpret_cast<float4*>(out + (((long)b * Hp + py) * Wp + px) * 64 + c4 * 4) = m;
    }
}

// network.py L2Norm in front of GeM: nrm[p] = max(|x[p, :]|, 1e-12), one wave per pixel of x [P, F] (F a multiple of 256)
__global__ __launch_bounds__(256) void pl_norm_kernel(const float* __restrict__ x, int F, long P, float* __restrict__ nrm) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;  // (wave-uniform)
    float ss = 0.0f;
    for (int c = lane * 4; c < F; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + p * F + c);
        ss = fmaf(v.x, v.x, ss);
        ss = fmaf(v.y, v.y, ss);
        ss = fmaf(v.z, v.z, ss);
        ss = fmaf(v.w, v.w, ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) nrm[p] = fmaxf(sqrtf(ss), 1e-12f);
}
// GeM over one chunk of PL_CHUNK pixels of image b: thread = channel c of workgroup (chunk, c / 256, b):
// part[b, chunk, c] = sum_n clamp(x[n, c] / nrm[n], 1e-6) ** p in ascending n
__global__ __launch_bounds__(256) void pl_gem_part_kernel(const float* __restrict__ x, const float* __restrict__ nrm, const float* __restrict__ pp, int F, int N,
                                                          int nchunk, float* __restrict__ part) {
    const int c = blockIdx.y * 256 + threadIdx.x, chunk = blockIdx.x, b = blockIdx.z;
    const float p = pp[0];
    const int n1 = min((chunk + 1) * PL_CHUNK, N);
    float acc = 0.0f;
    for (int n = chunk * PL_CHUNK; n < n1; ++n) {
        const long px = (long)b * N + n;
        acc += powf(fmaxf(x[px * F + c] / nrm[px], 1e-6f), p);
    }
    part[((long)b * nchunk + chunk) * F + c] = acc;
}
// out[b, c] = (sum of the partials in chunk order / N) ** (1 / p)
__global__ __launch_bounds__(256) void pl_gem_fold_kernel(const float* __restrict__ part, const float* __restrict__ pp, int F, int N, int nchunk,
                                                          float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    float s = 0.0f;
    for (int k = 0; k < nchunk; ++k) s += part[((long)b * nchunk + k) * F + c];
    out[(long)b * F + c] = powf(s / (float)N, 1.0f / pp[0]);
}

// nn.Linear(F, D): wave = output feature d of workgroup (d / 4, 4 batch rows): lane l takes f = 4 l, 4 l + 256, .. of the weight row once
// and applies it to the (up to) 4 rows; a row's sum is one chain per lane in ascending f, then the wave butterfly, then the bias: it does
// not depend on the other rows or on B.  F a multiple of 4.
__global__ __launch_bounds__(256) void pl_head_kernel(const float* __restrict__ Wt, const float* __restrict__ bias, const float* __restrict__ g, int B, int F, int D,
                                                      float* __restrict__ y) {
    const int lane = threadIdx.x & 63, d = blockIdx.x * 4 + (threadIdx.x >> 6), b0 = blockIdx.y * 4;
    if (d >= D) return;  // (wave-uniform)
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* wr = Wt + (long)d * F;
    for (int f = lane * 4; f < F; f += 256) {
        const float4 w = *reinterpret_cast<const float4*>(wr + f);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (b0 + r < B) {
                const float4 v = *reinterpret_cast<const float4*>(g + (long)(b0 + r) * F + f);
                float a = acc[r];
                a = fmaf(w.x, v.x, a);
                a = fmaf(w.y, v.y, a);
                a = fmaf(w.z, v.z, a);
                a = fmaf(w.w, v.w, a);
                acc[r] = a;
            }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float s = wave_sum(acc[r]) + bias[d];
        if (lane == 0 && b0 + r < B) y[(long)(b0 + r) * D + d] = s;
    }
}
// network.py's last L2Norm, in place: y[b] / max(|y[b]|, 1e-12); one workgroup per row, the squares in one fixed order
__global__ __launch_bounds__(256) void pl_l2_kernel(float* __restrict__ y, int D) {
    __shared__ float s4[4];
    float* yb = y + (long)blockIdx.x * D;
    float ss = 0.0f;
    for (int d = threadIdx.x; d < D; d += 256) ss = fmaf(yb[d], yb[d], ss);
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(((s4[0] + s4[1]) + s4[2]) + s4[3]), 1e-12f);
    for (int d = threadIdx.x; d < D; d += 256) yb[d] = yb[d] / nrm;  // (a thread's own elements)
}

}  // namespace

// ------------------------------------------------------------------ launch helpers
static int pl_down(int n) { return (n - 1) / 2 + 1; }  // 7x7 / 2 pad 3, 3x3 / 2 pad 1 and 1x1 / 2 pad 0 all give this size

static int pl_stem_launch(imcui_hip_t* h, const float* P, const PlNet& n, const float* image, int B, int H, int W, float* out, hipStream_t stream) {
    const int Hc = pl_down(H), Wc = pl_down(W), Hp = pl_down(Hc), Wp = pl_down(Wc);
    hipLaunchKernelGGL(pl_stem_kernel, dim3(cdiv(Wp, PL_TPW), cdiv(Hp, PL_TPH), B), dim3(256), 0, stream, image, P + n.w0, P + n.b0, out, H, W, Hc, Wc, Hp, Wp);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// one convolution + folded BatchNorm (+ residual) (+ ReLU) on the NHWC map in [B, hin, win, cin] -> out [B, hout, wout, cout]
static int pl_conv(imcui_hip_t* h, const float* P, const PlConv& v, const float* in, int B, int hin, int win, int hout, int wout, const float* resid, int act,
                   float* out, hipStream_t stream) {
    GemmP g;
    g.epi = EPI_CONV;
    g.A = in;
    g.lda = v.cin;
    gemm_set_weights(g, P, v.g, v.cout, v.k * v.k * v.cin, h->precision == 1);
    if (v.k == 3 || v.stride != 1) gemm_set_conv(g, v.k, v.stride, v.k == 3 ? 1 : 0, hin, win, hout, wout, v.cin);
    g.M = B * hout * wout;
    g.C = out;
    g.ldc = v.cout;
    g.resid = resid;
    g.ldr = v.cout;
    g.act = act;
    return gemm_launch(h, g, stream);
}
// BasicBlock / Bottleneck.forward: in [B, hh, ww, cin] -> out [B, ho, wo, cout]; ds (cout wide), t1, t2 (mid wide): scratch maps
static int pl_block(imcui_hip_t* h, const float* P, const PlNet& n, const PlBlock& b, const float* in, int B, int hh, int ww, float* out, float* ds, float* t1,
                    float* t2, hipStream_t stream) {
    const int ho = b.stride == 2 ? pl_down(hh) : hh, wo = b.stride == 2 ? pl_down(ww) : ww;
    int rc;
    const float* idn = in;
    if (b.ds >= 0) {
        IMCUI_RUN(pl_conv(h, P, n.convs[b.ds], in, B, hh, ww, ho, wo, nullptr, 0, ds, stream));
        idn = ds;
    }
    if (n.bott) {
        IMCUI_RUN(pl_conv(h, P, n.convs[b.c[0]], in, B, hh, ww, hh, ww, nullptr, 1, t1, stream));
        IMCUI_RUN(pl_conv(h, P, n.convs[b.c[1]], t1, B, hh, ww, ho, wo, nullptr, 1, t2, stream));
        IMCUI_RUN(pl_conv(h, P, n.convs[b.c[2]], t2, B, ho, wo, ho, wo, idn, 1, out, stream));
    } else {
        IMCUI_RUN(pl_conv(h, P, n.convs[b.c[0]], in, B, hh, ww, ho, wo, nullptr, 1, t1, stream));
        IMCUI_RUN(pl_conv(h, P, n.convs[b.c[1]], t1, B, ho, wo, ho, wo, idn, 1, out, stream));
    }
    return IMCUI_OK;
}
// L2Norm + GeM + Flatten on maps x [B, N, F] -> out [B, F]
static int pl_gem_launch(imcui_hip_t* h, const float* P, const PlNet& n, const float* x, int B, int N, float* nrm, float* part, float* out, hipStream_t stream) {
    const long pix = (long)B * N;
    const int nchunk = cdiv(N, PL_CHUNK);
    hipLaunchKernelGGL(pl_norm_kernel, dim3((unsigned)((pix + 3) / 4)), dim3(256), 0, stream, x, n.F, pix, nrm);
    IMCUI_CHECK_LAUNCH(h);
    hipLaunchKernelGGL(pl_gem_part_kernel, dim3(nchunk, n.F / 256, B), dim3(256), 0, stream, x, nrm, P + n.p, n.F, N, nchunk, part);
    IMCUI_CHECK_LAUNCH(h);
    hipLaunchKernelGGL(pl_gem_fold_kernel, dim3(n.F / 256, B), dim3(256), 0, stream, part, P + n.p, n.F, N, nchunk, out);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
// Linear + L2Norm: g [B, F] -> out [B, D]
static int pl_head_launch(imcui_hip_t* h, const float* P, const PlNet& n, const float* g, int B, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(pl_head_kernel, dim3(cdiv(n.D, 4), cdiv(B, 4)), dim3(256), 0, stream, P + n.hw, P + n.hb, g, B, n.F, n.D, out);
    IMCUI_CHECK_LAUNCH(h);
    hipLaunchKernelGGL(pl_l2_kernel, dim3(B), dim3(256), 0, stream, out, n.D);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ workspace
struct PlWs {
    float *xa, *xb, *ds, *t1, *t2, *nrm, *part, *gem;
    size_t total;
    bool ok;
};
// floats of the largest block input / output (mx) and of the largest map inside a block (mt) over blocks [first, last] entered at hh x ww
static void pl_extent(const PlNet& n, int first, int last, int B, int hh, int ww, size_t* mx, size_t* mt, int* hout, int* wout) {
    *mx = *mt = 0;
    for (int i = first; i <= last; ++i) {
        const PlBlock& b = n.blocks[i];
        const int ho = b.stride == 2 ? pl_down(hh) : hh, wo = b.stride == 2 ? pl_down(ww) : ww;
        const size_t pin = (size_t)B * hh * ww, pout = (size_t)B * ho * wo;
        *mx = std::max(*mx, std::max(pin * b.cin, pout * b.cout));
        *mt = std::max(*mt, (n.bott ? pin : pout) * b.mid);
        hh = ho;
        ww = wo;
    }
    *hout = hh;
    *wout = ww;
}
static PlWs pl_carve(void* ws, size_t bytes, const PlNet& n, int B, size_t mx, size_t mt, size_t N, bool trunk) {
    WsAlloc a(ws, bytes);
    PlWs s;
    s.xa = a.get<float>(trunk ? mx : 0);
    s.xb = a.get<float>(trunk ? mx : 0);
    s.ds = a.get<float>(mx);
    s.t1 = a.get<float>(mt);
    s.t2 = a.get<float>(mt);
    s.nrm = a.get<float>((size_t)B * N);
    s.part = a.get<float>((size_t)B * ((N + PL_CHUNK - 1) / PL_CHUNK) * n.F);
    s.gem = a.get<float>(N ? (size_t)B * n.F : 0);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}
static bool pl_range_ok(int B, int H, int W) {  // every map index of one call below 2^31 (the widest map: 256 channels at the pooled size)
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long)B * pl_down(pl_down(H)) * pl_down(pl_down(W)) <= 0x7fffffffL / 256 && (long)B * H * W <= 0x7fffffffL / 4;
}
extern "C" size_t imcui_hip_places_workspace_bytes(int backbone, int fc_output_dim, int B, int H, int W) {
    PlNet n;
    if (!pl_net(backbone, fc_output_dim, n) || !pl_range_ok(B, H, W)) return 0;
    size_t mx, mt;
    int h4, w4;
    pl_extent(n, 0, (int)n.blocks.size() - 1, B, pl_down(pl_down(H)), pl_down(pl_down(W)), &mx, &mt, &h4, &w4);
    return pl_carve(nullptr, 0, n, B, mx, mt, (size_t)h4 * w4, true).total;
}

extern "C" int imcui_hip_places_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, int backbone, int fc_output_dim,
                                        float* descriptor, float* map, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    PlNet n;
    if (!pl_net(backbone, fc_output_dim, n))
        return imcui_set_err(h, IMCUI_ERR_ARG, "places: unknown backbone %d (18, 50, 101 or 152 for ResNet-18 / 50 / 101 / 152) or fc_output_dim %d", backbone,
                             fc_output_dim);
    if (C != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "places: the image has %d channels, 3 (RGB) are needed", C);
    if (!pl_range_ok(B, H, W)) return imcui_set_err(h, IMCUI_ERR_ARG, "places: B=%d images of %dx%d exceed the 2^31 index range of one call", B, H, W);
    if (!packed || !image || !descriptor) return imcui_set_err(h, IMCUI_ERR_ARG, "places: null argument");
    const int Hp = pl_down(pl_down(H)), Wp = pl_down(pl_down(W));
    size_t mx, mt;
    int h4, w4;
    pl_extent(n, 0, (int)n.blocks.size() - 1, B, Hp, Wp, &mx, &mt, &h4, &w4);
    const PlWs s = pl_carve(ws, ws_bytes, n, B, mx, mt, (size_t)h4 * w4, true);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "places: workspace too small (%zu < %zu)", ws_bytes, s.total);
    int rc;
    IMCUI_RUN(pl_stem_launch(h, packed, n, image, B, H, W, s.xa, stream));
    float *cur = s.xa, *oth = s.xb;
    int hh = Hp, ww = Wp;
    for (const PlBlock& b : n.blocks) {
        IMCUI_RUN(pl_block(h, packed, n, b, cur, B, hh, ww, oth, s.ds, s.t1, s.t2, stream));
        std::swap(cur, oth);
        if (b.stride == 2) {
            hh = pl_down(hh);
            ww = pl_down(ww);
        }
    }
    if (map) hipMemcpyAsync(map, cur, (size_t)B * hh * ww * n.F * sizeof(float), hipMemcpyDeviceToDevice, stream);
    IMCUI_RUN(pl_gem_launch(h, packed, n, cur, B, hh * ww, s.nrm, s.part, s.gem, stream));
    return pl_head_launch(h, packed, n, s.gem, B, descriptor, stream);
}

// ------------------------------------------------------------------ test entries
static int pl_find_block(const PlNet& n, int layer, int block) {
    for (size_t i = 0; i < n.blocks.size(); ++i)
        if (n.blocks[i].layer == layer && n.blocks[i].idx == block) return (int)i;
    return -1;
}
extern "C" size_t imcui_hip_places_probe_workspace_bytes(int backbone, int fc_output_dim, int op, int B, int H, int W, int layer, int block) {
    PlNet n;
    if (!pl_net(backbone, fc_output_dim, n) || B < 1 || H < 1 || W < 1) return 0;
    if (op == 1) {
        const int i = pl_find_block(n, layer, block);
        if (i < 0) return 0;
        size_t mx, mt;
        int ho, wo;
        pl_extent(n, i, i, B, H, W, &mx, &mt, &ho, &wo);
        return pl_carve(nullptr, 0, n, B, mx, mt, 0, false).total;
    }
    if (op == 2) return pl_carve(nullptr, 0, n, B, 0, 0, (size_t)H * W, false).total;
    return 256;
}
// test entry: one stage alone, through the launch code of the forward.  op 0: stem + pool, in = image [B, 3, H, W] RGB in [0, 1] -> out
// [B, Hp, Wp, 64]; op 1: block `block` of layer 1 .. 4, in [B, H, W, cin] -> out [B, Ho, Wo, cout], in the handle's arithmetic mode; op 2:
// L2Norm + GeM, in [B, H, W, F] -> out [B, F]; op 3: Linear + L2Norm, in [B, F] (H = W = 1) -> out [B, D]
extern "C" int imcui_hip_places_layer_probe(imcui_hip_t* h, int op, int backbone, int fc_output_dim, const float* packed, const float* in, int B, int H, int W,
                                            int layer, int block, float* out, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    PlNet n;
    if (!pl_net(backbone, fc_output_dim, n)) return imcui_set_err(h, IMCUI_ERR_ARG, "places layer probe: unknown backbone %d or fc_output_dim %d", backbone, fc_output_dim);
    if (!packed || !in || !out || !pl_range_ok(B, H, W) || (long)B * H * W > 0x7fffffffL / 2048) return imcui_set_err(h, IMCUI_ERR_ARG, "places layer probe: shape");
    const size_t need = imcui_hip_places_probe_workspace_bytes(backbone, fc_output_dim, op, B, H, W, layer, block);
    if (op == 0) return pl_stem_launch(h, packed, n, in, B, H, W, out, stream);
    if (op == 1) {
        const int i = pl_find_block(n, layer, block);
        if (i < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "places layer probe: ResNet-%d has no block %d in layer %d", backbone, block, layer);
        size_t mx, mt;
        int ho, wo;
        pl_extent(n, i, i, B, H, W, &mx, &mt, &ho, &wo);
        const PlWs s = pl_carve(ws, ws_bytes, n, B, mx, mt, 0, false);
        if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "places layer probe: workspace too small (%zu < %zu)", ws_bytes, need);
        return pl_block(h, packed, n, n.blocks[i], in, B, H, W, out, s.ds, s.t1, s.t2, stream);
    }
    if (op == 2) {
        const PlWs s = pl_carve(ws, ws_bytes, n, B, 0, 0, (size_t)H * W, false);
        if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "places layer probe: workspace too small (%zu < %zu)", ws_bytes, need);
        return pl_gem_launch(h, packed, n, in, B, H * W, s.nrm, s.part, out, stream);
    }
    if (op == 3) return pl_head_launch(h, packed, n, in, B, out, stream);
    return imcui_set_err(h, IMCUI_ERR_ARG, "places layer probe: op %d", op);
}
