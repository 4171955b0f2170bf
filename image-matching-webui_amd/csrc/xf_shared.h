// What XFeat (xfeat.hip) and LiftFeat (liftfeat.hip, whose dense part is the XFeat trunk) both use: the layer table and packed layout of
// XFeatModel, the InstanceNorm statistics, block1 on the VALU, the unfold / fuse / soft-max kernels, the trunk's launch sequence
// (xf_trunk_feats, xf_trunk_kpts), the 5x5 NMS predicate and the float32 grid arithmetic of InterpolateSparse2d with its three sampling
// rules.  What a network does around the trunk (input stage, heads, selection rule) stays in its own file.
#pragma once
#include <math.h>

#include "gemm.h"
#include "imcui_hip.h"
#include "net_kernels.h"
#include "netpack.h"
#include "select.h"

namespace {  // internal linkage: two translation units include these kernels

// ------------------------------------------------------------------ layer table and packed weight layout
struct XfLayer {
    const char* name;  // state-dict prefix
    int cin, cout, k, stride;
    int bn;    // BasicLayer: Conv2d(bias=False) + BatchNorm2d(affine=False) + ReLU; else Conv2d with bias, no activation
    int cpad;  // input channels as stored (GEMM layers: a multiple of 32)
    int npad;  // output channels as stored
};
#define XF_NL 26
#define XF_NSTEM 4
#define XF_L_HEAT 21  // heatmap_head.2 (64 -> 1): evaluated in the head epilogue
static const XfLayer XF_LAYERS[XF_NL] = {
    {"block1.0", 1, 4, 3, 1, 1, 1, 4},           {"block1.1", 4, 8, 3, 2, 1, 4, 8},          {"block1.2", 8, 8, 3, 1, 1, 8, 8},
    {"block1.3", 8, 24, 3, 2, 1, 8, 32},         {"block2.0", 24, 24, 3, 1, 1, 32, 32},      {"block2.1", 24, 24, 3, 1, 1, 32, 32},
    {"block3.0", 24, 64, 3, 2, 1, 32, 64},       {"block3.1", 64, 64, 3, 1, 1, 64, 64},      {"block3.2", 64, 64, 1, 1, 1, 64, 64},
    {"block4.0", 64, 64, 3, 2, 1, 64, 64},       {"block4.1", 64, 64, 3, 1, 1, 64, 64},      {"block4.2", 64, 64, 3, 1, 1, 64, 64},
    {"block5.0", 64, 128, 3, 2, 1, 64, 128},     {"block5.1", 128, 128, 3, 1, 1, 128, 128},  {"block5.2", 128, 128, 3, 1, 1, 128, 128},
    {"block5.3", 128, 64, 1, 1, 1, 128, 64},     {"block_fusion.0", 64, 64, 3, 1, 1, 64, 64}, {"block_fusion.1", 64, 64, 3, 1, 1, 64, 64},
    {"block_fusion.2", 64, 64, 1, 1, 0, 64, 64}, {"heatmap_head.0", 64, 64, 1, 1, 1, 64, 64}, {"heatmap_head.1", 64, 64, 1, 1, 1, 64, 64},
    {"heatmap_head.2", 64, 1, 1, 1, 0, 64, 1},   {"keypoint_head.0", 64, 64, 1, 1, 1, 64, 64}, {"keypoint_head.1", 64, 64, 1, 1, 1, 64, 64},
    {"keypoint_head.2", 64, 64, 1, 1, 1, 64, 64}, {"keypoint_head.3", 64, 65, 1, 1, 0, 64, 65},
};
#define XF_BN_EPS 1e-5

static bool xf_is_gemm(int i) { return i >= XF_NSTEM && i != XF_L_HEAT; }

// The buffer begins with block1.0 folded with its BatchNorm as [9 taps][1][4] floats, followed (from float 64) by its 4 folded biases.
struct XfLayout {
    GemmLayerOff g[XF_NL];  // stem / heat: w = [tap][cin][cout] and b only; GEMM: [npad][tap][cpad] + f16 planes
    size_t skw, skb;        // skip1.1: weight [24], bias [24]
    size_t total;
};

static XfLayout xf_layout() {
    XfLayout l;
    PackCursor c;
    for (int i = 0; i < XF_NL; ++i) {
        const XfLayer& L = XF_LAYERS[i];
        if (!xf_is_gemm(i)) {
            l.g[i].w = c.get((size_t)L.k * L.k * L.cin * L.cout);
            l.g[i].b = c.get(L.cout);
        } else {
            l.g[i].place(c, L.npad, L.k * L.k * L.cpad);
        }
    }
    l.skw = c.get(24);
    l.skb = c.get(24);
    l.total = c.off;
    return l;
}

// tensors: skip1.1.weight, skip1.1.bias, then per layer (upstream's module order) `layer.0.weight`, `layer.1.running_mean`,
// `layer.1.running_var` for a BasicLayer and `weight`, `bias` for a plain convolution
static int xf_tensor_of_layer(int layer) {
    int t = 2;
    for (int i = 0; i < layer; ++i) t += XF_LAYERS[i].bn ? 3 : 2;
    return t;
}
static int xf_num_tensors() { return xf_tensor_of_layer(XF_NL); }

// ------------------------------------------------------------------ input stage
// image [B, C, H, W] (C = 1 or 3) -> gray [B, Hr, Wr]: every channel resized (skipped when the sizes are equal: the interpolation is
// then the identity), then the channel mean, summed in double so that three equal channels give the channel itself
__global__ __launch_bounds__(256) void xf_gray_kernel(const float* __restrict__ img, float* __restrict__ gray, int C, int H, int W, int Hr, int Wr,
                                                      float sh, float sw, long npix) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % Wr);
    const long q = p / Wr;
    const int y = (int)(q % Hr);
    const long b = q / Hr;
    double acc = 0.0;
    if (H == Hr && W == Wr) {
        for (int c = 0; c < C; ++c) acc += (double)img[((b * C + c) * H + y) * (long)W + x];
    } else {
        int y0, y1, x0, x1;
        float hy0, hy1, wx0, wx1;
        bilinear_src_half_pixel(y, sh, H, &y0, &y1, &hy0, &hy1);
        bilinear_src_half_pixel(x, sw, W, &x0, &x1, &wx0, &wx1);
        for (int c = 0; c < C; ++c) {
            const float* pl = img + (b * C + c) * (long)H * W;
            const float v00 = pl[(long)y0 * W + x0], v01 = pl[(long)y0 * W + x1], v10 = pl[(long)y1 * W + x0], v11 = pl[(long)y1 * W + x1];
            const float top = __fadd_rn(__fmul_rn(wx0, v00), __fmul_rn(wx1, v01)), bot = __fadd_rn(__fmul_rn(wx0, v10), __fmul_rn(wx1, v11));
            acc += (double)__fadd_rn(__fmul_rn(hy0, top), __fmul_rn(hy1, bot));
        }
    }
    gray[p] = (float)(acc / (double)C);
}

// InstanceNorm2d(1) statistics, deterministic.  pass 1: block (chunk, b) sums XF_STAT_CHUNK pixels in double (thread t takes pixels
// t, t + 256, ...; the 256 sums are added by a fixed tree) -> part [b][chunk][2] = (sum, sum of squares)
#define XF_STAT_CHUNK 4096
__global__ __launch_bounds__(256) void xf_stats_part_kernel(const float* __restrict__ gray, long npix, int nchunk, double* __restrict__ part) {
    __shared__ double s1[256], s2[256];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const long p0 = (long)chunk * XF_STAT_CHUNK, p1 = min(p0 + XF_STAT_CHUNK, npix);
    const float* src = gray + (long)b * npix;
    double a = 0.0, q = 0.0;
    for (long p = p0 + tid; p < p1; p += 256) {
        const double v = (double)src[p];
        a += v;
        q += v * v;
    }
    s1[tid] = a;
    s2[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            s1[tid] += s1[tid + o];
            s2[tid] += s2[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[((size_t)b * nchunk + chunk) * 2 + 0] = s1[0];
        part[((size_t)b * nchunk + chunk) * 2 + 1] = s2[0];
    }
}
// pass 2: one thread per image adds the chunk partials in chunk order; biased variance, eps 1e-5.  norm [b][2] = (alpha, beta) of
// ATen's out = x * alpha + beta, alpha = invstd, beta = -mean * invstd
__global__ __launch_bounds__(64) void xf_stats_fin_kernel(const double* __restrict__ part, long npix, int nchunk, int B, float* __restrict__ norm) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double sa = 0.0, sq = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        sa += part[((size_t)b * nchunk + k) * 2 + 0];
        sq += part[((size_t)b * nchunk + k) * 2 + 1];
    }
    const double m = sa / (double)npix;
    const double var = fmax(sq / (double)npix - m * m, 0.0);
    const float al = (float)(1.0 / sqrt(var + 1e-5));
    norm[2 * b + 0] = al;
    norm[2 * b + 1] = __fmul_rn(-(float)m, al);
}
__device__ __forceinline__ float xf_norm(float v, float al, float be) { return __fadd_rn(__fmul_rn(v, al), be); }

// ------------------------------------------------------------------ stem: block1 on the VALU
// 3x3, pad 1, stride S, folded bias, ReLU; NHWC in [B, hi, wi, CIN] -> out [B, ho, wo, OST] (channels COUT .. OST - 1 zero).  One
// thread per output pixel, the weights [tap][CIN][COUT] in LDS; fp32 FMA in (tap, channel) order.
// FIRST: the input is the gray image, normalised while it is loaded (the zero padding is the NORMALISED image's).
// SKIP:  adds skip1(x) after the ReLU: the 4x4 average of the normalised gray image around this 1/4-resolution pixel, times skw + skb.
template <int CIN, int COUT, int OST, int S, bool FIRST, bool SKIP>
__global__ __launch_bounds__(256) void xf_stem_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, int hi, int wi, int ho, int wo, long npix, const float* __restrict__ norm,
                                                      const float* __restrict__ gray, const float* __restrict__ skw, const float* __restrict__ skb) {
    __shared__ float sw[9 * CIN * COUT + COUT + 2 * COUT];
    for (int i = threadIdx.x; i < 9 * CIN * COUT; i += 256) sw[i] = w[i];
    if (threadIdx.x < COUT) {
        sw[9 * CIN * COUT + threadIdx.x] = bias[threadIdx.x];
        if (SKIP) {
            sw[9 * CIN * COUT + COUT + threadIdx.x] = skw[threadIdx.x];
            sw[9 * CIN * COUT + 2 * COUT + threadIdx.x] = skb[threadIdx.x];
        }
    }
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % wo);
    const long q = p / wo;
    const int y = (int)(q % ho);
    const long b = q / ho;
    float al = 1.0f, be = 0.0f;
    if (FIRST || SKIP) {
        al = norm[2 * b];
        be = norm[2 * b + 1];
    }
    float acc[COUT];
#pragma unroll
    for (int c = 0; c < COUT; ++c) acc[c] = sw[9 * CIN * COUT + c];
    const float* src = in + b * (long)hi * wi * CIN;
    // (the tap loops stay rolled: unrolled, the compiler hoists all 9 CIN COUT weight reads and spills)
#pragma unroll 1
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y * S - 1 + ky;
#pragma unroll 1
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x * S - 1 + kx;
            const bool inside = iy >= 0 && iy < hi && ix >= 0 && ix < wi;
            float v[CIN];
            if (FIRST) {
                v[0] = inside ? xf_norm(src[(long)iy * wi + ix], al, be) : 0.0f;
            } else {
#pragma unroll
                for (int c4 = 0; c4 < CIN / 4; ++c4) {
                    const float4 t = inside ? *reinterpret_cast<const float4*>(src + ((long)iy * wi + ix) * CIN + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                    v[4 * c4 + 0] = t.x;
                    v[4 * c4 + 1] = t.y;
                    v[4 * c4 + 2] = t.z;
                    v[4 * c4 + 3] = t.w;
                }
            }
            const float* k = sw + (ky * 3 + kx) * CIN * COUT;
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                for (int c = 0; c < COUT; ++c) acc[c] = fmaf(v[ci], k[ci * COUT + c], acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < COUT; ++c) acc[c] = fmaxf(acc[c], 0.0f);
    if (SKIP) {  // avg_pool2d(4, 4): ATen sums the window in row-major order and divides by 16
        const float* g = gray + b * (long)(4 * ho) * (4 * wo) + (long)(4 * y) * (4 * wo) + 4 * x;
        float s = 0.0f;
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) s = __fadd_rn(s, xf_norm(g[(long)dy * (4 * wo) + dx], al, be));
        s = s / 16.0f;
#pragma unroll
        for (int c = 0; c < COUT; ++c) acc[c] = __fadd_rn(acc[c], fmaf(s, sw[9 * CIN * COUT + COUT + c], sw[9 * CIN * COUT + 2 * COUT + c]));
    }
    float4* o = reinterpret_cast<float4*>(out + p * OST);
#pragma unroll
    for (int c = 0; c < COUT / 4; ++c) o[c] = make_float4(acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]);
#pragma unroll
    for (int c = COUT / 4; c < OST / 4; ++c) o[c] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// the 8x8 cells of the normalised gray image as 64 channels (channel = dy * 8 + dx): [B, Hr, Wr] -> [B, Hr/8, Wr/8, 64]
__global__ __launch_bounds__(256) void xf_unfold_kernel(const float* __restrict__ gray, const float* __restrict__ norm, float* __restrict__ out, int h8,
                                                        int w8, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c4 = (int)(i & 15);
    long t = i >> 4;
    const int x = (int)(t % w8);
    t /= w8;
    const int y = (int)(t % h8);
    const long b = t / h8;
    const float al = norm[2 * b], be = norm[2 * b + 1];
    const int dy = c4 >> 1, dx = (c4 & 1) * 4;
    const float4 v = *reinterpret_cast<const float4*>(gray + (b * 8 * h8 + 8 * y + dy) * (long)(8 * w8) + 8 * x + dx);
    *reinterpret_cast<float4*>(out + i * 4) = make_float4(xf_norm(v.x, al, be), xf_norm(v.y, al, be), xf_norm(v.z, al, be), xf_norm(v.w, al, be));
}

// ------------------------------------------------------------------ x3 + up(x4) + up(x5): bilinear, align_corners=False (ATen's formula)
__device__ __forceinline__ float4 xf_bilinear4(const float* __restrict__ m, int h, int w, float scale, int oy, int ox, int c) {
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    bilinear_src_half_pixel(oy, scale, h, &y0, &y1, &hy0, &hy1);
    bilinear_src_half_pixel(ox, scale, w, &x0, &x1, &wx0, &wx1);
    const float4 v00 = *reinterpret_cast<const float4*>(m + ((long)y0 * w + x0) * 64 + c), v01 = *reinterpret_cast<const float4*>(m + ((long)y0 * w + x1) * 64 + c);
    const float4 v10 = *reinterpret_cast<const float4*>(m + ((long)y1 * w + x0) * 64 + c), v11 = *reinterpret_cast<const float4*>(m + ((long)y1 * w + x1) * 64 + c);
    float4 o;
    o.x = hy0 * (wx0 * v00.x + wx1 * v01.x) + hy1 * (wx0 * v10.x + wx1 * v11.x);
    o.y = hy0 * (wx0 * v00.y + wx1 * v01.y) + hy1 * (wx0 * v10.y + wx1 * v11.y);
    o.z = hy0 * (wx0 * v00.z + wx1 * v01.z) + hy1 * (wx0 * v10.z + wx1 * v11.z);
    o.w = hy0 * (wx0 * v00.w + wx1 * v01.w) + hy1 * (wx0 * v10.w + wx1 * v11.w);
    return o;
}
// x3 [B, h, w, 64], x4 [B, h/2, w/2, 64], x5 [B, h/4, w/4, 64] -> out [B, h, w, 64] = (x3 + up(x4)) + up(x5)
__global__ __launch_bounds__(256) void xf_fuse_kernel(const float* __restrict__ x3, const float* __restrict__ x4, const float* __restrict__ x5,
                                                      float* __restrict__ out, int h, int w, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)(i & 15) * 4;
    long t = i >> 4;
    const int x = (int)(t % w);
    t /= w;
    const int y = (int)(t % h);
    const long b = t / h;
    const float4 a = *reinterpret_cast<const float4*>(x3 + i * 4);
    const float4 u4 = xf_bilinear4(x4 + b * (long)(h / 2) * (w / 2) * 64, h / 2, w / 2, 0.5f, y, x, c);
    const float4 u5 = xf_bilinear4(x5 + b * (long)(h / 4) * (w / 4) * 64, h / 4, w / 4, 0.25f, y, x, c);
    *reinterpret_cast<float4*>(out + i * 4) = make_float4((a.x + u4.x) + u5.x, (a.y + u4.y) + u5.y, (a.z + u4.z) + u5.z, (a.w + u4.w) + u5.w);
}

// ------------------------------------------------------------------ head epilogues
// One wave per 1/8-resolution pixel, lane = channel: reliability = sigmoid(hh . w + b) (heatmap_head.2), M1 = feats / max(|feats|, 1e-12)
__global__ __launch_bounds__(256) void xf_heads_kernel(const float* __restrict__ feats, const float* __restrict__ hh, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ m1, float* __restrict__ rel, long npix) {
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= npix) return;
    const float f = feats[p * 64 + lane];
    const float nrm = sqrtf(wave_sum(f * f));
    m1[p * 64 + lane] = f / fmaxf(nrm, 1e-12f);
    const float d = wave_sum(hh[p * 64 + lane] * w[lane]);
    if (lane == 0) rel[p] = sigmoidf_(d + bias[0]);
}

// One wave per 8x8 cell: soft-max over the 65 logits (lane c: logit c, lane 0 also the dustbin), the dustbin dropped, channel
// c = dy * 8 + dx written to pixel (8 y + dy, 8 x + dx) of K1h [B, Hr, Wr]
__global__ __launch_bounds__(256) void xf_softmax_kernel(const float* __restrict__ logits, float* __restrict__ k1h, int h8, int w8, long ncell) {
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= ncell) return;
    const float v = logits[p * 65 + lane], dust = logits[p * 65 + 64];
    const float m = fmaxf(wave_max(v), dust);
    const float e = expf(v - m);
    const float sum = wave_sum(e) + expf(dust - m);
    const int x = (int)(p % w8);
    const long t = p / w8;
    const int y = (int)(t % h8);
    const long b = t / h8;
    k1h[(b * 8 * h8 + 8 * y + (lane >> 3)) * (long)(8 * w8) + 8 * x + (lane & 7)] = e / sum;
}

// ------------------------------------------------------------------ selection
// NMS: a pixel is a key-point iff it equals max_pool2d(5, stride 1, pad 2) of its map (no neighbour is greater: an exact plateau keeps
// every member) and exceeds the threshold (strict)
struct XfKeep {
    int h, w;
    float thr;
    __device__ void bind(int) {}
    __device__ bool operator()(const float* hm, int idx) const {
        const int y = idx / w, x = idx - y * w;
        const float v = hm[idx];
        if (!(v > thr)) return false;
        for (int dy = -2; dy <= 2; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= h) continue;
            for (int dx = -2; dx <= 2; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= w) continue;
                if (hm[(long)yy * w + xx] > v) return false;
            }
        }
        return true;
    }
};

// The reference samples with F.grid_sample(align_corners=False) at grid = 2 * (p / (full - 1)) - 1 (float32, p the integer pixel of the
// Hr x Wr image, full = Wr or Hr) whatever the size of the sampled map.  Source coordinate: ATen's vectorised CPU kernel evaluates
// (grid + 1) * (size / 2) - 0.5 with ONE rounding for the multiply-subtract (its build contracts it to an FMA), reproduced here
__device__ __forceinline__ float xf_coord(int p, int full, int size) {
    const float g = __fsub_rn(__fmul_rn(2.0f, __fdiv_rn((float)p, (float)(full - 1))), 1.0f);
    return fmaf(__fadd_rn(g, 1.0f), 0.5f * (float)size, -0.5f);
}
// mode nearest: nearbyint (half to even), zeros outside
__device__ __forceinline__ float xf_sample_nearest(const float* __restrict__ m, int h, int w, float fx, float fy) {
    const float rx = rintf(fx), ry = rintf(fy);
    if (!(rx >= 0.0f && rx < (float)w && ry >= 0.0f && ry < (float)h)) return 0.0f;
    return m[(long)(int)ry * w + (int)rx];
}
// mode bilinear, zeros outside: nw * (x1 - x)(y1 - y) + ne * (x - x0)(y1 - y) + sw * (x1 - x)(y - y0) + se * (x - x0)(y - y0)
__device__ __forceinline__ float xf_sample_bilinear(const float* __restrict__ m, int h, int w, float fx, float fy) {
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
    const float wnw = __fmul_rn(__fsub_rn(x1, fx), __fsub_rn(y1, fy)), wne = __fmul_rn(__fsub_rn(fx, x0), __fsub_rn(y1, fy));
    const float wsw = __fmul_rn(__fsub_rn(x1, fx), __fsub_rn(fy, y0)), wse = __fmul_rn(__fsub_rn(fx, x0), __fsub_rn(fy, y0));
    const int ix0 = (int)x0, iy0 = (int)y0, ix1 = ix0 + 1, iy1 = iy0 + 1;
    auto at = [&](int yy, int xx) { return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? m[(long)yy * w + xx] : 0.0f; };
    float r = __fmul_rn(at(iy0, ix0), wnw);  // ATen: nw * w_nw + ne * w_ne + ..., the additions contracted to FMAs
    r = fmaf(at(iy0, ix1), wne, r);
    r = fmaf(at(iy1, ix0), wsw, r);
    r = fmaf(at(iy1, ix1), wse, r);
    return r;
}
// ATen's cubic convolution coefficients, A = -0.75
__device__ __forceinline__ void xf_cubic(float t, float* c) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}
// mode bicubic, zeros outside, of channel `lane` of the NHWC map m [h, w, 64]: rows interpolated along x, then along y
__device__ __forceinline__ float xf_sample_bicubic(const float* __restrict__ m, int h, int w, float fx, float fy, int lane) {
    const float x0 = floorf(fx), y0 = floorf(fy);
    float cx[4], cy[4];
    xf_cubic(fx - x0, cx);
    xf_cubic(fy - y0, cy);
    const int ix = (int)x0 - 1, iy = (int)y0 - 1;
    float r = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = iy + j;
        float row = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xx = ix + i;
            const float v = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? m[((long)yy * w + xx) * 64 + lane] : 0.0f;
            row += v * cx[i];
        }
        r += row * cy[j];
    }
    return r;
}

// score of candidate i = nearest(K1h) x bilinear(reliability); a key-point at exactly (0, 0) is taken for padding: -1.
// npos [b] counts the positive scores (integer atomics: order-free).  Grid (cdiv(ccap, 256), B).
__global__ __launch_bounds__(256) void xf_score_kernel(const float* __restrict__ k1h, const float* __restrict__ rel, const int* __restrict__ cidx,
                                                       const int* __restrict__ ncand, int ccap, int Hr, int Wr, float* __restrict__ cfinal,
                                                       int* __restrict__ npos) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(ncand[b], ccap)) return;
    const int idx = cidx[(long)b * ccap + i];
    const int y = idx / Wr, x = idx - y * Wr;
    const int h8 = Hr / 8, w8 = Wr / 8;
    const float a = xf_sample_nearest(k1h + (long)b * Hr * Wr, Hr, Wr, xf_coord(x, Wr, Wr), xf_coord(y, Hr, Hr));
    const float r = xf_sample_bilinear(rel + (long)b * h8 * w8, h8, w8, xf_coord(x, Wr, w8), xf_coord(y, Hr, h8));
    float s = __fmul_rn(a, r);
    if (idx == 0) s = -1.0f;
    cfinal[(long)b * ccap + i] = s;
    if (s > 0.0f) atomicAdd(npos + b, 1);
}

// how many key-points image b returns: the sorted list cut by Python's [:top_k] (negative: all but the last -top_k), then score > 0
// (the positive scores are a prefix of the sorted list), then the output capacity
__device__ __forceinline__ int xf_count(int n, int npos, int top_k, int kcap, bool* overflow) {
    const int limit = top_k >= 0 ? min(top_k, n) : max(n + top_k, 0);
    const int want = min(limit, npos);
    *overflow = want > kcap;
    return min(want, kcap);
}

// rank of candidate i in (score descending, flat index ascending) order: the candidates are in row-major order, so among equal scores
// the earlier list entry goes first.  Candidates whose rank is below the count are written to row `rank` of the outputs; crank [b][i]
// = that row or -1.  Grid (cdiv(ccap, 256), B); every block walks the image's whole list through LDS.
__global__ __launch_bounds__(256) void xf_rank_kernel(const float* __restrict__ cfinal, const int* __restrict__ cidx, const int* __restrict__ ncand,
                                                      const int* __restrict__ npos, int ccap, int top_k, int kcap, int Wr, float rw, float rh,
                                                      float* __restrict__ kpts, float* __restrict__ scores, int* __restrict__ crank) {
    __shared__ float ss[256];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(ncand[b], ccap);
    if (blockIdx.x * 256 >= n) return;
    const float* cs = cfinal + (long)b * ccap;
    const float mine = i < n ? cs[i] : 0.0f;
    int rank = 0;
    for (int base = 0; base < n; base += 256) {
        __syncthreads();
        if (base + threadIdx.x < n) ss[threadIdx.x] = cs[base + threadIdx.x];
        __syncthreads();
        const int m = min(256, n - base);
        for (int j = 0; j < m; ++j) {
            const float o = ss[j];
            rank += (o > mine || (o == mine && base + j < i)) ? 1 : 0;
        }
    }
    if (i >= n) return;
    bool ovf;
    const int cnt = xf_count(n, npos[b], top_k, kcap, &ovf);
    const bool keep = rank < cnt;
    crank[(long)b * ccap + i] = keep ? rank : -1;
    if (keep) {
        const int idx = cidx[(long)b * ccap + i];
        const int y = idx / Wr, x = idx - y * Wr;
        kpts[((long)b * kcap + rank) * 2 + 0] = __fmul_rn((float)x, rw);
        kpts[((long)b * kcap + rank) * 2 + 1] = __fmul_rn((float)y, rh);
        scores[(long)b * kcap + rank] = mine;
    }
}

// rows past the count are zero; the count and the status word.  Grid (cdiv(kcap, 4), B), one wave per output row.
__global__ __launch_bounds__(256) void xf_finish_kernel(const int* __restrict__ ncand, const int* __restrict__ npos, int ccap, int top_k, int kcap,
                                                        float* __restrict__ kpts, float* __restrict__ scores, float* __restrict__ desc,
                                                        int* __restrict__ nkpts, int* __restrict__ status) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    bool ovf;
    const int cnt = xf_count(min(ncand[b], ccap), npos[b], top_k, kcap, &ovf);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        nkpts[b] = cnt;
        if (ovf) atomicOr(status, 2);  // output capacity too small
    }
    if (row >= kcap || row < cnt) return;
    desc[((long)b * kcap + row) * 64 + lane] = 0.0f;
    if (lane < 2) kpts[((long)b * kcap + row) * 2 + lane] = 0.0f;
    if (lane == 2) scores[(long)b * kcap + row] = 0.0f;
}

// descriptors: one wave per kept candidate (grid-stride over the list), lane = channel: bicubic sample of M1 [h8, w8, 64], L2 norm
__global__ __launch_bounds__(256) void xf_desc_kernel(const float* __restrict__ m1, const int* __restrict__ cidx, const int* __restrict__ crank,
                                                      const int* __restrict__ ncand, int ccap, int kcap, int Hr, int Wr, float* __restrict__ desc) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int n = min(ncand[b], ccap), h8 = Hr / 8, w8 = Wr / 8;
    const float* m = m1 + (long)b * h8 * w8 * 64;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const int row = crank[(long)b * ccap + i];
        if (row < 0) continue;
        const int idx = cidx[(long)b * ccap + i];
        const int y = idx / Wr, x = idx - y * Wr;
        const float v = xf_sample_bicubic(m, h8, w8, xf_coord(x, Wr, w8), xf_coord(y, Hr, h8), lane);
        const float nrm = sqrtf(wave_sum(v * v));
        desc[((long)b * kcap + row) * 64 + lane] = v / fmaxf(nrm, 1e-12f);
    }
}

// test entry: the three sampling rules at n integer pixels of an H x W image.  One wave per point.
__global__ __launch_bounds__(256) void xf_probe_kernel(const float* __restrict__ k1h, const float* __restrict__ rel, const float* __restrict__ m1,
                                                       int H, int W, const int* __restrict__ xy, int n, float* __restrict__ o_near,
                                                       float* __restrict__ o_bil, float* __restrict__ o_cub) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int x = xy[2 * i], y = xy[2 * i + 1], h8 = H / 8, w8 = W / 8;
    const float v = xf_sample_bicubic(m1, h8, w8, xf_coord(x, W, w8), xf_coord(y, H, h8), lane);
    o_cub[(long)i * 64 + lane] = v;
    if (lane == 0) {
        o_near[i] = xf_sample_nearest(k1h, H, W, xf_coord(x, W, W), xf_coord(y, H, H));
        o_bil[i] = xf_sample_bilinear(rel, h8, w8, xf_coord(x, W, w8), xf_coord(y, H, h8));
    }
}


// ------------------------------------------------------------------ the trunk's launches
// scratch of the trunk for B images of Hr x Wr (multiples of 32)
struct XfTrunkBufs {
    float *gray, *norm, *s1, *s2, *s3, *q0, *q1, *q2, *e0, *e1, *e2, *e3, *x4a, *x4b, *x5a, *x5b, *x5c, *logits;
    double* part;
    void carve(WsAlloc& a, int B, int Hr, int Wr) {
        const size_t P = (size_t)B * Hr * Wr;
        gray = a.get<float>(P);
        norm = a.get<float>((size_t)2 * B);
        part = a.get<double>((size_t)B * cdiv(Hr * Wr, XF_STAT_CHUNK) * 2);
        s1 = a.get<float>(P * 4);        // block1.0
        s2 = a.get<float>(P / 4 * 8);    // block1.1
        s3 = a.get<float>(P / 4 * 8);    // block1.2
        q0 = a.get<float>(P / 16 * 32);  // 1/4 resolution, 24 channels stored as 32
        q1 = a.get<float>(P / 16 * 32);
        q2 = a.get<float>(P / 16 * 32);
        e0 = a.get<float>(P / 64 * 64);  // 1/8 resolution
        e1 = a.get<float>(P / 64 * 64);
        e2 = a.get<float>(P / 64 * 64);
        e3 = a.get<float>(P / 64 * 64);
        x4a = a.get<float>(P / 256 * 64);
        x4b = a.get<float>(P / 256 * 64);
        x5a = a.get<float>(P / 1024 * 128);
        x5b = a.get<float>(P / 1024 * 128);
        x5c = a.get<float>(P / 1024 * 64);
        logits = a.get<float>(P / 64 * 65);
    }
};

// InstanceNorm2d(1) statistics of gray [B, npix] -> norm [B][2]
static inline void xf_stats(hipStream_t stream, const float* gray, long npix, int B, double* part, float* norm) {
    const int nch = cdiv((int)npix, XF_STAT_CHUNK);
    hipLaunchKernelGGL(xf_stats_part_kernel, dim3(nch, B), dim3(256), 0, stream, gray, npix, nch, part);
    hipLaunchKernelGGL(xf_stats_fin_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, part, npix, nch, B, norm);
}

// layer L on the map `in` at level lev_in (pixel stride = the layer's stored input channels) -> `out` (pixel stride ldo)
static inline int xf_layer(imcui_hip_t* h, const float* P, const XfLayout& l, int L, const float* in, int lev_in, float* out, int ldo, int B, int Hr, int Wr,
                           hipStream_t stream) {
    const XfLayer& X = XF_LAYERS[L];
    const int lev_out = lev_in + (X.stride == 2 ? 1 : 0);
    GemmP g;
    g.epi = EPI_CONV;
    g.A = in;
    gemm_set_weights(g, P, l.g[L], X.npad, X.k * X.k * X.cpad, h->precision == 1);
    g.M = (int)(B * ((long)(Hr >> lev_out) * (Wr >> lev_out)));
    g.C = out;
    g.ldc = ldo;
    g.act = X.bn ? 1 : 0;
    if (X.k == 3)
        gemm_set_conv(g, 3, X.stride, 1, Hr >> lev_in, Wr >> lev_in, Hr >> lev_out, Wr >> lev_out, X.cpad);
    else
        g.lda = X.cpad;
    return gemm_launch(h, g, stream);
}

// s.gray [B, Hr, Wr] and s.norm -> feats = s.e3 [B, Hr/8, Wr/8, 64]: block1 + skip1 (VALU), block2 .. block5, the fusion (s.e1 and s.e2
// are free afterwards, s.e0 holds x3)
static inline int xf_trunk_feats(imcui_hip_t* h, const float* P, const XfLayout& l, const XfTrunkBufs& s, int B, int Hr, int Wr, hipStream_t stream) {
    int rc;
    auto px = [&](int lev) { return (long)(Hr >> lev) * (Wr >> lev); };
    auto layer = [&](int L, const float* in, int lev_in, float* out, int ldo) -> int { return xf_layer(h, P, l, L, in, lev_in, out, ldo, B, Hr, Wr, stream); };
    const long np0 = (long)B * px(0);
    const float* nul = nullptr;
    hipLaunchKernelGGL((xf_stem_kernel<1, 4, 4, 1, true, false>), dim3(blocks_256(np0)), dim3(256), 0, stream, s.gray, P + l.g[0].w, P + l.g[0].b, s.s1, Hr, Wr, Hr,
                       Wr, np0, s.norm, nul, nul, nul);
    hipLaunchKernelGGL((xf_stem_kernel<4, 8, 8, 2, false, false>), dim3(blocks_256(B * px(1))), dim3(256), 0, stream, s.s1, P + l.g[1].w, P + l.g[1].b, s.s2, Hr, Wr,
                       Hr / 2, Wr / 2, B * px(1), nul, nul, nul, nul);
    hipLaunchKernelGGL((xf_stem_kernel<8, 8, 8, 1, false, false>), dim3(blocks_256(B * px(1))), dim3(256), 0, stream, s.s2, P + l.g[2].w, P + l.g[2].b, s.s3, Hr / 2,
                       Wr / 2, Hr / 2, Wr / 2, B * px(1), nul, nul, nul, nul);
    hipLaunchKernelGGL((xf_stem_kernel<8, 24, 32, 2, false, true>), dim3(blocks_256(B * px(2))), dim3(256), 0, stream, s.s3, P + l.g[3].w, P + l.g[3].b, s.q0, Hr / 2,
                       Wr / 2, Hr / 4, Wr / 4, B * px(2), s.norm, s.gray, P + l.skw, P + l.skb);
    IMCUI_CHECK_LAUNCH(h);
    // ---- block2 .. block5
    IMCUI_RUN(layer(4, s.q0, 2, s.q1, 32));
    IMCUI_RUN(layer(5, s.q1, 2, s.q2, 32));
    IMCUI_RUN(layer(6, s.q2, 2, s.e0, 64));
    IMCUI_RUN(layer(7, s.e0, 3, s.e1, 64));
    IMCUI_RUN(layer(8, s.e1, 3, s.e0, 64));  // x3 = e0
    IMCUI_RUN(layer(9, s.e0, 3, s.x4a, 64));
    IMCUI_RUN(layer(10, s.x4a, 4, s.x4b, 64));
    IMCUI_RUN(layer(11, s.x4b, 4, s.x4a, 64));  // x4 = x4a
    IMCUI_RUN(layer(12, s.x4a, 4, s.x5a, 128));
    IMCUI_RUN(layer(13, s.x5a, 5, s.x5b, 128));
    IMCUI_RUN(layer(14, s.x5b, 5, s.x5a, 128));
    IMCUI_RUN(layer(15, s.x5a, 5, s.x5c, 64));  // x5 = x5c
    // ---- fusion
    const long np3 = (long)B * px(3);
    hipLaunchKernelGGL(xf_fuse_kernel, dim3(blocks_256(np3 * 16)), dim3(256), 0, stream, s.e0, s.x4a, s.x5c, s.e1, Hr / 8, Wr / 8, np3 * 16);
    IMCUI_CHECK_LAUNCH(h);
    IMCUI_RUN(layer(16, s.e1, 3, s.e2, 64));
    IMCUI_RUN(layer(17, s.e2, 3, s.e1, 64));
    IMCUI_RUN(layer(18, s.e1, 3, s.e3, 64));  // feats = e3
    return IMCUI_OK;
}

// keypoint_head on the 8x8 cells of the normalised image, 65-way soft-max, dustbin dropped -> k1h [B, Hr, Wr] (uses s.e0, s.e1, s.e2)
static inline int xf_trunk_kpts(imcui_hip_t* h, const float* P, const XfLayout& l, const XfTrunkBufs& s, int B, int Hr, int Wr, float* k1h, hipStream_t stream) {
    int rc;
    auto layer = [&](int L, const float* in, int lev_in, float* out, int ldo) -> int { return xf_layer(h, P, l, L, in, lev_in, out, ldo, B, Hr, Wr, stream); };
    const int h8 = Hr / 8, w8 = Wr / 8;
    const long np3 = (long)B * h8 * w8;
    hipLaunchKernelGGL(xf_unfold_kernel, dim3(blocks_256(np3 * 16)), dim3(256), 0, stream, s.gray, s.norm, s.e0, h8, w8, np3 * 16);
    IMCUI_CHECK_LAUNCH(h);
    IMCUI_RUN(layer(22, s.e0, 3, s.e1, 64));
    IMCUI_RUN(layer(23, s.e1, 3, s.e2, 64));
    IMCUI_RUN(layer(24, s.e2, 3, s.e1, 64));
    IMCUI_RUN(layer(25, s.e1, 3, s.logits, 65));
    hipLaunchKernelGGL(xf_softmax_kernel, dim3((unsigned)((np3 + 3) / 4)), dim3(256), 0, stream, s.logits, k1h, h8, w8, np3);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

}  // namespace
