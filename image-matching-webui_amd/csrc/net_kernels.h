// Small device stages shared by the VGG- and ResNet-style extractors (the device-side sibling of netpack.h): the 3x3 first layer, the 2x2
// pools of an NHWC map, ATen's bilinear source index and the planar bilinear resize.  The MECHANICS live here; what a network feeds
// them -- how an input pixel is read and normalised, which index rule its resize follows -- stays with its owner as a functor.
// Several translation units include this header under different -ffp-contract settings (build.py).  The first layer's sums are fmaf
// chains and mean the same everywhere.  The resize is written with __fmul_rn / __fadd_rn, which are plain operators to this compiler:
// an includer compiled with contraction on gets one product of each sum fused, and which one is the compiler's choice -- a new
// instance in such a file is checked bitwise against what it replaces (R2D2's resize stayed a kernel of its own for that reason).
#pragma once
#include "common.h"

namespace {  // internal linkage: several translation units include these kernels

// ------------------------------------------------------------------ first layer
// 3 -> COUT, 3x3, pad 1, (folded BatchNorm,) ReLU, NHWC out; one thread per pixel, the 27 window values in registers, the weights
// [tap][cin][COUT] in LDS (wave-uniform reads); taps and channels summed in ascending order.  img is planar [B, 3, h, wd].
//   Load: float operator()(const float* img, long b, int c, int h, int w, int yy, int xx) const
//         -- the network-input value of input channel c at pixel (yy, xx) of image b (inside the image: the padding is zero in
//         normalised units)
template <int COUT, class Load>
__global__ __launch_bounds__(256) void stem3x3_kernel(const float* __restrict__ img, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, int h, int wd, Load load, long npix) {
    __shared__ float sw[27 * COUT + COUT];
    for (int i = threadIdx.x; i < 27 * COUT + COUT; i += 256) sw[i] = i < 27 * COUT ? w[i] : bias[i - 27 * COUT];
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % wd);
    const long q = p / wd;
    const int y = (int)(q % h);
    const long b = q / h;
    float win[27];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = x + kx - 1;
            const bool in = yy >= 0 && yy < h && xx >= 0 && xx < wd;
#pragma unroll
            for (int c = 0; c < 3; ++c) win[(ky * 3 + kx) * 3 + c] = in ? load(img, b, c, h, wd, yy, xx) : 0.0f;
        }
    float* o = out + p * COUT;
    constexpr int UNROLL = COUT <= 32 ? COUT / 4 : 2;  // the output loop: in full at 32 channels, by two at 64
#pragma unroll UNROLL
    for (int c0 = 0; c0 < COUT; c0 += 4) {
        float a[4] = {sw[27 * COUT + c0], sw[27 * COUT + c0 + 1], sw[27 * COUT + c0 + 2], sw[27 * COUT + c0 + 3]};
#pragma unroll
        for (int t = 0; t < 27; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = fmaf(win[t], sw[t * COUT + c0 + j], a[j]);
        *reinterpret_cast<float4*>(o + c0) = make_float4(fmaxf(a[0], 0.0f), fmaxf(a[1], 0.0f), fmaxf(a[2], 0.0f), fmaxf(a[3], 0.0f));
    }
}

// ------------------------------------------------------------------ 2x2 pools of an NHWC map
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// MODE 0: nn.MaxPool2d(2, 2), flooring: [B, hi, wi, C] -> [B, hi / 2, wi / 2, C] (the last row / column of an odd map is not read).
// MODE 1: nn.AvgPool2d(2, stride=1): -> [B, hi - 1, wi - 1, C], the window summed row-major, then / 4.  n4 = float4s of the output
template <int MODE>
__global__ __launch_bounds__(256) void pool2x2_kernel(const float* __restrict__ src, float* __restrict__ dst, int hi, int wi, int ho, int wo, int C, long n4) {
    const int C4 = C >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        long t = i / C4;
        const int x = (int)(t % wo);
        t /= wo;
        const int y = (int)(t % ho);
        const long b = t / ho;
        const int st = MODE == 0 ? 2 : 1;
        const float* s = src + ((b * hi + (long)st * y) * wi + (long)st * x) * C + c;
        const float4 v00 = *reinterpret_cast<const float4*>(s), v01 = *reinterpret_cast<const float4*>(s + C),
                     v10 = *reinterpret_cast<const float4*>(s + (long)wi * C), v11 = *reinterpret_cast<const float4*>(s + (long)wi * C + C);
        float4 o;
        if (MODE == 0) {
            o = max4(max4(v00, v01), max4(v10, v11));
        } else {
            o = add4(add4(add4(v00, v01), v10), v11);
            o = make_float4(o.x * 0.25f, o.y * 0.25f, o.z * 0.25f, o.w * 0.25f);
        }
        *reinterpret_cast<float4*>(dst + i * 4) = o;
    }
}

// ------------------------------------------------------------------ bilinear resize
// ATen's upsample_bilinear2d source index of output o, align_corners=False: scale * (dst + 0.5) - 0.5, clamped at 0 (scale = in / out)
__device__ __forceinline__ void bilinear_src_half_pixel(int o, float scale, int in, int* i0, int* i1, float* l0, float* l1) {
    const float s = fmaxf(__fsub_rn(__fmul_rn(scale, __fadd_rn((float)o, 0.5f)), 0.5f), 0.0f);
    const int a = min((int)s, in - 1);
    *i0 = a;
    *i1 = a + (a < in - 1 ? 1 : 0);
    *l1 = __fsub_rn(s, (float)a);
    *l0 = __fsub_rn(1.0f, *l1);
}
// the same with align_corners=True: scale * dst with scale = (in - 1) / (out - 1)
__device__ __forceinline__ void bilinear_src_align_corners(int o, float scale, int in, int* i0, int* i1, float* l0, float* l1) {
    const float s = __fmul_rn(scale, (float)o);
    const int a = min((int)s, in - 1);
    *i0 = a;
    *i1 = a + (a < in - 1 ? 1 : 0);
    *l1 = fminf(fmaxf(__fsub_rn(s, (float)a), 0.0f), 1.0f);
    *l0 = __fsub_rn(1.0f, *l1);
}

// planar [P, hi, wi] -> [P, ho, wo] (P planes: batch x channels), one thread per output value, the two rows mixed first; n = P ho wo.
//   Index: one of the two source-index rules above
//   Load:  float operator()(float v, long plane) const   -- the value the resize sees for the source value v of plane `plane`
template <void (*Index)(int, float, int, int*, int*, float*, float*), class Load>
__global__ __launch_bounds__(256) void resize_planar_kernel(const float* __restrict__ src, float* __restrict__ dst, int hi, int wi, int ho, int wo, float sh,
                                                            float sw, Load load, long n) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % wo);
    const long q = p / wo;
    const int y = (int)(q % ho);
    const long plane = q / ho;
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    Index(y, sh, hi, &y0, &y1, &hy0, &hy1);
    Index(x, sw, wi, &x0, &x1, &wx0, &wx1);
    const float* pl = src + plane * (long)hi * wi;
    const float v00 = load(pl[(long)y0 * wi + x0], plane), v01 = load(pl[(long)y0 * wi + x1], plane), v10 = load(pl[(long)y1 * wi + x0], plane),
                v11 = load(pl[(long)y1 * wi + x1], plane);
    const float top = __fadd_rn(__fmul_rn(wx0, v00), __fmul_rn(wx1, v01)), bot = __fadd_rn(__fmul_rn(wx0, v10), __fmul_rn(wx1, v11));
    dst[p] = __fadd_rn(__fmul_rn(hy0, top), __fmul_rn(hy1, bot));
}

}  // namespace
