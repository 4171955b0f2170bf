// Kernels and helpers that ALIKED (aliked.hip) and its predecessor ALIKE (alike.hip) both use: the 3x3 convolution on the VALU (LDS
// tiles), the align_corners=True tap of a bilinear up-sampling, the mean / threshold kernels of DKD and its candidate predicate.
// Device code and launch helpers only; what a network does with them stays in its own file.
#pragma once
#include "common.h"

namespace {  // internal linkage: two translation units include these kernels

// ------------------------------------------------------------------ device helpers
// SELU as ATen evaluates it: x > 0 ? scale x : scale alpha expm1(x)
__device__ __forceinline__ float ak_selu(float x) {
    return x > 0.0f ? 1.0507009873554804934193349852946f * x : 1.7580993408473768599402175208123f * expm1f(x);
}
template <int ACT>
__device__ __forceinline__ float ak_act(float x) {
    if (ACT == 1) return ak_selu(x);
    if (ACT == 2) return sigmoidf_(x);
    if (ACT == 3) return fmaxf(x, 0.0f);
    return x;
}

// ------------------------------------------------------------------ 3x3 convolution on the VALU (pad 1, fp32 FMA, LDS tiles)
// 16 x 16 outputs per workgroup; the 18 x 18 input window is staged CC channels at a time with the chunk's weights; the sum runs in
// (channel chunk, tap, channel) order.  `planar` == 2: the image [B,3,ih,iw] zero-padded at the bottom and right to H x W, every value
// passed through (x * 255) / 255 (ALIKE).  `planar` == 1: the image [B,3,ih,iw], replicate-padded to H x W with (pt, pl) rows / columns
// before it (InputPadder); otherwise an NHWC map [B,H,W,ldi] (zero outside).  Output: channels [0, COUT) of [B,oh,ow,ldo], the crop
// of the H x W result that starts at (ot, ol).
struct AkConvP {
    const float* in;
    int planar, ih, iw, pt, pl, ldi, cin;
    const float *w, *bias;
    float* out;
    int ldo, H, W, oh, ow, ot, ol;
};
template <int COUT, int CC, int ACT>
__global__ __launch_bounds__(256) void ak_conv3_kernel(AkConvP p) {
    constexpr int CS = CC | 1;  // odd pixel stride: lanes along a row hit distinct banks
    __shared__ float S[18 * 18 * CS];
    __shared__ float sw[9 * CC * COUT];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int ty = tid >> 4, tx = tid & 15;
    const int y0 = blockIdx.y * 16 - 1, x0 = blockIdx.x * 16 - 1;
    float acc[COUT];
#pragma unroll
    for (int c = 0; c < COUT; ++c) acc[c] = p.bias[c];
    for (int c0 = 0; c0 < p.cin; c0 += CC) {
        __syncthreads();
        if (p.planar) {
            for (int i = tid; i < 18 * 18 * CC; i += 256) {
                const int c = i / 324, pix = i - c * 324;
                const int yy = y0 + pix / 18, xx = x0 + pix % 18;
                float v = 0.0f;
                if (p.planar == 2) {  // ALIKE: zero outside the image, and the wrapper's x 255 / 255 round trip in float32
                    if (yy >= 0 && yy < p.ih && xx >= 0 && xx < p.iw) v = __fdiv_rn(__fmul_rn(p.in[(((long)b * p.cin + c0 + c) * p.ih + yy) * p.iw + xx], 255.0f), 255.0f);
                } else if (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) {
                    const int sy = min(max(yy - p.pt, 0), p.ih - 1), sx = min(max(xx - p.pl, 0), p.iw - 1);
                    v = p.in[(((long)b * p.cin + c0 + c) * p.ih + sy) * p.iw + sx];
                }
                S[pix * CS + c] = v;
            }
        } else {
            for (int i = tid; i < 18 * 18 * CC; i += 256) {
                const int pix = i / CC, c = i - pix * CC;
                const int yy = y0 + pix / 18, xx = x0 + pix % 18;
                S[pix * CS + c] = (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) ? p.in[(((long)b * p.H + yy) * p.W + xx) * p.ldi + c0 + c] : 0.0f;
            }
        }
        for (int i = tid; i < 9 * CC * COUT; i += 256) {
            const int co = i % COUT, r = i / COUT;  // r = tap * CC + c
            const int tap = r / CC, c = r - tap * CC;
            sw[i] = p.w[((long)tap * p.cin + c0 + c) * COUT + co];
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float* s = S + ((ty + tap / 3) * 18 + tx + tap % 3) * CS;
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const float v = s[c];
                const float* k = sw + (tap * CC + c) * COUT;
#pragma unroll
                for (int co = 0; co < COUT; ++co) acc[co] = fmaf(v, k[co], acc[co]);
            }
        }
    }
    const int y = blockIdx.y * 16 + ty - p.ot, x = blockIdx.x * 16 + tx - p.ol;
    if (y < 0 || y >= p.oh || x < 0 || x >= p.ow) return;
    float* o = p.out + (((long)b * p.oh + y) * p.ow + x) * p.ldo;
    if constexpr (COUT % 4 == 0) {
#pragma unroll
        for (int c = 0; c < COUT; c += 4)
            *reinterpret_cast<float4*>(o + c) = make_float4(ak_act<ACT>(acc[c]), ak_act<ACT>(acc[c + 1]), ak_act<ACT>(acc[c + 2]), ak_act<ACT>(acc[c + 3]));
    } else {
#pragma unroll
        for (int c = 0; c < COUT; ++c) o[c] = ak_act<ACT>(acc[c]);
    }
}

// ------------------------------------------------------------------ bilinear up-sampling, align_corners=True (ATen's index rule)
struct AkTap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ AkTap ak_tap(int dst, int nin, int nout) {
    const float scale = nout > 1 ? (float)(nin - 1) / (float)(nout - 1) : 0.0f;
    const float s = scale * (float)dst;
    AkTap t;
    t.i0 = min((int)s, nin - 1);
    t.i1 = t.i0 + (t.i0 < nin - 1 ? 1 : 0);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// ------------------------------------------------------------------ DKD: threshold, candidates, cut, refinement
// mean of an image's score map in a fixed order: thread t sums pixels t, t + 1024, ... in double, then a fixed tree
__global__ __launch_bounds__(1024) void ak_mean_kernel(const float* __restrict__ score, int npix, float* __restrict__ mean) {
    __shared__ double s[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* src = score + (long)b * npix;
    double a = 0.0;
    for (int i = tid; i < npix; i += 1024) a += (double)src[i];
    s[tid] = a;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) s[tid] += s[tid + o];
        __syncthreads();
    }
    if (tid == 0) mean[b] = (float)(s[0] / (double)npix);
}
// mode 0: thr[b] = base (the given threshold; 0 for top-k); mode 1: thr[b] = mean[b]; mode 2: thr[b] = mean[b] where ncand[b] == 0
__global__ void ak_thr_kernel(float* __restrict__ thr, const float* __restrict__ mean, const int* __restrict__ ncand, float base, int mode, int B) {
    const int b = threadIdx.x;
    if (b >= B) return;
    if (mode == 0) thr[b] = base;
    if (mode == 1 || (mode == 2 && ncand[b] == 0)) thr[b] = mean[b];
}

// candidate: nms score above the image's threshold and inside the band: rows [r0, h - r1), columns [r0, w - r1)
struct AkIsCand {
    int h, w, r0, r1;
    const float* thr;  // [B]
    float t;  // thr[b], set by bind
    __device__ void bind(int b) { t = thr[b]; }
    __device__ bool operator()(const float* img, int idx) const {
        const float s = img[idx];
        const int y = idx / w, x = idx - y * w;
        return (s > t) & (y >= r0) & (y < h - r1) & (x >= r0) & (x < w - r1);  // (no branch on the score: the division does not wait for it)
    }
};

static int ak_pad32(int v) { return (v + 31) / 32 * 32; }
static unsigned ak_grid(long n) { return (unsigned)min((n + 255) / 256, (long)65536); }

template <int COUT, int CC, int ACT>
static void ak_conv3(const AkConvP& p, int B, hipStream_t stream) {
    hipLaunchKernelGGL((ak_conv3_kernel<COUT, CC, ACT>), dim3(cdiv(p.W, 16), cdiv(p.H, 16), B), dim3(256), 0, stream, p);
}


}  // namespace
