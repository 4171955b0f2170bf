// Kernels and helpers that ALIKED (aliked.hip) and its predecessor ALIKE (alike.hip) both use: the 3x3 convolution on the VALU (LDS
// tiles), the pooling kernel, the align_corners=True tap of a bilinear up-sampling and the candidate stage of DKD (mean / threshold
// kernels, the candidate predicate, the count / scan / compact sequence with its mean fallback).
// Device code and launch helpers only; what a network does with them stays in its own file.
#pragma once
#include "common.h"
#include "select.h"

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

// ------------------------------------------------------------------ avg_pool2d(k) / max_pool2d(k) of an NHWC map: C channels of
// [n, k ho, k wo, lds] -> [n, ho, wo, ldd]; channels [C, ldd) are written as zero (the implicit GEMM's channel padding).  C, lds, ldd
// multiples of 4.  Average: row-major window sum from zero, then / k^2.  Maximum: starts from the window's first element.
template <bool MAX>
__global__ __launch_bounds__(256) void ak_pool_kernel(const float* __restrict__ src, int lds, int C, float* __restrict__ dst, int ldd, int k, int ho,
                                                      int wo, long n4) {
    const int D4 = ldd >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % D4) * 4;
        long t = i / D4;
        const int x = (int)(t % wo);
        t /= wo;
        const int y = (int)(t % ho);
        const long b = t / ho;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            const int wi = k * wo;
            const float* s = src + ((b * k * ho + (long)k * y) * wi + (long)k * x) * lds + c;
            if (MAX) o = *reinterpret_cast<const float4*>(s);
            for (int dy = 0; dy < k; ++dy)
                for (int dx = 0; dx < k; ++dx) {
                    const float4 v = *reinterpret_cast<const float4*>(s + ((long)dy * wi + dx) * lds);
                    if (MAX) {
                        o.x = fmaxf(o.x, v.x);
                        o.y = fmaxf(o.y, v.y);
                        o.z = fmaxf(o.z, v.z);
                        o.w = fmaxf(o.w, v.w);
                    } else {
                        o.x += v.x;
                        o.y += v.y;
                        o.z += v.z;
                        o.w += v.w;
                    }
                }
            if (!MAX) {
                const float d = (float)(k * k);
                o = make_float4(o.x / d, o.y / d, o.z / d, o.w / d);
            }
        }
        *reinterpret_cast<float4*>(dst + i * 4) = o;
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

template <int COUT, int CC, int ACT>
static void ak_conv3(const AkConvP& p, int B, hipStream_t stream) {
    hipLaunchKernelGGL((ak_conv3_kernel<COUT, CC, ACT>), dim3(cdiv(p.W, 16), cdiv(p.H, 16), B), dim3(256), 0, stream, p);
}

// The candidate stage of DKD on the NMS map `nms` of the score map `smap` [B, H, W]: per-image threshold (the given one; 0 on the top-k
// route; the image's mean when threshold <= 0 without top-k), candidates = nms > threshold inside rows / columns
// [band_lo, size - band_hi), and where an image has no candidate above a given threshold its mean takes the threshold's place.  The
// candidates leave in row-major order in cscore / cidx [B][H W], their counts in ncand [B].  *status is zeroed first.
struct AkDkdWs {
    float *mean, *thr;
    CandScan scan;        // (total = ncand)
    ScoreIndexList cand;  // [B][H W]: every pixel is a candidate of a flat score map
    void carve(WsAlloc& a, int B, int H, int W) {
        mean = a.get<float>(B);
        thr = a.get<float>(B);
        scan.carve(a, B, (size_t)H * W);
        cand.carve(a, B, H * W);
    }
};
static int ak_dkd_candidates(imcui_hip_s* h, const float* smap, const float* nms, int H, int W, int B, int band_lo, int band_hi, float threshold, bool topk,
                             const AkDkdWs& s, int* status, hipStream_t stream) {
    hipMemsetAsync(status, 0, sizeof(int), stream);
    hipLaunchKernelGGL(ak_mean_kernel, dim3(B), dim3(1024), 0, stream, smap, H * W, s.mean);
    hipLaunchKernelGGL(ak_thr_kernel, dim3(1), dim3(1024), 0, stream, s.thr, s.mean, s.scan.total, topk ? 0.0f : threshold, (topk || threshold > 0.0f) ? 0 : 1, B);
    const AkIsCand is_cand{H, W, band_lo, band_hi, s.thr};
    cand_count_scan(stream, nms, H * W, B, is_cand, s.scan);
    if (!topk && threshold > 0.0f) {  // no candidate above the threshold: the mean of the score map takes its place (per image)
        hipLaunchKernelGGL(ak_thr_kernel, dim3(1), dim3(1024), 0, stream, s.thr, s.mean, s.scan.total, 0.0f, 2, B);
        cand_count_scan(stream, nms, H * W, B, is_cand, s.scan);
    }
    cand_compact(stream, nms, H * W, B, is_cand, s.scan, s.cand.cap, s.cand.emit());
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

}  // namespace
