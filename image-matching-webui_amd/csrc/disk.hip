// DISK forward on MI355X: the kornia U-Net (5x5 convolutions, InstanceNorm + PReLU on each convolution's input, avg-pool down,
// bilinear x2 up, concat), the heatmap (channel 128 of the last convolution), NMS with max_pool2d's first-maximum tie rule,
// the `n + 1`-th value cut-off of heatmap_to_keypoints, and descriptors evaluated only at the selected pixels.  Replaces the
// `self.model(image, n=..., window_size=..., score_threshold=..., pad_if_not_divisible=...)` call of
// imcui/hloc/extractors/disk.py:18-36.
//
// Data flow (NHWC maps, Hp x Wp = the image padded to multiples of 16, level l = 1/2^l):
//   conv0 3->16 (VALU, no norm / gate)                         -> cat3[:, 64:80]
//   down i = 1..4: avg-pool of the previous block's output      -> pooled map; stats; norm+PReLU -> X; 5x5 GEMM -> next slot
//   up j = 0..3:   bilinear x2 of the bottom map -> cat[:, 0:64] (the skip already sits in cat[:, 64:]); stats; norm+PReLU -> X
//   up 0..2: 5x5 GEMM -> the next bottom map.  up 3 (80 -> 129): X is the input of the last convolution; channel 128 (the heatmap)
//   is evaluated densely on the VALU, channels 0..127 (descriptors) only on the 5x5 windows of the selected pixels.
// The producers write straight into their channel slice of the consumer's concat buffer, so the concat is never copied.
// InstanceNorm statistics are reduced in a fixed order (per-chunk partials in double, summed in chunk order): an image's outputs
// do not depend on the batch it is in.  No host synchronisation: every grid is sized by shapes or capacities.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "gemm.h"
#include "imcui_hip.h"
#include "netpack.h"
#include "select.h"

// ------------------------------------------------------------------ packed weight layout
// GEMM layers (5x5, pad 2): down 1..4, up 0..3 (the last one: descriptor rows 0..127 only)
#define DK_NL 8
static const int DK_CIN[DK_NL] = {16, 32, 64, 64, 128, 128, 96, 80};
static const int DK_CPAD[DK_NL] = {32, 32, 64, 64, 128, 128, 96, 96};  // input channels as stored (multiple of 32, zero padded)
static const int DK_COUT[DK_NL] = {32, 64, 64, 64, 64, 64, 64, 128};
#define DK_NT 26
#define DK_DESC_ROWS 4096  // key-points per descriptor GEMM launch (the gather buffer is sized by it, not by the output capacity)

struct DkLayout {
    size_t w0, b0;  // first convolution [16][3][5][5], bias [16]
    size_t slope[DK_NL];
    GemmLayerOff g[DK_NL];
    size_t hw, hb;  // heatmap row of the last convolution: [80 channels][25 taps], bias [1]
    size_t total;
};

static DkLayout dk_layout() {
    DkLayout l;
    PackCursor c;
    l.w0 = c.get(16 * 3 * 25);
    l.b0 = c.get(16);
    for (int i = 0; i < DK_NL; ++i) {
        l.slope[i] = c.get(DK_CIN[i]);
        l.g[i].place(c, DK_COUT[i], 25 * DK_CPAD[i]);
    }
    l.hw = c.get(80 * 25);
    l.hb = c.get(1);
    l.total = c.off;
    return l;
}

extern "C" size_t imcui_hip_disk_packed_floats(void) { return dk_layout().total; }
extern "C" int imcui_hip_disk_num_tensors(void) { return DK_NT; }

// tensor i of the packer = the kornia state-dict key (DISK.unet: path_down.0 has no norm / gate, so no PReLU weight)
extern "C" const char* imcui_hip_disk_tensor_name(int i) {
    static thread_local char buf[64];
    if (i < 0 || i >= DK_NT) return nullptr;
    if (i < 2) return i == 0 ? "unet.path_down.0.1.3.weight" : "unet.path_down.0.1.3.bias";
    static const char* const kinds[3] = {"1.weight", "3.weight", "3.bias"};
    const int j = i - 2, blk = j / 3, kind = j % 3;
    if (blk < 4)
        snprintf(buf, sizeof buf, "unet.path_down.%d.1.%s", blk + 1, kinds[kind]);
    else
        snprintf(buf, sizeof buf, "unet.path_up.%d.conv.%s", blk - 4, kinds[kind]);
    return buf;
}

// t: host pointers of the 26 tensors in imcui_hip_disk_tensor_name order (shapes checked by the caller)
extern "C" int imcui_hip_disk_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    for (int i = 0; i < DK_NT; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const DkLayout l = dk_layout();
    memset(packed, 0, l.total * sizeof(float));
    memcpy(packed + l.w0, t[0], 16 * 3 * 25 * sizeof(float));
    memcpy(packed + l.b0, t[1], 16 * sizeof(float));
    for (int i = 0; i < DK_NL; ++i) {
        const float* slope = t[2 + 3 * i];
        const float* w = t[3 + 3 * i];  // OIHW [Cout (129 for the last)][Cin][5][5]
        const float* b = t[4 + 3 * i];
        const int K = 25 * DK_CPAD[i];
        memcpy(packed + l.slope[i], slope, DK_CIN[i] * sizeof(float));
        pack_conv_gemm(w, DK_COUT[i], DK_CIN[i], 5, DK_CPAD[i], packed + l.g[i].w);
        memcpy(packed + l.g[i].b, b, DK_COUT[i] * sizeof(float));
        l.g[i].split_planes(packed, DK_COUT[i], K);
        if (i == DK_NL - 1) {  // output channel 128: the heatmap
            memcpy(packed + l.hw, w + (size_t)128 * 80 * 25, 80 * 25 * sizeof(float));
            packed[l.hb] = b[128];
        }
    }
    return IMCUI_OK;
}

// ------------------------------------------------------------------ first convolution 3 -> 16 (no norm / gate), VALU
// image [B,3,h,w] (planar, zero outside h x w: the right / bottom padding and the convolution's own zero padding);
// out: channels [off, off + 16) of the NHWC map [B, Hp, Wp, ldo].  One thread per output pixel.
__global__ __launch_bounds__(256) void dk_conv0_kernel(const float* __restrict__ img, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int h, int wd, int Hp, int Wp, int ldo, int off, long npix) {
    __shared__ float sw[16 * 75 + 16];
    for (int i = threadIdx.x; i < 16 * 75; i += 256) {
        const int co = i / 75, r = i - co * 75;  // r = ci * 25 + tap
        sw[r * 16 + co] = w[i];
    }
    if (threadIdx.x < 16) sw[16 * 75 + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % Wp);
    const long q = p / Wp;
    const int y = (int)(q % Hp);
    const long b = q / Hp;
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = sw[16 * 75 + c];
    for (int ci = 0; ci < 3; ++ci) {
        const float* pl = img + (b * 3 + ci) * (long)h * wd;
        for (int ky = 0; ky < 5; ++ky) {
            const int iy = y - 2 + ky;
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const int ix = x - 2 + kx;
                const float v = (iy >= 0 && iy < h && ix >= 0 && ix < wd) ? pl[(long)iy * wd + ix] : 0.0f;
                const float* k = sw + (ci * 25 + ky * 5 + kx) * 16;
#pragma unroll
                for (int c = 0; c < 16; ++c) acc[c] = fmaf(v, k[c], acc[c]);
            }
        }
    }
    float4* o = reinterpret_cast<float4*>(out + p * ldo + off);
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = make_float4(acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]);
}

// ------------------------------------------------------------------ avg_pool2d(2): ATen's order ((((0 + a) + b) + c) + d) / 4
// src: channels [soff, soff + C) of [n, 2 ho, 2 wo, lds]; dst contiguous [n, ho, wo, C].  C % 4 == 0.
__global__ __launch_bounds__(256) void dk_pool_kernel(const float* __restrict__ src, int lds, int soff, float* __restrict__ dst, int ho, int wo, int C,
                                                      long n4) {
    const int C4 = C >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long t = i / C4;
        const int x = (int)(t % wo);
        t /= wo;
        const int y = (int)(t % ho);
        const long b = t / ho;
        const int wi = 2 * wo;
        const float* s = src + ((b * 2 * ho + 2 * y) * (long)wi + 2 * x) * lds + soff + c4 * 4;
        const float4 a = *reinterpret_cast<const float4*>(s), bb = *reinterpret_cast<const float4*>(s + lds);
        const float4 c = *reinterpret_cast<const float4*>(s + (long)wi * lds), d = *reinterpret_cast<const float4*>(s + (long)wi * lds + lds);
        float4 o;
        o.x = (((a.x + bb.x) + c.x) + d.x) / 4.0f;
        o.y = (((a.y + bb.y) + c.y) + d.y) / 4.0f;
        o.z = (((a.z + bb.z) + c.z) + d.z) / 4.0f;
        o.w = (((a.w + bb.w) + c.w) + d.w) / 4.0f;
        *reinterpret_cast<float4*>(dst + i * 4) = o;
    }
}

// ------------------------------------------------------------------ bilinear x2, align_corners=False (ATen's formula and order)
// src contiguous [n, h, w, 64] -> channels [0, 64) of [n, 2h, 2w, ldd]
__global__ __launch_bounds__(256) void dk_up_kernel(const float* __restrict__ in, float* __restrict__ out, int ldd, int h, int w, long n4) {
    const int Ho = 2 * h, Wo = 2 * w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i & 15);
        long t = i >> 4;
        const int ox = (int)(t % Wo);
        t /= Wo;
        const int oy = (int)(t % Ho);
        const long b = t / Ho;
        const float fy = fmaxf(0.5f * ((float)oy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(0.5f * ((float)ox + 0.5f) - 0.5f, 0.0f);
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float hy = 1.0f - ly, hx = 1.0f - lx;
        const float* base = in + b * (long)h * w * 64 + c4 * 4;
        const float4 v00 = *reinterpret_cast<const float4*>(base + ((long)y0 * w + x0) * 64);
        const float4 v01 = *reinterpret_cast<const float4*>(base + ((long)y0 * w + x1) * 64);
        const float4 v10 = *reinterpret_cast<const float4*>(base + ((long)y1 * w + x0) * 64);
        const float4 v11 = *reinterpret_cast<const float4*>(base + ((long)y1 * w + x1) * 64);
        float4 o;
        o.x = hy * (hx * v00.x + lx * v01.x) + ly * (hx * v10.x + lx * v11.x);
        o.y = hy * (hx * v00.y + lx * v01.y) + ly * (hx * v10.y + lx * v11.y);
        o.z = hy * (hx * v00.z + lx * v01.z) + ly * (hx * v10.z + lx * v11.z);
        o.w = hy * (hx * v00.w + lx * v01.w) + ly * (hx * v10.w + lx * v11.w);
        *reinterpret_cast<float4*>(out + ((b * Ho + oy) * (long)Wo + ox) * ldd + c4 * 4) = o;
    }
}

// ------------------------------------------------------------------ InstanceNorm statistics (deterministic)
// pass 1: block (chunk, b) sums DK_STAT_CHUNK pixels of a contiguous [n, npix, C] map per channel in double (thread (r, c) takes
// pixels r, r + R, ... of the chunk; the R row sums are added in r order) -> part [b][chunk][C][2] = (sum, sum of squares)
#define DK_STAT_CHUNK 1024
__global__ __launch_bounds__(256) void dk_stats_part_kernel(const float* __restrict__ x, int C, long npix, int nchunk, double* __restrict__ part) {
    __shared__ double s1[256], s2[256];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int R = 256 / C;
    const int r = tid / C, c = tid - r * C;
    const long p0 = (long)chunk * DK_STAT_CHUNK;
    const long p1 = min(p0 + DK_STAT_CHUNK, npix);
    double a = 0.0, q = 0.0;
    if (r < R) {
        const float* src = x + ((long)b * npix) * C + c;
        for (long p = p0 + r; p < p1; p += R) {
            const double v = (double)src[p * C];
            a += v;
            q += v * v;
        }
    }
    s1[tid] = a;
    s2[tid] = q;
    __syncthreads();
    if (tid < C) {
        double sa = 0.0, sq = 0.0;
        for (int rr = 0; rr < R; ++rr) {
            sa += s1[rr * C + tid];
            sq += s2[rr * C + tid];
        }
        double* o = part + (((size_t)b * nchunk + chunk) * C + tid) * 2;
        o[0] = sa;
        o[1] = sq;
    }
}

// pass 2: thread c of block b adds the chunk partials in chunk order; biased variance, eps 1e-5 (InstanceNorm2d defaults)
__global__ __launch_bounds__(128) void dk_stats_fin_kernel(const double* __restrict__ part, int C, long npix, int nchunk, float* __restrict__ mean,
                                                           float* __restrict__ rstd) {
    const int b = blockIdx.x, c = threadIdx.x;
    if (c >= C) return;
    double sa = 0.0, sq = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        const double* o = part + (((size_t)b * nchunk + k) * C + c) * 2;
        sa += o[0];
        sq += o[1];
    }
    const double m = sa / (double)npix;
    const double var = fmax(sq / (double)npix - m * m, 0.0);
    mean[b * 128 + c] = (float)m;
    rstd[b * 128 + c] = (float)(1.0 / sqrt(var + 1e-5));
}

// normalised + gated copy: X[p][c] = prelu((x - mean) * rstd) for c < C, 0 for C <= c < Cpad (the GEMM's zero padding)
__global__ __launch_bounds__(256) void dk_norm_kernel(const float* __restrict__ x, int C, int Cpad, long npix, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ slope, float* __restrict__ out, long n4) {
    const int P4 = Cpad >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % P4) * 4;
        const long p = i / P4;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            const int b = (int)(p / npix);
            const float4 v = *reinterpret_cast<const float4*>(x + p * C + c);
            float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // ATen: out = x * alpha + beta with alpha = invstd, beta = -mean * invstd (separate roundings)
                const float al = rstd[b * 128 + c + j];
                const float be = __fmul_rn(-mean[b * 128 + c + j], al);
                const float y = __fadd_rn(__fmul_rn(r[j], al), be);
                r[j] = y >= 0.0f ? y : __fmul_rn(slope[c + j], y);
            }
            o = make_float4(r[0], r[1], r[2], r[3]);
        }
        *reinterpret_cast<float4*>(out + i * 4) = o;
    }
}

// ------------------------------------------------------------------ heatmap: channel 128 of the last convolution (80 -> 1, 5x5)
// X [B, Hp, Wp, 96] (normalised + gated, channels 80.. zero); heat [B, h, w] (the crop).  16 x 16 outputs per workgroup, the
// 20 x 20 input window staged 16 channels at a time; fp32 FMA in (channel chunk, tap, channel) order.
#define DK_HT 16
#define DK_HS 20
__global__ __launch_bounds__(256) void dk_heat_kernel(const float* __restrict__ X, const float* __restrict__ hw, const float* __restrict__ hb,
                                                      float* __restrict__ heat, int h, int w, int Hp, int Wp) {
    __shared__ float4 S[DK_HS * DK_HS * 4];
    __shared__ float sw[80 * 25];
    const int tid = threadIdx.x, b = blockIdx.z;
    for (int i = tid; i < 80 * 25; i += 256) sw[i] = hw[i];
    const int ty = tid >> 4, tx = tid & 15;
    const int y0 = blockIdx.y * DK_HT - 2, x0 = blockIdx.x * DK_HT - 2;
    const float* img = X + (long)b * Hp * Wp * 96;
    float acc = hb[0];
    for (int c0 = 0; c0 < 80; c0 += 16) {
        __syncthreads();
        for (int i = tid; i < DK_HS * DK_HS * 4; i += 256) {
            const int pix = i >> 2, q = i & 3;
            const int yy = y0 + pix / DK_HS, xx = x0 + pix % DK_HS;
            S[i] = (yy >= 0 && yy < Hp && xx >= 0 && xx < Wp) ? *reinterpret_cast<const float4*>(img + ((long)yy * Wp + xx) * 96 + c0 + q * 4)
                                                               : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const int tap = ky * 5 + kx;
                const float4* s = S + ((ty + ky) * DK_HS + tx + kx) * 4;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = s[q];
                    const int c = c0 + 4 * q;
                    acc = fmaf(v.x, sw[(c + 0) * 25 + tap], acc);
                    acc = fmaf(v.y, sw[(c + 1) * 25 + tap], acc);
                    acc = fmaf(v.z, sw[(c + 2) * 25 + tap], acc);
                    acc = fmaf(v.w, sw[(c + 3) * 25 + tap], acc);
                }
            }
    }
    const int y = blockIdx.y * DK_HT + ty, x = blockIdx.x * DK_HT + tx;
    if (y < h && x < w) heat[((long)b * h + y) * w + x] = acc;
}

// ------------------------------------------------------------------ NMS + threshold, row-major compaction
// A pixel survives iff max_pool2d(heat, window, stride 1, padding window // 2, return_indices=True) returns its own index (the
// first maximum in row-major order wins a tie: strictly greater than every earlier pixel of its window, >= every later one)
// and heat > threshold.
__device__ __forceinline__ bool dk_keep(const float* __restrict__ hm, int y, int x, int h, int w, int r, float thr) {
    const float v = hm[(long)y * w + x];
    if (!(v > thr)) return false;
    for (int dy = -r; dy <= r; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= h) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= w || (dy == 0 && dx == 0)) continue;
            const float u = hm[(long)yy * w + xx];
            const bool earlier = dy < 0 || (dy == 0 && dx < 0);
            if (earlier ? !(v > u) : (u > v)) return false;
        }
    }
    return true;
}

struct DkKeep {
    int h, w, r;
    float thr;
    __device__ void bind(int) {}
    __device__ bool operator()(const float* hm, int idx) const { return dk_keep(hm, idx / w, idx % w, h, w, r, thr); }
};

// ------------------------------------------------------------------ selection (heatmap_to_keypoints with n given)
// n_ = min(n + 1, count); t = the n_-th largest score (radix select on order-preserving keys); keep score > t (strict), then the
// first n in row-major order.  n < 0 (None): every candidate.  Zero candidates: zero key-points (the reference raises there).
// One workgroup per image.  Outputs past the count are zero.
__global__ __launch_bounds__(1024) void dk_select_kernel(const float* __restrict__ cscore, const int* __restrict__ cidx, int ccap,
                                                         const int* __restrict__ ncand, int maxk, int kcap, int w, float* __restrict__ kpts,
                                                         float* __restrict__ scores, int* __restrict__ nkpts, int* __restrict__ status) {
    __shared__ int wcnt[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* cs = cscore + (long)b * ccap;
    const int* ci = cidx + (long)b * ccap;
    const int n = min(ncand[b], ccap);
    bool filter = false;
    unsigned kth = 0;
    int limit = n;
    if (maxk >= 0 && n > 0) {
        filter = true;
        limit = min(maxk, n);
        // the n_-th largest key (n_ >= 1: maxk >= 0, n > 0)
        kth = radix_select_kth<1024, unsigned>([&](int i) { return order_key(cs[i]); }, n, min(maxk + 1, n));
    }
    if (limit > kcap) {
        if (tid == 0) atomicOr(status, 2);  // output capacity too small
        limit = kcap;
    }
    // ordered compaction of the kept candidates, 1024 at a time
    float* kp = kpts + (long)b * kcap * 2;
    float* sc = scores + (long)b * kcap;
    int run = 0;
    for (int base = 0; base < n; base += 1024) {
        if (run >= limit) break;
        const int i = base + tid;
        bool keep = false;
        float v = 0.0f;
        int idx = 0;
        if (i < n) {
            v = cs[i];
            idx = ci[i];
            keep = !filter || order_key(v) > kth;
        }
        int tot;
        const int pos = run + block_ordered_rank<16>(keep, wcnt, &tot);
        if (keep && pos < limit) {
            kp[2 * pos + 0] = (float)(idx % w);
            kp[2 * pos + 1] = (float)(idx / w);
            sc[pos] = v;
        }
        run += tot;
    }
    const int cnt = min(run, limit);
    for (int i = cnt + tid; i < kcap; i += 1024) {
        kp[2 * i + 0] = 0.0f;
        kp[2 * i + 1] = 0.0f;
        sc[i] = 0.0f;
    }
    if (tid == 0) nkpts[b] = cnt;
}

// The detection stage as `forward` launches it, on the heat map: status memset, count / scan / compact of the NMS survivors, selection.
// The one launcher of both imcui_hip_disk_forward and the test entry imcui_hip_disk_select_probe.
static int dk_select_launch(imcui_hip_t* h, const float* heat, int B, int H, int W, int window, float threshold, int max_keypoints, int kcap,
                            const CandScan& scan, const ScoreIndexList& c, float* keypoints, float* scores, int* num_keypoints, int* st, hipStream_t stream) {
    hipMemsetAsync(st, 0, sizeof(int), stream);
    cand_list(stream, heat, H * W, B, DkKeep{H, W, window / 2, threshold}, scan, c.cap, c.emit());
    hipLaunchKernelGGL(dk_select_kernel, dim3(B), dim3(1024), 0, stream, c.cscore, c.cidx, c.cap, scan.total, max_keypoints, kcap, W, keypoints, scores, num_keypoints, st);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ sparse descriptors
// rows [r0, r0 + DK_DESC_ROWS) of the key-point list: A[b][row - r0] = the 5x5 x 96 window of X around the key-point, (tap, channel)
// order (the GEMM weight layout of pack_conv_gemm); zero outside the padded map.  One wave per key-point; rows past the count exit.
// Block (0, b) also stores this launch's row count for the GEMM (mcnt).
__global__ __launch_bounds__(256) void dk_gather_kernel(const float* __restrict__ X, const float* __restrict__ kpts, const int* __restrict__ nkpts,
                                                        int kcap, int r0, int Hp, int Wp, float* __restrict__ A, int* __restrict__ rows) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int nk = min(nkpts[b], kcap);
    if (blockIdx.x == 0 && threadIdx.x == 0) rows[b] = max(0, min(nk - r0, DK_DESC_ROWS));
    const int lr = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int i = r0 + lr;
    if (lr >= DK_DESC_ROWS || i >= nk) return;
    const int x = (int)kpts[((long)b * kcap + i) * 2 + 0], y = (int)kpts[((long)b * kcap + i) * 2 + 1];
    const float* img = X + (long)b * Hp * Wp * 96;
    float* dst = A + ((long)b * DK_DESC_ROWS + lr) * (25 * 96);
    for (int e = lane; e < 25 * 24; e += 64) {
        const int tap = e / 24, c4 = e - tap * 24;
        const int yy = y - 2 + tap / 5, xx = x - 2 + tap % 5;
        const float4 v = (yy >= 0 && yy < Hp && xx >= 0 && xx < Wp) ? *reinterpret_cast<const float4*>(img + ((long)yy * Wp + xx) * 96 + c4 * 4)
                                                                     : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(dst + tap * 96 + c4 * 4) = v;
    }
}

// F.normalize(dim=0): x / max(|x|, 1e-12); rows past the count are zero.  One wave per row of 128.
__global__ __launch_bounds__(256) void dk_l2norm_kernel(float* __restrict__ desc, const int* __restrict__ nkpts, int kcap) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= kcap) return;
    float2* row = reinterpret_cast<float2*>(desc + ((long)b * kcap + i) * 128) + lane;
    if (i >= min(nkpts[b], kcap)) {
        *row = make_float2(0.f, 0.f);
        return;
    }
    const float2 v = *row;
    const float nrm = sqrtf(wave_sum(v.x * v.x + v.y * v.y));
    const float d = fmaxf(nrm, 1e-12f);
    *row = make_float2(v.x / d, v.y / d);
}

// ------------------------------------------------------------------ workspace
struct DkWs {
    float *cat3, *cat2, *cat1, *cat0, *f5, *u0, *u1, *u2, *X, *pool, *mean, *rstd, *heat, *gA;
    double* part;
    CandScan scan;
    ScoreIndexList cand;
    int *rows, *status;
    size_t total;
    bool ok;
};

static int dk_pad16(int v) { return (v + 15) / 16 * 16; }

static DkWs dk_carve(void* ws, size_t bytes, int B, int h, int w, int Hp, int Wp) {
    WsAlloc a(ws, bytes);
    DkWs s;
    const size_t P0 = (size_t)Hp * Wp, P1 = P0 / 4, P2 = P0 / 16, P3 = P0 / 64, P4 = P0 / 256;
    s.cat3 = a.get<float>(B * P0 * 80);
    s.cat2 = a.get<float>(B * P1 * 96);
    s.cat1 = a.get<float>(B * P2 * 128);
    s.cat0 = a.get<float>(B * P3 * 128);
    s.f5 = a.get<float>(B * P4 * 64);
    s.u0 = a.get<float>(B * P3 * 64);
    s.u1 = a.get<float>(B * P2 * 64);
    s.u2 = a.get<float>(B * P1 * 64);
    s.X = a.get<float>(B * P0 * 96);
    s.pool = a.get<float>(B * P1 * 16);  // the largest pooled map (1/2, 16 channels)
    s.mean = a.get<float>((size_t)B * 128);
    s.rstd = a.get<float>((size_t)B * 128);
    s.part = a.get<double>((size_t)B * cdiv((int)P0, DK_STAT_CHUNK) * 128 * 2);
    s.heat = a.get<float>((size_t)B * h * w);
    s.scan.carve(a, B, (size_t)h * w);
    s.cand.carve(a, B, h * w);  // every pixel can be a candidate when window = 1
    s.gA = a.get<float>((size_t)B * DK_DESC_ROWS * 25 * 96);
    s.rows = a.get<int>(B);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

extern "C" size_t imcui_hip_disk_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return dk_carve(nullptr, 0, B, H, W, dk_pad16(H), dk_pad16(W)).total;
}

// survivors of the NMS are pairwise >= window // 2 + 1 apart (Chebyshev), so this is an exact bound on the key-point count
extern "C" int imcui_hip_disk_max_keypoints_bound(int H, int W, int window) {
    const int s = (window < 1 ? 1 : window) / 2 + 1;
    return cdiv(H, s) * cdiv(W, s);
}

extern "C" int imcui_hip_disk_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, int pad_if_not_divisible,
                                      int window, float threshold, int max_keypoints, int kcap, float* keypoints, float* scores, float* descriptors,
                                      int* num_keypoints, int* status, float* heatmap, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (H <= 0 || W <= 0) return imcui_set_err(h, IMCUI_ERR_ARG, "disk: H=%d W=%d must be positive", H, W);
    if (!pad_if_not_divisible && (H % 16 || W % 16))
        return imcui_set_err(h, IMCUI_ERR_ARG, "disk: H=%d W=%d are not multiples of 16 and pad_if_not_divisible is off", H, W);
    if (window < 1 || window % 2 == 0) return imcui_set_err(h, IMCUI_ERR_ARG, "disk: window_size=%d must be odd", window);
    if (kcap <= 0 || !packed || !image || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "disk: null argument or kcap<=0");
    const int Hp = dk_pad16(H), Wp = dk_pad16(W);
    DkWs s = dk_carve(ws, ws_bytes, B, H, W, Hp, Wp);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "disk: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const DkLayout l = dk_layout();
    const float* P = packed;
    const bool split = h->precision == 1;
    int rc;
    auto px = [&](int lev) { return (long)(Hp >> lev) * (Wp >> lev); };
    // InstanceNorm statistics of the contiguous map x [B, px(lev), C], then X = prelu(norm(x)) with Cpad channels
    auto norm = [&](int L, const float* x, int lev) -> int {
        const int C = DK_CIN[L], Cp = DK_CPAD[L];
        const long np = px(lev);
        const int nch = cdiv((int)np, DK_STAT_CHUNK);
        hipLaunchKernelGGL(dk_stats_part_kernel, dim3(nch, B), dim3(256), 0, stream, x, C, np, nch, s.part);
        hipLaunchKernelGGL(dk_stats_fin_kernel, dim3(B), dim3(128), 0, stream, s.part, C, np, nch, s.mean, s.rstd);
        const long n4 = (long)B * np * Cp / 4;
        hipLaunchKernelGGL(dk_norm_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, x, C, Cp, np, s.mean, s.rstd, P + l.slope[L], s.X, n4);
        IMCUI_CHECK_LAUNCH(h);
        return IMCUI_OK;
    };
    // 5x5 convolution of X (level lev) -> channels [0, Cout) of `out` (pixel stride ldo)
    auto conv = [&](int L, int lev, float* out, int ldo) -> int {
        GemmP g;
        g.epi = EPI_CONV;
        g.A = s.X;
        gemm_set_weights(g, P, l.g[L], DK_COUT[L], 25 * DK_CPAD[L], split);
        gemm_set_conv(g, 5, 1, 2, Hp >> lev, Wp >> lev, Hp >> lev, Wp >> lev, DK_CPAD[L]);
        g.M = (int)(B * px(lev));
        g.C = out;
        g.ldc = ldo;
        return gemm_launch(h, g, stream);
    };
    auto pool = [&](const float* src, int lds, int soff, int lev_out, int C) {
        const long n4 = (long)B * px(lev_out) * C / 4;
        hipLaunchKernelGGL(dk_pool_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, src, lds, soff, s.pool, Hp >> lev_out, Wp >> lev_out, C, n4);
    };
    auto up = [&](const float* src, int lev_in, float* dst, int ldd) {
        const long n4 = (long)B * px(lev_in - 1) * 16;
        hipLaunchKernelGGL(dk_up_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, src, dst, ldd, Hp >> lev_in, Wp >> lev_in, n4);
    };
    // ---- down path
    {
        const long np = (long)B * px(0);
        hipLaunchKernelGGL(dk_conv0_kernel, dim3(blocks_256(np)), dim3(256), 0, stream, image, P + l.w0, P + l.b0, s.cat3, H, W, Hp, Wp,
                           80, 64, np);
        IMCUI_CHECK_LAUNCH(h);
    }
    pool(s.cat3, 80, 64, 1, 16);
    IMCUI_RUN(norm(0, s.pool, 1));
    IMCUI_RUN(conv(0, 1, s.cat2 + 64, 96));
    pool(s.cat2, 96, 64, 2, 32);
    IMCUI_RUN(norm(1, s.pool, 2));
    IMCUI_RUN(conv(1, 2, s.cat1 + 64, 128));
    pool(s.cat1, 128, 64, 3, 64);
    IMCUI_RUN(norm(2, s.pool, 3));
    IMCUI_RUN(conv(2, 3, s.cat0 + 64, 128));
    pool(s.cat0, 128, 64, 4, 64);
    IMCUI_RUN(norm(3, s.pool, 4));
    IMCUI_RUN(conv(3, 4, s.f5, 64));
    // ---- up path: [bilinear x2 of the bottom map | skip]
    up(s.f5, 4, s.cat0, 128);
    IMCUI_RUN(norm(4, s.cat0, 3));
    IMCUI_RUN(conv(4, 3, s.u0, 64));
    up(s.u0, 3, s.cat1, 128);
    IMCUI_RUN(norm(5, s.cat1, 2));
    IMCUI_RUN(conv(5, 2, s.u1, 64));
    up(s.u1, 2, s.cat2, 96);
    IMCUI_RUN(norm(6, s.cat2, 1));
    IMCUI_RUN(conv(6, 1, s.u2, 64));
    up(s.u2, 1, s.cat3, 80);
    IMCUI_RUN(norm(7, s.cat3, 0));
    // ---- heatmap (cropped to H x W), detection
    float* heat = heatmap ? heatmap : s.heat;
    hipLaunchKernelGGL(dk_heat_kernel, dim3(cdiv(W, DK_HT), cdiv(H, DK_HT), B), dim3(256), 0, stream, s.X, P + l.hw, P + l.hb, heat, H, W, Hp, Wp);
    IMCUI_CHECK_LAUNCH(h);
    IMCUI_RUN(dk_select_launch(h, heat, B, H, W, window, threshold, max_keypoints, kcap, s.scan, s.cand, keypoints, scores,
                               num_keypoints, status ? status : s.status, stream));
    // ---- descriptors at the selected pixels: gather the windows, [rows, 2400] x [2400, 128] + bias, L2 norm
    const int L = DK_NL - 1;
    for (int r0 = 0; r0 < kcap; r0 += DK_DESC_ROWS) {
        hipLaunchKernelGGL(dk_gather_kernel, dim3(DK_DESC_ROWS / 4, B), dim3(256), 0, stream, s.X, keypoints, num_keypoints, kcap, r0, Hp, Wp, s.gA,
                           s.rows);
        IMCUI_CHECK_LAUNCH(h);
        GemmP g;
        g.epi = EPI_BIAS;
        g.A = s.gA;
        g.lda = 25 * 96;
        g.a_bs = (long)DK_DESC_ROWS * 25 * 96;
        gemm_set_weights(g, P, l.g[L], 128, 25 * 96, split);
        g.C = descriptors + (size_t)r0 * 128;
        g.ldc = 128;
        g.c_bs = (long)kcap * 128;
        g.M = DK_DESC_ROWS;
        g.batch = B;
        g.mcnt = s.rows;
        g.cnt_stride = 1;
        IMCUI_RUN(gemm_launch(h, g, stream));
    }
    hipLaunchKernelGGL(dk_l2norm_kernel, dim3(cdiv(kcap, 4), B), dim3(256), 0, stream, descriptors, num_keypoints, kcap);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// test entry: the detection stage alone, through the launcher `forward` calls, on a heat map given by the caller
struct DkSelWs {
    CandScan scan;
    ScoreIndexList cand;
    size_t total;
    bool ok;
};
static DkSelWs dk_select_carve(void* ws, size_t bytes, int B, int H, int W, int ccap) {
    WsAlloc a(ws, bytes);
    DkSelWs s;
    s.scan.carve(a, B, (size_t)H * W);
    s.cand.carve(a, B, ccap);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}
static bool dk_select_shape_ok(int B, int H, int W, int ccap) {
    return B >= 1 && B <= 1024 && H >= 1 && W >= 1 && (long)H * W <= (1L << 24) && ccap >= 1 && ccap <= (1 << 24);
}
extern "C" size_t imcui_hip_disk_select_workspace_bytes(int B, int H, int W, int ccap) {
    return dk_select_shape_ok(B, H, W, ccap) ? dk_select_carve(nullptr, 0, B, H, W, ccap).total : 0;
}
extern "C" int imcui_hip_disk_select_probe(imcui_hip_t* h, const float* heat, int B, int H, int W, int window, float threshold, int max_keypoints, int kcap, int ccap,
                                           float* keypoints, float* scores, int* num_keypoints, int* status, void* ws, size_t ws_bytes, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    if (!dk_select_shape_ok(B, H, W, ccap) || kcap < 1 || kcap > (1 << 24))
        return imcui_set_err(h, IMCUI_ERR_ARG, "disk select probe: B=%d map %dx%d kcap=%d ccap=%d", B, H, W, kcap, ccap);
    if (window < 1 || window % 2 == 0) return imcui_set_err(h, IMCUI_ERR_ARG, "disk select probe: window_size=%d must be odd", window);
    if (!heat || !keypoints || !scores || !num_keypoints || !status) return imcui_set_err(h, IMCUI_ERR_ARG, "disk select probe: null argument");
    DkSelWs s = dk_select_carve(ws, ws_bytes, B, H, W, ccap);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "disk select probe: workspace too small (%zu < %zu)", ws_bytes, s.total);
    return dk_select_launch(h, heat, B, H, W, window, threshold, max_keypoints, kcap, s.scan, s.cand, keypoints, scores,
                            num_keypoints, status, (hipStream_t)stream_);
}
