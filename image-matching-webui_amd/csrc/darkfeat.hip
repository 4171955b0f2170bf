// DarkFeat forward on MI355X (zoo entry darkfeat + NN-mutual; extractor conf darkfeat): imcui/hloc/extractors/darkfeat.py:31-44 around
// darkfeat.DarkFeat(model_path) as one batched call.  The network is NOT in the reference checkout (third_party/DarkFeat is an empty
// submodule): it is restated in tests/darkfeat_reference.py, and that file is the definition this one is tested against
// ("DarkFeat: what is pinned").
//
//   image       [B, 3, H, W] RGB; per image mean and unbiased std over its 3 H W values (fixed chunks of DF_IMCHUNK values, double
//               partial sums folded in chunk order), (x - mean) / std applied where layer 0 READS the image, so its zero padding is zero
//               in normalised units.  std == 0 (a flat image; NaN upstream): status bit 4 and zero key-points for that image.
//   layer 0     3 -> 32 on the VALU (df_stem_kernel: stem3x3_kernel's sum order without its ReLU -- InstanceNorm stands between the
//               convolution and the ReLU here, so the shared kernel cannot serve)
//   layers 1..  DF_LAYERS, 3x3 on the shared implicit GEMM (gemm.hip, both arithmetic modes, stride 1 / 2, no activation)
//   InstanceNorm (non-affine, eps 1e-5, biased variance) is a pass of its own over the RAW map: per (image, channel) double partial sums
//               over fixed chunks of DF_STCHUNK pixels (df_in_partial_kernel), folded in chunk order (df_in_fold_kernel), applied in place
//               as relu((x - m) * rsqrt(v + eps)) with 16-byte accesses (df_in_apply_kernel).  The raw map of a score level is read by
//               the peakiness pass BEFORE it is normalised in place, so no second copy of it exists.
//   peakiness   df_peak_kernel<C, D>: an 8 x 8 tile with a halo of D (reflected indices) of x / moving_avg in LDS, per pixel
//               max_c softplus(x - box3x3_D(x)) * softplus(x - mean_c(x)): ONE float per pixel, no alpha / beta volume
//   score       df_clf_kernel (soft-max(clf(desc^2))[1] at the 1/4 resolution it lives at) and df_score_kernel: the align_corners=True
//               up-samplings of the three level maps and of that map, the weights 1/6, 2/6, 3/6 and the product, one float per pixel
//   detector    df_detect_kernel: score > thld, 3x3 maximum, border band, dilation-3 Hessian edge test (IEEE, no FMA: build.py compiles
//               this file with -ffp-contract=off) -> the score where all hold, -inf elsewhere; select.h cand_list in row-major order
//               over a list that holds every pixel; cand_cut to min(kpt_n, max_keypoints or all); ranked_rows_kernel with DfRow:
//               ascending stable (score, pixel) order
//   describe    one wave per key-point: ASLFeat's bilinear rule on the 1/4-resolution map (floor / ceil corners clamped, weights from the
//               unclamped fractions), d / max(|d|, 1e-12)
// Fixed summation orders, no float atomics, grids sized by shapes or capacities: a row's bits do not depend on its batch or on replay;
// no host synchronisation.
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

#define DF_DIM 128       // descriptor width
#define DF_MAGIC 17478.0f  // "DF"
#define DF_IMCHUNK 4096  // image values per partial sum of the image statistics
#define DF_STCHUNK 1024  // pixels per partial sum of the InstanceNorm statistics
#define DF_MIN_SIDE 16
#define DF_STATUS_FLAT 4

// ------------------------------------------------------------------ the layer table (the ONE place that states the backbone)
// name, cin, cout, stride, norm (InstanceNorm + ReLU behind it), tap (the RAW output is score level `tap`; -1 none).  conv1 / conv3 are
// bare upstream and followed by bn1 / bn3: the same arithmetic as norm = 1, with the raw map tapped in between.
struct DfLayer {
    const char* name;
    int cin, cout, stride, norm, tap;
};
static const DfLayer DF_LAYERS[] = {
    {"conv0", 3, 32, 1, 1, -1},      {"conv1", 32, 32, 1, 1, 0},      {"conv2", 32, 64, 2, 1, -1},
    {"conv3", 64, 64, 1, 1, 1},      {"conv4", 64, 128, 2, 1, -1},    {"conv5", 128, 128, 1, 1, -1},
    {"conv6_0", 128, 128, 1, 1, -1}, {"conv6_1", 128, 128, 1, 1, -1}, {"conv6_2", 128, 128, 1, 0, 2},
};
#define DF_NL ((int)(sizeof(DF_LAYERS) / sizeof(DF_LAYERS[0])))
static const int DF_DIL[3] = {3, 2, 1};                                // box dilation of score level 0, 1, 2
static const float DF_LEVEL_W[3] = {1.0f / 6.0f, 2.0f / 6.0f, 3.0f / 6.0f};  // (1, 2, 3) / 6

// what the kernels below are built for: layer 0 is 3 -> 32 at stride 1, widths 32 / 64 / 128, level l tapped at resolution 1 / 2^l
// with width 32 / 64 / 128, the last layer is the bare 128-wide descriptor layer
static bool df_table_ok() {
    if (DF_LAYERS[0].cin != 3 || DF_LAYERS[0].cout != 32 || DF_LAYERS[0].stride != 1 || !DF_LAYERS[0].norm || DF_LAYERS[0].tap >= 0) return false;
    int res = 0, next_tap = 0;
    for (int i = 1; i < DF_NL; ++i) {
        const DfLayer& L = DF_LAYERS[i];
        if (L.cin != DF_LAYERS[i - 1].cout || (L.cout != 32 && L.cout != 64 && L.cout != 128) || (L.stride != 1 && L.stride != 2)) return false;
        if (L.stride == 2) ++res;
        if (L.tap >= 0) {
            if (L.tap != next_tap || res != L.tap || L.cout != (32 << L.tap)) return false;
            ++next_tap;
        }
        if (!L.norm && i != DF_NL - 1) return false;
    }
    return next_tap == 3 && !DF_LAYERS[DF_NL - 1].norm && DF_LAYERS[DF_NL - 1].tap == 2;
}

extern "C" int imcui_hip_darkfeat_num_layers() { return DF_NL; }
// out5 = cin, cout, stride, norm, tap
extern "C" const char* imcui_hip_darkfeat_layer(int i, int* out5) {
    if (i < 0 || i >= DF_NL) return nullptr;
    const DfLayer& L = DF_LAYERS[i];
    if (out5) out5[0] = L.cin, out5[1] = L.cout, out5[2] = L.stride, out5[3] = L.norm, out5[4] = L.tap;
    return L.name;
}

static const TensorTable& df_tensors() {
    static const TensorTable t = [] {
        TensorTable t;
        for (int i = 0; i < DF_NL; ++i) {
            t.add(std::string(DF_LAYERS[i].name) + ".0.weight", (size_t)DF_LAYERS[i].cout * DF_LAYERS[i].cin * 9);
            t.add(std::string(DF_LAYERS[i].name) + ".0.bias", DF_LAYERS[i].cout);  // (zeros when the checkpoint has none: backend.pack_darkfeat)
        }
        t.add("clf.weight", 2 * DF_DIM);
        t.add("clf.bias", 2);
        for (int i = 0; i < 3; ++i) t.add("moving_avg_params." + std::to_string(i), 1);
        return t;
    }();
    return t;
}
extern "C" int imcui_hip_darkfeat_num_tensors() { return df_tensors().size(); }
extern "C" const char* imcui_hip_darkfeat_tensor_name(int i) { return df_tensors().name(i); }

// ------------------------------------------------------------------ packed layout
// hdr [64]: magic, moving_avg_params 0..2.  w0 / b0: layer 0 for the VALU kernel [tap][cin 3][32] + [32].  g[1..]: the other layers
// [cout][tap][cin] with their bias.  clfw [2][128], clfb [2].
struct DfLayout {
    size_t hdr, w0, b0, clfw, clfb;
    GemmLayerOff g[DF_NL];
    size_t total;
};
static DfLayout df_layout() {
    DfLayout l;
    PackCursor p;
    l.hdr = p.get(64);
    l.w0 = p.get((size_t)27 * DF_LAYERS[0].cout);
    l.b0 = p.get(DF_LAYERS[0].cout);
    for (int i = 1; i < DF_NL; ++i) l.g[i].place(p, DF_LAYERS[i].cout, 9 * DF_LAYERS[i].cin);
    l.clfw = p.get(2 * DF_DIM);
    l.clfb = p.get(2);
    l.total = p.off;
    return l;
}
extern "C" size_t imcui_hip_darkfeat_packed_floats() { return df_table_ok() ? df_layout().total : 0; }

// t: host pointers of the tensors in imcui_hip_darkfeat_tensor_name order (shapes checked by the caller)
extern "C" int imcui_hip_darkfeat_pack_weights(const float* const* t, float* packed) {
    if (!df_table_ok() || !t || !packed) return IMCUI_ERR_ARG;
    const TensorTable& names = df_tensors();
    for (int i = 0; i < names.size(); ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const DfLayout l = df_layout();
    memset(packed, 0, l.total * sizeof(float));
    auto T = [&](const std::string& name) { return t[names.find(name)]; };
    packed[l.hdr] = DF_MAGIC;
    for (int i = 0; i < 3; ++i) packed[l.hdr + 1 + i] = T("moving_avg_params." + std::to_string(i))[0];
    for (int i = 0; i < DF_NL; ++i) {
        const DfLayer& L = DF_LAYERS[i];
        const float *w = T(std::string(L.name) + ".0.weight"), *b = T(std::string(L.name) + ".0.bias");
        if (i == 0) {
            for (int co = 0; co < L.cout; ++co)
                for (int ci = 0; ci < 3; ++ci)
                    for (int k = 0; k < 9; ++k) packed[l.w0 + ((size_t)k * 3 + ci) * L.cout + co] = w[((size_t)co * 3 + ci) * 9 + k];
            memcpy(packed + l.b0, b, L.cout * sizeof(float));
            continue;
        }
        pack_conv_gemm(w, L.cout, L.cin, 3, L.cin, packed + l.g[i].w);
        memcpy(packed + l.g[i].b, b, L.cout * sizeof(float));
        l.g[i].split_planes(packed, L.cout, 9 * L.cin);
    }
    memcpy(packed + l.clfw, T("clf.weight"), 2 * DF_DIM * sizeof(float));
    memcpy(packed + l.clfb, T("clf.bias"), 2 * sizeof(float));
    return IMCUI_OK;
}

namespace {

// the sum of the 256 per-thread values of a workgroup in a fixed tree order (every thread calls it; the result is in sh[0])
__device__ __forceinline__ void df_block_sum2(double* sh0, double* sh1, double a, double b) {
    const int tid = threadIdx.x;
    sh0[tid] = a;
    sh1[tid] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            sh0[tid] += sh0[tid + o];
            sh1[tid] += sh1[tid + o];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ image statistics
// grid (nchunk, B): partial sum and sum of squares of DF_IMCHUNK consecutive values of image b (n = 3 H W values) -> part [B][nchunk][2]
__global__ __launch_bounds__(256) void df_imstat_partial_kernel(const float* __restrict__ img, long n, double* __restrict__ part, int nchunk) {
    __shared__ double sh0[256], sh1[256];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* p = img + (long)b * n;
    double s = 0.0, ss = 0.0;
    for (int j = 0; j < DF_IMCHUNK / 256; ++j) {
        const long i = (long)chunk * DF_IMCHUNK + j * 256 + threadIdx.x;
        if (i < n) {
            const double v = (double)p[i];
            s += v;
            ss += v * v;
        }
    }
    df_block_sum2(sh0, sh1, s, ss);
    if (threadIdx.x == 0) {
        part[((long)b * nchunk + chunk) * 2] = sh0[0];
        part[((long)b * nchunk + chunk) * 2 + 1] = sh1[0];
    }
}
// one thread per image folds the partials in chunk order: imstat [B][2] = mean, unbiased std (1 for a flat image), flat [B], status bit
__global__ void df_imstat_fold_kernel(const double* __restrict__ part, int nchunk, long n, int B, float* __restrict__ imstat, int* __restrict__ flat,
                                      int* __restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0, ss = 0.0;
    for (int c = 0; c < nchunk; ++c) {
        s += part[((long)b * nchunk + c) * 2];
        ss += part[((long)b * nchunk + c) * 2 + 1];
    }
    const double mean = s / (double)n, var = (ss - s * mean) / (double)(n - 1);
    const float sd = (float)sqrt(var > 0.0 ? var : 0.0);
    const bool is_flat = !(sd > 0.0f) || !(sd < INFINITY);
    imstat[2 * b] = (float)mean;
    imstat[2 * b + 1] = is_flat ? 1.0f : sd;
    flat[b] = is_flat ? 1 : 0;
    if (is_flat) atomicOr(status, DF_STATUS_FLAT);
}

// ------------------------------------------------------------------ layer 0
// stem3x3_kernel (net_kernels.h) without the ReLU and with the per-image normalisation where the image is read: 3 -> COUT, 3x3, pad 1,
// one thread per pixel, weights [tap][cin][COUT] in LDS, taps and channels summed in ascending order.  img planar [B, 3, h, wd].
template <int COUT>
__global__ __launch_bounds__(256) void df_stem_kernel(const float* __restrict__ img, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ imstat, float* __restrict__ out, int h, int wd, long npix) {
    __shared__ float sw[27 * COUT + COUT];
    for (int i = threadIdx.x; i < 27 * COUT + COUT; i += 256) sw[i] = i < 27 * COUT ? w[i] : bias[i - 27 * COUT];
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % wd);
    const long q = p / wd;
    const int y = (int)(q % h);
    const long b = q / h;
    const float mean = imstat[2 * b], sd = imstat[2 * b + 1];
    float win[27];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = x + kx - 1;
            const bool in = yy >= 0 && yy < h && xx >= 0 && xx < wd;
#pragma unroll
            for (int c = 0; c < 3; ++c) win[(ky * 3 + kx) * 3 + c] = in ? __fdiv_rn(__fsub_rn(img[((b * 3 + c) * h + yy) * (long)wd + xx], mean), sd) : 0.0f;
        }
    float* o = out + p * COUT;
#pragma unroll
    for (int c0 = 0; c0 < COUT; c0 += 4) {
        float a[4] = {sw[27 * COUT + c0], sw[27 * COUT + c0 + 1], sw[27 * COUT + c0 + 2], sw[27 * COUT + c0 + 3]};
#pragma unroll
        for (int t = 0; t < 27; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = fmaf(win[t], sw[t * COUT + c0 + j], a[j]);
        *reinterpret_cast<float4*>(o + c0) = make_float4(a[0], a[1], a[2], a[3]);
    }
}

// ------------------------------------------------------------------ InstanceNorm
// grid (nchunk, B): x [B][np][C] NHWC; the partial sum and sum of squares of every channel over DF_STCHUNK consecutive pixels.  Thread
// t owns channel quad t % (C / 4) of the pixels t / (C / 4), + 256 / (C / 4), ...; the pixel lanes meet in LDS and are added in ascending
// order -> part [B][nchunk][C][2].
template <int C>
__global__ __launch_bounds__(256) void df_in_partial_kernel(const float* __restrict__ x, int np, double* __restrict__ part, int nchunk) {
    constexpr int Q = C / 4, PL = 256 / Q;
    __shared__ double sh[256 * 8];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, q = tid % Q, pl = tid / Q;
    const int p1 = min(np, (chunk + 1) * DF_STCHUNK);
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = chunk * DF_STCHUNK + pl; p < p1; p += PL) {
        const float4 v = *reinterpret_cast<const float4*>(x + ((long)b * np + p) * C + 4 * q);
        const double d[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] += d[j];
            s[4 + j] += d[j] * d[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[(pl * Q + q) * 8 + j] = s[j];
    __syncthreads();
    if (tid < Q * 8) {
        const int qq = tid / 8, k = tid % 8;
        double a = 0.0;
        for (int l = 0; l < PL; ++l) a += sh[(l * Q + qq) * 8 + k];
        part[(((long)b * nchunk + chunk) * C + 4 * qq + (k & 3)) * 2 + (k >> 2)] = a;
    }
}
// grid (B), C threads: the partials folded in chunk order -> stat [B][C][2] = mean, 1 / sqrt(biased variance + 1e-5)
__global__ void df_in_fold_kernel(const double* __restrict__ part, int nchunk, int np, int C, float* __restrict__ stat) {
    const int b = blockIdx.x, c = threadIdx.x;
    if (c >= C) return;
    double s = 0.0, ss = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        const double* p = part + (((long)b * nchunk + k) * C + c) * 2;
        s += p[0];
        ss += p[1];
    }
    const double mean = s / (double)np;
    double var = ss / (double)np - mean * mean;
    if (!(var > 0.0)) var = 0.0;
    stat[((long)b * C + c) * 2] = (float)mean;
    stat[((long)b * C + c) * 2 + 1] = (float)(1.0 / sqrt(var + 1e-5));
}
// relu((x - m) * r), one thread per float4, in place or not; n4 = B np C / 4
__global__ __launch_bounds__(256) void df_in_apply_kernel(const float* __restrict__ x, const float* __restrict__ stat, float* __restrict__ out, int np, int C, long n4) {
    const int C4 = C >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const long b = (i / C4) / np;
        const float4 v = *reinterpret_cast<const float4*>(x + i * 4);
        const float* st = stat + (b * C + c) * 2;
        float4 o;
        o.x = fmaxf(__fmul_rn(__fsub_rn(v.x, st[0]), st[1]), 0.0f);
        o.y = fmaxf(__fmul_rn(__fsub_rn(v.y, st[2]), st[3]), 0.0f);
        o.z = fmaxf(__fmul_rn(__fsub_rn(v.z, st[4]), st[5]), 0.0f);
        o.w = fmaxf(__fmul_rn(__fsub_rn(v.w, st[6]), st[7]), 0.0f);
        *reinterpret_cast<float4*>(out + i * 4) = o;
    }
}

// ------------------------------------------------------------------ peakiness
// F.softplus (beta 1, threshold 20)
__device__ __forceinline__ float df_softplus(float v) { return v > 20.0f ? v : log1pf(expf(v)); }
// index i of a map of n under reflect padding (needs the pad width below n); tile positions no output pixel reads are clamped into the map
__device__ __forceinline__ int df_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}
__device__ __forceinline__ float df_half_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float df_half_max(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// grid (cdiv(w, 8), cdiv(h, 8), B), 256 threads: x [B, h, w, C] raw -> out [B, h, w].  The (8 + 2 D)^2 x C tile of x / *mavg is staged
// in LDS (25 / 36 / 50 KiB at (C, D) = (32, 3), (64, 2), (128, 1)).  Thread t owns channels (t & 31) + 32 k of tile row t >> 5 and walks its 8
// pixels: the channel sum is added per thread in ascending k, then over the 32 lanes by the butterfly (16, 8, 4, 2, 1); the box sums its 9
// taps row-major and is divided by 9; the maximum takes the same route.  A map narrower than the tile is the same code (pixels outside
// are not written); one narrower than D + 1 has no reflect padding and is refused by the callers.
template <int C, int D>
__global__ __launch_bounds__(256) void df_peak_kernel(const float* __restrict__ x, const float* __restrict__ mavg, float* __restrict__ out, int h, int w) {
    constexpr int TW = 8 + 2 * D, NP = TW * TW, C4 = C / 4;
    __shared__ float tile[NP * C];
    const int b = blockIdx.z, y0 = blockIdx.y * 8, x0 = blockIdx.x * 8, tid = threadIdx.x;
    const float m = *mavg;
    const float* xb = x + (long)b * h * w * C;
    for (int e = tid; e < NP * C4; e += 256) {
        const int pp = e / C4, q = e - pp * C4, ty = pp / TW, tx = pp - ty * TW;
        const int gy = df_reflect(y0 + ty - D, h), gx = df_reflect(x0 + tx - D, w);
        const float4 v = *reinterpret_cast<const float4*>(xb + ((long)gy * w + gx) * C + 4 * q);
        *reinterpret_cast<float4*>(tile + pp * C + 4 * q) = make_float4(__fdiv_rn(v.x, m), __fdiv_rn(v.y, m), __fdiv_rn(v.z, m), __fdiv_rn(v.w, m));
    }
    __syncthreads();
    const int lane = tid & 31, row = tid >> 5;
    for (int px = 0; px < 8; ++px) {
        const int cp = (row + D) * TW + px + D;
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < C / 32; ++k) s += tile[cp * C + lane + 32 * k];
        const float mean = __fdiv_rn(df_half_sum(s), (float)C);
        float best = -INFINITY;
#pragma unroll
        for (int k = 0; k < C / 32; ++k) {
            const int c = lane + 32 * k;
            float box = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) box += tile[(cp + dy * D * TW + dx * D) * C + c];
            box = __fdiv_rn(box, 9.0f);
            const float v = tile[cp * C + c];
            best = fmaxf(best, df_softplus(v - box) * df_softplus(v - mean));
        }
        best = df_half_max(best);
        if (lane == 0 && y0 + row < h && x0 + px < w) out[((long)b * h + y0 + row) * w + x0 + px] = best;
    }
}

// ------------------------------------------------------------------ score assembly
// soft-max(clf(desc^2))[1] per 1/4-resolution pixel: 32 lanes per pixel, lane l owns channels 4 l .. 4 l + 3 (fmaf chains in channel
// order), the butterfly, + bias, the 2-way soft-max in torch's form (exp(a - max) / sum)
__global__ __launch_bounds__(256) void df_clf_kernel(const float* __restrict__ desc, const float* __restrict__ cw, const float* __restrict__ cb,
                                                     float* __restrict__ prob, long total) {
    const int lane = threadIdx.x & 31;
    const long p = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = p < total;
    float a0 = 0.0f, a1 = 0.0f;
    if (live) {
        const float4 d = *reinterpret_cast<const float4*>(desc + p * DF_DIM + 4 * lane);
        const float4 w0 = *reinterpret_cast<const float4*>(cw + 4 * lane), w1 = *reinterpret_cast<const float4*>(cw + DF_DIM + 4 * lane);
        const float q[4] = {d.x * d.x, d.y * d.y, d.z * d.z, d.w * d.w};
        const float u0[4] = {w0.x, w0.y, w0.z, w0.w}, u1[4] = {w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a0 = fmaf(q[j], u0[j], a0);
            a1 = fmaf(q[j], u1[j], a1);
        }
    }
    a0 = df_half_sum(a0) + cb[0];
    a1 = df_half_sum(a1) + cb[1];
    if (live && lane == 0) {
        const float mx = fmaxf(a0, a1), e0 = expf(a0 - mx), e1 = expf(a1 - mx);
        prob[p] = __fdiv_rn(e1, e0 + e1);
    }
}

// bilinear sample of the planar map m [hi, wi] at output pixel (y, x) with ATen's align_corners=True rule, rows mixed first
__device__ __forceinline__ float df_up(const float* __restrict__ m, int hi, int wi, int y0, int y1, int x0, int x1, float hy0, float hy1, float wx0, float wx1) {
    const float v00 = m[(long)y0 * wi + x0], v01 = m[(long)y0 * wi + x1], v10 = m[(long)y1 * wi + x0], v11 = m[(long)y1 * wi + x1];
    const float top = __fadd_rn(__fmul_rn(wx0, v00), __fmul_rn(wx1, v01)), bot = __fadd_rn(__fmul_rn(wx0, v10), __fmul_rn(wx1, v11));
    return __fadd_rn(__fmul_rn(hy0, top), __fmul_rn(hy1, bot));
}
// one thread per pixel: score = ((w0 s0 + w1 up(s1)) + w2 up(s2)) * up(prob); s0 [B, H, W] (its up-sampling to its own size is the
// identity), s1 [B, h1, w1], s2 and prob [B, h2, w2]; sc = the four align_corners scales (h1, w1, h2, w2)
__global__ __launch_bounds__(256) void df_score_kernel(const float* __restrict__ s0, const float* __restrict__ s1, const float* __restrict__ s2,
                                                       const float* __restrict__ prob, int H, int W, int h1, int w1, int h2, int w2, float sh1, float sw1,
                                                       float sh2, float sw2, float lw0, float lw1, float lw2, float* __restrict__ score, long npix) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % W);
    const long q = p / W;
    const int y = (int)(q % H);
    const long b = q / H;
    int ya, yb, xa, xb;
    float hy0, hy1, wx0, wx1;
    bilinear_src_align_corners(y, sh1, h1, &ya, &yb, &hy0, &hy1);
    bilinear_src_align_corners(x, sw1, w1, &xa, &xb, &wx0, &wx1);
    const float u1 = df_up(s1 + b * h1 * w1, h1, w1, ya, yb, xa, xb, hy0, hy1, wx0, wx1);
    bilinear_src_align_corners(y, sh2, h2, &ya, &yb, &hy0, &hy1);
    bilinear_src_align_corners(x, sw2, w2, &xa, &xb, &wx0, &wx1);
    const float u2 = df_up(s2 + b * h2 * w2, h2, w2, ya, yb, xa, xb, hy0, hy1, wx0, wx1);
    const float up = df_up(prob + b * h2 * w2, h2, w2, ya, yb, xa, xb, hy0, hy1, wx0, wx1);
    const float sum = __fadd_rn(__fadd_rn(__fmul_rn(lw0, s0[p]), __fmul_rn(lw1, u1)), __fmul_rn(lw2, u2));
    score[p] = __fmul_rn(sum, up);
}

// ------------------------------------------------------------------ detector
// one thread per pixel of score [B, H, W] -> det [B, H, W]: the score where the pixel is a key-point candidate, -inf elsewhere.
//   s > thld; s == the maximum of its 3x3 window inside the map (nms); eof <= y < H - eof, eof <= x < W - eof;
//   dii = (s(y-3, x) - 2 s) + s(y+3, x), djj likewise along x, dij = 0.25 * (((s(y-3, x-3) - s(y-3, x+3)) - s(y+3, x-3)) + s(y+3, x+3)),
//   zero outside the map; det = dii djj - dij dij > 0 and (tr tr) / det <= ethr with tr = dii + djj.  Every operation rounds once.
__global__ __launch_bounds__(256) void df_detect_kernel(const float* __restrict__ score, const int* __restrict__ flat, int H, int W, float thld, int nms,
                                                        int eof, float ethr, float* __restrict__ det, long npix) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % W);
    const long q = p / W;
    const int y = (int)(q % H);
    const long b = q / H;
    const float* m = score + b * H * W;
    const float s = m[(long)y * W + x];
    bool keep = s > thld && !(flat && flat[b]) && y >= eof && y < H - eof && x >= eof && x < W - eof;
    if (keep && nms) {
        float mx = s;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) mx = fmaxf(mx, m[(long)yy * W + xx]);
            }
        keep = s == mx;
    }
    if (keep) {
        const auto at = [&](int yy, int xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? m[(long)yy * W + xx] : 0.0f; };
        const float s2 = __fmul_rn(2.0f, s);
        const float dii = __fadd_rn(__fsub_rn(at(y - 3, x), s2), at(y + 3, x));
        const float djj = __fadd_rn(__fsub_rn(at(y, x - 3), s2), at(y, x + 3));
        const float dij = __fmul_rn(0.25f, __fadd_rn(__fsub_rn(__fsub_rn(at(y - 3, x - 3), at(y - 3, x + 3)), at(y + 3, x - 3)), at(y + 3, x + 3)));
        const float dt = __fsub_rn(__fmul_rn(dii, djj), __fmul_rn(dij, dij));
        const float tr = __fadd_rn(dii, djj);
        keep = dt > 0.0f && __fdiv_rn(__fmul_rn(tr, tr), dt) <= ethr;
    }
    det[p] = keep ? s : -INFINITY;
}

struct DfPred {
    __device__ void bind(int) {}
    __device__ bool operator()(const float* img, int idx) const { return img[idx] > -INFINITY; }
};

// The rows of ranked_rows_kernel (ascending (score, pixel) order), one thread each: (x, y) and the score.  Rows past the count are zero.
struct DfRow {
    const int* cidx;
    int np, W, kout;
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
        const int slot = ks[i0 + j], r = rank[j], pix = cidx[(long)b * np + slot];
        float* kp = kpts + (long)b * kout * 2;
        kp[2 * r] = (float)(pix % W);
        kp[2 * r + 1] = (float)(pix / W);
        scores[(long)b * kout + r] = cs[slot];
    }
};

// ------------------------------------------------------------------ describe
// One wave per key-point row (grid (cdiv(kcap, 4), B)): pos = (y, x) / 4 on the map dmap [B, h, w, 128]; corners floor / ceil clamped to
// the map, weights from the unclamped fractions, ((w_tl f_tl + w_tr f_tr) + w_bl f_bl) + w_br f_br; lane l owns channels 2 l, 2 l + 1;
// the squares meet in wave_sum; d / max(|d|, 1e-12) (F.normalize).  Rows past the count (nkpts[b], or nprobe when null) are zero.
__global__ __launch_bounds__(256) void df_describe_kernel(const float* __restrict__ dmap, int h, int w, const float* __restrict__ kpts,
                                                          const int* __restrict__ nkpts, int nprobe, int kcap, float* __restrict__ desc) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= kcap) return;  // (wave-uniform)
    float* o = desc + ((long)b * kcap + i) * DF_DIM + 2 * lane;
    const int n = min(nkpts ? nkpts[b] : nprobe, kcap);
    if (i >= n) {
        *reinterpret_cast<float2*>(o) = make_float2(0.0f, 0.0f);
        return;
    }
    const float* kp = kpts + ((long)b * kcap + i) * 2;
    const float px = __fdiv_rn(kp[0], 4.0f), py = __fdiv_rn(kp[1], 4.0f);
    const float fx = floorf(px), fy = floorf(py);
    const float dj = __fsub_rn(px, fx), di = __fsub_rn(py, fy);
    const int xl = min(max((int)fx, 0), w - 1), yt = min(max((int)fy, 0), h - 1);
    const int xr = min(max((int)ceilf(px), 0), w - 1), yb = min(max((int)ceilf(py), 0), h - 1);
    const float wi0 = __fsub_rn(1.0f, di), wj0 = __fsub_rn(1.0f, dj);
    const float wtl = __fmul_rn(wi0, wj0), wtr = __fmul_rn(wi0, dj), wbl = __fmul_rn(di, wj0), wbr = __fmul_rn(di, dj);
    const float* mb = dmap + (long)b * h * w * DF_DIM + 2 * lane;
    const float2 ftl = *reinterpret_cast<const float2*>(mb + ((long)yt * w + xl) * DF_DIM), ftr = *reinterpret_cast<const float2*>(mb + ((long)yt * w + xr) * DF_DIM),
                 fbl = *reinterpret_cast<const float2*>(mb + ((long)yb * w + xl) * DF_DIM), fbr = *reinterpret_cast<const float2*>(mb + ((long)yb * w + xr) * DF_DIM);
    const float d0 = ((wtl * ftl.x + wtr * ftr.x) + wbl * fbl.x) + wbr * fbr.x;
    const float d1 = ((wtl * ftl.y + wtr * ftr.y) + wbl * fbl.y) + wbr * fbr.y;
    const float nrm = fmaxf(sqrtf(wave_sum(d0 * d0 + d1 * d1)), 1e-12f);
    *reinterpret_cast<float2*>(o) = make_float2(__fdiv_rn(d0, nrm), __fdiv_rn(d1, nrm));
}

}  // namespace

// ------------------------------------------------------------------ host: launches
static int df_down(int n) { return (n - 1) / 2 + 1; }  // rows / columns behind a stride-2 layer

static int df_conv(imcui_hip_t* h, const float* P, const GemmLayerOff& o, const float* in, float* out, int B, int hin, int win, int cin, int cout, int stride,
                   hipStream_t stream) {
    const int ho = stride == 2 ? df_down(hin) : hin, wo = stride == 2 ? df_down(win) : win;
    GemmP g;
    g.epi = EPI_CONV;
    g.A = in;
    gemm_set_weights(g, P, o, cout, 9 * cin, h->precision == 1);
    gemm_set_conv(g, 3, stride, 1, hin, win, ho, wo, cin);
    g.M = B * ho * wo;
    g.C = out;
    g.ldc = cout;
    g.act = 0;
    return gemm_launch(h, g, stream);
}

static int df_imstat_chunks(long n) { return (int)((n + DF_IMCHUNK - 1) / DF_IMCHUNK); }
static int df_in_chunks(int np) { return cdiv(np, DF_STCHUNK); }

// per-image statistics and layer 0: image [B, 3, H, W] -> out [B, H, W, 32] raw; status is OR-ed, never cleared here
static int df_stem(imcui_hip_t* h, const DfLayout& l, const float* P, const float* img, int B, int H, int W, double* part, float* imstat, int* flat, int* status,
                   float* out, hipStream_t stream) {
    const long n = 3L * H * W, npix = (long)B * H * W;
    const int nchunk = df_imstat_chunks(n);
    hipLaunchKernelGGL(df_imstat_partial_kernel, dim3(nchunk, B), dim3(256), 0, stream, img, n, part, nchunk);
    hipLaunchKernelGGL(df_imstat_fold_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, part, nchunk, n, B, imstat, flat, status);
    hipLaunchKernelGGL(df_stem_kernel<32>, dim3(blocks_256(npix)), dim3(256), 0, stream, img, P + l.w0, P + l.b0, imstat, out, H, W, npix);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// InstanceNorm + ReLU of x [B, np, C] -> out (may be x); part holds B * df_in_chunks(np) * C * 2 doubles, stat B * C * 2 floats
static int df_inorm(imcui_hip_t* h, const float* x, float* out, int B, int np, int C, double* part, float* stat, hipStream_t stream) {
    const int nchunk = df_in_chunks(np);
    const dim3 grid(nchunk, B);
    if (C == 32)
        hipLaunchKernelGGL(df_in_partial_kernel<32>, grid, dim3(256), 0, stream, x, np, part, nchunk);
    else if (C == 64)
        hipLaunchKernelGGL(df_in_partial_kernel<64>, grid, dim3(256), 0, stream, x, np, part, nchunk);
    else if (C == 128)
        hipLaunchKernelGGL(df_in_partial_kernel<128>, grid, dim3(256), 0, stream, x, np, part, nchunk);
    else
        return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: InstanceNorm is built for 32 / 64 / 128 channels, not %d", C);
    hipLaunchKernelGGL(df_in_fold_kernel, dim3(B), dim3(128), 0, stream, part, nchunk, np, C, stat);
    const long n4 = (long)B * np * (C / 4);
    hipLaunchKernelGGL(df_in_apply_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, x, stat, out, np, C, n4);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// peakiness of level `lev` (its C and dilation) on x [B, hh, ww, C] -> out [B, hh, ww]
static int df_peak(imcui_hip_t* h, const float* x, const float* mavg, float* out, int B, int hh, int ww, int C, int d, hipStream_t stream) {
    if (hh < d + 1 || ww < d + 1) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: a %dx%d map has no reflect padding of width %d", hh, ww, d);
    const dim3 grid(cdiv(ww, 8), cdiv(hh, 8), B);
    if (C == 32 && d == 3)
        hipLaunchKernelGGL((df_peak_kernel<32, 3>), grid, dim3(256), 0, stream, x, mavg, out, hh, ww);
    else if (C == 64 && d == 2)
        hipLaunchKernelGGL((df_peak_kernel<64, 2>), grid, dim3(256), 0, stream, x, mavg, out, hh, ww);
    else if (C == 128 && d == 1)
        hipLaunchKernelGGL((df_peak_kernel<128, 1>), grid, dim3(256), 0, stream, x, mavg, out, hh, ww);
    else
        return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: the peakiness pass is built for (C, d) = (32, 3), (64, 2), (128, 1), not (%d, %d)", C, d);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

static float df_ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }  // ATen, align_corners=True

// pk0 [B, H, W], pk1 [B, h1, w1], pk2 [B, h2, w2], dmap [B, h2, w2, 128] -> prob [B, h2, w2], score [B, H, W]
static int df_assemble(imcui_hip_t* h, const DfLayout& l, const float* P, const float* pk0, const float* pk1, const float* pk2, const float* dmap, int B, int H, int W,
                       float* prob, float* score, hipStream_t stream) {
    const int h1 = df_down(H), w1 = df_down(W), h2 = df_down(h1), w2 = df_down(w1);
    const long nq = (long)B * h2 * w2, npix = (long)B * H * W;
    hipLaunchKernelGGL(df_clf_kernel, dim3((unsigned)((nq + 7) / 8)), dim3(256), 0, stream, dmap, P + l.clfw, P + l.clfb, prob, nq);
    hipLaunchKernelGGL(df_score_kernel, dim3(blocks_256(npix)), dim3(256), 0, stream, pk0, pk1, pk2, prob, H, W, h1, w1, h2, w2, df_ac_scale(h1, H),
                       df_ac_scale(w1, W), df_ac_scale(h2, H), df_ac_scale(w2, W), DF_LEVEL_W[0], DF_LEVEL_W[1], DF_LEVEL_W[2], score, npix);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

struct DfDet {
    float score_thld, edge_thld;
    int nms_size, eof_mask, kpt_n;
};
static int df_det_check(imcui_hip_t* h, const DfDet& d, int np, int max_keypoints, int kout) {
    if (d.nms_size != 0 && d.nms_size != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: nms_size=%d (0 or 3)", d.nms_size);
    if (d.eof_mask < 0 || d.kpt_n < 1 || !(d.edge_thld > 0.0f))
        return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: eof_mask=%d (>= 0), kpt_n=%d (>= 1), edge_thld=%g (> 0)", d.eof_mask, d.kpt_n, (double)d.edge_thld);
    if (max_keypoints < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: max_keypoints=%d is negative (0 keeps every key-point)", max_keypoints);
    const int need = std::min(np, max_keypoints > 0 ? std::min(max_keypoints, d.kpt_n) : d.kpt_n);
    if (kout < need || kout < 1) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: kout=%d below min(kpt_n, max_keypoints or all, %d pixels) = %d", kout, np, need);
    return IMCUI_OK;
}

struct DfSel {
    float* det;
    CandScan scan;
    ScoreIndexList cand;  // (holds every pixel)
    CutList cut;
};
static void df_carve_sel(WsAlloc& a, DfSel& s, int B, int np) {
    s.det = a.get<float>((size_t)B * np);
    s.scan.carve(a, B, (size_t)np);
    s.cand.carve(a, B, np);
    s.cut.carve(a, B, np);
}
// the detector on score [B, H, W], the candidate list (every pixel fits: it cannot overflow), the cut, the ranked rows
static int df_detect(imcui_hip_t* h, const DfSel& s, const float* score, const int* flat, int B, int H, int W, const DfDet& d, int max_keypoints, int kout,
                     float* keypoints, float* scores, int* num_keypoints, int* status, hipStream_t stream) {
    const int np = H * W;
    const long npix = (long)B * np;
    const float ethr = (float)(((double)d.edge_thld + 1.0) * ((double)d.edge_thld + 1.0) / (double)d.edge_thld);
    const int limit = max_keypoints > 0 ? std::min(max_keypoints, d.kpt_n) : d.kpt_n;
    hipLaunchKernelGGL(df_detect_kernel, dim3(blocks_256(npix)), dim3(256), 0, stream, score, flat, H, W, d.score_thld, d.nms_size, d.eof_mask, ethr, s.det, npix);
    cand_list(stream, s.det, np, B, DfPred{}, s.scan, np, s.cand.emit());
    cand_cut(stream, s.cand.cscore, s.scan.total, np, limit, s.cut, status, B);
    ranked_rows(stream, s.cand.cscore, np, s.cut, kout, num_keypoints, DfRow{s.cand.cidx, np, W, kout, keypoints, scores}, B);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

static void df_describe(const float* dmap, int h4, int w4, const float* kpts, const int* nkpts, int nprobe, int kcap, int B, float* desc, hipStream_t stream) {
    hipLaunchKernelGGL(df_describe_kernel, dim3(cdiv(kcap, 4), B), dim3(256), 0, stream, dmap, h4, w4, kpts, nkpts, nprobe, kcap, desc);
}

struct DfWs {
    float *buf[3][2], *pk[3], *prob, *score, *imstat, *stat;
    double *impart, *inpart;
    int *flat, *status;
    DfSel sel;
    size_t total;
    bool ok;
};
// the doubles the InstanceNorm partials of the largest layer need, per image
static size_t df_inpart_doubles(int H, int W) {
    size_t m = 0;
    int hh = H, ww = W;
    for (int i = 0; i < DF_NL; ++i) {
        if (DF_LAYERS[i].stride == 2) hh = df_down(hh), ww = df_down(ww);
        m = std::max(m, (size_t)df_in_chunks(hh * ww) * DF_LAYERS[i].cout * 2);
    }
    return m;
}
static DfWs df_carve(void* ws, size_t bytes, int B, int H, int W) {
    WsAlloc a(ws, bytes);
    DfWs s;
    memset(&s, 0, sizeof s);
    int hh = H, ww = W;
    for (int r = 0; r < 3; ++r) {
        const size_t n = (size_t)B * hh * ww * (32 << r);
        s.buf[r][0] = a.get<float>(n);
        s.buf[r][1] = a.get<float>(n);
        s.pk[r] = a.get<float>((size_t)B * hh * ww);
        if (r == 2) s.prob = a.get<float>((size_t)B * hh * ww);
        hh = df_down(hh), ww = df_down(ww);
    }
    s.score = a.get<float>((size_t)B * H * W);
    s.impart = a.get<double>((size_t)B * df_imstat_chunks(3L * H * W) * 2);
    s.imstat = a.get<float>((size_t)B * 2);
    s.flat = a.get<int>(B);
    s.inpart = a.get<double>((size_t)B * df_inpart_doubles(H, W));
    s.stat = a.get<float>((size_t)B * DF_DIM * 2);
    df_carve_sel(a, s.sel, B, H * W);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

static int df_check(imcui_hip_t* h, int B, int H, int W) {
    if (!df_table_ok()) return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "darkfeat: the layer table is not one the kernels are built for");
    if (B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: B=%d above 1024", B);
    if (H < DF_MIN_SIDE || W < DF_MIN_SIDE)
        return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: H=%d W=%d: every side needs at least %d pixels (the 1/4-resolution map and the dilation-3 box need them)", H, W,
                             DF_MIN_SIDE);
    if ((long)H * W * 32 > 0x7fffffffL / B) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: B=%d images of %dx%d exceed the 2^31 index range of one call", B, H, W);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_darkfeat_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || B > 1024 || H < DF_MIN_SIDE || W < DF_MIN_SIDE) return 0;
    return df_carve(nullptr, 0, B, H, W).total;
}

extern "C" int imcui_hip_darkfeat_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, float score_thld, float edge_thld,
                                          int nms_size, int eof_mask, int kpt_n, int max_keypoints, int kout, float* keypoints, float* scores, float* descriptors,
                                          int* num_keypoints, int* status, float* dbg_score, float* dbg_desc, float* dbg_peak0, float* dbg_peak1, float* dbg_peak2,
                                          float* dbg_prob, int dbg_layer, float* dbg_raw, float* dbg_norm, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (C != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: %d image channels; the network reads RGB (3)", C);
    int rc;
    IMCUI_RUN(df_check(h, B, H, W));
    const DfDet det{score_thld, edge_thld, nms_size, eof_mask, kpt_n};
    IMCUI_RUN(df_det_check(h, det, H * W, max_keypoints, kout));
    if (!packed || !image || !keypoints || !scores || !descriptors || !num_keypoints) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat: null argument");
    const DfLayout l = df_layout();
    DfWs s = df_carve(ws, ws_bytes, B, H, W);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "darkfeat: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const float* P = packed;
    int* st = status ? status : s.status;
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, st, 1);
    // ---- backbone: convolution (raw) -> peakiness of a tapped level -> InstanceNorm + ReLU in place
    int hh = H, ww = W, res = 0;
    float* cur = s.buf[0][0];
    IMCUI_RUN(df_stem(h, l, P, image, B, H, W, s.impart, s.imstat, s.flat, st, cur, stream));
    for (int i = 0; i < DF_NL; ++i) {
        const DfLayer& L = DF_LAYERS[i];
        if (i > 0) {
            if (L.stride == 2) ++res;
            float* dst = s.buf[res][0] == cur ? s.buf[res][1] : s.buf[res][0];
            IMCUI_RUN(df_conv(h, P, l.g[i], cur, dst, B, hh, ww, L.cin, L.cout, L.stride, stream));
            if (L.stride == 2) hh = df_down(hh), ww = df_down(ww);
            cur = dst;
        }
        const size_t nmap = (size_t)B * hh * ww * L.cout * sizeof(float);
        if (i == dbg_layer) copy_if(dbg_raw, cur, nmap, stream);
        if (L.tap >= 0) IMCUI_RUN(df_peak(h, cur, P + l.hdr + 1 + L.tap, s.pk[L.tap], B, hh, ww, L.cout, DF_DIL[L.tap], stream));
        if (L.norm) IMCUI_RUN(df_inorm(h, cur, cur, B, hh * ww, L.cout, s.inpart, s.stat, stream));
        if (i == dbg_layer) copy_if(dbg_norm, cur, nmap, stream);
    }
    const float* dmap = cur;  // [B, h4, w4, 128]
    const int h1 = df_down(H), w1 = df_down(W), h4 = hh, w4 = ww;
    // ---- score, detector, descriptors
    IMCUI_RUN(df_assemble(h, l, P, s.pk[0], s.pk[1], s.pk[2], dmap, B, H, W, s.prob, s.score, stream));
    copy_if(dbg_score, s.score, (size_t)B * H * W * sizeof(float), stream);
    copy_if(dbg_desc, dmap, (size_t)B * h4 * w4 * DF_DIM * sizeof(float), stream);
    copy_if(dbg_peak0, s.pk[0], (size_t)B * H * W * sizeof(float), stream);
    copy_if(dbg_peak1, s.pk[1], (size_t)B * h1 * w1 * sizeof(float), stream);
    copy_if(dbg_peak2, s.pk[2], (size_t)B * h4 * w4 * sizeof(float), stream);
    copy_if(dbg_prob, s.prob, (size_t)B * h4 * w4 * sizeof(float), stream);
    IMCUI_RUN(df_detect(h, s.sel, s.score, s.flat, B, H, W, det, max_keypoints, kout, keypoints, scores, num_keypoints, st, stream));
    df_describe(dmap, h4, w4, keypoints, num_keypoints, 0, kout, B, descriptors, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ test entries
struct DfProbeWs {
    double* part;
    float *stat, *prob;
    int* flat;
    DfSel sel;
    size_t total;
    bool ok;
};
// scratch of the probes below for B maps of H x W with up to 128 channels
static DfProbeWs df_probe_carve(void* ws, size_t bytes, int B, int H, int W) {
    WsAlloc a(ws, bytes);
    DfProbeWs s;
    memset(&s, 0, sizeof s);
    const size_t np = (size_t)H * W;
    s.part = a.get<double>((size_t)B * std::max((size_t)df_imstat_chunks(3L * H * W) * 2, (size_t)df_in_chunks((int)np) * DF_DIM * 2));
    s.stat = a.get<float>((size_t)B * DF_DIM * 2);
    s.flat = a.get<int>(B);
    s.prob = a.get<float>((size_t)B * np);
    df_carve_sel(a, s.sel, B, (int)np);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}
static bool df_probe_shape(int B, int H, int W) { return B >= 1 && B <= 1024 && H >= 1 && W >= 1 && (long)H * W * DF_DIM <= 0x7fffffffL / B; }
extern "C" size_t imcui_hip_darkfeat_probe_workspace_bytes(int B, int H, int W) { return df_probe_shape(B, H, W) ? df_probe_carve(nullptr, 0, B, H, W).total : 0; }

#define DF_PROBE_WS(who)                                                                                                  \
    if (!h) return IMCUI_ERR_ARG;                                                                                         \
    if (!df_probe_shape(B, H, W)) return imcui_set_err(h, IMCUI_ERR_ARG, who ": shape B=%d %dx%d", B, H, W);              \
    DfProbeWs s = df_probe_carve(ws, ws_bytes, B, H, W);                                                                  \
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, who ": workspace too small (%zu < %zu)", ws_bytes, s.total); \
    hipStream_t stream = (hipStream_t)stream_

// image statistics + layer 0: image [B, 3, H, W] -> out [B, H, W, 32] RAW (before InstanceNorm), imstat [B, 2] = mean, std (1 when flat),
// status OR-ed with bit 4 for a flat image (the caller zeroes it)
extern "C" int imcui_hip_darkfeat_stem_probe(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, float* out, float* imstat, int* status,
                                             void* ws, size_t ws_bytes, void* stream_) {
    DF_PROBE_WS("darkfeat stem probe");
    if (!packed || !image || !out || !imstat || !status) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat stem probe: null argument");
    return df_stem(h, df_layout(), packed, image, B, H, W, s.part, imstat, s.flat, status, out, stream);
}
// InstanceNorm + ReLU of x [B, H, W, C] (C = 32 / 64 / 128) -> out, stat [B, C, 2] = mean, 1 / sqrt(var + eps)
extern "C" int imcui_hip_darkfeat_inorm_probe(imcui_hip_t* h, const float* x, int B, int H, int W, int C, float* out, float* stat, void* ws, size_t ws_bytes,
                                              void* stream_) {
    DF_PROBE_WS("darkfeat inorm probe");
    if (!x || !out) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat inorm probe: null argument");
    int rc;
    IMCUI_RUN(df_inorm(h, x, out, B, H * W, C, s.part, s.stat, stream));
    copy_if(stat, s.stat, (size_t)B * C * 2 * sizeof(float), stream);
    return IMCUI_OK;
}
// the peakiness pass on x [B, H, W, C] with dilation d and the divisor *mavg (device) -> out [B, H, W]
extern "C" int imcui_hip_darkfeat_peak_probe(imcui_hip_t* h, const float* x, const float* mavg, int B, int H, int W, int C, int d, float* out, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    if (!df_probe_shape(B, H, W) || !x || !mavg || !out) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat peak probe: shape or null argument");
    return df_peak(h, x, mavg, out, B, H, W, C, d, (hipStream_t)stream_);
}
// score assembly from given level maps pk0 [B, H, W], pk1 [B, h1, w1], pk2 [B, h2, w2] and dmap [B, h2, w2, 128] -> score [B, H, W]
extern "C" int imcui_hip_darkfeat_score_probe(imcui_hip_t* h, const float* packed, const float* pk0, const float* pk1, const float* pk2, const float* dmap, int B,
                                              int H, int W, float* score, void* ws, size_t ws_bytes, void* stream_) {
    DF_PROBE_WS("darkfeat score probe");
    if (H < 2 || W < 2 || !packed || !pk0 || !pk1 || !pk2 || !dmap || !score) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat score probe: shape or null argument");
    return df_assemble(h, df_layout(), packed, pk0, pk1, pk2, dmap, B, H, W, s.prob, score, stream);
}
// detector, cut and ranked rows on a given score map [B, H, W]; det_map (optional) [B, H, W] = the score at candidates, -inf elsewhere
extern "C" int imcui_hip_darkfeat_detect_probe(imcui_hip_t* h, const float* score, int B, int H, int W, float score_thld, float edge_thld, int nms_size,
                                               int eof_mask, int kpt_n, int max_keypoints, int kout, float* keypoints, float* scores, int* num_keypoints,
                                               int* num_candidates, int* status, float* det_map, void* ws, size_t ws_bytes, void* stream_) {
    DF_PROBE_WS("darkfeat detect probe");
    const DfDet det{score_thld, edge_thld, nms_size, eof_mask, kpt_n};
    int rc;
    IMCUI_RUN(df_det_check(h, det, H * W, max_keypoints, kout));
    if (!score || !keypoints || !scores || !num_keypoints || !status) return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat detect probe: null argument");
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, status, 1);
    IMCUI_RUN(df_detect(h, s.sel, score, nullptr, B, H, W, det, max_keypoints, kout, keypoints, scores, num_keypoints, status, stream));
    copy_if(det_map, s.sel.det, (size_t)B * H * W * sizeof(float), stream);
    copy_if(num_candidates, s.sel.scan.total, (size_t)B * sizeof(int), stream);
    return IMCUI_OK;
}
// describe on a given 1/4-resolution map dmap [B, h4, w4, 128] at keypoints [B, K, 2] (x, y in image pixels), nkpts [B] -> [B, K, 128]
extern "C" int imcui_hip_darkfeat_describe_probe(imcui_hip_t* h, const float* dmap, int B, int h4, int w4, const float* keypoints, const int* nkpts, int K,
                                                 float* descriptors, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    if (!df_probe_shape(B, h4, w4) || K < 1 || !dmap || !keypoints || !nkpts || !descriptors)
        return imcui_set_err(h, IMCUI_ERR_ARG, "darkfeat describe probe: shape, K < 1 or null argument");
    df_describe(dmap, h4, w4, keypoints, nkpts, 0, K, B, descriptors, (hipStream_t)stream_);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
