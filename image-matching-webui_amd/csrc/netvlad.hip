// NetVLAD global descriptors on MI355X (retrieval_zoo entry netvlad; extractor conf `netvlad`): imcui/hloc/extractors/netvlad.py:122-146
// `_forward` -- clamp(x * 255, 0, 255) - mean, VGG-16 to conv5_3 (without its ReLU and pool, :66-68), F.normalize per pixel, NetVLADLayer
// (:27-38), the 32768 -> 4096 whitening and its normalisation -- as one batched call, and the top-k of pairs_from_retrieval.py over the
// similarity matrix.  The whole network is in the reference checkout, so this file is pinned to the reference's own output
// (tests/golden/make_netvlad_golden.py), not to a restatement.
//
//   layer 0     3 -> 64 on the VALU; clamp(x * 255, 0, 255) - mean (the three floats of the packed buffer; RGB, no flip) is applied as
//               the raw image is read, so the zero padding stays zero in normalised units
//   conv1_2 .. conv5_3   the patch-staging 3x3 convolutions (conv.hip, both arithmetic modes), ReLU on all but conv5_3 (activation 0);
//               pools behind conv1_2, 2_2, 3_3, 4_3: fused where the map is even, else the un-pooled launch and pool2x2_kernel<0> (flooring).
//               The five 512 -> 512 layers (K = 4608) are summed in two levels, 8 launches over 64 input channels each (nv_conv_grouped):
//               one chain over K = 4608 missed the float64 bar of conv5_3 in both modes
//   assign      one wave per pixel: x^ = x / max(|x|, 1e-12), the 64 scores (lane = cluster, score_proj transposed [512][64]), soft-max
//   aggregate   V[d, k] = sum_n a[n, k] (x^[n, d] - c[d, k]) AS WRITTEN in the reference (one subtraction and one fused multiply-add per
//               term), over chunks of NV_CHUNK = 256 pixels: one partial [512][64] per chunk
//   finish      one workgroup per image folds the partials in chunk order, divides every cluster's 512-vector by max(norm, 1e-12),
//               flattens d * 64 + k and divides by max(global norm, 1e-12)
//   whitening   y = W x + b with W [4096][32768] f32 streamed once: split-K skinny GEMM (nv_whiten_kernel), partial sums in the workspace,
//               nv_whiten_fold_kernel folds them in slice order, adds the bias and normalises
// fp32 FMA on the VALU in both arithmetic modes behind the trunk.  No float atomics; chunks and slices have fixed sizes and are folded
// in a fixed order; every image (row) is computed independently of the batch it rides in.  Nothing synchronises with the host.
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

#define NV_NL 13
#define NV_D 512
#define NV_K 64
#define NV_VLAD (NV_D * NV_K)
#define NV_OUT 4096
#define NV_CHUNK 256    // pixels per partial of the aggregation
#define NV_KG 64        // 512-input-channel layers (K = 4608): input channels per partial convolution ...
#define NV_NG 8         // ... and their number: K is summed in two levels, 8 chains of 576
#define NW_KC 512       // whitening: k per LDS chunk
#define NW_SLICE 2048   // whitening: k per workgroup (one partial sum)
#define NW_RMAX 16      // whitening: batch rows held per launch

// ------------------------------------------------------------------ the network and its tensor table
struct NvLayer {
    int cin, cout, pool, op;  // op = index in torchvision vgg16().features; pool: MaxPool2d(2, 2) behind it
};
static const NvLayer NV_LAYERS[NV_NL] = {{3, 64, 0, 0},     {64, 64, 1, 2},    {64, 128, 0, 5},   {128, 128, 1, 7},  {128, 256, 0, 10},
                                         {256, 256, 0, 12}, {256, 256, 1, 14}, {256, 512, 0, 17}, {512, 512, 0, 19}, {512, 512, 1, 21},
                                         {512, 512, 0, 24}, {512, 512, 0, 26}, {512, 512, 0, 28}};

static TensorTable nv_table(int whiten) {
    TensorTable t;
    for (int i = 0; i < NV_NL; ++i) {
        const std::string p = "backbone." + std::to_string(NV_LAYERS[i].op);
        t.add(p + ".weight", (size_t)NV_LAYERS[i].cout * NV_LAYERS[i].cin * 9);
        t.add(p + ".bias", (size_t)NV_LAYERS[i].cout);
    }
    t.add("netvlad.score_proj.weight", (size_t)NV_K * NV_D);
    t.add("netvlad.centers", (size_t)NV_D * NV_K);
    t.add("preprocess.mean", 3);
    if (whiten) {
        t.add("whiten.weight", (size_t)NV_OUT * NV_VLAD);
        t.add("whiten.bias", NV_OUT);
    }
    return t;
}
extern "C" int imcui_hip_netvlad_num_tensors(int whiten) { return nv_table(whiten).size(); }
extern "C" const char* imcui_hip_netvlad_tensor_name(int whiten, int i) {
    static thread_local std::string name;
    const TensorTable t = nv_table(whiten);
    if (!t.name(i)) return nullptr;
    name = t.name(i);
    return name.c_str();
}

// packed: layer 0 [tap][cin 3 (RGB)][64] + bias + mean; layers 1..12 in both layouts of conv.h + bias; score_proj transposed [512][64];
// centers [512][64]; with whitening W [4096][32768] (f32 only: it is streamed by the VALU kernel) + bias
struct NvLayout {
    size_t w0, b0, mean;
    size_t w[NV_NL], b[NV_NL], wh[NV_NL], wl[NV_NL], ws[NV_NL];
    size_t zero, score, cen, ww, wb, total;  // zero: a bias of 512 zeros (the partial convolutions behind the first)
};
static bool nv_grouped(int i) { return NV_LAYERS[i].cin == NV_D; }
static NvLayout nv_layout(int whiten) {
    NvLayout l;
    PackCursor c;
    l.w0 = c.get(27 * 64);
    l.b0 = c.get(64);
    l.mean = c.get(3);
    for (int i = 1; i < NV_NL; ++i) {
        const size_t n = (size_t)NV_LAYERS[i].cout * NV_LAYERS[i].cin * 9;
        l.w[i] = c.get(n);
        l.b[i] = c.get(NV_LAYERS[i].cout);
        l.wh[i] = c.get(n / 2);
        l.wl[i] = c.get(n / 2);
        l.ws[i] = c.get(nv_grouped(i) ? NV_NG : 1);  // (a grouped layer: NV_NG sub-layers of n / NV_NG weights each, one scale per group)
    }
    l.zero = c.get(NV_D);
    l.score = c.get((size_t)NV_D * NV_K);
    l.cen = c.get((size_t)NV_D * NV_K);
    l.ww = l.wb = 0;
    if (whiten) {
        l.ww = c.get((size_t)NV_OUT * NV_VLAD);
        l.wb = c.get(NV_OUT);
    }
    l.total = c.off;
    return l;
}
extern "C" size_t imcui_hip_netvlad_packed_floats(int whiten) { return nv_layout(whiten).total; }

extern "C" int imcui_hip_netvlad_pack_weights(int whiten, const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    const int nt = nv_table(whiten).size();
    for (int i = 0; i < nt; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const NvLayout l = nv_layout(whiten);
    memset(packed, 0, (whiten ? l.ww : l.total) * sizeof(float));  // (the whitening matrix is copied over its whole extent below)
    for (int i = 0; i < NV_NL; ++i) {
        const NvLayer& L = NV_LAYERS[i];
        const float *w = t[2 * i], *b = t[2 * i + 1];
        if (i == 0) {
            for (int co = 0; co < 64; ++co)
                for (int ci = 0; ci < 3; ++ci)
                    for (int k = 0; k < 9; ++k) packed[l.w0 + ((size_t)k * 3 + ci) * 64 + co] = w[((size_t)co * 3 + ci) * 9 + k];
            memcpy(packed + l.b0, b, 64 * sizeof(float));
        } else if (nv_grouped(i)) {  // input channels [NV_KG g, NV_KG (g + 1)) as a layer of its own
            const size_t ng = (size_t)L.cout * NV_KG * 9;
            std::vector<float> wg(ng);
            for (int g = 0; g < NV_NG; ++g) {
                for (int co = 0; co < L.cout; ++co)
                    memcpy(wg.data() + (size_t)co * NV_KG * 9, w + ((size_t)co * L.cin + (size_t)g * NV_KG) * 9, (size_t)NV_KG * 9 * sizeof(float));
                pack_conv3x3(wg.data(), L.cout, NV_KG, packed + l.w[i] + g * ng);
                packed[l.ws[i] + g] = pack_conv3x3_split(wg.data(), L.cout, NV_KG, reinterpret_cast<unsigned short*>(packed + l.wh[i] + g * (ng / 2)),
                                                         reinterpret_cast<unsigned short*>(packed + l.wl[i] + g * (ng / 2)));
            }
            memcpy(packed + l.b[i], b, L.cout * sizeof(float));
        } else {
            pack_conv3x3(w, L.cout, L.cin, packed + l.w[i]);
            memcpy(packed + l.b[i], b, L.cout * sizeof(float));
            packed[l.ws[i]] = pack_conv3x3_split(w, L.cout, L.cin, reinterpret_cast<unsigned short*>(packed + l.wh[i]),
                                                 reinterpret_cast<unsigned short*>(packed + l.wl[i]));
        }
    }
    const float *sw = t[2 * NV_NL], *cw = t[2 * NV_NL + 1], *mean = t[2 * NV_NL + 2];
    for (int k = 0; k < NV_K; ++k)
        for (int d = 0; d < NV_D; ++d) packed[l.score + (size_t)d * NV_K + k] = sw[(size_t)k * NV_D + d];
    memcpy(packed + l.cen, cw, (size_t)NV_D * NV_K * sizeof(float));
    memcpy(packed + l.mean, mean, 3 * sizeof(float));
    if (whiten) {
        memcpy(packed + l.ww, t[2 * NV_NL + 3], (size_t)NV_OUT * NV_VLAD * sizeof(float));
        memset(packed + l.wb, 0, align_up(NV_OUT, 64) * sizeof(float));
        memcpy(packed + l.wb, t[2 * NV_NL + 4], NV_OUT * sizeof(float));
    }
    return IMCUI_OK;
}

namespace {

// what layer 0 reads (netvlad.py:126-129): clamp(x * 255, 0, 255) - mean, one rounding each; mean = the three packed channel means
struct NvStemLoad {
    const float* mean;
    __device__ float operator()(const float* __restrict__ img, long b, int c, int h, int w, int yy, int xx) const {
        return fminf(fmaxf(img[((b * 3 + c) * h + yy) * (long)w + xx] * 255.0f, 0.0f), 255.0f) - mean[c];
    }
};

// dst [P, NV_KG] = channels [c0, c0 + NV_KG) of src [P, 512]; n4 = float4s of dst
__global__ __launch_bounds__(256) void nv_slice_kernel(const float* __restrict__ src, float* __restrict__ dst, int c0, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const long p = i / (NV_KG / 4);
        const int q = (int)(i - p * (NV_KG / 4));
        reinterpret_cast<float4*>(dst)[i] = *reinterpret_cast<const float4*>(src + p * NV_D + c0 + q * 4);
    }
}
// acc += part (relu: then max(., 0)); n4 float4s
__global__ __launch_bounds__(256) void nv_accum_kernel(float* __restrict__ acc, const float* __restrict__ part, int relu, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 a = reinterpret_cast<float4*>(acc)[i];
        const float4 p = reinterpret_cast<const float4*>(part)[i];
        a = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
        if (relu) a = make_float4(fmaxf(a.x, 0.0f), fmaxf(a.y, 0.0f), fmaxf(a.z, 0.0f), fmaxf(a.w, 0.0f));
        reinterpret_cast<float4*>(acc)[i] = a;
    }
}

// netvlad.py:138 F.normalize(descriptors, dim=1) and :29-30 score_proj + soft-max.  One wave = 4 pixels of x [P, 512] (P = B N pixels, a
// pixel's result does not depend on its neighbours): lane l holds channels l, l + 64, ..; x^ -> xn [P, 512] and LDS; lane k then owns
// cluster k: score = sum_d sT[d][k] x^[d] in ascending d, soft-max over the wave -> asg [P, 64]
__global__ __launch_bounds__(256) void nv_assign_kernel(const float* __restrict__ x, const float* __restrict__ sT, float* __restrict__ xn,
                                                        float* __restrict__ asg, long P) {
    __shared__ float xs[4][4][NV_D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long p0 = ((long)blockIdx.x * 4 + wv) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = p0 + j;
        float v[8];
        float ss = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = p < P ? x[p * NV_D + i * 64 + lane] : 0.0f;
            ss = fmaf(v[i], v[i], ss);
        }
        const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float u = v[i] / nrm;
            xs[wv][j][i * 64 + lane] = u;
            if (p < P) xn[p * NV_D + i * 64 + lane] = u;
        }
    }
    __syncthreads();
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int d = 0; d < NV_D; ++d) {
        const float w = sT[d * NV_K + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = fmaf(xs[wv][j][d], w, s[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float m = wave_max(s[j]);
        const float e = expf(s[j] - m);
        const float a = e / wave_sum(e);
        if (p0 + j < P) asg[(p0 + j) * NV_K + lane] = a;
    }
}

// netvlad.py:31-32 over one chunk of NV_CHUNK pixels of image b: lane = cluster k, wave w of workgroup (chunk, dt, b) owns the 16 rows
// d = 64 dt + 16 w ..: acc[d] = sum_n a[n, k] (x^[n, d] - c[d, k]) in ascending n -> part [B, nchunk, 512, 64]
__global__ __launch_bounds__(256) void nv_aggregate_kernel(const float* __restrict__ xn, const float* __restrict__ asg, const float* __restrict__ cen, int N,
                                                           int nchunk, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int chunk = blockIdx.x, b = blockIdx.z, d0 = blockIdx.y * 64 + wv * 16;
    const float* xb = xn + (long)b * N * NV_D + d0;
    const float* ab = asg + (long)b * N * NV_K + lane;
    float c[16], acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        c[j] = cen[(d0 + j) * NV_K + lane];
        acc[j] = 0.0f;
    }
    const int n1 = min((chunk + 1) * NV_CHUNK, N);
    for (int n = chunk * NV_CHUNK; n < n1; ++n) {
        const float a = ab[(long)n * NV_K];
        const float4* xr = reinterpret_cast<const float4*>(xb + (long)n * NV_D);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = xr[q];
            acc[4 * q] = fmaf(a, v.x - c[4 * q], acc[4 * q]);
            acc[4 * q + 1] = fmaf(a, v.y - c[4 * q + 1], acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(a, v.z - c[4 * q + 2], acc[4 * q + 2]);
            acc[4 * q + 3] = fmaf(a, v.w - c[4 * q + 3], acc[4 * q + 3]);
        }
    }
    float* pb = part + (((long)b * nchunk + chunk) * NV_D + d0) * NV_K + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) pb[j * NV_K] = acc[j];
}

// netvlad.py:33-37: one workgroup per image, thread (k = tid & 63, g = tid >> 6) owns d = 32 g .. 32 g + 31 of cluster k.  The partials
// are folded in chunk order; intranorm, the flattening d * 64 + k and the global norm follow.  All sums in one fixed order.
__global__ __launch_bounds__(1024) void nv_finish_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ out) {
    __shared__ float red[16][NV_K];
    __shared__ float wsum[16];
    const int b = blockIdx.x, k = threadIdx.x & 63, g = threadIdx.x >> 6;
    const float* pb = part + (long)b * nchunk * NV_VLAD;
    float v[32];
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        float s = 0.0f;
        for (int c = 0; c < nchunk; ++c) s += pb[(long)c * NV_VLAD + (g * 32 + i) * NV_K + k];
        v[i] = s;
        ss = fmaf(s, s, ss);
    }
    red[g][k] = ss;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) tot += red[j][k];
    const float nk = fmaxf(sqrtf(tot), 1e-12f);
    float gs = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        v[i] = v[i] / nk;
        gs = fmaf(v[i], v[i], gs);
    }
    gs = wave_sum(gs);
    if (k == 0) wsum[g] = gs;
    __syncthreads();
    float gt = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) gt += wsum[j];
    const float gn = fmaxf(sqrtf(gt), 1e-12f);
    float* ob = out + (long)b * NV_VLAD;
#pragma unroll
    for (int i = 0; i < 32; ++i) ob[(g * 32 + i) * NV_K + k] = v[i] / gn;
}

// The whitening's matrix product, split over K.  Workgroup (slice, tile): k in [NW_SLICE slice, ..) in LDS chunks of NW_KC, output rows
// o = 4 O tile + O wave + (0 .. O - 1) (O = 8, or 4 with 16 batch rows: O x R accumulators per lane).  Rows r0 .. r0 + R - 1 of x [Btot, in_dim] are staged per chunk in LDS (zeros past Btot / in_dim);
// every weight element is loaded once (16-byte loads, lane l takes k = 4 l and 4 (l + 64) of the chunk) and applied to the R rows.  A
// row's sum is one chain per lane in ascending k, then the wave butterfly: it does not depend on R, on the other rows or on Btot.
// part [nslice, Btot, out_dim].  in_dim % 4 == 0.
__device__ __forceinline__ float4 nv_load4_if(bool ok, const float* p) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ok) v = *reinterpret_cast<const float4*>(p);
    return v;
}
template <int R, int O>
__global__ __launch_bounds__(256) void nv_whiten_kernel(const float* __restrict__ W, const float* __restrict__ x, int r0, int Btot, int in_dim, int out_dim,
                                                        float* __restrict__ part) {
    __shared__ float4 xs[R * (NW_KC / 4)];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int slice = blockIdx.x, obase = (blockIdx.y * 4 + wv) * O;
    const int kbeg = slice * NW_SLICE, kend = min(kbeg + NW_SLICE, in_dim);
    float acc[O][R];
#pragma unroll
    for (int o = 0; o < O; ++o)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[o][r] = 0.0f;
#pragma unroll 1
    for (int kc = kbeg; kc < kend; kc += NW_KC) {
        __syncthreads();
        for (int i = threadIdx.x; i < R * (NW_KC / 4); i += 256) {
            const int r = i / (NW_KC / 4), k = kc + (i % (NW_KC / 4)) * 4;
            xs[i] = nv_load4_if(r0 + r < Btot && k < kend, x + (long)(r0 + r) * in_dim + k);
        }
        __syncthreads();
#pragma unroll
        for (int og = 0; og < O / 4; ++og)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int q = half * 64 + lane, k = kc + q * 4;
                float4 w[4];
#pragma unroll
                for (int oo = 0; oo < 4; ++oo) {
                    const int o = obase + og * 4 + oo;
                    w[oo] = nv_load4_if(o < out_dim && k < kend, W + (long)o * in_dim + k);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 xv = xs[r * (NW_KC / 4) + q];
#pragma unroll
                    for (int oo = 0; oo < 4; ++oo) {
                        float a = acc[og * 4 + oo][r];
                        a = fmaf(w[oo].x, xv.x, a);
                        a = fmaf(w[oo].y, xv.y, a);
                        a = fmaf(w[oo].z, xv.z, a);
                        a = fmaf(w[oo].w, xv.w, a);
                        acc[og * 4 + oo][r] = a;
                    }
                }
            }
    }
#pragma unroll
    for (int o = 0; o < O; ++o)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s = wave_sum(acc[o][r]);
            if (lane == r && r0 + r < Btot && obase + o < out_dim) part[((long)slice * Btot + r0 + r) * out_dim + obase + o] = s;
        }
}

// y[b] = bias + the partial sums in slice order (netvlad.py:143), then F.normalize (:144).  One workgroup of 1024 threads per row (the
// slice loop is unrolled by 8 so that a thread's loads are in flight together: with 256 threads and a rolled loop the fold took 86 us).
__global__ __launch_bounds__(1024) void nv_whiten_fold_kernel(const float* __restrict__ part, const float* __restrict__ bias, int nslice, int B, int out_dim,
                                                              float* __restrict__ out) {
    __shared__ float s16[16];
    const int b = blockIdx.x;
    float* ob = out + (long)b * out_dim;
    float ss = 0.0f;
    for (int o = threadIdx.x; o < out_dim; o += 1024) {
        float s = 0.0f;
#pragma unroll 8
        for (int sl = 0; sl < nslice; ++sl) s += part[((long)sl * B + b) * out_dim + o];
        s += bias[o];
        ob[o] = s;
        ss = fmaf(s, s, ss);
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) s16[threadIdx.x >> 6] = ss;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) tot += s16[j];
    const float nrm = fmaxf(sqrtf(tot), 1e-12f);
    for (int o = threadIdx.x; o < out_dim; o += 1024) ob[o] = ob[o] / nrm;  // (a thread's own elements)
}

// pairs_from_retrieval.py:112-117: sim[q, j] = <Q[q], Db[j]> in float32 (one wave per entry, lanes stride over D in ascending order, then
// the butterfly), -inf where `invalid` or below min_score
__global__ __launch_bounds__(256) void nv_sim_kernel(const float* __restrict__ qd, const float* __restrict__ db, int Q, int N, int D,
                                                     const unsigned char* __restrict__ invalid, int has_min, float min_score, float* __restrict__ sim) {
    const int lane = threadIdx.x & 63;
    const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= (long)Q * N) return;  // (wave-uniform)
    const int q = (int)(e / N), j = (int)(e - (long)q * N);
    const float *a = qd + (long)q * D, *b = db + (long)j * D;
    float s = 0.0f;
    for (int d = lane; d < D; d += 64) s = fmaf(a[d], b[d], s);
    s = wave_sum(s);
    if ((invalid && invalid[e]) || (has_min && s < min_score)) s = -INFINITY;
    if (lane == 0) sim[e] = s;
}
// the `num_select` highest of a row in descending score, equal scores by ascending index: entry j goes to its rank.  Slots past N hold
// index -1 and -inf.
__global__ __launch_bounds__(256) void nv_topk_kernel(const float* __restrict__ sim, int N, int num_select, int* __restrict__ idx, float* __restrict__ score) {
    const int q = blockIdx.x;
    const float* s = sim + (long)q * N;
    for (int j = threadIdx.x; j < N; j += 256) {
        const float v = s[j];
        int rank = 0;
        for (int i = 0; i < N; ++i) {
            const float o = s[i];
            rank += (o > v || (o == v && i < j)) ? 1 : 0;
        }
        if (rank < num_select) {
            idx[(long)q * num_select + rank] = j;
            score[(long)q * num_select + rank] = v;
        }
    }
    for (int t = N + threadIdx.x; t < num_select; t += 256) {
        idx[(long)q * num_select + t] = -1;
        score[(long)q * num_select + t] = -INFINITY;
    }
}

}  // namespace

// ------------------------------------------------------------------ launch helpers
// layer 0 on the raw planar image [B, 3, H, W] -> out [B, H, W, 64]
static void nv_stem(const NvLayout& l, const float* P, const float* img, int B, int H, int W, float* out, hipStream_t stream) {
    const long npix = (long)B * H * W;
    hipLaunchKernelGGL((stem3x3_kernel<64, NvStemLoad>), dim3(blocks_256(npix)), dim3(256), 0, stream, img, P + l.w0, P + l.b0, out, H, W, NvStemLoad{P + l.mean},
                       npix);
}
// the flooring 2x2 max-pool, [B, hi, wi, C] -> [B, hi / 2, wi / 2, C]
static void nv_pool(const float* src, float* dst, int B, int hi, int wi, int C, hipStream_t stream) {
    const long n4 = (long)B * (hi / 2) * (wi / 2) * (C / 4);
    hipLaunchKernelGGL(pool2x2_kernel<0>, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, src, dst, hi, wi, hi / 2, wi / 2, C, n4);
}

// A 512 -> 512 layer (K = 4608) as NV_NG partial convolutions over NV_KG input channels each, summed in group order: the patch-staging
// kernels sum K in one chain per output, and at K = 4608 that chain alone is 5 .. 8 x the float32 error of a blocked sum (conv5_3 on a
// 3 x 4 map against float64: one launch 1.07e-06 split / 1.80e-06 exact, 16 groups of 32 3.1e-07 / 2.8e-07, 8 groups of 64 3.6e-07 /
// 3.8e-07 at two thirds of the extra time; bar 6.8e-07, tests/test_gpu_netvlad_layers.py).  in, out
// [B, hh, ww, 512] (un-pooled); scratch: nv_grouped_scratch(B hh ww) floats.  Split mode: the kernel reads its channel group in place
// (cin_stride 512) and adds the running sum as its residual map, out and scratch alternating; exact mode: slice, convolve, accumulate.
static size_t nv_grouped_scratch(size_t pix) { return align_up(pix * NV_D, 64) + align_up(pix * NV_KG, 64); }
static int nv_conv_grouped(imcui_hip_t* h, const float* P, const NvLayout& l, int i, const float* in, int B, int hh, int ww, int act, float* out, float* scratch,
                           hipStream_t stream) {
    const NvLayer& L = NV_LAYERS[i];
    const size_t pix = (size_t)B * hh * ww, ng = (size_t)L.cout * NV_KG * 9;
    float *other = scratch, *tmp = scratch + align_up(pix * NV_D, 64);
    int rc;
    for (int g = 0; g < NV_NG; ++g) {
        const float* bias = P + (g == 0 ? l.b[i] : l.zero);
        const int last = g == NV_NG - 1;
        if (h->precision == 1) {
            float* dst = (g & 1) ? out : other;  // NV_NG is even: the last group writes `out`
            const float* prev = g == 0 ? nullptr : ((g & 1) ? other : out);
            IMCUI_RUN(conv3x3_split_launch(h, in + (size_t)g * NV_KG, reinterpret_cast<const unsigned short*>(P + l.wh[i] + g * (ng / 2)),
                                           reinterpret_cast<const unsigned short*>(P + l.wl[i] + g * (ng / 2)), P + l.ws[i] + g, bias, dst, B, hh, ww, NV_KG, L.cout,
                                           last ? act : 0, 0, stream, prev, NV_D));
        } else {
            const long s4 = (long)pix * (NV_KG / 4), o4 = (long)pix * (NV_D / 4);
            hipLaunchKernelGGL(nv_slice_kernel, dim3(grid_stride_blocks(s4)), dim3(256), 0, stream, in, tmp, g * NV_KG, s4);
            IMCUI_CHECK_LAUNCH(h);
            IMCUI_RUN(conv3x3_launch(h, tmp, P + l.w[i] + g * ng, bias, g == 0 ? out : other, B, hh, ww, NV_KG, L.cout, 0, 0, stream));
            if (g > 0) {
                hipLaunchKernelGGL(nv_accum_kernel, dim3(grid_stride_blocks(o4)), dim3(256), 0, stream, out, other, last ? act : 0, o4);
                IMCUI_CHECK_LAUNCH(h);
            }
        }
    }
    return IMCUI_OK;
}
static int nv_whiten_nslice(int in_dim) { return cdiv(in_dim, NW_SLICE); }
static size_t nv_whiten_part_floats(int B, int in_dim, int out_dim) { return (size_t)nv_whiten_nslice(in_dim) * B * out_dim; }

// out [B, out_dim] = normalize(W x + bias); part: nv_whiten_part_floats(B, ..) floats
static int nv_whiten_launch(imcui_hip_t* h, const float* W, const float* bias, const float* x, int B, int in_dim, int out_dim, float* part, float* out,
                            hipStream_t stream) {
        for (int r0 = 0; r0 < B; r0 += NW_RMAX) {
        const int rows = std::min(B - r0, NW_RMAX);
        const dim3 grid(nv_whiten_nslice(in_dim), cdiv(out_dim, rows <= 8 ? 32 : 16));
        if (rows <= 4)
            hipLaunchKernelGGL((nv_whiten_kernel<4, 8>), grid, dim3(256), 0, stream, W, x, r0, B, in_dim, out_dim, part);
        else if (rows <= 8)
            hipLaunchKernelGGL((nv_whiten_kernel<8, 8>), grid, dim3(256), 0, stream, W, x, r0, B, in_dim, out_dim, part);
        else
            hipLaunchKernelGGL((nv_whiten_kernel<16, 4>), grid, dim3(256), 0, stream, W, x, r0, B, in_dim, out_dim, part);
        IMCUI_CHECK_LAUNCH(h);
    }
    hipLaunchKernelGGL(nv_whiten_fold_kernel, dim3(B), dim3(1024), 0, stream, part, bias, nv_whiten_nslice(in_dim), B, out_dim, out);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// the NetVLAD layer on maps feat [B, N, 512] -> out [B, 32768]
static int nv_vlad_launch(imcui_hip_t* h, const float* P, const NvLayout& l, const float* feat, int B, int N, float* xn, float* asg, float* part, float* out,
                          hipStream_t stream) {
    const long pix = (long)B * N;
    const int nchunk = cdiv(N, NV_CHUNK);
    hipLaunchKernelGGL(nv_assign_kernel, dim3((unsigned)((pix + 15) / 16)), dim3(256), 0, stream, feat, P + l.score, xn, asg, pix);
    IMCUI_CHECK_LAUNCH(h);
    hipLaunchKernelGGL(nv_aggregate_kernel, dim3(nchunk, NV_D / 64, B), dim3(256), 0, stream, xn, asg, P + l.cen, N, nchunk, part);
    IMCUI_CHECK_LAUNCH(h);
    hipLaunchKernelGGL(nv_finish_kernel, dim3(B), dim3(1024), 0, stream, part, nchunk, out);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ workspace
struct NvWs {
    float *fa, *fb, *xn, *asg, *part, *vlad, *wpart;
    size_t total;
    bool ok;
};
// imgpix: pixels of the image (0: no trunk, the probe); N: pixels of the conv5_3 map
static NvWs nv_carve(void* ws, size_t bytes, int B, size_t imgpix, size_t N, int whiten) {
    WsAlloc a(ws, bytes);
    NvWs s;
    s.fa = a.get<float>((size_t)B * imgpix * 64);
    s.fb = a.get<float>((size_t)B * imgpix * 64);
    s.xn = a.get<float>((size_t)B * N * NV_D);
    s.asg = a.get<float>((size_t)B * N * NV_K);
    s.part = a.get<float>((size_t)B * ((N + NV_CHUNK - 1) / NV_CHUNK) * NV_VLAD);
    s.vlad = a.get<float>(whiten ? (size_t)B * NV_VLAD : 0);
    s.wpart = a.get<float>(whiten ? nv_whiten_part_floats(B, NV_VLAD, NV_OUT) : 0);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}
static void nv_map_size(int H, int W, int* fh, int* fw) {
    *fh = H / 2 / 2 / 2 / 2;
    *fw = W / 2 / 2 / 2 / 2;
}
extern "C" size_t imcui_hip_netvlad_workspace_bytes(int B, int H, int W, int whiten) {
    if (B <= 0 || H < 16 || W < 16) return 0;
    int fh, fw;
    nv_map_size(H, W, &fh, &fw);
    return nv_carve(nullptr, 0, B, (size_t)H * W, (size_t)fh * fw, whiten).total;
}

extern "C" int imcui_hip_netvlad_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, int whiten,
                                         float* descriptor, float* dbg_feat, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (C != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad: the image has %d channels, 3 (RGB) are needed", C);
    if (H < 16 || W < 16)
        return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad: a %dx%d image has an empty conv5_3 map: every side needs at least 16 pixels", H, W);
    if (B > 1024 || (long)B * H * W > 0x7fffffffL / 64)
        return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad: B=%d images of %dx%d exceed the 2^31 index range of one call", B, H, W);
    if (!packed || !image || !descriptor) return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad: null argument");
    int fh, fw;
    nv_map_size(H, W, &fh, &fw);
    const int N = fh * fw;
    const NvLayout l = nv_layout(whiten);
    const NvWs s = nv_carve(ws, ws_bytes, B, (size_t)H * W, (size_t)N, whiten);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "netvlad: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const bool split = h->precision == 1;
    const float* P = packed;
    int rc;
    nv_stem(l, P, image, B, H, W, s.fa, stream);
    IMCUI_CHECK_LAUNCH(h);
    float *cur = s.fa, *oth = s.fb;
    int hh = H, ww = W;
    for (int i = 1; i < NV_NL; ++i) {
        const NvLayer& L = NV_LAYERS[i];
        const int fused = (L.pool && !nv_grouped(i) && !((hh | ww) & 1)) ? 1 : 0, act = i == NV_NL - 1 ? 0 : 1;
        if (nv_grouped(i))  // (the scratch lies behind the layer's output in the same buffer: 8.25 B H W floats at most of its 64 B H W)
            IMCUI_RUN(nv_conv_grouped(h, P, l, i, cur, B, hh, ww, act, oth, oth + align_up((size_t)B * hh * ww * NV_D, 64), stream));
        else if (split)
            IMCUI_RUN(conv3x3_split_launch(h, cur, reinterpret_cast<const unsigned short*>(P + l.wh[i]), reinterpret_cast<const unsigned short*>(P + l.wl[i]),
                                           P + l.ws[i], P + l.b[i], oth, B, hh, ww, L.cin, L.cout, act, fused, stream));
        else
            IMCUI_RUN(conv3x3_launch(h, cur, P + l.w[i], P + l.b[i], oth, B, hh, ww, L.cin, L.cout, act, fused, stream));
        std::swap(cur, oth);
        if (L.pool) {
            const int ho = hh / 2, wo = ww / 2;
            if (!fused) {  // an odd map: nn.MaxPool2d floors (also behind conv4_3, which is summed in groups and has no fused pool)
                nv_pool(cur, oth, B, hh, ww, L.cout, stream);
                IMCUI_CHECK_LAUNCH(h);
                std::swap(cur, oth);
            }
            hh = ho;
            ww = wo;
        }
    }
    if (dbg_feat) hipMemcpyAsync(dbg_feat, cur, (size_t)B * N * NV_D * sizeof(float), hipMemcpyDeviceToDevice, stream);
    IMCUI_RUN(nv_vlad_launch(h, P, l, cur, B, N, s.xn, s.asg, s.part, whiten ? s.vlad : descriptor, stream));
    if (whiten) IMCUI_RUN(nv_whiten_launch(h, P + l.ww, P + l.wb, s.vlad, B, NV_VLAD, NV_OUT, s.wpart, descriptor, stream));
    return IMCUI_OK;
}

// ------------------------------------------------------------------ test entries
extern "C" size_t imcui_hip_netvlad_probe_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return std::max(nv_carve(nullptr, 0, B, 0, (size_t)N, 0).total, align_up(nv_grouped_scratch((size_t)B * N) * sizeof(float), 256));
}

// test entry: one stage alone.  op 0: layer 0 with the wrapper's normalisation, in = image [B, 3, H, W] RGB in [0, 1] -> out [B, H, W, 64];
// op 1: the flooring 2x2 max-pool, in [B, H, W, C] -> out [B, H / 2, W / 2, C]; op 2: the NetVLAD layer (pre-normalisation included) on
// maps in [B, H, W, 512] -> out [B, 32768] (needs the workspace of imcui_hip_netvlad_probe_workspace_bytes(B, H W))
extern "C" int imcui_hip_netvlad_layer_probe(imcui_hip_t* h, int op, const float* packed, const float* in, int B, int H, int W, int C, float* out, void* ws,
                                             size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B < 1 || B > 1024 || H < 1 || W < 1 || !in || !out || (long)B * H * W > 0x7fffffffL / 512) return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad layer probe: shape");
    const NvLayout l = nv_layout(0);
    if (op == 0) {
        if (!packed) return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad layer probe: layer 0 needs the packed weights");
        nv_stem(l, packed, in, B, H, W, out, stream);
    } else if (op == 1) {
        if (C < 4 || C % 4 || C > 512 || H < 2 || W < 2) return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad layer probe: C=%d (a multiple of 4 up to 512), %dx%d", C, H, W);
        nv_pool(in, out, B, H, W, C, stream);
    } else if (op == 2) {
        if (!packed || C != NV_D) return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad layer probe: the NetVLAD layer needs the packed weights and C=512, got %d", C);
        const NvWs s = nv_carve(ws, ws_bytes, B, 0, (size_t)H * W, 0);
        if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "netvlad layer probe: workspace too small (%zu < %zu)", ws_bytes, s.total);
        return nv_vlad_launch(h, packed, l, in, B, H * W, s.xn, s.asg, s.part, out, stream);
    } else if (op == 3) {  // conv5_3 (no ReLU) as the forward launches it, in the handle's arithmetic mode: in, out [B, H, W, 512]
        const size_t need = align_up(nv_grouped_scratch((size_t)B * H * W) * sizeof(float), 256);
        if (!packed || C != NV_D) return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad layer probe: conv5_3 needs the packed weights and C=512, got %d", C);
        if (!ws || ws_bytes < need) return imcui_set_err(h, IMCUI_ERR_WS, "netvlad layer probe: workspace too small (%zu < %zu)", ws_bytes, need);
        return nv_conv_grouped(h, packed, l, NV_NL - 1, in, B, H, W, 0, out, (float*)ws, stream);
    } else {
        return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad layer probe: op %d", op);
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_netvlad_whiten_workspace_bytes(int B, int in_dim, int out_dim) {
    if (B <= 0 || in_dim <= 0 || out_dim <= 0) return 0;
    return align_up(nv_whiten_part_floats(B, in_dim, out_dim) * sizeof(float), 256);
}
// test entry: out [B, out_dim] = normalize(weight [out_dim, in_dim] x + bias) for x [B, in_dim], any B >= 1, in_dim a multiple of 4
extern "C" int imcui_hip_netvlad_whiten_probe(imcui_hip_t* h, const float* weight, const float* bias, const float* x, int B, int in_dim, int out_dim, float* out,
                                              void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B < 1 || B > 65535 || in_dim < 4 || in_dim % 4 || out_dim < 1 || !weight || !bias || !x || !out || (long)B * out_dim > 0x7fffffffL / 64 ||
        (long)out_dim * in_dim > (1L << 40))
        return imcui_set_err(h, IMCUI_ERR_ARG, "netvlad whitening probe: B=%d, in_dim=%d (a multiple of 4), out_dim=%d", B, in_dim, out_dim);
    const size_t need = imcui_hip_netvlad_whiten_workspace_bytes(B, in_dim, out_dim);
    if (!ws || ws_bytes < need) return imcui_set_err(h, IMCUI_ERR_WS, "netvlad whitening probe: workspace too small (%zu < %zu)", ws_bytes, need);
    return nv_whiten_launch(h, weight, bias, x, B, in_dim, out_dim, (float*)ws, out, stream);
}

// ------------------------------------------------------------------ retrieval
extern "C" size_t imcui_hip_retrieval_topk_workspace_bytes(int Q, int N) {
    if (Q <= 0 || N <= 0) return 0;
    return align_up((size_t)Q * N * sizeof(float), 256);
}
extern "C" int imcui_hip_retrieval_topk(imcui_hip_t* h, const float* query, const float* db, int Q, int N, int D, const unsigned char* invalid, int has_min_score,
                                        float min_score, int num_select, int* indices, float* scores, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (Q <= 0) return IMCUI_OK;
    if (N < 1 || D < 1 || num_select < 1 || !query || !db || !indices || !scores || (long)Q * N > 0x7fffffffL / 4 || (long)Q * num_select > 0x7fffffffL / 4 ||
        Q > 0x7fffffff / 4)
        return imcui_set_err(h, IMCUI_ERR_ARG, "retrieval top-k: Q=%d queries, N=%d database rows, D=%d, num_select=%d", Q, N, D, num_select);
    const size_t need = imcui_hip_retrieval_topk_workspace_bytes(Q, N);
    if (!ws || ws_bytes < need) return imcui_set_err(h, IMCUI_ERR_WS, "retrieval top-k: workspace too small (%zu < %zu)", ws_bytes, need);
    float* sim = (float*)ws;
    const long e = (long)Q * N;
    hipLaunchKernelGGL(nv_sim_kernel, dim3((unsigned)((e + 3) / 4)), dim3(256), 0, stream, query, db, Q, N, D, invalid, has_min_score, min_score, sim);
    hipLaunchKernelGGL(nv_topk_kernel, dim3(Q), dim3(256), 0, stream, sim, N, num_select, indices, scores);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
