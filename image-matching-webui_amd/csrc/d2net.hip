// D2-Net / RoRD forward on MI355X (zoo entries d2net and rord; extractor confs d2net-ss, d2net-ms, rord): the extraction of
// imcui/hloc/extractors/d2net.py:37-60 (rord.py is the same file) -- mihaidusmanu/d2-net lib/model_test.py (VGG-16 cut at conv4_3,
// HardDetectionModule, HandcraftedLocalizationModule) under lib/pyramid.py process_multiscale -- as one batched call.
//
// Per level, in list order (the level list comes from the binding, which evaluates floor(H * s) in float64):
//   image       the level that IS the image is read in place; every other level is ATen's bilinear resize (align_corners=True) of the
//               normalised image, planar.  The wrapper's flip to BGR and `x * 255 - mean` are applied where the image is READ (two
//               float32 roundings), so the zero padding of layer 0 stays zero in normalised units
//   layer 0     3 -> 64 on the VALU, NHWC out
//   conv1_2 .. conv3_3   the patch-staging 3x3 convolutions (conv.hip, both arithmetic modes) with the fused 2x2 max-pool where the
//               map is even; an odd map takes the un-pooled launch and pool2x2_kernel<0> (flooring, as nn.MaxPool2d)
//   avg-pool    2x2, stride 1: (h, w) -> (h - 1, w - 1)
//   conv4_1 .. conv4_3   dilation 2 on the implicit GEMM (gemm.hip, GemmP.conv_dil = 2; K = 2304 / 4608 summed in two levels there),
//               ReLU in the epilogue (conv4_3: use_relu)
//   sum         f += bilinear(f of the previous level) in a pass of its own (d2_addup_kernel): the sum follows conv4_3's ReLU, and the
//               GEMM epilogue adds its residual BEFORE the activation
//   detector    one wave per pixel: the 512 channels once, their maximum, and for the channel(s) equal to it the 8 neighbours in that
//               channel only: 3x3 maximum, Hessian edge test, localization step, |step| < 0.5, the four bilinear corners inside the
//               map; the previous level's banned mask (nearest) is applied and this level's is written.  Kept (channel, pixel)
//               pairs leave as bit planes; select.h's count / scan / compact walks them channel-major, upstream's nonzero order
// After the last level: radix select of the max_keypoints-th largest (score, candidate index) key, output in ascending (score, index)
// order -- a stable argsort of upstream's concatenation --, one wave per key-point redoes the step, gathers the four corners of the
// level's map (kept in the workspace) and normalises.  No float atomics, explicit float32 order in the detector (no fused
// multiply-add: the __f*_rn helpers are plain operators, so build.py compiles this file with -ffp-contract=off; IEEE division),
// grids sized by shapes or capacities: batch-independent, bitwise reproducible, no host synchronisation.
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

#define D2_NL 10      // convolutions
#define D2_MAXLEV 8   // levels per call
#define D2_DIM 512

// ------------------------------------------------------------------ the network and its tensor table
struct D2Layer {
    int cin, cout, dil, pool, op;  // op = index in DenseFeatureExtractionModule.model (nn.Sequential); pool: MaxPool2d(2, 2) behind it
};
static const D2Layer D2_LAYERS[D2_NL] = {{3, 64, 1, 0, 0},    {64, 64, 1, 1, 2},    {64, 128, 1, 0, 5},   {128, 128, 1, 1, 7},  {128, 256, 1, 0, 10},
                                         {256, 256, 1, 0, 12}, {256, 256, 1, 0, 14}, {256, 512, 2, 0, 17}, {512, 512, 2, 0, 19}, {512, 512, 2, 0, 21}};

static const TensorTable& d2_tensors() {
    static TensorTable t;
    static bool done = [] {
        for (int i = 0; i < D2_NL; ++i) {
            const std::string p = "dense_feature_extraction.model." + std::to_string(D2_LAYERS[i].op);
            t.add(p + ".weight", (size_t)D2_LAYERS[i].cout * D2_LAYERS[i].cin * 9);
            t.add(p + ".bias", (size_t)D2_LAYERS[i].cout);
        }
        return true;
    }();
    (void)done;
    return t;
}
extern "C" int imcui_hip_d2net_num_tensors(void) { return d2_tensors().size(); }
extern "C" const char* imcui_hip_d2net_tensor_name(int i) { return d2_tensors().name(i); }

// packed: layer 0 [tap][cin 3 (BGR)][64] + bias; layers 1..6 in both layouts of conv.h (f32: pack_conv3x3, split: f16 hi / lo planes
// and their scale) + bias; layers 7..9 as GEMM layers [cout][tap][cin]
struct D2Layout {
    size_t w0, b0;
    size_t w[D2_NL], b[D2_NL], wh[D2_NL], wl[D2_NL], ws[D2_NL];  // layers 1..6
    GemmLayerOff g[D2_NL];                                        // layers 7..9
    size_t total;
};
static D2Layout d2_layout() {
    D2Layout l;
    PackCursor c;
    l.w0 = c.get(27 * 64);
    l.b0 = c.get(64);
    for (int i = 1; i < D2_NL; ++i) {
        const D2Layer& L = D2_LAYERS[i];
        const size_t n = (size_t)L.cout * L.cin * 9;
        if (L.dil == 1) {
            l.w[i] = c.get(n);
            l.b[i] = c.get(L.cout);
            l.wh[i] = c.get(n / 2);
            l.wl[i] = c.get(n / 2);
            l.ws[i] = c.get(1);
        } else {
            l.g[i].place(c, L.cout, 9 * L.cin);
        }
    }
    l.total = c.off;
    return l;
}
extern "C" size_t imcui_hip_d2net_packed_floats(void) { return d2_layout().total; }

extern "C" int imcui_hip_d2net_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    for (int i = 0; i < 2 * D2_NL; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const D2Layout l = d2_layout();
    memset(packed, 0, l.total * sizeof(float));
    for (int i = 0; i < D2_NL; ++i) {
        const D2Layer& L = D2_LAYERS[i];
        const float *w = t[2 * i], *b = t[2 * i + 1];
        if (i == 0) {
            for (int co = 0; co < 64; ++co)
                for (int ci = 0; ci < 3; ++ci)
                    for (int k = 0; k < 9; ++k) packed[l.w0 + ((size_t)k * 3 + ci) * 64 + co] = w[((size_t)co * 3 + ci) * 9 + k];
            memcpy(packed + l.b0, b, 64 * sizeof(float));
        } else if (L.dil == 1) {
            pack_conv3x3(w, L.cout, L.cin, packed + l.w[i]);
            memcpy(packed + l.b[i], b, L.cout * sizeof(float));
            packed[l.ws[i]] = pack_conv3x3_split(w, L.cout, L.cin, reinterpret_cast<unsigned short*>(packed + l.wh[i]),
                                                 reinterpret_cast<unsigned short*>(packed + l.wl[i]));
        } else {
            pack_conv_gemm(w, L.cout, L.cin, 3, L.cin, packed + l.g[i].w);
            memcpy(packed + l.g[i].b, b, L.cout * sizeof(float));
            l.g[i].split_planes(packed, L.cout, 9 * L.cin);
        }
    }
    return IMCUI_OK;
}

// what the emit kernel needs to know about the levels: where each map lies in the workspace, its shape, and the float32 factors
// h_init / h_level, w_init / w_level of pyramid.py
struct D2Levels {
    long off[D2_MAXLEV];  // floats from the first level's map to this level's [B, h, w, C]
    int h[D2_MAXLEV], w[D2_MAXLEV];
    float rs[D2_MAXLEV], cs[D2_MAXLEV];
};

namespace {

// d2net.py:39-41 for image channel c (RGB): x * 255 - mean, one rounding each (mean is the BGR triple 103.939, 116.779, 123.68)
__device__ __forceinline__ float d2_norm(float x, int c) {
    const float mean = c == 0 ? 123.68f : (c == 1 ? 116.779f : 103.939f);
    return __fsub_rn(__fmul_rn(x, 255.0f), mean);
}

static float d2_ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }  // align_corners=True

// what the level resize reads: the normalised image (channels stay RGB; layer 0 flips)
struct D2ResizeLoad {
    __device__ float operator()(float v, long plane) const { return d2_norm(v, (int)(plane % 3)); }
};
// what layer 0 reads: input channel c of the network is image channel 2 - c; norm: the image is the raw one
struct D2StemLoad {
    int norm;
    __device__ float operator()(const float* __restrict__ img, long b, int c, int h, int w, int yy, int xx) const {
        const float v = img[((b * 3 + (2 - c)) * h + yy) * (long)w + xx];
        return norm ? d2_norm(v, 2 - c) : v;
    }
};

// pyramid.py `dense_features += F.interpolate(previous_dense_features, size=[h, w], mode='bilinear', align_corners=True)`, NHWC, in
// place on f [B, h, w, C]; prev [B, ph, pw, C]
__global__ __launch_bounds__(256) void d2_addup_kernel(float* __restrict__ f, const float* __restrict__ prev, int h, int w, int ph, int pw, int C, float sh,
                                                       float sw, long n4) {
    const int C4 = C >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        long t = i / C4;
        const int x = (int)(t % w);
        t /= w;
        const int y = (int)(t % h);
        const long b = t / h;
        int y0, y1, x0, x1;
        float hy0, hy1, wx0, wx1;
        bilinear_src_align_corners(y, sh, ph, &y0, &y1, &hy0, &hy1);
        bilinear_src_align_corners(x, sw, pw, &x0, &x1, &wx0, &wx1);
        const float* pb = prev + b * (long)ph * pw * C + c;
        const float4 v00 = *reinterpret_cast<const float4*>(pb + ((long)y0 * pw + x0) * C), v01 = *reinterpret_cast<const float4*>(pb + ((long)y0 * pw + x1) * C),
                     v10 = *reinterpret_cast<const float4*>(pb + ((long)y1 * pw + x0) * C), v11 = *reinterpret_cast<const float4*>(pb + ((long)y1 * pw + x1) * C);
        float4 o = *reinterpret_cast<float4*>(f + i * 4);
#define D2_UP(m) o.m = __fadd_rn(o.m, __fadd_rn(__fmul_rn(hy0, __fadd_rn(__fmul_rn(wx0, v00.m), __fmul_rn(wx1, v01.m))), \
                                              __fmul_rn(hy1, __fadd_rn(__fmul_rn(wx0, v10.m), __fmul_rn(wx1, v11.m)))))
        D2_UP(x);
        D2_UP(y);
        D2_UP(z);
        D2_UP(w);
#undef D2_UP
        *reinterpret_cast<float4*>(f + i * 4) = o;
    }
}

// HardDetectionModule (edge_threshold 5) and HandcraftedLocalizationModule in ONE channel c of one image's map x [h, w, C] at pixel
// (i, j), whose value there is v.  The Hessian filters see zero padding, the 3x3 maximum sees the map only (max_pool2d pads with -inf).
// One explicit float32 order, no fused multiply-add, IEEE division (tests/d2net_reference.py carries the same):
//   dii = (up - 2c) + down, djj = (left - 2c) + right, dij = 0.25 (((ul - ur) - dl) + dr), det = dii djj - dij dij (both products
//   rounded), (tr tr) / det <= 7.2, det > 0;  step_i = -((djj / det) di + (-dij / det) dj), step_j = -((-dij / det) di + (dii / det) dj)
// detected: upstream's `detections` entry (given that v is the channel-wise maximum).  kept: it also passes |step| < 0.5 and has the
// four corners floor / ceil of p = (i, j) + step inside the map.
__device__ __forceinline__ void d2_eval(const float* __restrict__ x, int h, int w, int C, int i, int j, int c, float v, bool* detected, bool* kept, float* pi,
                                        float* pj) {
    float nb[9];
    bool lmax = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int ii = i + dy, jj = j + dx;
            float u = 0.0f;
            if (ii >= 0 && ii < h && jj >= 0 && jj < w) {
                u = x[((long)ii * w + jj) * C + c];
                lmax = lmax && !(u > v);
            }
            nb[(dy + 1) * 3 + dx + 1] = u;
        }
    const float ul = nb[0], up = nb[1], ur = nb[2], lf = nb[3], rt = nb[5], dl = nb[6], dn = nb[7], dr = nb[8];
    const float c2 = __fmul_rn(2.0f, v);
    const float dii = __fadd_rn(__fsub_rn(up, c2), dn);
    const float djj = __fadd_rn(__fsub_rn(lf, c2), rt);
    const float dij = __fmul_rn(0.25f, __fadd_rn(__fsub_rn(__fsub_rn(ul, ur), dl), dr));
    const float det = __fsub_rn(__fmul_rn(dii, djj), __fmul_rn(dij, dij));
    const float tr = __fadd_rn(dii, djj);
    const float ratio = __fdiv_rn(__fmul_rn(tr, tr), det);
    const bool d = lmax && (ratio <= 7.2f) && (det > 0.0f);
    const float di = __fmul_rn(0.5f, __fsub_rn(dn, up)), dj = __fmul_rn(0.5f, __fsub_rn(rt, lf));
    const float h00 = __fdiv_rn(djj, det), h01 = __fdiv_rn(-dij, det), h11 = __fdiv_rn(dii, det);
    const float si = -__fadd_rn(__fmul_rn(h00, di), __fmul_rn(h01, dj));
    const float sj = -__fadd_rn(__fmul_rn(h01, di), __fmul_rn(h11, dj));
    const float p_i = __fadd_rn((float)i, si), p_j = __fadd_rn((float)j, sj);
    const bool inside = floorf(p_i) >= 0.0f && floorf(p_j) >= 0.0f && ceilf(p_i) <= (float)(h - 1) && ceilf(p_j) <= (float)(w - 1);
    *detected = d;
    *kept = d && (fabsf(si) < 0.5f) && (fabsf(sj) < 0.5f) && inside;
    *pi = p_i;
    *pj = p_j;
}

// One wave per pixel.  planes [B][C / 64][npix]: bit q of word k = channel 64 k + q of the pixel is kept.  ban_prev [B, ph, pw] (or
// null: first level) is looked up with ATen's nearest rule min(floor(dst * (in / out)), in - 1); ban_out [B, h, w] = banned before or
// detected here (detected, not kept: pyramid.py updates `banned` ahead of the step filter).
__global__ __launch_bounds__(256) void d2_detect_kernel(const float* __restrict__ feat, int h, int w, int C, const unsigned char* __restrict__ ban_prev, int ph,
                                                        int pw, float bsh, float bsw, unsigned char* __restrict__ ban_out,
                                                        unsigned long long* __restrict__ planes, long total) {
    const int lane = threadIdx.x & 63;
    const long gp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gp >= total) return;  // (wave-uniform)
    const int npix = h * w, nk = C >> 6;
    const long b = gp / npix;
    const int pix = (int)(gp - b * npix);
    const int i = pix / w, j = pix - i * w;
    const float* x = feat + b * (long)npix * C;
    const float* px = x + (long)pix * C;
    float v[8];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[k] = k < nk ? px[k * 64 + lane] : -INFINITY;
        m = fmaxf(m, v[k]);
    }
    m = wave_max(m);
    bool banned = false;
    if (ban_prev) {
        const int si = min((int)floorf(__fmul_rn((float)i, bsh)), ph - 1), sj = min((int)floorf(__fmul_rn((float)j, bsw)), pw - 1);
        banned = ban_prev[(b * ph + si) * (long)pw + sj] != 0;
    }
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= nk) break;  // (uniform)
        bool det = false, kept = false;
        float pi, pj;
        if (!banned && v[k] == m) d2_eval(x, h, w, C, i, j, k * 64 + lane, v[k], &det, &kept, &pi, &pj);
        const unsigned long long bd = __ballot(det), bk = __ballot(kept);
        if (lane == 0) planes[(b * nk + k) * (long)npix + pix] = bk;
        any = any || bd != 0ull;
    }
    if (lane == 0) ban_out[gp] = (banned || any) ? 1 : 0;
}

// The candidate domain of select.h is (channel, pixel), channel-major: torch.nonzero's order on detections[0] ([C, h, w]).
struct D2Pred {
    const unsigned long long* planes_all;
    const unsigned long long* planes;
    int npix, nk;
    __device__ void bind(int b) { planes = planes_all + (long)b * nk * npix; }
    __device__ bool operator()(const float*, int idx) const {
        const int c = idx / npix, pix = idx - c * npix;
        return (planes[(long)(c >> 6) * npix + pix] >> (c & 63)) & 1ull;
    }
};
// candidate number pos of image b AT THIS LEVEL goes to slot base[b] + pos of the image's list (slots past kcap are counted only);
// the score is pyramid.py's dense_features[c, i, j] / (idx + 1)
struct D2Emit {
    const int* base;
    const float* feat;  // this level's maps [B, npix, C]
    float* cscore;
    int* clc;   // level * 512 + channel
    int* cpix;
    int kcap, level, npix, C;
    __device__ void operator()(int b, int pos, int idx, float) const {
        const long s = (long)base[b] + pos;
        if (s >= kcap) return;
        const int c = idx / npix, pix = idx - c * npix;
        cscore[(long)b * kcap + s] = __fdiv_rn(feat[((long)b * npix + pix) * C + c], (float)(level + 1));
        clc[(long)b * kcap + s] = level * 512 + c;
        cpix[(long)b * kcap + s] = pix;
    }
};

// The rows of ranked_rows_kernel (ascending (score, slot) order: the kept list is in slot order), one wave each: the step again (d2_eval: the same arithmetic as the detector's), interpolate_dense_features' four corners with
// weights (1 - di)(1 - dj) .. di dj summed tl, tr, bl, br, F.normalize (eps 1e-12), upscale_positions (twice p * 2 + 0.5) and the
// level's factors.  feat0 = the first level's maps; keypoints (x, y): d2net.py:49 swaps the columns.  Rows past the count are zero.
struct D2Row {
    const int *clc, *cpix;
    const float* feat0;
    int kcap, kout;
    D2Levels lv;
    int C;
    float *kpts, *scores, *desc;
    __device__ void clear(int b, int lo, int hi) const {
        const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nk = C >> 6;
        float* kp = kpts + (long)b * kout * 2;
        float* de = desc + (long)b * kout * C;
        for (int i = lo + tid; i < hi; i += 256) kp[2 * i] = kp[2 * i + 1] = scores[(long)b * kout + i] = 0.0f;
        for (int i = lo + wv; i < hi; i += 4)
            for (int k = 0; k < nk; ++k) de[(long)i * C + k * 64 + lane] = 0.0f;
    }
    __device__ void emit(int b, int i0, int m, const int* ks, const int* rank, const float* cs) const {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nk = C >> 6;
        float* kp = kpts + (long)b * kout * 2;
        float* sc = scores + (long)b * kout;
        float* de = desc + (long)b * kout * C;
        for (int q = wv; q < m; q += 4) {
            const int slot = ks[i0 + q], r = rank[q];
            const int lc = clc[(long)b * kcap + slot], pix = cpix[(long)b * kcap + slot];
            const int l = lc >> 9, c = lc & 511;
            const int h = lv.h[l], w = lv.w[l];
            const float* x = feat0 + lv.off[l] + (long)b * h * w * C;
            const int pi_ = pix / w, pj_ = pix - pi_ * w;
            bool det, kept;
            float p_i, p_j;
            d2_eval(x, h, w, C, pi_, pj_, c, x[(long)pix * C + c], &det, &kept, &p_i, &p_j);
            // (a listed candidate is kept: its corners lie inside the map; the clamps keep a wrong list from reading outside it)
            const int it = min(max((int)floorf(p_i), 0), h - 1), ib = min(max((int)ceilf(p_i), 0), h - 1);
            const int jl = min(max((int)floorf(p_j), 0), w - 1), jr = min(max((int)ceilf(p_j), 0), w - 1);
            const float di = __fsub_rn(p_i, floorf(p_i)), dj = __fsub_rn(p_j, floorf(p_j));
            const float wtl = __fmul_rn(__fsub_rn(1.0f, di), __fsub_rn(1.0f, dj)), wtr = __fmul_rn(__fsub_rn(1.0f, di), dj),
                        wbl = __fmul_rn(di, __fsub_rn(1.0f, dj)), wbr = __fmul_rn(di, dj);
            const float *ptl = x + ((long)it * w + jl) * C, *ptr = x + ((long)it * w + jr) * C, *pbl = x + ((long)ib * w + jl) * C,
                        *pbr = x + ((long)ib * w + jr) * C;
            float d[8];
            float ss = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                d[k] = 0.0f;
                if (k < nk) {
                    const int ch = k * 64 + lane;
                    d[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(wtl, ptl[ch]), __fmul_rn(wtr, ptr[ch])), __fmul_rn(wbl, pbl[ch])), __fmul_rn(wbr, pbr[ch]));
                    ss += d[k] * d[k];
                }
            }
            const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < nk) de[(long)r * C + k * 64 + lane] = d[k] / nrm;
            if (lane == 0) {
                const float ui = __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p_i, 2.0f), 0.5f), 2.0f), 0.5f);
                const float uj = __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p_j, 2.0f), 0.5f), 2.0f), 0.5f);
                kp[2 * r] = __fmul_rn(uj, lv.cs[l]);
                kp[2 * r + 1] = __fmul_rn(ui, lv.rs[l]);
                sc[r] = cs[slot];
            }
        }
    }
};

}  // namespace

// layer 0 on the planar image [B, 3, H, W] -> out [B, H, W, 64]
static void d2_stem(const D2Layout& l, const float* P, const float* img, int norm, int B, int H, int W, float* out, hipStream_t stream) {
    const long npix = (long)B * H * W;
    hipLaunchKernelGGL((stem3x3_kernel<64, D2StemLoad>), dim3(blocks_256(npix)), dim3(256), 0, stream, img, P + l.w0, P + l.b0, out, H, W, D2StemLoad{norm}, npix);
}
// MODE 0: the flooring 2x2 max-pool, [B, hi, wi, C] -> [B, hi / 2, wi / 2, C]; MODE 1: the 2x2 stride-1 average -> [B, hi - 1, wi - 1, C]
template <int MODE>
static void d2_pool(const float* src, float* dst, int B, int hi, int wi, int C, hipStream_t stream) {
    const int ho = MODE == 0 ? hi / 2 : hi - 1, wo = MODE == 0 ? wi / 2 : wi - 1;
    const long n4 = (long)B * ho * wo * (C / 4);
    hipLaunchKernelGGL(pool2x2_kernel<MODE>, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, src, dst, hi, wi, ho, wo, C, n4);
}

// ------------------------------------------------------------------ workspace
struct D2Ws {
    float *img, *fa, *fb, *feat, *cscore;
    unsigned long long* planes;
    unsigned char* ban[2];
    CandScan scan;  // (total = this level's count)
    CutList cut;
    int *base, *clc, *cpix, *status;
    size_t total;
    bool ok;
};
// imgpix: pixels of the largest level image (0: no trunk, the probe); fpix_sum / fpix_max: pixels of the levels' feature maps
static D2Ws d2_carve(void* ws, size_t bytes, int B, size_t imgpix, size_t fpix_sum, size_t fpix_max, int C, int kcap, bool own_feat) {
    WsAlloc a(ws, bytes);
    D2Ws s;
    s.img = a.get<float>((size_t)B * 3 * imgpix);
    s.fa = a.get<float>((size_t)B * imgpix * 64);
    s.fb = a.get<float>((size_t)B * imgpix * 64);
    s.feat = a.get<float>(own_feat ? (size_t)B * fpix_sum * C : 0);
    s.planes = a.get<unsigned long long>((size_t)B * (C / 64) * fpix_max);
    s.ban[0] = a.get<unsigned char>((size_t)B * fpix_max);
    s.ban[1] = a.get<unsigned char>((size_t)B * fpix_max);
    s.scan.carve(a, B, fpix_max * C);
    s.base = a.get<int>(B);
    s.cscore = a.get<float>((size_t)B * kcap);
    s.clc = a.get<int>((size_t)B * kcap);
    s.cpix = a.get<int>((size_t)B * kcap);
    s.cut.carve(a, B, kcap);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

struct D2Sizes {
    size_t imgpix, fpix_sum, fpix_max;
};
static int d2_check(imcui_hip_t* h, int B, int H, int W, int nlev, const int* lh, const int* lw, D2Sizes* z) {
    if (B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "d2net: B=%d above 1024", B);
    if (H < 1 || W < 1 || nlev < 1 || nlev > D2_MAXLEV || !lh || !lw)
        return imcui_set_err(h, IMCUI_ERR_ARG, "d2net: H=%d W=%d, %d levels (1..%d) and the two level arrays are needed", H, W, nlev, D2_MAXLEV);
    z->imgpix = z->fpix_sum = z->fpix_max = 0;
    for (int l = 0; l < nlev; ++l) {
        if (lh[l] < 1 || lw[l] < 1) return imcui_set_err(h, IMCUI_ERR_ARG, "d2net: level %d is %dx%d", l, lh[l], lw[l]);
        const int fh = lh[l] / 4 - 1, fw = lw[l] / 4 - 1;
        if (fh < 1 || fw < 1)
            return imcui_set_err(h, IMCUI_ERR_ARG, "d2net: level %d (%dx%d) has an empty feature map: every level needs at least 8x8 pixels", l, lh[l], lw[l]);
        z->imgpix = std::max(z->imgpix, (size_t)lh[l] * lw[l]);
        z->fpix_sum += (size_t)fh * fw;
        z->fpix_max = std::max(z->fpix_max, (size_t)fh * fw);
    }
    // int indices: pixels of a level's 64-channel maps over the batch, the (channel, pixel) candidate domain of one image
    if ((long)B * (long)z->imgpix > 0x7fffffffL / 64 || (long)z->fpix_max * D2_DIM > 0x7fffffffL || (long)B * (long)z->fpix_max > 0x7fffffffL / 4)
        return imcui_set_err(h, IMCUI_ERR_ARG, "d2net: B=%d images with levels up to %zu pixels exceed the 2^31 index range of one call", B, z->imgpix);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_d2net_workspace_bytes(int B, int nlev, const int* lh, const int* lw, int kcap) {
    if (B <= 0 || nlev <= 0 || !lh || !lw || kcap <= 0) return 0;
    size_t imgpix = 0, fsum = 0, fmax = 0;
    for (int l = 0; l < nlev; ++l) {
        const size_t fh = (size_t)std::max(lh[l] / 4 - 1, 0), fw = (size_t)std::max(lw[l] / 4 - 1, 0);
        imgpix = std::max(imgpix, (size_t)std::max(lh[l], 0) * (size_t)std::max(lw[l], 0));
        fsum += fh * fw;
        fmax = std::max(fmax, fh * fw);
    }
    return d2_carve(nullptr, 0, B, imgpix, fsum, fmax, D2_DIM, kcap, true).total;
}

// the trunk on the planar level image `img` [B, 3, H, W] (norm: it is the raw image); the map [B, H / 4 - 1, W / 4 - 1, 512] -> out
static int d2_trunk(imcui_hip_t* h, const D2Layout& l, const float* P, const float* img, int norm, int B, int H, int W, int use_relu, const D2Ws& s,
                    float* out, hipStream_t stream) {
    const bool split = h->precision == 1;
    int rc;
    d2_stem(l, P, img, norm, B, H, W, s.fa, stream);
    IMCUI_CHECK_LAUNCH(h);
    float *cur = s.fa, *oth = s.fb;
    int hh = H, ww = W;
    auto conv = [&](int i, int pool) -> int {
        const D2Layer& L = D2_LAYERS[i];
        if (split)
            return conv3x3_split_launch(h, cur, reinterpret_cast<const unsigned short*>(P + l.wh[i]), reinterpret_cast<const unsigned short*>(P + l.wl[i]),
                                        P + l.ws[i], P + l.b[i], oth, B, hh, ww, L.cin, L.cout, 1, pool, stream);
        return conv3x3_launch(h, cur, P + l.w[i], P + l.b[i], oth, B, hh, ww, L.cin, L.cout, 1, pool, stream);
    };
    for (int i = 1; i <= 6; ++i) {
        const D2Layer& L = D2_LAYERS[i];
        const bool fused = L.pool && !((hh | ww) & 1);
        IMCUI_RUN(conv(i, fused ? 1 : 0));
        std::swap(cur, oth);
        if (L.pool) {
            if (!fused) {  // an odd map: nn.MaxPool2d floors
                d2_pool<0>(cur, oth, B, hh, ww, L.cout, stream);
                IMCUI_CHECK_LAUNCH(h);
                std::swap(cur, oth);
            }
            hh /= 2;
            ww /= 2;
        }
    }
    d2_pool<1>(cur, oth, B, hh, ww, 256, stream);  // nn.AvgPool2d(2, stride=1)
    IMCUI_CHECK_LAUNCH(h);
    std::swap(cur, oth);
    --hh;
    --ww;
    for (int i = 7; i < D2_NL; ++i) {
        const D2Layer& L = D2_LAYERS[i];
        GemmP g;
        g.epi = EPI_CONV;
        g.A = cur;
        gemm_set_weights(g, P, l.g[i], L.cout, 9 * L.cin, split);
        gemm_set_conv(g, 3, 1, L.dil, hh, ww, hh, ww, L.cin);
        g.conv_dil = L.dil;
        g.M = B * hh * ww;
        g.C = i == D2_NL - 1 ? out : oth;
        g.ldc = L.cout;
        g.act = (i == D2_NL - 1 && !use_relu) ? 0 : 1;
        IMCUI_RUN(gemm_launch(h, g, stream));
        std::swap(cur, oth);
    }
    return IMCUI_OK;
}

// detector + candidate list of one level (maps `feat` [B, fh, fw, C]); ban_prev of shape [B, ph, pw] or null
static int d2_detect_level(imcui_hip_t* h, const D2Ws& s, const float* feat, int B, int fh, int fw, int C, int level, const unsigned char* ban_prev, int ph,
                           int pw, unsigned char* ban_out, int kcap, hipStream_t stream) {
    const int npix = fh * fw;
    const long total = (long)B * npix;
    hipLaunchKernelGGL(d2_detect_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, feat, fh, fw, C, ban_prev, ph, pw,
                       ban_prev ? (float)ph / (float)fh : 0.0f, ban_prev ? (float)pw / (float)fw : 0.0f, ban_out, s.planes, total);
    IMCUI_CHECK_LAUNCH(h);
    const int dom = npix * C;
    const D2Pred pred{s.planes, nullptr, npix, C / 64};
    const D2Emit emit{s.base, feat, s.cscore, s.clc, s.cpix, kcap, level, npix, C};
    // (the `map` argument of the shared kernels is read at a candidate's index and handed to the emit functor, which ignores it: the
    // level's own maps have exactly `dom` floats per image)
    cand_list(stream, feat, dom, B, pred, s.scan, dom, emit);
    hipLaunchKernelGGL(advance_base_kernel<>, dim3(cdiv(B, 256)), dim3(256), 0, stream, s.base, s.scan.total, B);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

extern "C" int imcui_hip_d2net_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, int nlev, const int* lh, const int* lw,
                                       int use_relu, int max_keypoints, int kcap, int kout, float* keypoints, float* scores, float* descriptors,
                                       int* num_keypoints, int* status, float* dbg_feat, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    D2Sizes z;
    int rc;
    IMCUI_RUN(d2_check(h, B, H, W, nlev, lh, lw, &z));
    if (kcap <= 0 || kout <= 0 || kout > kcap || !packed || !image || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "d2net: null argument, kcap<=0 or kout outside 1..kcap");
    if ((long)B * kcap > 0x7fffffffL / 2) return imcui_set_err(h, IMCUI_ERR_ARG, "d2net: B=%d lists of kcap=%d candidates exceed 2^30", B, kcap);
    if (max_keypoints > 0 && kout > max_keypoints) return imcui_set_err(h, IMCUI_ERR_ARG, "d2net: kout=%d above max_keypoints=%d", kout, max_keypoints);
    const D2Layout l = d2_layout();
    D2Ws s = d2_carve(ws, ws_bytes, B, z.imgpix, z.fpix_sum, z.fpix_max, D2_DIM, kcap, true);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "d2net: workspace too small (%zu < %zu)", ws_bytes, s.total);
    int* st = status ? status : s.status;
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(cdiv(B, 256)), dim3(256), 0, stream, s.base, B);
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, st, 1);
    D2Levels lv;
    for (int i = 0; i < D2_MAXLEV; ++i) lv.off[i] = 0, lv.h[i] = lv.w[i] = 1, lv.rs[i] = lv.cs[i] = 1.0f;
    long off = 0;
    int ph = 0, pw = 0;
    for (int lev = 0; lev < nlev; ++lev) {
        const int ch = lh[lev], cw = lw[lev], fh = ch / 4 - 1, fw = cw / 4 - 1;
        lv.off[lev] = off;
        lv.h[lev] = fh;
        lv.w[lev] = fw;
        lv.rs[lev] = (float)((double)H / (double)ch);  // pyramid.py multiplies the float32 rows by the Python float h_init / h_level
        lv.cs[lev] = (float)((double)W / (double)cw);
        const float* cur = image;
        const bool same = ch == H && cw == W;  // align_corners=True at scale 1 is the identity
        if (!same) {
            const long n = (long)B * 3 * ch * cw;
            hipLaunchKernelGGL((resize_planar_kernel<bilinear_src_align_corners, D2ResizeLoad>), dim3(blocks_256(n)), dim3(256), 0, stream, image, s.img, H, W,
                               ch, cw, d2_ac_scale(H, ch), d2_ac_scale(W, cw), D2ResizeLoad{}, n);
            IMCUI_CHECK_LAUNCH(h);
            cur = s.img;
        }
        float* f = s.feat + off;
        IMCUI_RUN(d2_trunk(h, l, packed, cur, same ? 1 : 0, B, ch, cw, use_relu, s, f, stream));
        const long nf = (long)B * fh * fw * D2_DIM;
        if (lev > 0) {
            hipLaunchKernelGGL(d2_addup_kernel, dim3(grid_stride_blocks(nf / 4)), dim3(256), 0, stream, f, s.feat + lv.off[lev - 1], fh, fw, ph, pw, D2_DIM,
                               d2_ac_scale(ph, fh), d2_ac_scale(pw, fw), nf / 4);
            IMCUI_CHECK_LAUNCH(h);
        }
        copy_if(dbg_feat ? dbg_feat + off : nullptr, f, nf * sizeof(float), stream);
        IMCUI_RUN(d2_detect_level(h, s, f, B, fh, fw, D2_DIM, lev, lev > 0 ? s.ban[(lev - 1) & 1] : nullptr, ph, pw, s.ban[lev & 1], kcap, stream));
        off += nf;
        ph = fh;
        pw = fw;
    }
    cand_cut(stream, s.cscore, s.base, kcap, max_keypoints, s.cut, st, B);
    ranked_rows(stream, s.cscore, kcap, s.cut, kout, num_keypoints, D2Row{s.clc, s.cpix, s.feat, kcap, kout, lv, D2_DIM, keypoints, scores, descriptors}, B);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// test entry: one of the small kernels of the trunk alone.  op 0: layer 0 with the wrapper's normalisation, in = image [B, 3, H, W] RGB
// in [0,1] -> out [B, H, W, 64]; op 1: the flooring 2x2 max-pool, in [B, H, W, C] -> out [B, H / 2, W / 2, C]; op 2: the 2x2 stride-1
// average pool -> out [B, H - 1, W - 1, C]
extern "C" int imcui_hip_d2net_layer_probe(imcui_hip_t* h, int op, const float* packed, const float* in, int B, int H, int W, int C, float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B < 1 || H < 1 || W < 1 || !in || !out || (long)B * H * W > 0x7fffffffL / 512) return imcui_set_err(h, IMCUI_ERR_ARG, "d2net layer probe: shape");
    if (op == 0) {
        if (!packed) return imcui_set_err(h, IMCUI_ERR_ARG, "d2net layer probe: layer 0 needs the packed weights");
        d2_stem(d2_layout(), packed, in, 1, B, H, W, out, stream);
    } else if (op == 1 || op == 2) {
        const int ho = op == 1 ? H / 2 : H - 1, wo = op == 1 ? W / 2 : W - 1;
        if (C < 4 || C % 4 || C > 512 || ho < 1 || wo < 1) return imcui_set_err(h, IMCUI_ERR_ARG, "d2net layer probe: C=%d (a multiple of 4 up to 512), %dx%d", C, H, W);
        if (op == 1)
            d2_pool<0>(in, out, B, H, W, C, stream);
        else
            d2_pool<1>(in, out, B, H, W, C, stream);
    } else {
        return imcui_set_err(h, IMCUI_ERR_ARG, "d2net layer probe: op %d", op);
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_d2net_probe_workspace_bytes(int B, int fh, int fw, int C, int kcap) {
    if (B <= 0 || fh <= 0 || fw <= 0 || C <= 0 || kcap <= 0) return 0;
    return d2_carve(nullptr, 0, B, 0, (size_t)fh * fw, (size_t)fh * fw, C, kcap, false).total;
}

// test entry: detector, localization, candidate list, cut and descriptors on maps GIVEN by the caller as one level whose image is the
// level itself (factors 1): crafted maps reach the selection code without the trunk
extern "C" int imcui_hip_d2net_detect_probe(imcui_hip_t* h, const float* feat, int B, int fh, int fw, int C, int max_keypoints, int kcap, int kout,
                                            float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, void* ws, size_t ws_bytes,
                                            void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (B > 1024 || fh < 1 || fw < 1 || C < 64 || C > D2_DIM || C % 64 || (long)fh * fw * C > 0x7fffffffL / 4 || (long)B * fh * fw > 0x7fffffffL / 4)
        return imcui_set_err(h, IMCUI_ERR_ARG, "d2net probe: B=%d map %dx%d with C=%d (a multiple of 64 up to %d)", B, fh, fw, C, D2_DIM);
    if (kcap <= 0 || kout <= 0 || kout > kcap || (long)B * kcap > 0x7fffffffL / 2 || !feat || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "d2net probe: null argument, kcap<=0 or kout outside 1..kcap");
    if (max_keypoints > 0 && kout > max_keypoints) return imcui_set_err(h, IMCUI_ERR_ARG, "d2net probe: kout=%d above max_keypoints=%d", kout, max_keypoints);
    D2Ws s = d2_carve(ws, ws_bytes, B, 0, (size_t)fh * fw, (size_t)fh * fw, C, kcap, false);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "d2net probe: workspace too small (%zu < %zu)", ws_bytes, s.total);
    int* st = status ? status : s.status;
    int rc;
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(cdiv(B, 256)), dim3(256), 0, stream, s.base, B);
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, st, 1);
    D2Levels lv;
    for (int i = 0; i < D2_MAXLEV; ++i) lv.off[i] = 0, lv.h[i] = lv.w[i] = 1, lv.rs[i] = lv.cs[i] = 1.0f;
    lv.h[0] = fh;
    lv.w[0] = fw;
    IMCUI_RUN(d2_detect_level(h, s, feat, B, fh, fw, C, 0, nullptr, 0, 0, s.ban[0], kcap, stream));
    cand_cut(stream, s.cscore, s.base, kcap, max_keypoints, s.cut, st, B);
    ranked_rows(stream, s.cscore, kcap, s.cut, kout, num_keypoints, D2Row{s.clc, s.cpix, feat, kcap, kout, lv, C, keypoints, scores, descriptors}, B);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
