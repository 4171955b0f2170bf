// R2D2 forward on MI355X (r2d2_WASF_N16 / r2d2_WASF_N8 / r2d2_WAF_N16: Quad_L2Net_ConfCFS): the multi-scale extraction of
// imcui/hloc/extractors/r2d2.py:49-73 (naver/r2d2: extract.py extract_multiscale + NonMaxSuppression, nets/patchnet.py) as one call.
//
// Per pyramid level (levels one after another in one workspace sized for the largest; the level list comes from the binding, which
// evaluates upstream's float64 schedule):
//   level l + 1 = ATen bilinear (align_corners=False, no anti-aliasing) of level l, planar [B, 3, nh, nw]; the wrapper's
//                 tvf.Normalize is applied where level 0 is READ (by layer 0 and by the first resize), so padding stays zero
//   layer 0     3 -> 32, 3x3, folded BatchNorm + ReLU, fp32 FMA on the VALU, planar in, NHWC out
//   layers 1-8  implicit-GEMM convolutions with dilated taps (gemm.hip, GemmP.conv_dil; both arithmetic modes): 3x3 d 1, 2, 2, 4 and
//               2x2 d 4, 8, 16 with pad d / 2; BatchNorm (affine=False) folded at pack time, ReLU in the epilogue of layers 1-5
//   head        one pass over the 128-channel map: x^2, the rows of clf (2) and sal (1), soft-max / softplus -> reliability and
//               repeatability, TWO floats per pixel; the normalised descriptor map is never written
//   detector    (rep == 3x3 max, -inf outside) & rep >= rep_thr & rel >= rel_thr as a candidate predicate of select.h; the level's
//               candidates append, row-major, to one list per image (score = rel * rep, level, flat index) and their RAW 128-vectors
//               are parked beside it, because the level's map is overwritten by the next level
// After the last level: radix select of the max_keypoints-th largest (score, candidate index) key, output in ascending (score, index)
// order -- torch.argsort(stable=True)[-K:] --, one wave per key-point normalises the parked vector (F.normalize, eps 1e-12).
// No float atomics, fixed summation orders, every grid sized by shapes or capacities: batch-independent, bitwise reproducible, no
// host synchronisation.
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

#define R2_NL 9        // convolutions
#define R2_MAXLEV 32   // pyramid levels per call
#define R2_DIM 128

// ------------------------------------------------------------------ the network and its tensor table
struct R2Layer {
    int cin, cout, k, dil, bn, relu, op;  // op = index of the convolution in upstream's flat `ops` ModuleList (its BatchNorm: op + 1)
};
static const R2Layer R2_LAYERS[R2_NL] = {{3, 32, 3, 1, 1, 1, 0},     {32, 32, 3, 1, 1, 1, 3},    {32, 64, 3, 1, 1, 1, 6},
                                         {64, 64, 3, 2, 1, 1, 9},    {64, 128, 3, 2, 1, 1, 12},  {128, 128, 3, 4, 1, 1, 15},
                                         {128, 128, 2, 4, 1, 0, 18}, {128, 128, 2, 8, 1, 0, 20}, {128, 128, 2, 16, 0, 0, 22}};
static int r2_pad(const R2Layer& L) { return ((L.k - 1) * L.dil) / 2; }

static const TensorTable& r2_tensors() {
    static TensorTable t;
    static bool done = [] {
        for (int i = 0; i < R2_NL; ++i) {
            const R2Layer& L = R2_LAYERS[i];
            const std::string p = "ops." + std::to_string(L.op);
            t.add(p + ".weight", (size_t)L.cout * L.cin * L.k * L.k);
            t.add(p + ".bias", (size_t)L.cout);
            if (L.bn) {  // affine=False: running statistics only
                const std::string q = "ops." + std::to_string(L.op + 1);
                t.add(q + ".running_mean", (size_t)L.cout);
                t.add(q + ".running_var", (size_t)L.cout);
            }
        }
        t.add("clf.weight", 2 * R2_DIM);
        t.add("clf.bias", 2);
        t.add("sal.weight", R2_DIM);
        t.add("sal.bias", 1);
        return true;
    }();
    (void)done;
    return t;
}
extern "C" int imcui_hip_r2d2_num_tensors(void) { return r2_tensors().size(); }
extern "C" const char* imcui_hip_r2d2_tensor_name(int i) { return r2_tensors().name(i); }

// packed: layer 0 [tap][cin 3][32] + bias [32]; layers 1..8 as GEMM layers [cout][tap][cin]; the head rows [3][128] (clf 0, clf 1,
// sal) and their biases [3]
struct R2Layout {
    size_t w0, b0;
    GemmLayerOff g[R2_NL];  // (g[0] unused)
    size_t hw, hb;
    size_t total;
};
static R2Layout r2_layout() {
    R2Layout l;
    PackCursor c;
    l.w0 = c.get(27 * 32);
    l.b0 = c.get(32);
    for (int i = 1; i < R2_NL; ++i) l.g[i].place(c, R2_LAYERS[i].cout, R2_LAYERS[i].k * R2_LAYERS[i].k * R2_LAYERS[i].cin);
    l.hw = c.get(3 * R2_DIM);
    l.hb = c.get(3);
    l.total = c.off;
    return l;
}
extern "C" size_t imcui_hip_r2d2_packed_floats(void) { return r2_layout().total; }

extern "C" int imcui_hip_r2d2_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    const TensorTable& names = r2_tensors();
    for (int i = 0; i < names.size(); ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const R2Layout l = r2_layout();
    memset(packed, 0, l.total * sizeof(float));
    auto T = [&](const std::string& name) { return t[names.find(name)]; };
    std::vector<float> sc, sh, ones, zeros, tmp;
    for (int i = 0; i < R2_NL; ++i) {
        const R2Layer& L = R2_LAYERS[i];
        const std::string p = "ops." + std::to_string(L.op), q = "ops." + std::to_string(L.op + 1);
        const float *w = T(p + ".weight"), *b = T(p + ".bias");
        sc.assign(L.cout, 1.0f);
        sh.assign(L.cout, 0.0f);
        if (L.bn) {  // BatchNorm2d(affine=False, eval): weight 1, bias 0
            ones.assign(L.cout, 1.0f);
            zeros.assign(L.cout, 0.0f);
            const float* bn[4] = {ones.data(), zeros.data(), T(q + ".running_mean"), T(q + ".running_var")};
            bn_fold_f32(bn, L.cout, sc, sh);
        }
        for (int co = 0; co < L.cout; ++co) sh[co] = b[co] * sc[co] + sh[co];  // the convolution's own bias goes through the BatchNorm
        const int taps = L.k * L.k;
        if (i == 0) {
            for (int co = 0; co < L.cout; ++co)
                for (int ci = 0; ci < 3; ++ci)
                    for (int k = 0; k < 9; ++k) packed[l.w0 + ((size_t)k * 3 + ci) * 32 + co] = w[((size_t)co * 3 + ci) * 9 + k] * sc[co];
            memcpy(packed + l.b0, sh.data(), 32 * sizeof(float));
            continue;
        }
        const int K = taps * L.cin;
        tmp.assign((size_t)L.cout * K, 0.0f);
        pack_conv_gemm(w, L.cout, L.cin, L.k, L.cin, tmp.data());
        for (int co = 0; co < L.cout; ++co)
            for (int k = 0; k < K; ++k) tmp[(size_t)co * K + k] *= sc[co];
        memcpy(packed + l.g[i].w, tmp.data(), (size_t)L.cout * K * sizeof(float));
        memcpy(packed + l.g[i].b, sh.data(), L.cout * sizeof(float));
        l.g[i].split_planes(packed, L.cout, K);
    }
    memcpy(packed + l.hw, T("clf.weight"), 2 * R2_DIM * sizeof(float));
    memcpy(packed + l.hw + 2 * R2_DIM, T("sal.weight"), R2_DIM * sizeof(float));
    packed[l.hb] = T("clf.bias")[0];
    packed[l.hb + 1] = T("clf.bias")[1];
    packed[l.hb + 2] = T("sal.bias")[0];
    return IMCUI_OK;
}

struct R2Levels {
    int n;
    int nh[R2_MAXLEV], nw[R2_MAXLEV];
};

namespace {

// tvf.Normalize of channel c: (x - mean) / std, one rounding each
__device__ __forceinline__ float r2_norm(float x, int c) {
    const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    return __fdiv_rn(__fsub_rn(x, mean), sd);
}

// planar [B, 3, hi, wi] -> [B, 3, ho, wo]; norm: the source is the raw image (level 0) and is normalised as it is read.  (Not an
// instance of net_kernels.h's resize_planar_kernel: this file is compiled with floating-point contraction on, the compiler fuses one
// product of each row mix into the sum, and WHICH one it picked changed with the shape of the code; the bits of the levels follow.)
__global__ __launch_bounds__(256) void r2_resize_kernel(const float* __restrict__ src, float* __restrict__ dst, int hi, int wi, int ho, int wo, float sh,
                                                        float sw, int norm, long n) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % wo);
    const long q = p / wo;
    const int y = (int)(q % ho);
    const long bc = q / ho;
    const int c = (int)(bc % 3);
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    bilinear_src_half_pixel(y, sh, hi, &y0, &y1, &hy0, &hy1);
    bilinear_src_half_pixel(x, sw, wi, &x0, &x1, &wx0, &wx1);
    const float* pl = src + bc * (long)hi * wi;
    float v00 = pl[(long)y0 * wi + x0], v01 = pl[(long)y0 * wi + x1], v10 = pl[(long)y1 * wi + x0], v11 = pl[(long)y1 * wi + x1];
    if (norm) {
        v00 = r2_norm(v00, c);
        v01 = r2_norm(v01, c);
        v10 = r2_norm(v10, c);
        v11 = r2_norm(v11, c);
    }
    const float top = __fadd_rn(__fmul_rn(wx0, v00), __fmul_rn(wx1, v01)), bot = __fadd_rn(__fmul_rn(wx0, v10), __fmul_rn(wx1, v11));
    dst[p] = __fadd_rn(__fmul_rn(hy0, top), __fmul_rn(hy1, bot));
}

// what layer 0 reads; norm: the image is the raw one (level 0)
struct R2StemLoad {
    int norm;
    __device__ float operator()(const float* __restrict__ img, long b, int c, int h, int w, int yy, int xx) const {
        const float v = img[((b * 3 + c) * h + yy) * (long)w + xx];
        return norm ? r2_norm(v, c) : v;
    }
};

// head: u = W (x * x) + b for the three rows (clf 0, clf 1, sal); reliability = softmax(clf)[1], repeatability = softplus(sal) / (1 +
// softplus(sal)).  32 lanes per pixel, 4 channels per lane, a fixed xor tree over the 32 lanes
__global__ __launch_bounds__(256) void r2_head_kernel(const float* __restrict__ x, const float* __restrict__ hw, const float* __restrict__ hb,
                                                      float* __restrict__ rel, float* __restrict__ rep, long npix) {
    const int sub = threadIdx.x & 31;
    const float4 w0 = *reinterpret_cast<const float4*>(hw + 4 * sub), w1 = *reinterpret_cast<const float4*>(hw + R2_DIM + 4 * sub),
                 w2 = *reinterpret_cast<const float4*>(hw + 2 * R2_DIM + 4 * sub);
    const float b0 = hb[0], b1 = hb[1], b2 = hb[2];
    const long step = (long)gridDim.x * 8;
    const long pend = (npix + step - 1) / step * step;  // (every lane of a wave takes the shuffles)
    for (long p = (long)blockIdx.x * 8 + (threadIdx.x >> 5); p < pend; p += step) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < npix) v = *reinterpret_cast<const float4*>(x + p * R2_DIM + 4 * sub);
        v.x *= v.x, v.y *= v.y, v.z *= v.z, v.w *= v.w;
        float u0 = fmaf(v.w, w0.w, fmaf(v.z, w0.z, fmaf(v.y, w0.y, v.x * w0.x)));
        float u1 = fmaf(v.w, w1.w, fmaf(v.z, w1.z, fmaf(v.y, w1.y, v.x * w1.x)));
        float u2 = fmaf(v.w, w2.w, fmaf(v.z, w2.z, fmaf(v.y, w2.y, v.x * w2.x)));
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            u0 += __shfl_xor(u0, o, 64);
            u1 += __shfl_xor(u1, o, 64);
            u2 += __shfl_xor(u2, o, 64);
        }
        if (sub == 0 && p < npix) {
            u0 += b0, u1 += b1, u2 += b2;
            const float m = fmaxf(u0, u1), e0 = expf(u0 - m), e1 = expf(u1 - m);
            rel[p] = e1 / (e0 + e1);
            const float sp = u2 > 20.0f ? u2 : log1pf(expf(u2));  // F.softplus (beta 1, threshold 20)
            rep[p] = sp / (1.0f + sp);
        }
    }
}

// NonMaxSuppression.forward: a maximum of the 3x3 max filter (-inf outside, i.e. neighbours inside the map only) above both thresholds
struct R2Pred {
    const float* rel_all;
    const float* rel;
    int h, w;
    float rel_thr, rep_thr;
    __device__ void bind(int b) { rel = rel_all + (long)b * h * w; }
    __device__ bool operator()(const float* rep, int idx) const {
        const float v = rep[idx];
        if (!(v >= rep_thr) || !(rel[idx] >= rel_thr)) return false;
        const int y = idx / w, x = idx - y * w;
        float m = v;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= h) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx;
                if (xx >= 0 && xx < w) m = fmaxf(m, rep[yy * w + xx]);
            }
        }
        return v == m;
    }
};
// candidate number pos of image b AT THIS LEVEL goes to slot base[b] + pos of the image's list (slots past kcap are counted only)
struct R2Emit {
    const int* base;
    const float* rel_all;
    float* cscore;
    int* clev;
    int* cidx;
    int kcap, level, npix;
    __device__ void operator()(int b, int pos, int idx, float v) const {
        const long s = (long)base[b] + pos;
        if (s >= kcap) return;
        cscore[(long)b * kcap + s] = __fmul_rn(rel_all[(long)b * npix + idx], v);
        clev[(long)b * kcap + s] = level;
        cidx[(long)b * kcap + s] = idx;
    }
};

// park the raw 128-vectors of this level's candidates (slots base[b] .. base[b] + nlev[b], clipped to kcap): one wave per candidate
__global__ __launch_bounds__(256) void r2_park_kernel(const float* __restrict__ x, const int* __restrict__ base, const int* __restrict__ nlev,
                                                      const int* __restrict__ cidx, int kcap, int npix, float* __restrict__ cvec) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int s0 = base[b], s1 = min(s0 + nlev[b], kcap);
    for (int s = s0 + blockIdx.x * 4 + (threadIdx.x >> 6); s < s1; s += gridDim.x * 4) {
        const float* src = x + ((long)b * npix + cidx[(long)b * kcap + s]) * R2_DIM;
        *reinterpret_cast<float2*>(cvec + ((long)b * kcap + s) * R2_DIM + 2 * lane) = *reinterpret_cast<const float2*>(src + 2 * lane);
    }
}

// F.normalize(v, dim=channel) of one 128-vector held two floats per lane
__device__ __forceinline__ float2 r2_normalize(float2 v) {
    const float d = fmaxf(sqrtf(wave_sum(v.x * v.x + v.y * v.y)), 1e-12f);
    return make_float2(v.x / d, v.y / d);
}

// The rows of ranked_rows_kernel (ascending (score, slot) order: the kept list is in slot order), one wave each: x W / nw, y H / nh as
// float32 (x * W) / nw, the score, the normalised parked vector.  Rows past the count are zero.
struct R2Row {
    const int *clev, *cidx;
    const float* cvec;
    int kcap, kout;
    R2Levels lv;
    int H, W;
    float *kpts, *scores, *desc;
    __device__ void clear(int b, int lo, int hi) const {
        const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
        float* kp = kpts + (long)b * kout * 2;
        float* de = desc + (long)b * kout * R2_DIM;
        for (int i = lo + tid; i < hi; i += 256) kp[2 * i] = kp[2 * i + 1] = scores[(long)b * kout + i] = 0.0f;
        for (int i = lo + wv; i < hi; i += 4) *reinterpret_cast<float2*>(de + (long)i * R2_DIM + 2 * lane) = make_float2(0.0f, 0.0f);
    }
    __device__ void emit(int b, int i0, int m, const int* ks, const int* rank, const float* cs) const {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        float* kp = kpts + (long)b * kout * 2;
        float* de = desc + (long)b * kout * R2_DIM;
        for (int j = wv; j < m; j += 4) {
            const int slot = ks[i0 + j], r = rank[j];
            const float2 v = r2_normalize(*reinterpret_cast<const float2*>(cvec + ((long)b * kcap + slot) * R2_DIM + 2 * lane));
            *reinterpret_cast<float2*>(de + (long)r * R2_DIM + 2 * lane) = v;
            if (lane == 0) {
                const int l = clev[(long)b * kcap + slot], idx = cidx[(long)b * kcap + slot];
                const int nw = lv.nw[l], nh = lv.nh[l];
                const int y = idx / nw, x = idx - y * nw;
                kp[2 * r] = __fdiv_rn(__fmul_rn((float)x, (float)W), (float)nw);
                kp[2 * r + 1] = __fdiv_rn(__fmul_rn((float)y, (float)H), (float)nh);
                scores[(long)b * kout + r] = cs[slot];
            }
        }
    }
};

// test entry: F.normalize of the final map at n given pixels of one image
__global__ __launch_bounds__(256) void r2_probe_kernel(const float* __restrict__ x, int w, const int* __restrict__ xy, int n, float* __restrict__ desc) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const long p = (long)xy[2 * i + 1] * w + xy[2 * i];
        *reinterpret_cast<float2*>(desc + (long)i * R2_DIM + 2 * lane) = r2_normalize(*reinterpret_cast<const float2*>(x + p * R2_DIM + 2 * lane));
    }
}

}  // namespace

// ------------------------------------------------------------------ workspace
struct R2Ws {
    float *lev[2], *fa, *fb, *rel, *rep, *cscore, *cvec;
    CandScan scan;  // (total = this level's count)
    CutList cut;
    int *base, *clev, *cidx, *status;
    size_t total;
    bool ok;
};
static R2Ws r2_carve(void* ws, size_t bytes, int B, size_t npix_max, int kcap) {
    WsAlloc a(ws, bytes);
    R2Ws s;
    s.lev[0] = a.get<float>((size_t)B * 3 * npix_max);
    s.lev[1] = a.get<float>((size_t)B * 3 * npix_max);
    s.fa = a.get<float>((size_t)B * npix_max * R2_DIM);
    s.fb = a.get<float>((size_t)B * npix_max * R2_DIM);
    s.rel = a.get<float>((size_t)B * npix_max);
    s.rep = a.get<float>((size_t)B * npix_max);
    s.scan.carve(a, B, npix_max);
    s.base = a.get<int>(B);
    s.cscore = a.get<float>((size_t)B * kcap);
    s.clev = a.get<int>((size_t)B * kcap);
    s.cidx = a.get<int>((size_t)B * kcap);
    s.cut.carve(a, B, kcap);
    s.cvec = a.get<float>((size_t)B * kcap * R2_DIM);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

static int r2_check(imcui_hip_t* h, int B, int H, int W, int nlev, const int* nh, const int* nw, const int* run, size_t* npix_max, long* npix_run) {
    if (B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2: B=%d above 1024", B);
    if (H < 1 || W < 1 || nlev < 1 || nlev > R2_MAXLEV || !nh || !nw || !run)
        return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2: H=%d W=%d, %d levels (1..%d) and the three level arrays are needed", H, W, nlev, R2_MAXLEV);
    if (nh[0] != H || nw[0] != W) return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2: level 0 must be the image itself (%dx%d, got %dx%d)", H, W, nh[0], nw[0]);
    *npix_max = 0;
    *npix_run = 0;
    for (int l = 0; l < nlev; ++l) {
        if (nh[l] < 1 || nw[l] < 1 || nh[l] > H || nw[l] > W)
            return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2: level %d is %dx%d: levels lie between 1x1 and the image (max_scale <= 1)", l, nh[l], nw[l]);
        const size_t np = (size_t)nh[l] * nw[l];
        if (np > *npix_max) *npix_max = np;
        if (run[l]) *npix_run += (long)np;
    }
    if ((long)B * (long)*npix_max > 0x7fffffffL / 4) return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2: B=%d images of %dx%d exceed 2^29 pixels per call", B, H, W);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_r2d2_workspace_bytes(int B, int nlev, const int* nh, const int* nw, int kcap) {
    if (B <= 0 || nlev <= 0 || !nh || !nw || kcap <= 0) return 0;
    size_t npix_max = 0;
    for (int l = 0; l < nlev; ++l) npix_max = std::max(npix_max, (size_t)std::max(nh[l], 0) * (size_t)std::max(nw[l], 0));
    return r2_carve(nullptr, 0, B, npix_max, kcap).total;
}

// the nine convolutions on the planar level `img` [B, 3, nh, nw]; the final 128-channel NHWC map ends in s.fa
static int r2_net(imcui_hip_t* h, const R2Layout& l, const float* P, const float* img, int norm, int B, int nh, int nw, const R2Ws& s, hipStream_t stream) {
    const long npix = (long)B * nh * nw;
    const bool split = h->precision == 1;
    int rc;
    hipLaunchKernelGGL((stem3x3_kernel<32, R2StemLoad>), dim3(blocks_256(npix)), dim3(256), 0, stream, img, P + l.w0, P + l.b0, s.fa, nh, nw, R2StemLoad{norm}, npix);
    IMCUI_CHECK_LAUNCH(h);
    const float* in = s.fa;
    float* out = s.fb;
    for (int i = 1; i < R2_NL; ++i) {
        const R2Layer& L = R2_LAYERS[i];
        GemmP g;
        g.epi = EPI_CONV;
        g.A = in;
        gemm_set_weights(g, P, l.g[i], L.cout, L.k * L.k * L.cin, split);
        gemm_set_conv(g, L.k, 1, r2_pad(L), nh, nw, nh, nw, L.cin);
        g.conv_dil = L.dil;
        g.M = (int)npix;
        g.C = out;
        g.ldc = L.cout;
        g.act = L.relu;
        IMCUI_RUN(gemm_launch(h, g, stream));
        float* t = const_cast<float*>(in);
        in = out;
        out = t;
    }
    return IMCUI_OK;  // (eight swaps: the last output is s.fa)
}

extern "C" int imcui_hip_r2d2_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, int nlev, const int* nh,
                                      const int* nw, const int* run, float rel_thr, float rep_thr, int max_keypoints, int kcap, int kout,
                                      float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, float* dbg_rel,
                                      float* dbg_rep, float* dbg_map, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    size_t npix_max;
    long npix_run;
    int rc;
    IMCUI_RUN(r2_check(h, B, H, W, nlev, nh, nw, run, &npix_max, &npix_run));
    if (kcap <= 0 || kout <= 0 || kout > kcap || !packed || !image || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2: null argument, kcap<=0 or kout outside 1..kcap");
    if ((long)kcap > std::max(npix_run, 1L) || (long)B * kcap > 0x7fffffffL)
        return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2: kcap=%d above the pixels of the levels that run (%ld)", kcap, npix_run);
    if (max_keypoints > 0 && kout > max_keypoints) return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2: kout=%d above max_keypoints=%d", kout, max_keypoints);
    const R2Layout l = r2_layout();
    R2Ws s = r2_carve(ws, ws_bytes, B, npix_max, kcap);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "r2d2: workspace too small (%zu < %zu)", ws_bytes, s.total);
    int* st = status ? status : s.status;
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(cdiv(B, 256)), dim3(256), 0, stream, s.base, B);
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, st, 1);
    R2Levels lv;
    lv.n = nlev;
    for (int i = 0; i < R2_MAXLEV; ++i) lv.nh[i] = lv.nw[i] = 1;
    const float* cur = image;  // level 0: the raw image, normalised where it is read
    size_t dbg_off = 0;
    for (int lev = 0; lev < nlev; ++lev) {
        const int ch = nh[lev], cw = nw[lev];
        lv.nh[lev] = ch;
        lv.nw[lev] = cw;
        const int npix = ch * cw;
        if (lev > 0) {
            float* dst = s.lev[lev & 1];
            const long n = (long)B * 3 * npix;
            // ATen: scale = in / out in float32
            hipLaunchKernelGGL(r2_resize_kernel, dim3(blocks_256(n)), dim3(256), 0, stream, cur, dst, nh[lev - 1], nw[lev - 1], ch, cw,
                               (float)nh[lev - 1] / (float)ch, (float)nw[lev - 1] / (float)cw, lev == 1 ? 1 : 0, n);
            IMCUI_CHECK_LAUNCH(h);
            cur = dst;
        }
        if (!run[lev]) continue;
        IMCUI_RUN(r2_net(h, l, packed, cur, lev == 0 ? 1 : 0, B, ch, cw, s, stream));
        const long np = (long)B * npix;
        hipLaunchKernelGGL(r2_head_kernel, dim3((unsigned)std::min<long>((np + 7) / 8, 65536)), dim3(256), 0, stream, s.fa, packed + l.hw, packed + l.hb, s.rel,
                           s.rep, np);
        IMCUI_CHECK_LAUNCH(h);
        copy_if(dbg_rel ? dbg_rel + dbg_off : nullptr, s.rel, np * sizeof(float), stream);
        copy_if(dbg_rep ? dbg_rep + dbg_off : nullptr, s.rep, np * sizeof(float), stream);
        copy_if(dbg_map ? dbg_map + dbg_off * R2_DIM : nullptr, s.fa, np * R2_DIM * sizeof(float), stream);
        dbg_off += (size_t)np;
        // ---- detector: this level's candidates append to the image's list
        const R2Pred pred{s.rel, nullptr, ch, cw, rel_thr, rep_thr};
        const R2Emit emit{s.base, s.rel, s.cscore, s.clev, s.cidx, kcap, lev, npix};
        cand_list(stream, s.rep, npix, B, pred, s.scan, npix, emit);
        hipLaunchKernelGGL(r2_park_kernel, dim3(std::min(cdiv(std::min(npix, kcap), 4), 4096), B), dim3(256), 0, stream, s.fa, s.base, s.scan.total, s.cidx, kcap,
                           npix, s.cvec);
        hipLaunchKernelGGL(advance_base_kernel<>,dim3(cdiv(B, 256)), dim3(256), 0, stream, s.base, s.scan.total, B);
        IMCUI_CHECK_LAUNCH(h);
    }
    // ---- cut + emit
    cand_cut(stream, s.cscore, s.base, kcap, max_keypoints, s.cut, st, B);
    ranked_rows(stream, s.cscore, kcap, s.cut, kout, num_keypoints, R2Row{s.clev, s.cidx, s.cvec, kcap, kout, lv, H, W, keypoints, scores, descriptors}, B);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// test entry: the network at full resolution on ONE image, F.normalize of its final map at n caller-given integer pixels (x, y)
extern "C" int imcui_hip_r2d2_desc_probe(imcui_hip_t* h, const float* packed, const float* image, int H, int W, const int* xy, int n, float* descriptors,
                                         void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    const int one = 1;
    size_t npix_max;
    long npix_run;
    int rc;
    IMCUI_RUN(r2_check(h, 1, H, W, 1, &H, &W, &one, &npix_max, &npix_run));
    if (n <= 0 || n > H * W || !packed || !image || !xy || !descriptors) return imcui_set_err(h, IMCUI_ERR_ARG, "r2d2 probe: null argument or n outside 1..H*W");
    R2Ws s = r2_carve(ws, ws_bytes, 1, npix_max, 1);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "r2d2 probe: workspace too small (%zu < %zu)", ws_bytes, s.total);
    IMCUI_RUN(r2_net(h, r2_layout(), packed, image, 1, 1, H, W, s, stream));
    hipLaunchKernelGGL(r2_probe_kernel, dim3(std::min(cdiv(n, 4), 4096)), dim3(256), 0, stream, s.fa, W, xy, n, descriptors);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
