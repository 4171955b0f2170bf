// Patch descriptors on MI355X (extractor confs `sosnet` / `hardnet`, model `dog`): imcui/hloc/extractors/dog.py:87-105 -- kornia's
// laf_from_center_scale_ori + extract_patches_from_pyramid(PS = 32) and kornia.feature.HardNet / SOSNet on the patches -- as one batched
// call on key-points GIVEN by the caller (the detector is csrc/sift.hip, or anything else that has x, y, scale and orientation).
// kornia is not part of the reference checkout: tests/dog_reference.py restates the rules of one release (0.7.0: pyrdown = 5x5 binomial
// blur + bilinear halving, LAF / grid normalisation by w - 1), and the stage is parity-unpinned.
//
//   pyramid     level l + 1 = pyrdown(level l) while min(h, w) >= 32: dg_blur_kernel (reflect border, 25 taps in row-major order) and
//               resize_planar_kernel (ATen bilinear, align_corners=False, size (h / 2, w / 2)); planar [B, h, w]; only the levels a key-point
//               can choose are built (index <= max(0, min(H, W) / 32 - 1)); a level index the loop never reaches leaves a ZERO patch, as
//               kornia's `out = torch.zeros(..)` does
//   sampling    one workgroup per patch: the LAF (centre xy + 0.5, scale sigma mr_size / 2, angle -ori), normalised by the image and
//               de-normalised at the level floor(log2(2 laf_scale / 32)); F.affine_grid (align_corners=False) + F.grid_sample (bilinear,
//               border) -> [n, 32, 32, 1]
//   layer 1     per patch: mean, then the centred sum of squares (two passes, fixed reduction order); HardNet (x - mean) / (std + 1e-6)
//               with the unbiased std, SOSNet InstanceNorm2d (biased variance, eps 1e-5); 1 -> 32, 3x3, folded BatchNorm + ReLU on the
//               VALU from LDS -> NHWC
//   layers 2-6  the implicit-GEMM convolutions of gemm.hip (both arithmetic modes), patches as the batch dimension: 32 -> 32, 32 -> 64
//               s2, 64 -> 64, 64 -> 128 s2, 128 -> 128; BatchNorm (affine=False) folded at pack time, ReLU in the epilogue
//   layer 7     8x8 valid = [n, 8192] x [8192, 128]: DG_NG partial products over DG_KG = 1024 of K each (one batched GEMM launch), folded
//               in group order, then the BatchNorm shift (one chain over 8192 is what missed NetVLAD's float64 bar at 4608)
//   output      one wave per row: HardNet F.normalize (eps 1e-12); SOSNet LocalResponseNorm(256, alpha 256, beta 0.5, k 0) of x + 1e-10,
//               which over 128 channels is (x + 1e-10) / |x + 1e-10|
// Patches are processed per image in chunks of `chunk`; the launches are fixed by (B, kcap, chunk), the live rows of a chunk are read on
// the device (GemmP.mcnt and the kernels' own exits), so nothing synchronises with the host.  Every row of every GEMM is one chain over
// K: a descriptor does not depend on B, on the other images' counts or on `chunk`.  No float atomics.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "imcui_hip.h"
#include "net_kernels.h"
#include "netpack.h"
#include "select.h"

#define DG_NL 7
#define DG_PS 32
#define DG_PIX (DG_PS * DG_PS)
#define DG_DIM 128
#define DG_KF 8192     // K of the last layer: 8 x 8 x 128
#define DG_KG 1024     // ... summed in groups of this many
#define DG_NG (DG_KF / DG_KG)
#define DG_MAXLEV 16
#define DG_MAXCHUNK 8192

// ------------------------------------------------------------------ the networks and their tensor tables
struct DgLayer {
    int cin, cout, k, stride, hin, hout;
};
static const DgLayer DG_LAYERS[DG_NL] = {{1, 32, 3, 1, 32, 32},  {32, 32, 3, 1, 32, 32},  {32, 64, 3, 2, 32, 16}, {64, 64, 3, 1, 16, 16},
                                         {64, 128, 3, 2, 16, 8}, {128, 128, 3, 1, 8, 8}, {128, 128, 8, 1, 8, 1}};
// index of the convolution in kornia's nn.Sequential (its BatchNorm: + 1): HardNet.features / SOSNet.layers (InstanceNorm2d at 0)
static const int DG_OP[2][DG_NL] = {{0, 3, 6, 9, 12, 15, 19}, {1, 4, 7, 10, 13, 16, 20}};

static TensorTable dg_table(int model) {
    TensorTable t;
    const std::string root = model == 1 ? "layers." : "features.";
    for (int i = 0; i < DG_NL; ++i) {
        const DgLayer& L = DG_LAYERS[i];
        const int op = DG_OP[model == 1][i];
        t.add(root + std::to_string(op) + ".weight", (size_t)L.cout * L.cin * L.k * L.k);
        t.add(root + std::to_string(op + 1) + ".running_mean", (size_t)L.cout);
        t.add(root + std::to_string(op + 1) + ".running_var", (size_t)L.cout);
    }
    return t;
}
extern "C" int imcui_hip_patchdesc_num_tensors(int model) { return (model == 0 || model == 1) ? dg_table(model).size() : 0; }
extern "C" const char* imcui_hip_patchdesc_tensor_name(int model, int i) {
    static thread_local std::string name;
    if (model != 0 && model != 1) return nullptr;
    const TensorTable t = dg_table(model);
    if (!t.name(i)) return nullptr;
    name = t.name(i);
    return name.c_str();
}

// packed (the same layout for both networks): layer 1 [tap][32] + shift [32]; layers 2..6 as GEMM layers [cout][tap][cin]; layer 7 f32
// [128][8192] (K order tap, channel = the NHWC map flattened) TIMES 2^e, the power of two that puts the largest magnitude into
// [4096, 8192] -- the split arithmetic splits this matrix as it is read, and the scaling keeps the low halves out of the f16 subnormal
// range as split_weights_frag_host does for pre-split planes; exact in float32 --, the shift [128] and 2^-e
struct DgLayout {
    size_t w0, b0;
    GemmLayerOff g[DG_NL - 1];  // (g[0] unused)
    size_t wf, bf, fs;
    size_t total;
};
static DgLayout dg_layout() {
    DgLayout l;
    PackCursor c;
    l.w0 = c.get(9 * 32);
    l.b0 = c.get(32);
    for (int i = 1; i < DG_NL - 1; ++i) l.g[i].place(c, DG_LAYERS[i].cout, 9 * DG_LAYERS[i].cin);
    l.wf = c.get((size_t)DG_DIM * DG_KF);
    l.bf = c.get(DG_DIM);
    l.fs = c.get(1);
    l.total = c.off;
    return l;
}
extern "C" size_t imcui_hip_patchdesc_packed_floats(void) { return dg_layout().total; }

extern "C" int imcui_hip_patchdesc_pack_weights(int model, const float* const* t, float* packed) {
    if (!t || !packed || (model != 0 && model != 1)) return IMCUI_ERR_ARG;
    for (int i = 0; i < 3 * DG_NL; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const DgLayout l = dg_layout();
    memset(packed, 0, l.total * sizeof(float));
    std::vector<float> sc, sh, ones, zeros, tmp;
    for (int i = 0; i < DG_NL; ++i) {
        const DgLayer& L = DG_LAYERS[i];
        const float* w = t[3 * i];
        ones.assign(L.cout, 1.0f);  // BatchNorm2d(affine=False, eval): weight 1, bias 0
        zeros.assign(L.cout, 0.0f);
        const float* bn[4] = {ones.data(), zeros.data(), t[3 * i + 1], t[3 * i + 2]};
        bn_fold_f32(bn, L.cout, sc, sh);
        if (i == 0) {
            for (int co = 0; co < 32; ++co)
                for (int k = 0; k < 9; ++k) packed[l.w0 + (size_t)k * 32 + co] = w[(size_t)co * 9 + k] * sc[co];
            memcpy(packed + l.b0, sh.data(), 32 * sizeof(float));
            continue;
        }
        const int K = L.k * L.k * L.cin;
        tmp.assign((size_t)L.cout * K, 0.0f);
        pack_conv_gemm(w, L.cout, L.cin, L.k, L.cin, tmp.data());
        for (int co = 0; co < L.cout; ++co)
            for (int k = 0; k < K; ++k) tmp[(size_t)co * K + k] *= sc[co];
        if (i < DG_NL - 1) {
            memcpy(packed + l.g[i].w, tmp.data(), (size_t)L.cout * K * sizeof(float));
            memcpy(packed + l.g[i].b, sh.data(), L.cout * sizeof(float));
            l.g[i].split_planes(packed, L.cout, K);
            continue;
        }
        float mx = 0.0f;
        for (float v : tmp) mx = fmaxf(mx, fabsf(v));
        int e = 0;
        if (mx > 0.0f && std::isfinite(mx)) e = std::min(24, std::max(-8, (int)floorf(log2f(8192.0f / mx))));
        for (float& v : tmp) v = ldexpf(v, e);
        memcpy(packed + l.wf, tmp.data(), (size_t)DG_DIM * DG_KF * sizeof(float));
        memcpy(packed + l.bf, sh.data(), DG_DIM * sizeof(float));
        packed[l.fs] = ldexpf(1.0f, -e);
    }
    return IMCUI_OK;
}

// the pyramid of an H x W image: level 0 is the image; `n` levels are built, `maxidx` is kornia's clamp of the level index
struct DgLevels {
    int n, maxidx;
    int h[DG_MAXLEV], w[DG_MAXLEV];
    long off[DG_MAXLEV];  // first float of level l >= 1 in the pyramid buffer [B, h, w]
};
static DgLevels dg_levels(int B, int H, int W, size_t* pyr_floats) {
    DgLevels lv;
    memset(&lv, 0, sizeof(lv));
    lv.maxidx = std::max(0, std::min(H, W) / DG_PS - 1);
    lv.n = 1;
    lv.h[0] = H;
    lv.w[0] = W;
    size_t off = 0;
    int h = H, w = W;
    while (std::min(h, w) >= DG_PS && lv.n <= lv.maxidx && lv.n < DG_MAXLEV) {
        h /= 2;
        w /= 2;
        lv.h[lv.n] = h;
        lv.w[lv.n] = w;
        lv.off[lv.n] = (long)off;
        off += (size_t)B * h * w;
        ++lv.n;
    }
    if (pyr_floats) *pyr_floats = off;
    return lv;
}
extern "C" int imcui_hip_patchdesc_num_levels(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return dg_levels(1, H, W, nullptr).n;
}

namespace {

__device__ __forceinline__ int dg_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// kornia filter2d with the 5x5 binomial kernel [1 4 6 4 1]^T [1 4 6 4 1] / 256, border "reflect": planar [B, h, w] -> [B, h, w]; h, w >= 3
__global__ __launch_bounds__(256) void dg_blur_kernel(const float* __restrict__ src, float* __restrict__ dst, int h, int w, long n) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % w);
    const long q = p / w;
    const int y = (int)(q % h);
    const float* pl = src + (q / h) * (long)h * w;
    const float k1[5] = {1.0f, 4.0f, 6.0f, 4.0f, 1.0f};
    float acc = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) {
        const int yy = dg_reflect(y + ky - 2, h);
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
            const int xx = dg_reflect(x + kx - 2, w);
            acc = fmaf(pl[(long)yy * w + xx], k1[ky] * k1[kx] * (1.0f / 256.0f), acc);
        }
    }
    dst[p] = acc;
}

// what the pyramid's down-sampling (F.interpolate(size=(ho, wo), mode="bilinear", align_corners=False) of planar [B, hi, wi]) reads:
// the blurred level as it is
struct DgResizeLoad {
    __device__ float operator()(float v, long) const { return v; }
};

// live rows of chunk c of image b for the four row granularities of the network (pixels of a 32x32, 16x16, 8x8 map, patches) ->
// mc [B, nchunk, 4]; status bit 1: a count above kcap
__global__ __launch_bounds__(256) void dg_count_kernel(const int* __restrict__ cnt, int B, int nchunk, int chunk, int kcap, int* __restrict__ mc,
                                                       int* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * nchunk) return;
    const int b = i / nchunk, c = i - b * nchunk;
    const int n = cnt[b];
    if (n > kcap && c == 0) atomicOr(status, 1);
    const int live = max(0, min(min(max(n, 0), kcap) - c * chunk, chunk));
    mc[4 * i] = live * DG_PIX;
    mc[4 * i + 1] = live * 256;
    mc[4 * i + 2] = live * 64;
    mc[4 * i + 3] = live;
}
// test entries: the four live-row counts of a chunk that is full (n patches)
__global__ void dg_full_kernel(int* __restrict__ mc, int n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        mc[0] = n * DG_PIX;
        mc[1] = n * 256;
        mc[2] = n * 64;
        mc[3] = n;
    }
}

__device__ __forceinline__ bool dg_finite4(float a, float b, float c, float d) { return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d); }

// dog.py:88-98 for patch i of the chunk (one workgroup each): kp [n, 2], sc [n], od [n] (degrees) of ONE image whose level-0 plane is
// img0 [H, W] and whose level l >= 1 plane is pyr + lv.off[l] + img_index * h_l * w_l.  live: device count of the chunk (nullptr: n_static)
__global__ __launch_bounds__(256) void dg_sample_kernel(const float* __restrict__ img0, const float* __restrict__ pyr, DgLevels lv, int img_index,
                                                        const float* __restrict__ kp, const float* __restrict__ sc, const float* __restrict__ od,
                                                        const int* __restrict__ live, int n_static, float mr_size, float* __restrict__ patches,
                                                        float* __restrict__ dbg, int* __restrict__ status) {
    const int i = blockIdx.x;
    if (i >= (live ? *live : n_static)) return;
    float* out = patches + (long)i * DG_PIX;
    float* out2 = dbg ? dbg + (long)i * DG_PIX : nullptr;
    const float x = kp[2 * i], y = kp[2 * i + 1], s = sc[i], o = od[i];
    const int H = lv.h[0], W = lv.w[0];
    const bool bad = !dg_finite4(x, y, s, o);
    // laf_from_center_scale_ori: scale * [[cos a, sin a], [-sin a, cos a]] with a = deg2rad(-ori)
    const float ls = (s * mr_size) / 2.0f;
    const float rad = (-o) * 3.14159265358979323846f / 180.0f;
    const float cs = cosf(rad), sn = sinf(rad);
    const float a00 = ls * cs, a01 = ls * sn, a10 = ls * (-sn), a11 = ls * cs;
    // normalize_laf(laf, image)
    const float wf = (float)(W - 1), hf = (float)(H - 1), ms0 = fminf(wf, hf);
    const float rm = 1.0f / ms0;
    const float n00 = a00 * rm, n01 = a01 * rm, n10 = a10 * rm, n11 = a11 * rm;
    const float tnx = (x + 0.5f) * (1.0f / wf), tny = (y + 0.5f) * (1.0f / hf);
    // the level: get_laf_scale of the LAF de-normalised at level 0
    const float d00 = n00 * ms0, d01 = n01 * ms0, d10 = n10 * ms0, d11 = n11 * ms0;
    const float det = d00 * d11 - d10 * d01 + 1e-10f;
    const float psc = 2.0f * sqrtf(fabsf(det)) / (float)DG_PS;
    int level = psc >= 1.0f ? (int)floorf(log2f(psc)) : 0;
    level = max(0, min(level, lv.maxidx));
    if (bad || level >= lv.n) {  // (a level kornia's loop never reaches: its output stays zero)
        for (int p = threadIdx.x; p < DG_PIX; p += 256) {
            out[p] = 0.0f;
            if (out2) out2[p] = 0.0f;
        }
        if (bad && threadIdx.x == 0) atomicOr(status, 2);
        return;
    }
    const int hl = lv.h[level], wl = lv.w[level];
    const float* pl = level == 0 ? img0 : pyr + lv.off[level] + (long)img_index * hl * wl;
    const float wlf = (float)(wl - 1), hlf = (float)(hl - 1), msl = fminf(wlf, hlf);
    const float l00 = n00 * msl, l01 = n01 * msl, l10 = n10 * msl, l11 = n11 * msl;
    const float tx = tnx * wlf, ty = tny * hlf;
    for (int p = threadIdx.x; p < DG_PIX; p += 256) {
        const int py = p >> 5, px = p & 31;
        const float xb = (float)(2 * px + 1) / (float)DG_PS - 1.0f, yb = (float)(2 * py + 1) / (float)DG_PS - 1.0f;  // exact
        const float gx = fmaf(l01, yb, fmaf(l00, xb, tx)), gy = fmaf(l11, yb, fmaf(l10, xb, ty));
        const float gnx = 2.0f * gx / wlf - 1.0f, gny = 2.0f * gy / hlf - 1.0f;
        float ix = ((gnx + 1.0f) * (float)wl - 1.0f) / 2.0f, iy = ((gny + 1.0f) * (float)hl - 1.0f) / 2.0f;
        ix = fminf(fmaxf(ix, 0.0f), wlf);  // padding_mode="border" (fmaxf drops a NaN)
        iy = fminf(fmaxf(iy, 0.0f), hlf);
        const int x0 = max(0, min((int)floorf(ix), wl - 1)), y0 = max(0, min((int)floorf(iy), hl - 1));
        const int x1 = x0 + 1, y1 = y0 + 1;
        const float fx0 = (float)x0, fy0 = (float)y0, fx1 = (float)x1, fy1 = (float)y1;
        const float nw = (fx1 - ix) * (fy1 - iy), ne = (ix - fx0) * (fy1 - iy), sw = (fx1 - ix) * (iy - fy0), se = (ix - fx0) * (iy - fy0);
        const bool xin = x1 <= wl - 1, yin = y1 <= hl - 1;
        float v = pl[(long)y0 * wl + x0] * nw;
        if (xin) v += pl[(long)y0 * wl + x1] * ne;
        if (yin) v += pl[(long)y1 * wl + x0] * sw;
        if (xin && yin) v += pl[(long)y1 * wl + x1] * se;
        out[p] = v;
        if (out2) out2[p] = v;
    }
}

// sum over the 256 threads in a fixed order: lanes by butterfly, the four waves in ascending order
__device__ __forceinline__ float dg_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// input normalisation + layer 1, one workgroup per patch: patches [n, 1024] -> out NHWC [n, 32, 32, 32] (nullptr: not computed);
// normed optional [n, 1024], the normalised patch.  w [tap][32], bias [32] (the folded BatchNorm)
__global__ __launch_bounds__(256) void dg_layer1_kernel(const float* __restrict__ patches, const float* __restrict__ w, const float* __restrict__ bias, int model,
                                                        const int* __restrict__ live, int n_static, float* __restrict__ out, float* __restrict__ normed) {
    __shared__ float xs[34 * 34];
    __shared__ float sw[9 * 32 + 32];
    __shared__ float red[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i >= (live ? *live : n_static)) return;
    for (int k = tid; k < 34 * 34; k += 256) xs[k] = 0.0f;
    if (out)
        for (int k = tid; k < 9 * 32 + 32; k += 256) sw[k] = k < 9 * 32 ? w[k] : bias[k - 9 * 32];
    const float4 v = *reinterpret_cast<const float4*>(patches + (long)i * DG_PIX + 4 * tid);
    const float mean = dg_block_sum((v.x + v.y) + (v.z + v.w), red) / (float)DG_PIX;
    const float c0 = v.x - mean, c1 = v.y - mean, c2 = v.z - mean, c3 = v.w - mean;
    const float ss = dg_block_sum(fmaf(c3, c3, fmaf(c2, c2, fmaf(c1, c1, c0 * c0))), red);
    float u[4];
    if (model == 1) {  // InstanceNorm2d(1): biased variance, eps 1e-5
        const float r = 1.0f / sqrtf(ss / (float)DG_PIX + 1e-5f);
        u[0] = c0 * r, u[1] = c1 * r, u[2] = c2 * r, u[3] = c3 * r;
    } else {  // HardNet._normalize_input: (x - mean) / (std + 1e-6), unbiased std
        const float d = sqrtf(ss / (float)(DG_PIX - 1)) + 1e-6f;
        u[0] = c0 / d, u[1] = c1 / d, u[2] = c2 / d, u[3] = c3 / d;
    }
    const int py = (4 * tid) >> 5, px0 = (4 * tid) & 31;
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[(py + 1) * 34 + px0 + j + 1] = u[j];
    if (normed) *reinterpret_cast<float4*>(normed + (long)i * DG_PIX + 4 * tid) = make_float4(u[0], u[1], u[2], u[3]);
    __syncthreads();
    if (!out) return;
    for (int p = tid; p < DG_PIX; p += 256) {
        const int y = p >> 5, x = p & 31;
        float win[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) win[ky * 3 + kx] = xs[(y + ky) * 34 + x + kx];
        float* o = out + ((long)i * DG_PIX + p) * 32;
#pragma unroll
        for (int c = 0; c < 32; c += 4) {
            float a[4] = {sw[9 * 32 + c], sw[9 * 32 + c + 1], sw[9 * 32 + c + 2], sw[9 * 32 + c + 3]};
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = fmaf(win[t], sw[t * 32 + c + j], a[j]);
            *reinterpret_cast<float4*>(o + c) = make_float4(fmaxf(a[0], 0.0f), fmaxf(a[1], 0.0f), fmaxf(a[2], 0.0f), fmaxf(a[3], 0.0f));
        }
    }
}

// layer 7's K groups folded in group order, times the weights' 2^-e (exact), then the BatchNorm shift: part [DG_NG][stride rows][128] ->
// fin [n, 128]; one thread per four channels of a row
__global__ __launch_bounds__(256) void dg_fold_kernel(const float* __restrict__ part, const float* __restrict__ shift, const float* __restrict__ wscale, long stride,
                                                      const int* __restrict__ live, int n_static, float* __restrict__ fin) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;  // float4 index in fin
    if (i >= (long)(live ? *live : n_static) * (DG_DIM / 4)) return;
    float4 s = reinterpret_cast<const float4*>(part)[i];
#pragma unroll
    for (int g = 1; g < DG_NG; ++g) {
        const float4 v = reinterpret_cast<const float4*>(part + g * stride * DG_DIM)[i];
        s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
    }
    const float4 b = *reinterpret_cast<const float4*>(shift + 4 * (i % (DG_DIM / 4)));
    const float ws = wscale[0];
    reinterpret_cast<float4*>(fin)[i] = make_float4(__fadd_rn(__fmul_rn(s.x, ws), b.x), __fadd_rn(__fmul_rn(s.y, ws), b.y), __fadd_rn(__fmul_rn(s.z, ws), b.z),
                                                   __fadd_rn(__fmul_rn(s.w, ws), b.w));
}

// output normalisation, one wave per row: fin [n, 128] -> desc [n, 128].  kp / sc / od optional: a row with a non-finite entry is zero
__global__ __launch_bounds__(256) void dg_finish_kernel(const float* __restrict__ fin, int model, const int* __restrict__ live, int n_static,
                                                        const float* __restrict__ kp, const float* __restrict__ sc, const float* __restrict__ od,
                                                        float* __restrict__ desc) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (live ? *live : n_static)) return;  // (wave-uniform)
    float2 v = *reinterpret_cast<const float2*>(fin + (long)i * DG_DIM + 2 * lane);
    if (model == 1) {
        v.x += 1e-10f;
        v.y += 1e-10f;
        const float nrm = sqrtf(wave_sum(fmaf(v.y, v.y, v.x * v.x)));
        v.x /= nrm;
        v.y /= nrm;
    } else {
        const float nrm = fmaxf(sqrtf(wave_sum(fmaf(v.y, v.y, v.x * v.x))), 1e-12f);
        v.x /= nrm;
        v.y /= nrm;
    }
    if (kp && !dg_finite4(kp[2 * i], kp[2 * i + 1], sc[i], od[i])) v = make_float2(0.0f, 0.0f);
    *reinterpret_cast<float2*>(desc + (long)i * DG_DIM + 2 * lane) = v;
}

}  // namespace

// ------------------------------------------------------------------ launch helpers
// level l + 1 [B, h / 2, w / 2] = pyrdown(level l [B, h, w]); tmp: B h w floats
static int dg_pyrdown(imcui_hip_t* h, const float* src, float* tmp, float* dst, int B, int hh, int ww, hipStream_t stream) {
    const int ho = hh / 2, wo = ww / 2;
    const long n = (long)B * hh * ww, no = (long)B * ho * wo;
    hipLaunchKernelGGL(dg_blur_kernel, dim3(blocks_256(n)), dim3(256), 0, stream, src, tmp, hh, ww, n);
    hipLaunchKernelGGL((resize_planar_kernel<bilinear_src_half_pixel, DgResizeLoad>), dim3(blocks_256(no)), dim3(256), 0, stream, tmp, dst, hh, ww, ho, wo,
                       (float)hh / (float)ho, (float)ww / (float)wo, DgResizeLoad{}, no);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// layer i (1 .. 5 = the network's layers 2 .. 6) on n patches: in NHWC [n, hin, hin, cin] -> out [n, hout, hout, cout]; mcnt: device row count
static int dg_conv(imcui_hip_t* h, const float* P, const DgLayout& l, int i, const float* in, int n, float* out, const int* mcnt, hipStream_t stream) {
    const DgLayer& L = DG_LAYERS[i];
    GemmP g;
    g.epi = EPI_CONV;
    g.A = in;
    gemm_set_weights(g, P, l.g[i], L.cout, 9 * L.cin, h->precision == 1);
    gemm_set_conv(g, 3, L.stride, 1, L.hin, L.hin, L.hout, L.hout, L.cin);
    g.M = n * L.hout * L.hout;
    g.C = out;
    g.ldc = L.cout;
    g.act = 1;
    g.mcnt = mcnt;
    return gemm_launch(h, g, stream);
}
// layer 7: in [n, 8192] -> out [n, 128].  ONE batched GEMM launch computes the DG_NG partial products side by side (batch z = K group z:
// columns [DG_KG z, ..) of the activations and of the weights, no bias) into part [DG_NG][n][128]; dg_fold_kernel adds them in group order
// and then the BatchNorm shift.  (The groups as a chain of 8 launches through the epilogue's residual input had 8 workgroups per launch
// at n = 1024 and took 38 % of the descriptor stage.)  The weights are the float32 matrix in both modes: the split arithmetic splits
// the B operand as it is read, since per-batch offsets exist for W and not for pre-split planes; the matrix is packed times a power
// of two for that (DgLayout).
static int dg_final(imcui_hip_t* h, const float* P, const DgLayout& l, const float* in, int n, float* part, float* out, const int* mcnt, hipStream_t stream) {
    int rc;
    GemmP p;
    p.epi = EPI_BIAS;
    p.A = in;
    p.lda = DG_KF;
    p.a_bs = DG_KG;
    p.W = P + l.wf;
    p.ldw = DG_KF;
    p.w_bs = DG_KG;
    p.N = DG_DIM;
    p.K = DG_KG;
    p.M = n;
    p.C = part;
    p.ldc = DG_DIM;
    p.c_bs = (long)n * DG_DIM;
    p.batch = DG_NG;
    p.mcnt = mcnt;
    p.cnt_stride = 0;  // every group has the chunk's row count
    IMCUI_RUN(gemm_launch(h, p, stream));
    hipLaunchKernelGGL(dg_fold_kernel, dim3(cdiv(n * (DG_DIM / 4), 256)), dim3(256), 0, stream, part, P + l.bf, P + l.fs, (long)n, mcnt, n, out);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ workspace
struct DgWs {
    float *pyr, *tmp, *patch, *fa, *fb, *fin;
    int *mc, *status;
    size_t total;
    bool ok;
};
static DgWs dg_carve(void* ws, size_t bytes, size_t pyr_floats, size_t tmp_floats, int chunk, int nmc) {
    WsAlloc a(ws, bytes);
    DgWs s;
    s.pyr = a.get<float>(pyr_floats);
    s.tmp = a.get<float>(tmp_floats);
    s.patch = a.get<float>((size_t)chunk * DG_PIX);
    s.fa = a.get<float>((size_t)chunk * DG_PIX * 32);
    s.fb = a.get<float>((size_t)chunk * DG_PIX * 32);
    s.fin = a.get<float>((size_t)chunk * DG_DIM);
    s.mc = a.get<int>((size_t)nmc * 4);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}
// patches [n, 1024] -> fin [n, 128] (before the output normalisation); mc: the chunk's four live-row counts on the device, or nullptr
static int dg_net(imcui_hip_t* h, const float* P, const DgLayout& l, int model, int n, const DgWs& s, const int* mc, hipStream_t stream) {
    int rc;
    hipLaunchKernelGGL(dg_layer1_kernel, dim3(n), dim3(256), 0, stream, s.patch, P + l.w0, P + l.b0, model, mc ? mc + 3 : nullptr, n, s.fa, (float*)nullptr);
    IMCUI_CHECK_LAUNCH(h);
    IMCUI_RUN(dg_conv(h, P, l, 1, s.fa, n, s.fb, mc, stream));
    IMCUI_RUN(dg_conv(h, P, l, 2, s.fb, n, s.fa, mc ? mc + 1 : nullptr, stream));
    IMCUI_RUN(dg_conv(h, P, l, 3, s.fa, n, s.fb, mc ? mc + 1 : nullptr, stream));
    IMCUI_RUN(dg_conv(h, P, l, 4, s.fb, n, s.fa, mc ? mc + 2 : nullptr, stream));
    IMCUI_RUN(dg_conv(h, P, l, 5, s.fa, n, s.fb, mc ? mc + 2 : nullptr, stream));
    return dg_final(h, P, l, s.fb, n, s.fa, s.fin, mc ? mc + 3 : nullptr, stream);  // (s.fa is free: the partial products park there)
}

static bool dg_shape_ok(int B, int H, int W) { return B >= 1 && B <= 1024 && H >= 8 && W >= 8 && (long)B * H * W <= 0x7fffffffL / 4; }

extern "C" size_t imcui_hip_patchdesc_workspace_bytes(int B, int H, int W, int kcap, int chunk) {
    if (!dg_shape_ok(B, H, W) || kcap < 1 || chunk < 1 || chunk > DG_MAXCHUNK) return 0;
    size_t pyr;
    dg_levels(B, H, W, &pyr);
    return dg_carve(nullptr, 0, pyr, (size_t)B * H * W, chunk, B * cdiv(kcap, chunk)).total;
}

extern "C" int imcui_hip_patchdesc_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, const float* keypoints,
                                           const float* scales, const float* oris_deg, const int* num_keypoints, int kcap, int model, float mr_size, int chunk,
                                           float* descriptors, int* status, float* dbg_patches, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (model != 0 && model != 1) return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc: model %d (0 = hardnet, 1 = sosnet)", model);
    if (!dg_shape_ok(B, H, W)) return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc: B=%d images of %dx%d: 1..1024 images of at least 8x8, B H W below 2^29", B, H, W);
    if (kcap < 1 || chunk < 1 || chunk > DG_MAXCHUNK || (long)B * kcap > 0x7fffffffL / DG_PIX)
        return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc: kcap=%d, chunk=%d (1..%d), B kcap below 2^21", kcap, chunk, DG_MAXCHUNK);
    if (!(mr_size > 0.0f) || !std::isfinite(mr_size)) return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc: mr_size must be positive and finite");
    if (!packed || !image || !keypoints || !scales || !oris_deg || !num_keypoints || !descriptors) return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc: null argument");
    const int nchunk = cdiv(kcap, chunk);
    size_t pyr;
    const DgLevels lv = dg_levels(B, H, W, &pyr);
    const DgWs s = dg_carve(ws, ws_bytes, pyr, (size_t)B * H * W, chunk, B * nchunk);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "patchdesc: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const DgLayout l = dg_layout();
    int* st = status ? status : s.status;
    int rc;
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, st, 1);
    hipLaunchKernelGGL(dg_count_kernel, dim3(cdiv(B * nchunk, 256)), dim3(256), 0, stream, num_keypoints, B, nchunk, chunk, kcap, s.mc, st);
    IMCUI_CHECK_LAUNCH(h);
    for (int lev = 1; lev < lv.n; ++lev)
        IMCUI_RUN(dg_pyrdown(h, lev == 1 ? image : s.pyr + lv.off[lev - 1], s.tmp, s.pyr + lv.off[lev], B, lv.h[lev - 1], lv.w[lev - 1], stream));
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < nchunk; ++c) {
            const int n = std::min(chunk, kcap - c * chunk);
            const int* mc = s.mc + 4 * ((size_t)b * nchunk + c);
            const size_t row = (size_t)b * kcap + (size_t)c * chunk;
            const float *kp = keypoints + 2 * row, *sc = scales + row, *od = oris_deg + row;
            hipLaunchKernelGGL(dg_sample_kernel, dim3(n), dim3(256), 0, stream, image + (size_t)b * H * W, s.pyr, lv, b, kp, sc, od, mc + 3, n, mr_size, s.patch,
                               dbg_patches ? dbg_patches + row * DG_PIX : (float*)nullptr, st);
            IMCUI_CHECK_LAUNCH(h);
            IMCUI_RUN(dg_net(h, packed, l, model, n, s, mc, stream));
            hipLaunchKernelGGL(dg_finish_kernel, dim3(cdiv(n, 4)), dim3(256), 0, stream, s.fin, model, mc + 3, n, kp, sc, od, descriptors + row * DG_DIM);
            IMCUI_CHECK_LAUNCH(h);
        }
    return IMCUI_OK;
}

// ------------------------------------------------------------------ test entries
// test entry: dog.py:88-98 alone on ONE image [dev, H,W]: n key-points -> patches [dev, n,1024]
extern "C" size_t imcui_hip_patchdesc_patch_probe_workspace_bytes(int H, int W) {
    if (!dg_shape_ok(1, H, W)) return 0;
    size_t pyr;
    dg_levels(1, H, W, &pyr);
    return align_up(pyr * sizeof(float), 256) + align_up((size_t)H * W * sizeof(float), 256) + 256;
}
extern "C" int imcui_hip_patchdesc_patch_probe(imcui_hip_t* h, const float* image, int H, int W, const float* keypoints, const float* scales, const float* oris_deg,
                                               int n, float mr_size, float* patches, int* status, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (!dg_shape_ok(1, H, W) || n < 1 || n > (1 << 20) || !image || !keypoints || !scales || !oris_deg || !patches || !status)
        return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc patch probe: %dx%d, n=%d or a null argument", H, W, n);
    size_t pyr;
    const DgLevels lv = dg_levels(1, H, W, &pyr);
    WsAlloc a(ws, ws_bytes);
    float* pb = a.get<float>(pyr);
    float* tmp = a.get<float>((size_t)H * W);
    if (!ws || !a.ok) return imcui_set_err(h, IMCUI_ERR_WS, "patchdesc patch probe: workspace too small (%zu < %zu)", ws_bytes, a.off);
    int rc;
    hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, status, 1);
    for (int lev = 1; lev < lv.n; ++lev) IMCUI_RUN(dg_pyrdown(h, lev == 1 ? image : pb + lv.off[lev - 1], tmp, pb + lv.off[lev], 1, lv.h[lev - 1], lv.w[lev - 1], stream));
    hipLaunchKernelGGL(dg_sample_kernel, dim3(n), dim3(256), 0, stream, image, pb, lv, 0, keypoints, scales, oris_deg, (const int*)nullptr, n, mr_size, patches,
                       (float*)nullptr, status);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_patchdesc_probe_workspace_bytes(int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1) return 0;
    return 256 + align_up((size_t)n * std::max((size_t)H * W, (size_t)DG_NG * DG_DIM) * sizeof(float), 256);  // pyrdown's blur, or layer 7's partial products
}
// test entry: one launch alone on n rows.  op 0: pyrdown, in [n, H, W] -> out [n, H / 2, W / 2] (workspace: n H W floats); op 1: the input
// normalisation, [n, 1024] -> [n, 1024]; op 2: normalisation + layer 1, [n, 1024] -> [n, 32, 32, 32]; ops 3 .. 7: layers 2 .. 6 alone,
// NHWC in -> NHWC out; op 8: layer 7 with the folded shift, [n, 8192] -> [n, 128]; op 9: the output normalisation, [n, 128] -> [n, 128]
extern "C" int imcui_hip_patchdesc_layer_probe(imcui_hip_t* h, int op, int model, const float* packed, const float* in, int n, int H, int W, float* out, void* ws,
                                               size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (n < 1 || n > DG_MAXCHUNK || !in || !out || (model != 0 && model != 1)) return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc layer probe: n=%d (1..%d), model %d", n, DG_MAXCHUNK, model);
    if (op != 0 && op != 1 && op != 9 && !packed) return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc layer probe: op %d needs the packed weights", op);
    const DgLayout l = dg_layout();
    if (op == 0 && (H < 3 || W < 3 || (long)n * H * W > 0x7fffffffL / 4)) return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc layer probe: pyrdown of %d planes of %dx%d", n, H, W);
    const size_t need = imcui_hip_patchdesc_probe_workspace_bytes(n, op == 0 ? H : 1, op == 0 ? W : 1);
    if (!ws || ws_bytes < need) return imcui_set_err(h, IMCUI_ERR_WS, "patchdesc layer probe: workspace too small (%zu < %zu)", ws_bytes, need);
    int* mc = (int*)ws;  // the live-row counts are read on the device, as in the forward: the same kernel instantiations run
    hipLaunchKernelGGL(dg_full_kernel, dim3(1), dim3(64), 0, stream, mc, n);
    if (op == 0) {
        return dg_pyrdown(h, in, (float*)((char*)ws + 256), out, n, H, W, stream);
    } else if (op == 1 || op == 2) {
        hipLaunchKernelGGL(dg_layer1_kernel, dim3(n), dim3(256), 0, stream, in, op == 2 ? packed + l.w0 : (const float*)nullptr,
                           op == 2 ? packed + l.b0 : (const float*)nullptr, model, mc + 3, n, op == 2 ? out : (float*)nullptr, op == 1 ? out : (float*)nullptr);
    } else if (op >= 3 && op <= 7) {
        return dg_conv(h, packed, l, op - 2, in, n, out, mc + (op <= 3 ? 0 : op <= 5 ? 1 : 2), stream);
    } else if (op == 8) {
        return dg_final(h, packed, l, in, n, (float*)((char*)ws + 256), out, mc + 3, stream);
    } else if (op == 9) {
        hipLaunchKernelGGL(dg_finish_kernel, dim3(cdiv(n, 4)), dim3(256), 0, stream, in, model, mc + 3, n, (const float*)nullptr, (const float*)nullptr,
                           (const float*)nullptr, out);
    } else {
        return imcui_set_err(h, IMCUI_ERR_ARG, "patchdesc layer probe: op %d", op);
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
