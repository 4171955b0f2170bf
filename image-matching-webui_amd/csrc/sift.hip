// SIFT (OpenCV 4.x semantics, float pipeline) on MI355X: replaces `SIFT._forward` -> `extract_single_image` -> `run_opencv_sift`
// (imcui/hloc/extractors/sift.py:61-78,139-216, backend "opencv": cv2.SIFT_create(contrastThreshold, nfeatures, edgeThreshold,
// nOctaveLayers).detectAndCompute), `filter_dog_point` (:19-52), the score top-k (:188-193) and `sift_to_rootsift` (:55-58).
//
// Stages (every grid is sized by shapes or capacities, every count stays on the device: no host synchronisation):
//   sf_gray_up_kernel   gray (0.299 / 0.587 / 0.114 in float, each operation rounded), `(x * 255).astype(uint8)`, 2x INTER_LINEAR
//   sf_blur_kernel      separable Gaussian, rows then columns in ONE launch through an LDS tile with halo, BORDER_REFLECT_101 reflected
//                       repeatedly; the whole batch in one grid; every level is blurred from the previous level
//   sf_down_kernel      next octave = every second pixel of level `layers`
//   sf_extrema_kernel   26-neighbour extrema of the DoG (formed on the fly: L[i+1] - L[i] in fp32 is the stored DoG bit for bit); one
//                       ballot word per wave + one count per workgroup, then exclusive_scan_kernel (select.h) + sf_compact_kernel: the candidate list
//                       is in (octave, layer, row, column) order by construction (count + scan, no sort, no float atomics)
//   sf_refine_kernel    adjustLocalExtrema: up to 5 Newton steps, contrast and edge tests; one thread per candidate
//   sf_orient_kernel    36-bin orientation histogram, one wave per candidate (capped grid, workgroups walk the list), a private histogram per lane in LDS summed in lane order
//   sf_expand_kernel    one table row per (candidate, histogram peak): the key-point table in OpenCV's detection order
//   sf_sel_kernel<M>    removeDuplicated, retainBest(nfeatures), filter_dog_point (pixel maximum, lowest |angle|, NMS), top-k: each an
//                       all-pairs pass over the table (exact float comparisons, ties to the lower row)
//   sf_final_kernel     survivors in table order -- NOT sorted by score, like DISK and ALIKED (cv2's own order depends on its thread pool;
//                       the reference re-orders by score only when the top-k cuts)
//   sf_desc_kernel      4x4x8 gradient histogram, one wave per key-point, private histograms per lane, 0..255 integers, RootSIFT
// The angle of a gradient is atan2 (not cv2's fastAtan2 polynomial); the BIN of an orientation-histogram sample is decided in float64 so
// that the float64 restatement (tests/sift_reference.py) takes the same discrete decisions.  Results are bitwise reproducible: an
// image's outputs do not depend on its batch or on scheduling.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "common.h"
#include "imcui_hip.h"
#include "select.h"

#define SF_MAX_OCT 16
#define SF_BORDER 5
#define SF_MAXR 13  // blur radius at 3 layers (level 5: sigma 3.09)
#define SF_TW 64
#define SF_TH 16
#define SF_MAXP 18  // strict local maxima of a circular 36-bin histogram
#define SF_REC 16   // floats per refined candidate
#define SF_TAB 12   // floats per table row
#define SF_HS 65   // row stride of the per-lane histograms in LDS: 64 lanes + 1, so that the final per-bin sums (lane = bin) spread over the banks
#define SF_MAXWG 8192  // single-wave workgroups per image of the orientation / descriptor grids (256 CUs x 32: enough to fill the part at batch 1)
#define SF_EPS 1.1920929e-07f

struct SfGeom {
    int nOct, layers, L;
    int h[SF_MAX_OCT], w[SF_MAX_OCT];
    long pyr_off[SF_MAX_OCT];  // float offset of octave o: a block [B][L][h][w]
    unsigned px_off[SF_MAX_OCT + 1];  // offsets of the octaves in one image's search index space (layers x h x w each)
    long pyr_total;
};
struct SfTaps {
    float t[2 * SF_MAXR + 1];
    int r;
};

extern "C" int imcui_hip_sift_num_octaves(int H, int W) {
    if (H < 1 || W < 1) return 0;
    const int n = (int)rint(log2((double)(2 * (H < W ? H : W))) - 2.0) + 1;
    return n < 1 ? 1 : (n > SF_MAX_OCT ? SF_MAX_OCT : n);
}

static SfGeom sf_geom(int B, int H, int W, int layers) {
    SfGeom g;
    memset(&g, 0, sizeof(g));
    g.nOct = imcui_hip_sift_num_octaves(H, W);
    g.layers = layers;
    g.L = layers + 3;
    long off = 0;
    unsigned long px = 0;
    int h = 2 * H, w = 2 * W;
    for (int o = 0; o < g.nOct; ++o) {
        g.h[o] = h;
        g.w[o] = w;
        g.pyr_off[o] = off;
        g.px_off[o] = (unsigned)px;
        off += (long)B * g.L * h * w;
        px += (unsigned long)layers * h * w;
        h /= 2;
        w /= 2;
        if (h < 1 || w < 1) {
            g.nOct = o + 1;
            break;
        }
    }
    g.px_off[g.nOct] = (unsigned)px;
    g.pyr_total = off;
    return g;
}

extern "C" size_t imcui_hip_sift_pyramid_floats(int B, int H, int W, int layers) {
    if (B <= 0 || H < 8 || W < 8 || layers < 3 || layers > 5) return 0;
    return (size_t)sf_geom(B, H, W, layers).pyr_total;
}

static SfTaps sf_taps(double sigma) {
    SfTaps t;
    memset(&t, 0, sizeof(t));
    int ks = (int)rint(8.0 * sigma + 1.0) | 1;
    int r = ks / 2;
    if (r > SF_MAXR) r = SF_MAXR;  // (not reached for 3..5 layers)
    double k[2 * SF_MAXR + 1], s = 0.0;
    for (int i = -r; i <= r; ++i) {
        k[i + r] = exp(-((double)i * i) / (2.0 * sigma * sigma));
        s += k[i + r];
    }
    for (int i = 0; i <= 2 * r; ++i) t.t[i] = (float)(k[i] / s);
    t.r = r;
    return t;
}

__device__ __forceinline__ int sf_reflect(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// ------------------------------------------------------------------ base image
__device__ __forceinline__ float sf_u8(const float* img, int C, long plane, long idx) {
    float v;
    if (C == 3) {
        const float r = img[idx], g = img[plane + idx], b = img[2 * plane + idx];
        v = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, r), __fmul_rn(0.587f, g)), __fmul_rn(0.114f, b));
    } else {
        v = img[idx];
    }
    v = __fmul_rn(v, 255.0f);
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    return (float)(int)v;
}
__global__ __launch_bounds__(256) void sf_gray_up_kernel(const float* __restrict__ image, int C, int H, int W, float* __restrict__ up) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= 2 * W || y >= 2 * H) return;
    const long plane = (long)H * W;
    const float* img = image + (long)b * C * plane;
    float fx = (x + 0.5f) * 0.5f - 0.5f, fy = (y + 0.5f) * 0.5f - 0.5f;
    int sx = (int)floorf(fx), sy = (int)floorf(fy);
    fx -= sx;
    fy -= sy;
    if (sx < 0) sx = 0, fx = 0.f;
    if (sx >= W - 1) sx = W - 1, fx = 0.f;
    if (sy < 0) sy = 0, fy = 0.f;
    if (sy >= H - 1) sy = H - 1, fy = 0.f;
    const int sx1 = min(sx + 1, W - 1), sy1 = min(sy + 1, H - 1);
    const float a00 = sf_u8(img, C, plane, (long)sy * W + sx), a01 = sf_u8(img, C, plane, (long)sy * W + sx1);
    const float a10 = sf_u8(img, C, plane, (long)sy1 * W + sx), a11 = sf_u8(img, C, plane, (long)sy1 * W + sx1);
    // weights are multiples of 1/4 and the samples integers below 256: every product and sum is exact
    const float h0 = a00 * (1.f - fx) + a01 * fx, h1 = a10 * (1.f - fx) + a11 * fx;
    up[((long)b * 2 * H + y) * 2 * W + x] = h0 * (1.f - fy) + h1 * fy;
}

// ------------------------------------------------------------------ Gaussian blur: rows, then columns, one launch
__global__ __launch_bounds__(256) void sf_blur_kernel(const float* __restrict__ src, long src_img, float* __restrict__ dst, long dst_img, int h, int w,
                                                       SfTaps taps) {
    __shared__ float s_in[(SF_TH + 2 * SF_MAXR) * (SF_TW + 2 * SF_MAXR)];
    __shared__ float s_mid[(SF_TH + 2 * SF_MAXR) * SF_TW];
    const int r = taps.r, ih = SF_TH + 2 * r, iw = SF_TW + 2 * r;
    const int x0 = blockIdx.x * SF_TW, y0 = blockIdx.y * SF_TH;
    const float* s = src + (long)blockIdx.z * src_img;
    for (int i = threadIdx.x; i < ih * iw; i += 256) {
        const int ty = i / iw, tx = i - ty * iw;
        s_in[i] = s[(long)sf_reflect(y0 + ty - r, h) * w + sf_reflect(x0 + tx - r, w)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ih * SF_TW; i += 256) {
        const int ty = i / SF_TW, tx = i - ty * SF_TW;
        const float* p = s_in + ty * iw + tx;
        float acc = taps.t[0] * p[0];
        for (int k = 1; k <= 2 * r; ++k) acc = fmaf(taps.t[k], p[k], acc);
        s_mid[i] = acc;
    }
    __syncthreads();
    float* d = dst + (long)blockIdx.z * dst_img;
    for (int i = threadIdx.x; i < SF_TH * SF_TW; i += 256) {
        const int ty = i / SF_TW, tx = i - ty * SF_TW;
        if (y0 + ty >= h || x0 + tx >= w) continue;
        const float* p = s_mid + ty * SF_TW + tx;
        float acc = taps.t[0] * p[0];
        for (int k = 1; k <= 2 * r; ++k) acc = fmaf(taps.t[k], p[k * SF_TW], acc);
        d[(long)(y0 + ty) * w + x0 + tx] = acc;
    }
}

__global__ __launch_bounds__(256) void sf_down_kernel(const float* __restrict__ src, long src_img, int sw, float* __restrict__ dst, long dst_img, int h, int w) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    dst[(long)blockIdx.z * dst_img + (long)y * w + x] = src[(long)blockIdx.z * src_img + (long)(2 * y) * sw + 2 * x];
}

// ------------------------------------------------------------------ extrema
struct SfPos {
    int o, l, r, c;
};
__device__ __forceinline__ SfPos sf_decode(const SfGeom& g, unsigned i) {
    SfPos p;
    int o = 0;
    while (o + 1 < g.nOct && i >= g.px_off[o + 1]) ++o;
    const unsigned q = i - g.px_off[o];
    const unsigned lvl = (unsigned)g.h[o] * g.w[o];
    p.o = o;
    p.l = 1 + (int)(q / lvl);
    const unsigned rem = q % lvl;
    p.r = (int)(rem / g.w[o]);
    p.c = (int)(rem % g.w[o]);
    return p;
}
// level 0 of image b in octave o
__device__ __forceinline__ const float* sf_oct(const float* pyr, const SfGeom& g, int b, int o) {
    return pyr + g.pyr_off[o] + (long)b * g.L * g.h[o] * g.w[o];
}
#define SF_D(P, lvl, w, l, r, c) ((P)[(long)((l) + 1) * (lvl) + (long)(r) * (w) + (c)] - (P)[(long)(l) * (lvl) + (long)(r) * (w) + (c)])

__global__ __launch_bounds__(1024) void sf_extrema_kernel(const float* __restrict__ pyr, SfGeom g, float thr, unsigned long long* __restrict__ bits,
                                                           int* __restrict__ wgcnt, int nwg) {
    __shared__ int s_cnt[16];
    const int b = blockIdx.y;
    const unsigned i = blockIdx.x * 1024u + threadIdx.x;
    bool ext = false;
    if (i < g.px_off[g.nOct]) {
        const SfPos p = sf_decode(g, i);
        const int h = g.h[p.o], w = g.w[p.o];
        if (p.r >= SF_BORDER && p.r < h - SF_BORDER && p.c >= SF_BORDER && p.c < w - SF_BORDER) {
            const float* P = sf_oct(pyr, g, b, p.o);
            const long lvl = (long)h * w;
            const float v = SF_D(P, lvl, w, p.l, p.r, p.c);
            if (fabsf(v) > thr) {
                bool ge = true, le = true;
                for (int dl = -1; dl <= 1; ++dl)
                    for (int dr = -1; dr <= 1; ++dr)
                        for (int dc = -1; dc <= 1; ++dc) {
                            const float n = SF_D(P, lvl, w, p.l + dl, p.r + dr, p.c + dc);
                            ge = ge && v >= n;
                            le = le && v <= n;
                        }
                ext = (v > 0.f && ge) || (v < 0.f && le);
            }
        }
    }
    const unsigned long long m = __ballot(ext);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        bits[(long)b * nwg * 16 + (long)blockIdx.x * 16 + wave] = m;
        s_cnt[wave] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < 16; ++k) t += s_cnt[k];
        wgcnt[(long)b * nwg + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void sf_compact_kernel(const unsigned long long* __restrict__ bits, const int* __restrict__ wgoff, int nwg, unsigned total_px,
                                                           int ccap, int* __restrict__ cand) {
    const int b = blockIdx.y;
    const unsigned i = blockIdx.x * 1024u + threadIdx.x;
    if (i >= total_px) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long* wb = bits + (long)b * nwg * 16 + (long)blockIdx.x * 16;
    const unsigned long long m = wb[wave];
    if (!((m >> lane) & 1ull)) return;
    int slot = wgoff[(long)b * nwg + blockIdx.x];
    for (int k = 0; k < wave; ++k) slot += __popcll(wb[k]);
    slot += __popcll(m & ((1ull << lane) - 1ull));
    if (slot < ccap) cand[(long)b * ccap + slot] = (int)i;
}

// ------------------------------------------------------------------ refinement (adjustLocalExtrema)
__device__ __forceinline__ void sf_swap4(float* a, float* b) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = a[k];
        a[k] = b[k];
        b[k] = t;
    }
}
// H X = g by Gaussian elimination with partial pivoting; false when a pivot is below FLT_EPSILON
__device__ __forceinline__ bool sf_solve3(float A[3][4], float& x0, float& x1, float& x2) {
    if (fabsf(A[1][0]) > fabsf(A[0][0])) sf_swap4(A[0], A[1]);
    if (fabsf(A[2][0]) > fabsf(A[0][0])) sf_swap4(A[0], A[2]);
    if (fabsf(A[0][0]) < SF_EPS) return false;
    float f = A[1][0] / A[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) A[1][k] -= f * A[0][k];
    f = A[2][0] / A[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) A[2][k] -= f * A[0][k];
    if (fabsf(A[2][1]) > fabsf(A[1][1])) sf_swap4(A[1], A[2]);
    if (fabsf(A[1][1]) < SF_EPS) return false;
    f = A[2][1] / A[1][1];
#pragma unroll
    for (int k = 2; k < 4; ++k) A[2][k] -= f * A[1][k];
    if (fabsf(A[2][2]) < SF_EPS) return false;
    x2 = A[2][3] / A[2][2];
    x1 = (A[1][3] - A[1][2] * x2) / A[1][1];
    x0 = (A[0][3] - A[0][2] * x2 - A[0][1] * x1) / A[0][0];
    return true;
}

__global__ __launch_bounds__(256) void sf_refine_kernel(const float* __restrict__ pyr, SfGeom g, const int* __restrict__ cand, const int* __restrict__ ncand,
                                                         int ccap, float contrast, float edge, float* __restrict__ rec, int* __restrict__ status) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0 && ncand[b] > ccap) atomicOr(status, 2);
    if (j >= min(ncand[b], ccap)) return;
    const SfPos p = sf_decode(g, (unsigned)cand[(long)b * ccap + j]);
    const int h = g.h[p.o], w = g.w[p.o];
    const long lvl = (long)h * w;
    const float* P = sf_oct(pyr, g, b, p.o);
    int l = p.l, r = p.r, c = p.c;
    const float is = 1.f / 255.f, ds = is * 0.5f, cs = is * 0.25f;
    float xc = 0.f, xr = 0.f, xi = 0.f, gx = 0.f, gy = 0.f, gs = 0.f, dxx = 0.f, dyy = 0.f, dxy = 0.f, v = 0.f;
    bool ok = true;
    int it = 0;
    for (; it < 5; ++it) {
        v = SF_D(P, lvl, w, l, r, c);
        const float cl = SF_D(P, lvl, w, l, r, c - 1), cr = SF_D(P, lvl, w, l, r, c + 1);
        const float ru = SF_D(P, lvl, w, l, r - 1, c), rd = SF_D(P, lvl, w, l, r + 1, c);
        const float sp = SF_D(P, lvl, w, l - 1, r, c), sn = SF_D(P, lvl, w, l + 1, r, c);
        gx = (cr - cl) * ds;
        gy = (rd - ru) * ds;
        gs = (sn - sp) * ds;
        const float v2 = v * 2.f;
        dxx = (cr + cl - v2) * is;
        dyy = (rd + ru - v2) * is;
        const float dss = (sn + sp - v2) * is;
        dxy = (SF_D(P, lvl, w, l, r + 1, c + 1) - SF_D(P, lvl, w, l, r + 1, c - 1) - SF_D(P, lvl, w, l, r - 1, c + 1) + SF_D(P, lvl, w, l, r - 1, c - 1)) * cs;
        const float dxs = (SF_D(P, lvl, w, l + 1, r, c + 1) - SF_D(P, lvl, w, l + 1, r, c - 1) - SF_D(P, lvl, w, l - 1, r, c + 1) + SF_D(P, lvl, w, l - 1, r, c - 1)) * cs;
        const float dys = (SF_D(P, lvl, w, l + 1, r + 1, c) - SF_D(P, lvl, w, l + 1, r - 1, c) - SF_D(P, lvl, w, l - 1, r + 1, c) + SF_D(P, lvl, w, l - 1, r - 1, c)) * cs;
        float A[3][4] = {{dxx, dxy, dxs, gx}, {dxy, dyy, dys, gy}, {dxs, dys, dss, gs}};
        float x0, x1, x2;
        if (!sf_solve3(A, x0, x1, x2)) {
            ok = false;
            break;
        }
        xc = -x0;
        xr = -x1;
        xi = -x2;
        if (fabsf(xc) < 0.5f && fabsf(xr) < 0.5f && fabsf(xi) < 0.5f) break;
        if (!(fabsf(xc) < 7e8f && fabsf(xr) < 7e8f && fabsf(xi) < 7e8f)) {  // INT_MAX / 3 (also NaN)
            ok = false;
            break;
        }
        c += (int)rintf(xc);
        r += (int)rintf(xr);
        l += (int)rintf(xi);
        if (l < 1 || l > g.layers || c < SF_BORDER || c >= w - SF_BORDER || r < SF_BORDER || r >= h - SF_BORDER) {
            ok = false;
            break;
        }
    }
    if (it >= 5) ok = false;
    float contr = 0.f, eq = 0.f, det = 0.f;
    if (ok) {
        const float t = gx * xc + gy * xr + gs * xi;
        contr = v * is + t * 0.5f;
        if (fabsf(contr) * g.layers < contrast) ok = false;
        const float tr = dxx + dyy;
        det = dxx * dyy - dxy * dxy;
        eq = tr * tr * edge - (edge + 1.f) * (edge + 1.f) * det;
        if (det <= 0.f || eq >= 0.f) ok = false;
    }
    float* o = rec + ((long)b * ccap + j) * SF_REC;
    const float sc = (float)(1 << p.o);
    o[0] = ok ? 1.f : 0.f;
    o[1] = (float)p.o;
    o[2] = (float)l;
    o[3] = (float)r;
    o[4] = (float)c;
    o[5] = xc;
    o[6] = xr;
    o[7] = xi;
    o[8] = contr;
    o[9] = 1.6f * powf(2.f, ((float)l + xi) / (float)g.layers) * sc * 2.f;
    o[10] = ((float)c + xc) * sc;
    o[11] = ((float)r + xr) * sc;
    o[12] = eq;
    o[13] = det;
    o[14] = 0.f;
    o[15] = 0.f;
}

// ------------------------------------------------------------------ orientation histogram: one wave per candidate
__global__ __launch_bounds__(64) void sf_orient_kernel(const float* __restrict__ pyr, SfGeom g, const float* __restrict__ rec, const int* __restrict__ ncand, int ccap,
                                                        int* __restrict__ npeaks, float* __restrict__ peaks, float* __restrict__ dbg_hist) {
    __shared__ float hh[36 * SF_HS];
    __shared__ float raw[36], sm[36];
    const int b = blockIdx.y, lane = threadIdx.x;
    const int n = min(ncand[b], ccap);
    for (int j = blockIdx.x; j < n; j += gridDim.x) {  // (the grid is capped: a workgroup walks candidates j, j + grid, ...)
    const float* q = rec + ((long)b * ccap + j) * SF_REC;
    if (q[0] == 0.f) {
        if (lane == 0) npeaks[(long)b * ccap + j] = 0;
        continue;
    }
    const int o = (int)q[1], l = (int)q[2], r = (int)q[3], c = (int)q[4];
    const int h = g.h[o], w = g.w[o];
    const float* img = sf_oct(pyr, g, b, o) + (long)l * h * w;
    const float scl = q[9] * 0.5f / (float)(1 << o);
    const int radius = max(0, min((int)rintf(4.5f * scl), max(h, w)));  // (the window is clipped to the image anyway)
    const float sigma = 1.5f * scl, es = -1.f / (2.f * sigma * sigma);
    for (int k = 0; k < 36; ++k) hh[k * SF_HS + lane] = 0.f;
    const int side = 2 * radius + 1, total = side * side;
    for (int k = lane; k < total; k += 64) {
        const int i = k / side - radius, jj = k % side - radius;
        const int y = r + i, x = c + jj;
        if (y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) continue;
        const float xr_ = img[(long)y * w + x + 1], xl_ = img[(long)y * w + x - 1], yu = img[(long)(y - 1) * w + x], yd = img[(long)(y + 1) * w + x];
        const float dx = xr_ - xl_, dy = yu - yd;
        const float wgt = expf((float)(i * i + jj * jj) * es);
        const float mag = sqrtf(dx * dx + dy * dy);
        double ang = atan2((double)yu - (double)yd, (double)xr_ - (double)xl_) * 57.29577951308232;
        if (ang < 0.0) ang += 360.0;
        int bin = (int)rint(ang * 0.1);
        if (bin >= 36) bin -= 36;
        bin = min(max(bin, 0), 35);  // (only a non-finite pyramid value could get here)
        hh[bin * SF_HS + lane] += wgt * mag;
    }
    __syncthreads();
    if (lane < 36) {
        float s = 0.f;
        for (int k = 0; k < 64; ++k) s += hh[lane * SF_HS + k];
        raw[lane] = s;
    }
    __syncthreads();
    float hv = 0.f;
    if (lane < 36) {
        const float m2 = raw[(lane + 34) % 36], m1 = raw[(lane + 35) % 36], p1 = raw[(lane + 1) % 36], p2 = raw[(lane + 2) % 36];
        hv = (m2 + p2) * (1.f / 16.f) + (m1 + p1) * (4.f / 16.f) + raw[lane] * (6.f / 16.f);
        sm[lane] = hv;
        if (dbg_hist) dbg_hist[((long)b * ccap + j) * 36 + lane] = hv;
    }
    __syncthreads();
    const float mx = wave_max(lane < 36 ? hv : 0.f);
    const float thr = mx * 0.8f;
    bool pk = false;
    float ang = 0.f;
    if (lane < 36) {
        const float hl = sm[(lane + 35) % 36], hr = sm[(lane + 1) % 36];
        pk = hv > hl && hv > hr && hv >= thr;
        if (pk) {
            float bn = (float)lane + 0.5f * (hl - hr) / (hl - 2.f * hv + hr);
            bn = bn < 0.f ? 36.f + bn : (bn >= 36.f ? bn - 36.f : bn);
            ang = 360.f - 10.f * bn;
            if (fabsf(ang - 360.f) < SF_EPS) ang = 0.f;
        }
    }
    int npk;
    const int slot = wave_ordered_rank(pk, &npk);
    if (pk) peaks[((long)b * ccap + j) * SF_MAXP + slot] = ang;
    if (lane == 0) npeaks[(long)b * ccap + j] = npk;
    __syncthreads();  // the LDS histograms are re-used by the next candidate
    }
}

// one table row per (candidate, peak), in candidate order then bin order
__global__ __launch_bounds__(256) void sf_expand_kernel(const float* __restrict__ rec, const int* __restrict__ ncand, const int* __restrict__ npeaks,
                                                         const int* __restrict__ tabofs, const int* __restrict__ ntab, const float* __restrict__ peaks, int ccap,
                                                         float* __restrict__ table, int* __restrict__ status) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0 && ntab[b] > ccap) atomicOr(status, 2);
    if (j >= min(ncand[b], ccap)) return;
    const int n = npeaks[(long)b * ccap + j], ofs = tabofs[(long)b * ccap + j];
    const float* q = rec + ((long)b * ccap + j) * SF_REC;
    for (int k = 0; k < n; ++k) {
        if (ofs + k >= ccap) break;
        float* t = table + ((long)b * ccap + ofs + k) * SF_TAB;
        t[0] = q[1];
        t[1] = q[2];
        t[2] = q[3];
        t[3] = q[4];
        t[4] = q[5];
        t[5] = q[6];
        t[6] = q[7];
        t[7] = fabsf(q[8]);
        t[8] = q[9];
        t[9] = peaks[((long)b * ccap + j) * SF_MAXP + k];
        t[10] = q[10];
        t[11] = q[11];
    }
}

// ------------------------------------------------------------------ selection passes over the table (all pairs, exact comparisons)
// 0 removeDuplicated, 1 retainBest(K), 2 highest score of a pixel, 3 lowest |angle| of a pixel, 4 NMS (Chebyshev radius K), 5 top-K by score
template <int MODE>
__global__ __launch_bounds__(256) void sf_sel_kernel(const float* __restrict__ table, const int* __restrict__ ntab, int ccap, int W, int K, const int* __restrict__ alive_in,
                                                      int* __restrict__ alive_out) {
    __shared__ float4 s_a[256];
    __shared__ float s_s[256];
    __shared__ int s_p[256], s_l[256];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(ntab[b], ccap);
    if (blockIdx.x * 256 >= n) return;
    const float* tb = table + (long)b * ccap * SF_TAB;
    const int* ai = alive_in ? alive_in + (long)b * ccap : nullptr;
    auto load = [&](int k, float4& a, float& s, int& pix, int& live) {
        const float* t = tb + (long)k * SF_TAB;
        const float x = t[10] * 0.5f, y = t[11] * 0.5f;
        a = make_float4(x, y, t[8], MODE == 0 ? t[9] : __fmul_rn(t[9], 0.017453292519943295f));
        s = t[7];
        pix = (int)rintf(y - 0.5f) * W + (int)rintf(x - 0.5f);
        live = ai ? ai[k] : 1;
    };
    float4 a = make_float4(0, 0, 0, 0);
    float s = 0.f;
    int pix = 0, live = 0;
    if (i < n) load(i, a, s, pix, live);
    const int pr = pix / W, pc = pix % W;
    int cnt = 0;
    bool kill = false;
    for (int base = 0; base < n; base += 256) {
        const int k = base + threadIdx.x;
        if (k < n) {
            load(k, s_a[threadIdx.x], s_s[threadIdx.x], s_p[threadIdx.x], s_l[threadIdx.x]);
        } else {
            s_l[threadIdx.x] = 0;
        }
        __syncthreads();
        const int m = min(256, n - base);
        for (int t = 0; t < m; ++t) {
            if (!s_l[t]) continue;
            const int jdx = base + t;
            const float4 o = s_a[t];
            const float so = s_s[t];
            if (MODE == 0) {
                kill = kill || (jdx != i && o.x == a.x && o.y == a.y && o.z == a.z && o.w == a.w && (so > s || (so == s && jdx < i)));
            } else if (MODE == 1) {
                cnt += so > s;
            } else if (MODE == 2) {
                kill = kill || (s_p[t] == pix && so > s);
            } else if (MODE == 3) {
                kill = kill || (s_p[t] == pix && fabsf(o.w) < fabsf(a.w));
            } else if (MODE == 4) {
                const int qr = s_p[t] / W, qc = s_p[t] % W;
                kill = kill || (abs(qr - pr) <= K && abs(qc - pc) <= K && so > s);
            } else {
                cnt += (so > s || (so == s && jdx < i));
            }
        }
        __syncthreads();
    }
    if (i < n) {
        if (MODE == 1 || MODE == 5) kill = cnt >= K;
        alive_out[(long)b * ccap + i] = live && !kill;
    }
}

__global__ __launch_bounds__(256) void sf_final_kernel(const float* __restrict__ table, const int* __restrict__ ntab, const int* __restrict__ alive, const int* __restrict__ ofs,
                                                        const int* __restrict__ nfinal, int ccap, int kcap, float* __restrict__ kpts, float* __restrict__ scores,
                                                        float* __restrict__ scales, float* __restrict__ oris, int* __restrict__ rows, int* __restrict__ num, int* __restrict__ counts,
                                                        const int* __restrict__ ncand, int* __restrict__ status) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        if (nfinal[b] > kcap) atomicOr(status, 1);
        num[b] = min(nfinal[b], kcap);
        if (counts) {
            counts[3 * b] = ncand[b];
            counts[3 * b + 1] = ntab[b];
            counts[3 * b + 2] = nfinal[b];
        }
    }
    if (i >= min(ntab[b], ccap) || !alive[(long)b * ccap + i]) return;
    const int slot = ofs[(long)b * ccap + i];
    if (slot >= kcap) return;
    const float* t = table + ((long)b * ccap + i) * SF_TAB;
    const long d = (long)b * kcap + slot;
    kpts[2 * d] = t[10] * 0.5f;
    kpts[2 * d + 1] = t[11] * 0.5f;
    scores[d] = t[7];
    scales[d] = t[8] * 0.5f;
    oris[d] = __fmul_rn(t[9], 0.017453292519943295f);
    rows[d] = i;
}

// ------------------------------------------------------------------ descriptor: one wave per key-point
__global__ __launch_bounds__(64) void sf_desc_kernel(const float* __restrict__ pyr, SfGeom g, const float* __restrict__ table, const int* __restrict__ rows,
                                                      const int* __restrict__ num, int ccap, int kcap, int rootsift, float* __restrict__ desc, float* __restrict__ dbg_raw) {
    __shared__ float hh[128 * SF_HS];
    const int b = blockIdx.y, lane = threadIdx.x;
    for (int k = blockIdx.x; k < num[b]; k += gridDim.x) {
    const float* t = table + ((long)b * ccap + rows[(long)b * kcap + k]) * SF_TAB;
    const int o = (int)t[0], l = (int)t[1];
    const int h = g.h[o], w = g.w[o];
    const float* img = sf_oct(pyr, g, b, o) + (long)l * h * w;
    const float inv = 1.f / (float)(1 << o);
    const float px = t[10] * inv, py = t[11] * inv, scl = t[8] * inv * 0.5f;
    float ori = 360.f - t[9];
    if (fabsf(ori - 360.f) < SF_EPS) ori = 0.f;
    const int cx = (int)rintf(px), cy = (int)rintf(py);
    const float hw = 3.f * scl;
    int radius = (int)rintf(hw * 1.4142135623730951f * 5.f * 0.5f);
    radius = max(0, min(radius, (int)sqrtf((float)h * h + (float)w * w)));
    const float ct = cosf(ori * 0.017453292519943295f) / hw, st = sinf(ori * 0.017453292519943295f) / hw;
    for (int q = 0; q < 128; ++q) hh[q * SF_HS + lane] = 0.f;
    const int side = 2 * radius + 1, total = side * side;
    for (int q = lane; q < total; q += 64) {
        const int i = q / side - radius, j = q % side - radius;
        const float c_rot = j * ct - i * st, r_rot = j * st + i * ct;
        float rbin = r_rot + 1.5f, cbin = c_rot + 1.5f;
        const int y = cy + i, x = cx + j;
        if (!(rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f && y > 0 && y < h - 1 && x > 0 && x < w - 1)) continue;
        const float dx = img[(long)y * w + x + 1] - img[(long)y * w + x - 1], dy = img[(long)(y - 1) * w + x] - img[(long)(y + 1) * w + x];
        float ang = atan2f(dy, dx) * 57.29577951308232f;
        if (ang < 0.f) ang += 360.f;
        const float mag = sqrtf(dx * dx + dy * dy) * expf((c_rot * c_rot + r_rot * r_rot) * -0.125f);
        float obin = (ang - ori) * (8.f / 360.f);
        const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
        rbin -= r0f;
        cbin -= c0f;
        obin -= o0f;
        const int r0 = (int)r0f, c0 = (int)c0f;
        int o0 = (int)o0f;
        if (o0 < 0) o0 += 8;
        if (o0 >= 8) o0 -= 8;
        o0 &= 7;
        const int o1 = (o0 + 1) & 7;
        const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
        const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11, v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
        const float v111 = v_rc11 * obin, v110 = v_rc11 - v111, v101 = v_rc10 * obin, v100 = v_rc10 - v101;
        const float v011 = v_rc01 * obin, v010 = v_rc01 - v011, v001 = v_rc00 * obin, v000 = v_rc00 - v001;
        const bool ra = r0 >= 0, rb = r0 + 1 <= 3, ca = c0 >= 0, cb = c0 + 1 <= 3;
        if (ra && ca) {
            hh[((r0 * 4 + c0) * 8 + o0) * SF_HS + lane] += v000;
            hh[((r0 * 4 + c0) * 8 + o1) * SF_HS + lane] += v001;
        }
        if (ra && cb) {
            hh[((r0 * 4 + c0 + 1) * 8 + o0) * SF_HS + lane] += v010;
            hh[((r0 * 4 + c0 + 1) * 8 + o1) * SF_HS + lane] += v011;
        }
        if (rb && ca) {
            hh[(((r0 + 1) * 4 + c0) * 8 + o0) * SF_HS + lane] += v100;
            hh[(((r0 + 1) * 4 + c0) * 8 + o1) * SF_HS + lane] += v101;
        }
        if (rb && cb) {
            hh[(((r0 + 1) * 4 + c0 + 1) * 8 + o0) * SF_HS + lane] += v110;
            hh[(((r0 + 1) * 4 + c0 + 1) * 8 + o1) * SF_HS + lane] += v111;
        }
    }
    __syncthreads();
    float v0 = 0.f, v1 = 0.f;
    for (int q = 0; q < 64; ++q) {
        v0 += hh[lane * SF_HS + q];
        v1 += hh[(lane + 64) * SF_HS + q];
    }
    const float thr = sqrtf(wave_sum(v0 * v0 + v1 * v1)) * 0.2f;
    v0 = fminf(v0, thr);
    v1 = fminf(v1, thr);
    const float sc = 512.f / fmaxf(sqrtf(wave_sum(v0 * v0 + v1 * v1)), SF_EPS);
    v0 *= sc;
    v1 *= sc;
    const long d = ((long)b * kcap + k) * 128;
    if (dbg_raw) {
        dbg_raw[d + lane] = v0;
        dbg_raw[d + 64 + lane] = v1;
    }
    v0 = fminf(fmaxf(rintf(v0), 0.f), 255.f);
    v1 = fminf(fmaxf(rintf(v1), 0.f), 255.f);
    if (rootsift) {  // sift_to_rootsift: L1 normalise, clip at eps, square root, L2 normalise (eps 1e-6)
        const float l1 = fmaxf(wave_sum(v0 + v1), 1e-6f);
        v0 = sqrtf(fmaxf(v0 / l1, 1e-6f));
        v1 = sqrtf(fmaxf(v1 / l1, 1e-6f));
        const float l2 = fmaxf(sqrtf(wave_sum(v0 * v0 + v1 * v1)), 1e-6f);
        v0 /= l2;
        v1 /= l2;
    }
    desc[d + lane] = v0;
    desc[d + 64 + lane] = v1;
    __syncthreads();  // the LDS histograms are re-used by the next key-point
    }
}

// ------------------------------------------------------------------ host side
struct SfWs {
    float *up, *pyr, *rec, *peaks, *table;
    unsigned long long* bits;
    int *wgcnt, *ncand, *cand, *npeaks, *tabofs, *ntab, *alive0, *alive1, *fofs, *nfinal, *rows;
    int nwg;
    size_t total;
    bool ok;
};
static SfWs sf_carve(void* p, size_t cap, const SfGeom& g, int B, int H, int W, int ccap, int kcap, bool own_pyr) {
    WsAlloc a(p, cap);
    SfWs s;
    s.nwg = (int)((g.px_off[g.nOct] + 1023u) / 1024u);
    if (s.nwg < 1) s.nwg = 1;
    s.up = a.get<float>((size_t)B * 4 * H * W);
    s.pyr = own_pyr ? a.get<float>((size_t)g.pyr_total) : nullptr;
    s.bits = a.get<unsigned long long>((size_t)B * s.nwg * 16);
    s.wgcnt = a.get<int>((size_t)B * s.nwg);
    s.ncand = a.get<int>(B);
    s.cand = a.get<int>((size_t)B * ccap);
    s.rec = a.get<float>((size_t)B * ccap * SF_REC);
    s.npeaks = a.get<int>((size_t)B * ccap);
    s.peaks = a.get<float>((size_t)B * ccap * SF_MAXP);
    s.tabofs = a.get<int>((size_t)B * ccap);
    s.ntab = a.get<int>(B);
    s.table = a.get<float>((size_t)B * ccap * SF_TAB);
    s.alive0 = a.get<int>((size_t)B * ccap);
    s.alive1 = a.get<int>((size_t)B * ccap);
    s.fofs = a.get<int>((size_t)B * ccap);
    s.nfinal = a.get<int>(B);
    s.rows = a.get<int>((size_t)B * kcap);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

static const char* sf_check(int B, int H, int W, int layers, int ccap, int kcap) {
    if (B <= 0 || B > 1024) return "B outside 1..1024";
    if (layers < 3 || layers > 5) return "nOctaveLayers (the wrapper's `num_octaves`) outside 3..5";
    if (H < 8 || W < 8) return "images below 8 x 8";
    if ((double)H * W * 4.0 * layers * 1.34 > 2147483647.0) return "image too large (search index space above 2^31)";
    if (ccap <= 0 || kcap <= 0 || kcap > ccap) return "capacities: need 0 < kcap <= ccap";
    if ((double)B * ccap * SF_MAXP > 2147483647.0) return "B * ccap too large";
    return nullptr;
}

extern "C" size_t imcui_hip_sift_workspace_bytes(int B, int H, int W, int layers, int ccap, int kcap) {
    if (sf_check(B, H, W, layers, ccap, kcap)) return 0;
    const SfGeom g = sf_geom(B, H, W, layers);
    return sf_carve(nullptr, 0, g, B, H, W, ccap, kcap, true).total;
}

extern "C" int imcui_hip_sift_forward(imcui_hip_t* h, const float* image, int B, int C, int H, int W, int layers, float contrast_threshold, float edge_threshold,
                                      int nfeatures, int nms_radius, int max_keypoints, int rootsift, int ccap, int kcap, float* keypoints, float* scores,
                                      float* scales, float* oris, float* descriptors, int* num_keypoints, int* status, int* counts, float* dbg_pyramid,
                                      int* dbg_extrema, float* dbg_refined, float* dbg_hist, float* dbg_table, float* dbg_desc_raw, void* ws, size_t ws_bytes,
                                      void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (C != 1 && C != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "sift: image must have 1 or 3 channels, got %d", C);
    if (const char* why = sf_check(B, H, W, layers, ccap, kcap)) return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "sift: %s", why);
    if (nms_radius > 64) return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "sift: nms_radius=%d above 64", nms_radius);
    if (!image || !keypoints || !scores || !scales || !oris || !descriptors || !num_keypoints || !status)
        return imcui_set_err(h, IMCUI_ERR_ARG, "sift: null argument");
    const SfGeom g = sf_geom(B, H, W, layers);
    SfWs s = sf_carve(ws, ws_bytes, g, B, H, W, ccap, kcap, dbg_pyramid == nullptr);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "sift: workspace too small (%zu < %zu)", ws_bytes, s.total);
    float* pyr = dbg_pyramid ? dbg_pyramid : s.pyr;
    int* cand = dbg_extrema ? dbg_extrema : s.cand;
    float* rec = dbg_refined ? dbg_refined : s.rec;
    float* table = dbg_table ? dbg_table : s.table;
    if (hipMemsetAsync(status, 0, sizeof(int), stream) != hipSuccess) return imcui_set_err(h, IMCUI_ERR_HIP, "sift: memset failed");

    // ---- Gaussian pyramid
    hipLaunchKernelGGL(sf_gray_up_kernel, dim3(cdiv(2 * W, 64), cdiv(2 * H, 4), B), dim3(256), 0, stream, image, C, H, W, s.up);
    auto blur = [&](const float* src, long src_img, float* dst, long dst_img, int hh, int ww, double sigma) {
        hipLaunchKernelGGL(sf_blur_kernel, dim3(cdiv(ww, SF_TW), cdiv(hh, SF_TH), B), dim3(256), 0, stream, src, src_img, dst, dst_img, hh, ww, sf_taps(sigma));
    };
    double sig[8];
    {
        const double k = pow(2.0, 1.0 / layers);
        sig[0] = 1.6;
        for (int i = 1; i < g.L; ++i) {
            const double prev = pow(k, (double)(i - 1)) * 1.6, tot = prev * k;
            sig[i] = sqrt(tot * tot - prev * prev);
        }
    }
    for (int o = 0; o < g.nOct; ++o) {
        const int hh = g.h[o], ww = g.w[o];
        const long lvl = (long)hh * ww, img = lvl * g.L;
        float* P = pyr + g.pyr_off[o];
        if (o == 0) {
            blur(s.up, lvl, P, img, hh, ww, sqrt(fmax(1.6 * 1.6 - 4.0 * 0.5 * 0.5, 0.01)));
        } else {
            const int ph = g.h[o - 1], pw = g.w[o - 1];
            const long plvl = (long)ph * pw;
            hipLaunchKernelGGL(sf_down_kernel, dim3(cdiv(ww, 64), cdiv(hh, 4), B), dim3(256), 0, stream, pyr + g.pyr_off[o - 1] + layers * plvl, plvl * g.L, pw, P,
                               img, hh, ww);
        }
        for (int i = 1; i < g.L; ++i) blur(P + (i - 1) * lvl, img, P + i * lvl, img, hh, ww, sig[i]);
    }
    IMCUI_CHECK_LAUNCH(h);

    // ---- extrema -> candidate list in (octave, layer, row, column) order
    const unsigned total_px = g.px_off[g.nOct];
    const float thr = (float)(int)floor(0.5 * (double)contrast_threshold / layers * 255.0);
    hipLaunchKernelGGL(sf_extrema_kernel, dim3(s.nwg, B), dim3(1024), 0, stream, pyr, g, thr, s.bits, s.wgcnt, s.nwg);
    hipLaunchKernelGGL(exclusive_scan_kernel<int>, dim3(B), dim3(1024), 0, stream, s.wgcnt, s.wgcnt, s.ncand, (const int*)nullptr, s.nwg, (long)s.nwg);
    hipLaunchKernelGGL(sf_compact_kernel, dim3(s.nwg, B), dim3(1024), 0, stream, s.bits, s.wgcnt, s.nwg, total_px, ccap, cand);
    // ---- refinement, orientations, table
    hipLaunchKernelGGL(sf_refine_kernel, dim3(cdiv(ccap, 256), B), dim3(256), 0, stream, pyr, g, cand, s.ncand, ccap, contrast_threshold, edge_threshold, rec, status);
    hipLaunchKernelGGL(sf_orient_kernel, dim3(min(ccap, SF_MAXWG), B), dim3(64), 0, stream, pyr, g, rec, s.ncand, ccap, s.npeaks, s.peaks, dbg_hist);
    hipLaunchKernelGGL(exclusive_scan_kernel<int>, dim3(B), dim3(1024), 0, stream, s.npeaks, s.tabofs, s.ntab, s.ncand, ccap, (long)ccap);
    hipLaunchKernelGGL(sf_expand_kernel, dim3(cdiv(ccap, 256), B), dim3(256), 0, stream, rec, s.ncand, s.npeaks, s.tabofs, s.ntab, s.peaks, ccap, table, status);
    IMCUI_CHECK_LAUNCH(h);
    // ---- OpenCV's post-processing and the wrapper stages
    const dim3 sg(cdiv(ccap, 256), B), sb(256);
    int* cur = s.alive0;
    int* nxt = s.alive1;
    hipLaunchKernelGGL(sf_sel_kernel<0>, sg, sb, 0, stream, table, s.ntab, ccap, W, 0, (const int*)nullptr, cur);
    auto pass = [&](auto kern, int K) {
        hipLaunchKernelGGL(kern, sg, sb, 0, stream, table, s.ntab, ccap, W, K, cur, nxt);
        int* t = cur;
        cur = nxt;
        nxt = t;
    };
    if (nfeatures > 0) pass(sf_sel_kernel<1>, nfeatures);
    if (nms_radius >= 0) {
        pass(sf_sel_kernel<2>, 0);
        pass(sf_sel_kernel<3>, 0);
        if (nms_radius > 0) pass(sf_sel_kernel<4>, nms_radius);
    }
    if (max_keypoints > 0) pass(sf_sel_kernel<5>, max_keypoints);
    hipLaunchKernelGGL(exclusive_scan_kernel<int>, dim3(B), dim3(1024), 0, stream, cur, s.fofs, s.nfinal, s.ntab, ccap, (long)ccap);
    hipLaunchKernelGGL(sf_final_kernel, sg, sb, 0, stream, table, s.ntab, cur, s.fofs, s.nfinal, ccap, kcap, keypoints, scores, scales, oris, s.rows, num_keypoints, counts,
                       s.ncand, status);
    hipLaunchKernelGGL(sf_desc_kernel, dim3(min(kcap, SF_MAXWG), B), dim3(64), 0, stream, pyr, g, table, s.rows, num_keypoints, ccap, kcap, rootsift, descriptors, dbg_desc_raw);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
