// SuperGlue: what imcui/hloc/matchers/superglue.py:42-43 `self.net(data)` computes
// (upstream Vincentqyw/SuperGluePretrainedNetwork models/superglue.py), for B pairs at once.
//
// Same data layout as LightGlue: 2B sequences (image 0/1 of each pair) of R = roundup(ncap,128) token rows,
// x [2B*R,256] token-major, attention operands head-major, per-sequence counts on the device.  The packed weights, the
// attentional GNN up to the score matrix and the final arg-max / mutual check are glue_shared.h (IMP runs the same trunk);
// this file holds the first-layer kernel and the optimal transport.
// The optimal transport runs on the materialised score matrix [B,R,R] (dust-bin row / column are never stored:
// they are the constant bin_score): per Sinkhorn round one row pass and one column pass, each reading the matrix
// once -- HBM bound, 2 * iterations * 4*n0*n1 bytes per pair.
#include "glue_shared.h"

#define SG_RBANDS 8  // row bands of the Sinkhorn column pass (R > 2048)
#define SGF_ROWS 16  // rows per block of the fused Sinkhorn round (R <= 2048)
#define SGF_COLS 2048

// ------------------------------------------------------------------ packed weights (glue_shared.h, no input_proj, one final_proj)
static const std::vector<GlueTensor>& sg_table() {
    static const std::vector<GlueTensor> table = glue_table(false, 1);
    return table;
}
static const int SG_NUM_TENSORS = glue_t_bin(false, 1) + 1;

extern "C" size_t imcui_hip_superglue_packed_floats(void) { return glue_layout(false).total; }
extern "C" int imcui_hip_superglue_num_tensors(void) { return SG_NUM_TENSORS; }
extern "C" const char* imcui_hip_superglue_tensor_name(int i) { return (i < 0 || i >= SG_NUM_TENSORS) ? nullptr : sg_table()[i].name; }

extern "C" int imcui_hip_superglue_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    for (int i = 0; i < SG_NUM_TENSORS; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    glue_pack(glue_layout(false), t + GLUE_T_CONV, t + GLUE_T_BN, nullptr, t + glue_t_layer0(false), t + glue_t_final(false),
              t[glue_t_bin(false, 1)], packed);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ workspace
struct SgWs : GlueTrunkWs {
    float *u, *vv, *max0, *pm, *ps;
    size_t total;
    bool ok;
};

static SgWs sg_carve(void* ws, size_t bytes, int B, int R) {
    WsAlloc a(ws, bytes);
    SgWs w;
    glue_carve_tokens(a, w, B, R, false);
    w.u = a.get<float>((size_t)B * (R + 64));
    w.vv = a.get<float>((size_t)B * (R + 64));
    w.max0 = a.get<float>((size_t)B * R);
    const size_t nbmax = (R <= SGF_COLS) ? (size_t)R / SGF_ROWS : (size_t)SG_RBANDS;
    w.pm = a.get<float>((size_t)B * nbmax * R);  // column-pass partials (max, sum) per row band
    w.ps = a.get<float>((size_t)B * nbmax * R);
    glue_carve_pairs(a, w, B, R);
    w.total = a.off;
    w.ok = a.ok;
    return w;
}

extern "C" size_t imcui_hip_superglue_workspace_bytes(int B, int ncap) {
    const int R = (int)align_up((size_t)(ncap > 0 ? ncap : 1), 128);
    return sg_carve(nullptr, 0, B, R).total;
}

// ------------------------------------------------------------------ kernels
// one wave per row: output defaults, x = descriptor, first encoder layer relu(W0' [kx, ky, score] + b0') -> e32,
// identity rotation tables, Sinkhorn potentials u = v = 0
__global__ __launch_bounds__(256) void sg_init_kernel(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                      const float* __restrict__ sc0, const float* __restrict__ sc1,
                                                      const float* __restrict__ d0, const float* __restrict__ d1,
                                                      const int* __restrict__ cnt, int ncap, int R, float w0, float h0, float w1,
                                                      float h1, const float* __restrict__ k0w, float* __restrict__ x,
                                                      float* __restrict__ e32, float* __restrict__ one, float* __restrict__ zero,
                                                      float* __restrict__ u, float* __restrict__ v, int* __restrict__ matches0,
                                                      int* __restrict__ matches1, float* __restrict__ ms0,
                                                      float* __restrict__ ms1) {
    const int lane = threadIdx.x & 63;
    const int seq = blockIdx.y, b = seq >> 1, img = seq & 1;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= R) return;
    const int n = cnt[seq];
    const size_t row = (size_t)seq * R + i;
    if (lane == 0) {
        if (i < ncap) {
            (img ? matches1 : matches0)[(size_t)b * ncap + i] = -1;
            (img ? ms1 : ms0)[(size_t)b * ncap + i] = 0.0f;
        }
        (img ? v : u)[(size_t)b * (R + 64) + i] = 0.0f;
        if (i == 0) (img ? v : u)[(size_t)b * (R + 64) + R] = 0.0f;
    }
    if (lane < 32) {
        one[row * 32 + lane] = 1.0f;
        zero[row * 32 + lane] = 0.0f;
    }
    if (i >= n) return;
    const float* d = (img ? d1 : d0) + ((size_t)b * ncap + i) * 256;
    *reinterpret_cast<float4*>(x + row * 256 + lane * 4) = *reinterpret_cast<const float4*>(d + lane * 4);
    if (lane < 32) {
        const float* kp = (img ? kp1 : kp0) + ((size_t)b * ncap + i) * 2;
        const float s = (img ? sc1 : sc0)[(size_t)b * ncap + i];
        e32[row * 32 + lane] = glue_kenc0(kp, s, img ? w1 : w0, img ? h1 : h0, *reinterpret_cast<const float4*>(k0w + lane * 4));
    }
}

// exp() of the Sinkhorn passes: arguments are x - max <= 0, the terms that matter have |x| of a few units, so the
// hardware 2^x (v_exp_f32 of x * log2 e, ~1e-6 relative here) replaces the ~12-instruction library expf: with two
// exponentials per matrix element and round the library version made the fused round VALU-bound (200 us vs 100 us of
// HBM time).
__device__ __forceinline__ float sg_exp(float x) { return __expf(x); }
// streaming log-sum-exp: running maximum m, sum s of exp(x - m)
struct Lse {
    float m, s;
};
__device__ __forceinline__ void lse_add4(Lse& a, float x0, float x1, float x2, float x3) {
    const float cm = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
    if (cm == -INFINITY) return;
    const float mn = fmaxf(a.m, cm);
    a.s = a.s * sg_exp(a.m - mn) + ((sg_exp(x0 - mn) + sg_exp(x1 - mn)) + (sg_exp(x2 - mn) + sg_exp(x3 - mn)));
    a.m = mn;
}
__device__ __forceinline__ void lse_merge(Lse& a, float m, float s) {
    if (m == -INFINITY) return;
    const float mn = fmaxf(a.m, m);
    a.s = a.s * sg_exp(a.m - mn) + s * sg_exp(m - mn);
    a.m = mn;
}

// Sinkhorn row pass: u_i = log_mu_i - logsumexp_j(Z_ij + v_j), j over the n1 columns and the dust-bin column.
// One wave per row; row n0 is the dust-bin row (Z = bin_score everywhere).
__global__ __launch_bounds__(256) void sg_row_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
                                                     const int* __restrict__ active, int R, const float* __restrict__ binp,
                                                     const float* __restrict__ v, float* __restrict__ u) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    if (i > n0) return;
    const float alpha = binp[0];
    const float* vb = v + (size_t)b * (R + 64);
    const float* row = sim + ((size_t)b * R + (i < n0 ? i : 0)) * R;
    const bool bin = (i == n0);
    Lse a = {-INFINITY, 0.0f};
#pragma unroll 2
    for (int j = lane * 4; j < n1; j += 256) {
        const float4 z = bin ? make_float4(alpha, alpha, alpha, alpha) : *reinterpret_cast<const float4*>(row + j);
        const float4 vj = *reinterpret_cast<const float4*>(vb + j);
        lse_add4(a, z.x + vj.x, (j + 1 < n1) ? z.y + vj.y : -INFINITY, (j + 2 < n1) ? z.z + vj.z : -INFINITY,
                 (j + 3 < n1) ? z.w + vj.w : -INFINITY);
    }
    const float M = wave_max(a.m);
    float s = (a.m == -INFINITY) ? 0.0f : a.s * sg_exp(a.m - M);
    s = wave_sum(s);
    if (lane == 0) {
        Lse t = {M, s};
        lse_merge(t, alpha + vb[n1], 1.0f);  // dust-bin column
        const float norm = -logf((float)n0 + (float)n1);
        const float log_mu = bin ? logf((float)n1) + norm : norm;
        u[(size_t)b * (R + 64) + i] = log_mu - (t.m + logf(t.s));
    }
}

// Sinkhorn column pass: v_j = log_nu_j - logsumexp_i(Z_ij + u_i), in two launches.
// (1) partial statistics: block = 256 columns (one float4 per lane, a wave reads 1 KB of a row) x one band of rows,
//     the four waves take interleaved rows, 8 rows in flight per lane.  A walk down 64-column strips (one 256-byte
//     segment per row and wave) measured 0.8 - 2.1 TB/s; this shape streams like the row pass.
// (2) merge of the band partials and the dust-bin row; the last block is the dust-bin column.
__device__ __forceinline__ void lse_add8(Lse& a, const float (&x)[8]) {
    const float cm = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    if (cm == -INFINITY) return;
    const float mn = fmaxf(a.m, cm);
    a.s = a.s * sg_exp(a.m - mn) + (((sg_exp(x[0] - mn) + sg_exp(x[1] - mn)) + (sg_exp(x[2] - mn) + sg_exp(x[3] - mn))) +
                                  ((sg_exp(x[4] - mn) + sg_exp(x[5] - mn)) + (sg_exp(x[6] - mn) + sg_exp(x[7] - mn))));
    a.m = mn;
}
__device__ __forceinline__ int sg_band_rows(int n0) { return (n0 + SG_RBANDS - 1) / SG_RBANDS; }

__global__ __launch_bounds__(256) void sg_colpart_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
                                                         const int* __restrict__ active, int R, const float* __restrict__ u,
                                                         float* __restrict__ pm, float* __restrict__ ps) {
    __shared__ float sm[4][256], ss[4][256];
    const int b = blockIdx.z;
    if (!active[b]) return;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    const int j0 = blockIdx.x * 256;
    const int rb = sg_band_rows(n0), r0 = blockIdx.y * rb, r1 = min(n0, r0 + rb);
    if (j0 >= n1 || r0 >= n0) return;
    const int j = j0 + lane * 4;
    const float* base = sim + (size_t)b * R * R + j;
    const float* ub = u + (size_t)b * (R + 64);
    Lse a[4] = {{-INFINITY, 0.0f}, {-INFINITY, 0.0f}, {-INFINITY, 0.0f}, {-INFINITY, 0.0f}};
    if (j < n1)
        for (int i = r0 + g; i < r1; i += 32) {
            float4 z[8];
            float uu[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const bool ok = i + 4 * t < r1;
                z[t] = ok ? *reinterpret_cast<const float4*>(base + (size_t)(i + 4 * t) * R) : make_float4(0.f, 0.f, 0.f, 0.f);
                uu[t] = ok ? ub[i + 4 * t] : -INFINITY;
            }
            float x[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) x[t] = z[t].x + uu[t];
            lse_add8(a[0], x);
#pragma unroll
            for (int t = 0; t < 8; ++t) x[t] = z[t].y + uu[t];
            lse_add8(a[1], x);
#pragma unroll
            for (int t = 0; t < 8; ++t) x[t] = z[t].z + uu[t];
            lse_add8(a[2], x);
#pragma unroll
            for (int t = 0; t < 8; ++t) x[t] = z[t].w + uu[t];
            lse_add8(a[3], x);
        }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        sm[g][lane * 4 + c] = a[c].m;
        ss[g][lane * 4 + c] = a[c].s;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (j0 + t < n1) {
        Lse r = {sm[0][t], ss[0][t]};
        for (int gg = 1; gg < 4; ++gg) lse_merge(r, sm[gg][t], ss[gg][t]);
        const size_t o = ((size_t)b * SG_RBANDS + blockIdx.y) * R + j0 + t;
        pm[o] = r.m;
        ps[o] = r.s;
    }
}

// (2) merge: block = 256 columns (float4 per thread) x 16 groups of bands (fixed order inside a group and across groups)
#define SG_MG 16
__global__ __launch_bounds__(64 * SG_MG) void sg_colmerge_kernel(const int* __restrict__ cnt, const int* __restrict__ active, int R,
                                                          const float* __restrict__ binp, const float* __restrict__ u,
                                                          const float* __restrict__ pm, const float* __restrict__ ps,
                                                          float* __restrict__ v, int fused) {
    __shared__ float sm[SG_MG][256], ss[SG_MG][256];
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const float alpha = binp[0];
    const float* ub = u + (size_t)b * (R + 64);
    const float norm = -logf((float)n0 + (float)n1);
    if (blockIdx.x == gridDim.x - 1) {
        // dust-bin column: logsumexp_i(alpha + u_i) over the n0 rows and the dust-bin row
        Lse a = {-INFINITY, 0.0f};
        for (int i = threadIdx.x * 4; i <= n0; i += 256 * SG_MG)
            lse_add4(a, alpha + ub[i], (i + 1 <= n0) ? alpha + ub[i + 1] : -INFINITY, (i + 2 <= n0) ? alpha + ub[i + 2] : -INFINITY,
                     (i + 3 <= n0) ? alpha + ub[i + 3] : -INFINITY);
        const float M = wave_max(a.m);
        float s = (a.m == -INFINITY) ? 0.0f : a.s * sg_exp(a.m - M);
        s = wave_sum(s);
        if (c == 0) {
            sm[g][0] = M;
            ss[g][0] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            Lse t = {sm[0][0], ss[0][0]};
            for (int gg = 1; gg < SG_MG; ++gg) lse_merge(t, sm[gg][0], ss[gg][0]);
            v[(size_t)b * (R + 64) + n1] = (logf((float)n0) + norm) - (t.m + logf(t.s));
        }
        return;
    }
    if (blockIdx.x * 256 >= n1) return;
    const int j = blockIdx.x * 256 + c * 4;  // four columns per thread
    const int nbands = fused ? (n0 + SGF_ROWS - 1) / SGF_ROWS : (n0 + sg_band_rows(n0) - 1) / sg_band_rows(n0);
    const size_t stride = fused ? (size_t)(R / SGF_ROWS) : (size_t)SG_RBANDS;
    Lse t[4] = {{-INFINITY, 0.0f}, {-INFINITY, 0.0f}, {-INFINITY, 0.0f}, {-INFINITY, 0.0f}};
    if (j < n1) {
#pragma unroll 4
        for (int k = g; k < nbands; k += SG_MG) {
            const size_t o = ((size_t)b * stride + k) * R + j;
            const float4 m4 = *reinterpret_cast<const float4*>(pm + o);
            const float4 s4 = *reinterpret_cast<const float4*>(ps + o);
            lse_merge(t[0], m4.x, s4.x);
            lse_merge(t[1], m4.y, s4.y);
            lse_merge(t[2], m4.z, s4.z);
            lse_merge(t[3], m4.w, s4.w);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sm[g][c * 4 + q] = t[q].m;
        ss[g][c * 4 + q] = t[q].s;
    }
    __syncthreads();
    const int jj = blockIdx.x * 256 + threadIdx.x;  // one column per thread for the final combine
    if (threadIdx.x < 256 && jj < n1) {
        Lse r = {sm[0][threadIdx.x], ss[0][threadIdx.x]};
        for (int gg = 1; gg < SG_MG; ++gg) lse_merge(r, sm[gg][threadIdx.x], ss[gg][threadIdx.x]);
        lse_merge(r, alpha + ub[n0], 1.0f);  // dust-bin row
        v[(size_t)b * (R + 64) + jj] = norm - (r.m + logf(r.s));
    }
}

// Fused Sinkhorn round for R <= 2048 (one launch + the merge): a block owns SGF_ROWS rows of one pair at a time, keeps
// them in registers (2 rows x 32 columns per lane), computes its u_i from the staged v (row pass) and straight away
// the column statistics of the band with the new u (column pass): the matrix is read from HBM once per round
// instead of twice.  One band per block, two 512-thread blocks per CU (124 VGPRs, 74 KB LDS); a persistent variant
// that prefetched the next band into a second register set (194 VGPRs, one block per CU) measured 20 % slower.
// Block index == number of bands is the dust-bin row.
struct SgBandRows {
    float4 z0[8], z1[8];
};
__device__ __forceinline__ void sg_band_load(SgBandRows& t, const float* __restrict__ simb, int R, int band, int w, int lane, int n0,
                                             int n1) {
    const float NI = -INFINITY;
    const int i0 = band * SGF_ROWS + 2 * w;
    const bool ok0 = i0 < n0, ok1 = i0 + 1 < n0;
    const int nch = (n1 + 255) >> 8;
    const float* p0 = simb + (size_t)i0 * R + lane * 4;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int j = k * 256 + lane * 4;
        const bool in = (k < nch) && (j < R);
        t.z0[k] = (in && ok0) ? *reinterpret_cast<const float4*>(p0 + k * 256) : make_float4(NI, NI, NI, NI);
        t.z1[k] = (in && ok1) ? *reinterpret_cast<const float4*>(p0 + R + k * 256) : make_float4(NI, NI, NI, NI);
    }
}

__global__ __launch_bounds__(512, 4) void sg_band_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
                                                         const int* __restrict__ active, int R, const float* __restrict__ binp,
                                                         const float* __restrict__ v, float* __restrict__ u,
                                                         float* __restrict__ pm, float* __restrict__ ps) {
    __shared__ float4 lds4[(8 * SGF_COLS + SGF_COLS + 64) / 4];
    float* lm = reinterpret_cast<float*>(lds4);  // [8 waves][2048]: column maxima of a wave's rows, then its sums
    float* lv = lm + 8 * SGF_COLS;               // [2048 + 64]: staged v (row pass), then the block's column maxima
    float* lM = lv;
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    const int nbands = (n0 + SGF_ROWS - 1) / SGF_ROWS;
    if ((int)blockIdx.x > nbands) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float alpha = binp[0];
    const float NI = -INFINITY;
    const float* simb = sim + (size_t)b * R * R;
    const float* vb = v + (size_t)b * (R + 64);
    float* ub = u + (size_t)b * (R + 64);
    const float norm = -logf((float)n0 + (float)n1);
    SgBandRows cur;
    for (int j = tid; j < SGF_COLS + 64; j += 512) lv[j] = (j <= n1) ? vb[j] : 0.0f;
    __syncthreads();
    {
        const int band = blockIdx.x;
        if (band == nbands) {
            // dust-bin row: u = (log n1 + norm) - logsumexp_j(alpha + v_j), j = 0 .. n1 (dust-bin column included)
            float mx = -INFINITY;
            for (int j = tid; j <= n1; j += 512) mx = fmaxf(mx, alpha + lv[j]);
            mx = wave_max(mx);
            if (lane == 0) lm[w] = mx;
            __syncthreads();
            float M = lm[0];
            for (int k = 1; k < 8; ++k) M = fmaxf(M, lm[k]);
            float s = 0.0f;
            for (int j = tid; j <= n1; j += 512) s += sg_exp((alpha + lv[j]) - M);
            s = wave_sum(s);
            __syncthreads();
            if (lane == 0) lm[w] = s;
            __syncthreads();
            if (tid == 0) {
                float S = lm[0];
                for (int k = 1; k < 8; ++k) S += lm[k];
                ub[n0] = (logf((float)n1) + norm) - (M + logf(S));
            }
            return;
        }
        sg_band_load(cur, simb, R, band, w, lane, n0, n1);
        const int i0 = band * SGF_ROWS + 2 * w;
        const bool ok0 = i0 < n0, ok1 = i0 + 1 < n0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {  // columns >= n1 do not exist
            const int j = k * 256 + lane * 4;
            if (j + 0 >= n1) cur.z0[k].x = NI, cur.z1[k].x = NI;
            if (j + 1 >= n1) cur.z0[k].y = NI, cur.z1[k].y = NI;
            if (j + 2 >= n1) cur.z0[k].z = NI, cur.z1[k].z = NI;
            if (j + 3 >= n1) cur.z0[k].w = NI, cur.z1[k].w = NI;
        }
        // ---- row pass: u_i = norm - logsumexp_j(Z_ij + v_j) (max, then sum of exp, like torch.logsumexp)
        auto row_u = [&](const float4(&z)[8], int i) -> float {
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 vj = *reinterpret_cast<const float4*>(lv + k * 256 + lane * 4);
                mx = fmaxf(mx, fmaxf(fmaxf(z[k].x + vj.x, z[k].y + vj.y), fmaxf(z[k].z + vj.z, z[k].w + vj.w)));
            }
            const float M = wave_max(mx);
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 vj = *reinterpret_cast<const float4*>(lv + k * 256 + lane * 4);
                s += (sg_exp((z[k].x + vj.x) - M) + sg_exp((z[k].y + vj.y) - M)) + (sg_exp((z[k].z + vj.z) - M) + sg_exp((z[k].w + vj.w) - M));
            }
            s = wave_sum(s);
            const float xb = alpha + lv[n1];  // dust-bin column
            const float M2 = fmaxf(M, xb);
            const float ui = norm - (M2 + logf(s * sg_exp(M - M2) + sg_exp(xb - M2)));
            if (lane == 0) ub[i] = ui;
            return ui;
        };
        const float u0 = ok0 ? row_u(cur.z0, i0) : 0.0f;
        const float u1 = ok1 ? row_u(cur.z1, i0 + 1) : 0.0f;
        // ---- column pass over the band: block maximum per column first (through LDS), then the sum of exp(x - max)
        float* lmw = lm + w * SGF_COLS + lane * 4;
#pragma unroll
        for (int k = 0; k < 8; ++k) {  // x = Z + u_i in place (a masked row / column stays -inf)
            cur.z0[k].x += u0, cur.z0[k].y += u0, cur.z0[k].z += u0, cur.z0[k].w += u0;
            cur.z1[k].x += u1, cur.z1[k].y += u1, cur.z1[k].z += u1, cur.z1[k].w += u1;
            *reinterpret_cast<float4*>(lmw + k * 256) = make_float4(fmaxf(cur.z0[k].x, cur.z1[k].x), fmaxf(cur.z0[k].y, cur.z1[k].y),
                                                                    fmaxf(cur.z0[k].z, cur.z1[k].z), fmaxf(cur.z0[k].w, cur.z1[k].w));
        }
        __syncthreads();
        float4 M4 = *reinterpret_cast<const float4*>(lm + 4 * tid);
#pragma unroll
        for (int ww = 1; ww < 8; ++ww) {
            const float4 t = *reinterpret_cast<const float4*>(lm + ww * SGF_COLS + 4 * tid);
            M4 = make_float4(fmaxf(M4.x, t.x), fmaxf(M4.y, t.y), fmaxf(M4.z, t.z), fmaxf(M4.w, t.w));
        }
        *reinterpret_cast<float4*>(lM + 4 * tid) = M4;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float4 MM = *reinterpret_cast<const float4*>(lM + k * 256 + lane * 4);
            float4 r;  // exp(-inf - MM) = 0 for a masked row; MM = -inf only for a masked column
            r.x = (MM.x == NI) ? 0.0f : sg_exp(cur.z0[k].x - MM.x) + sg_exp(cur.z1[k].x - MM.x);
            r.y = (MM.y == NI) ? 0.0f : sg_exp(cur.z0[k].y - MM.y) + sg_exp(cur.z1[k].y - MM.y);
            r.z = (MM.z == NI) ? 0.0f : sg_exp(cur.z0[k].z - MM.z) + sg_exp(cur.z1[k].z - MM.z);
            r.w = (MM.w == NI) ? 0.0f : sg_exp(cur.z0[k].w - MM.w) + sg_exp(cur.z1[k].w - MM.w);
            *reinterpret_cast<float4*>(lmw + k * 256) = r;
        }
        __syncthreads();
        float4 S4 = *reinterpret_cast<const float4*>(lm + 4 * tid);
#pragma unroll
        for (int ww = 1; ww < 8; ++ww) {
            const float4 t = *reinterpret_cast<const float4*>(lm + ww * SGF_COLS + 4 * tid);
            S4 = make_float4(S4.x + t.x, S4.y + t.y, S4.z + t.z, S4.w + t.w);
        }
        if (4 * tid < R) {
            const size_t o = ((size_t)b * (R / SGF_ROWS) + band) * R + 4 * tid;
            *reinterpret_cast<float4*>(pm + o) = M4;
            *reinterpret_cast<float4*>(ps + o) = S4;
        }
    }
}

// ------------------------------------------------------------------ forward
extern "C" int imcui_hip_superglue_forward(imcui_hip_t* h, const float* packed, int B, int ncap, const float* keypoints0,
                                           const float* keypoints1, const float* scores0, const float* scores1,
                                           const float* descriptors0, const float* descriptors1, const int* n0, const int* n1,
                                           float w0, float h0, float w1, float h1, int sinkhorn_iterations, double match_threshold,
                                           int* matches0, int* matches1, float* mscores0, float* mscores1, void* ws,
                                           size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (ncap <= 0) return imcui_set_err(h, IMCUI_ERR_ARG, "superglue: ncap=%d must be positive", ncap);
    if (sinkhorn_iterations < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "superglue: sinkhorn_iterations=%d", sinkhorn_iterations);
    if (!packed || !keypoints0 || !keypoints1 || !scores0 || !scores1 || !descriptors0 || !descriptors1 || !n0 || !n1 ||
        !matches0 || !matches1 || !mscores0 || !mscores1)
        return imcui_set_err(h, IMCUI_ERR_ARG, "superglue: null argument");
    const int R = (int)align_up((size_t)ncap, 128);
    SgWs w = sg_carve(ws, ws_bytes, B, R);
    if (!ws || !w.ok) return imcui_set_err(h, IMCUI_ERR_WS, "superglue: workspace too small (%zu < %zu)", ws_bytes, w.total);
    const GlueLayout l = glue_layout(false);
    const float* P = packed;
    const dim3 blk(256);
    int rc;

    hipLaunchKernelGGL(glue_pairs_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, n0, n1, B, w.cnt, w.active);
    hipLaunchKernelGGL(sg_init_kernel, dim3(R / 4, 2 * B), blk, 0, stream, keypoints0, keypoints1, scores0, scores1, descriptors0,
                       descriptors1, w.cnt, ncap, R, w0, h0, w1, h1, P + l.k0, w.x, w.ctx, w.one, w.zero, w.u, w.vv, matches0, matches1,
                       mscores0, mscores1);
    IMCUI_CHECK_LAUNCH(h);

    static const bool ffn_unfused = getenv("IMCUI_LG_FFN_UNFUSED") != nullptr;  // A/B switch, as in lightglue.hip
    IMCUI_RUN(glue_trunk(h, P, l, w, B, R, GLUE_HEADS, ffn_unfused, stream));
    // ---- log-domain Sinkhorn with dust-bins, then mutual arg-max + threshold
    // (Running the rounds chunk-wise so that a chunk's matrices fit the 256 MB memory-side cache measured slower
    // at every chunk size: the passes stream at HBM rate either way and small launches lose occupancy.)
    const bool fused = R <= SGF_COLS;
    const dim3 rg(R / 4 + 1, B), cpg(cdiv(R, 256), SG_RBANDS, B), cmg(cdiv(R, 256) + 1, B), bg(R / SGF_ROWS + 1, B);
    for (int it = 0; it < sinkhorn_iterations; ++it) {
        if (fused) {
            hipLaunchKernelGGL(sg_band_kernel, bg, dim3(512), 0, stream, w.sim, w.cnt, w.active, R, P + l.bin, w.vv, w.u, w.pm, w.ps);
        } else {
            hipLaunchKernelGGL(sg_row_kernel, rg, blk, 0, stream, w.sim, w.cnt, w.active, R, P + l.bin, w.vv, w.u);
            hipLaunchKernelGGL(sg_colpart_kernel, cpg, blk, 0, stream, w.sim, w.cnt, w.active, R, w.u, w.pm, w.ps);
        }
        hipLaunchKernelGGL(sg_colmerge_kernel, cmg, dim3(64 * SG_MG), 0, stream, w.cnt, w.active, R, P + l.bin, w.u, w.pm, w.ps, w.vv, fused ? 1 : 0);
    }
    glue_match<SgScore, true>(w, w.u, w.vv, w.max0, B, ncap, R, (float)match_threshold, matches0, matches1, mscores0, mscores1, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
