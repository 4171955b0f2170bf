// IMP (`sfd2+imp` of the zoo): what imcui/hloc/matchers/imp.py:51 `self.net.produce_matches(data, p=0.2)` computes
// (pram.nets.gml.GML, restated in tests/imp_reference.py: the submodule is absent, see INTEGRATION.md "IMP: what is pinned"),
// for B pairs at once.
//
// Trunk = SuperGlue's (glue_shared.h: packed weights, tensor table, the launches up to the score matrix, and the final arg-max /
// mutual check): 2B sequences of R = roundup(ncap,128) token rows, x [2B*R,256] token-major, attention operands head-major,
// per-sequence counts on the device.  What differs: the descriptors are 128 wide and enter through input_proj (128 -> 256, the
// key-point encoding joins in the residual epilogue), and one of nine final projections (final_proj.8) feeds the similarity.
//
// Assignment = probability-domain Sinkhorn on the materialised matrix [B,R,R], hand-written here (imp_* kernels):
//   imp_softmax_kernel   M -> p in place (row soft-max over the n1 columns and the dust-bin column, which goes to a vector;
//                        the dust-bin row is the constant 1 / (n1 + 1) and is never stored)
//   imp_round_kernel     one round reads the matrix ONCE: a workgroup owns IMP_BAND rows, computes their u from the staged v
//                        and at once the band's contribution to the column sums with the new u
//   imp_merge_kernel     folds the band partials in band order, adds the dust-bin row's term, writes v
//   glue_rowarg / colarg / filter (ImpScore)   arg-maxima of p_ij u_i v_j, mutual check, strict threshold; P is never written
// Every sum has one fixed order (no float atomics), and the file is compiled with -ffp-contract=off: every operation rounds
// once, so tests/imp_reference.py `sinkhorn_explicit` states the same float32 order.
#include "glue_shared.h"

#define IMP_DESC GLUE_DESC_IN  // input_proj input width (anything else is refused by the binding)
#define IMP_FINAL 9            // final_proj.{0..8}: training supervises every layer pair, inference reads the last
#define IMP_EPS 1e-8f          // epsilon of the Sinkhorn divisions
#define IMP_BAND 16            // rows per workgroup of a round (8 waves x 2 rows)
#define IMP_NK 16              // float4 per lane and row: 16 x 256 = 4096 columns stay in registers
#define IMP_COLS (IMP_NK * 256)
#define IMP_HALF 2048  // columns per cross-wave fold through LDS
#define IMP_MG 16      // groups of the merge kernel = bands per group (16 x 16 = 4096 / IMP_BAND bands)
// marginals of the dust-bins: r = [1] * n0 + [n1], c = [1] * n1 + [n0]
#define IMP_ROW_BIN_MASS(n0, n1) ((float)(n1))
#define IMP_COL_BIN_MASS(n0, n1) ((float)(n0))

// ------------------------------------------------------------------ packed weights (glue_shared.h, with input_proj, nine final_proj)
static const std::vector<GlueTensor>& imp_table() {
    static const std::vector<GlueTensor> table = glue_table(true, IMP_FINAL);
    return table;
}
static const int IMP_NUM_TENSORS = glue_t_bin(true, IMP_FINAL) + 1;

extern "C" int imcui_hip_imp_num_tensors(void) { return IMP_NUM_TENSORS; }
extern "C" const char* imcui_hip_imp_tensor_name(int i) { return (i < 0 || i >= IMP_NUM_TENSORS) ? nullptr : imp_table()[i].name; }
extern "C" int imcui_hip_imp_tensor_shape(int i, int* dims) {
    if (i < 0 || i >= IMP_NUM_TENSORS || !dims) return -1;
    const GlueTensor& e = imp_table()[i];
    for (int k = 0; k < e.nd; ++k) dims[k] = e.d[k];
    return e.nd;
}
extern "C" size_t imcui_hip_imp_packed_floats(void) { return glue_layout(true).total; }

extern "C" int imcui_hip_imp_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    for (int i = 0; i < IMP_NUM_TENSORS; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    glue_pack(glue_layout(true), t + GLUE_T_CONV, t + GLUE_T_BN, t + GLUE_T_INPROJ, t + glue_t_layer0(true),
              t + glue_t_final(true) + 2 * (IMP_FINAL - 1),  // inference reads final_proj.8 only
              t[glue_t_bin(true, IMP_FINAL)], packed);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ workspace
struct ImpWs : GlueTrunkWs {
    float *u, *vv, *binc, *max0, *part;
    size_t total;
    bool ok;
};

static ImpWs imp_carve(void* ws, size_t bytes, int B, int R) {
    WsAlloc a(ws, bytes);
    ImpWs w;
    glue_carve_tokens(a, w, B, R, true);
    w.u = a.get<float>((size_t)B * (R + 64));
    w.vv = a.get<float>((size_t)B * (R + 64));
    w.binc = a.get<float>((size_t)B * R);  // dust-bin column of p
    w.max0 = a.get<float>((size_t)B * R);
    w.part = a.get<float>((size_t)B * (R / IMP_BAND) * R);  // column sums per row band
    glue_carve_pairs(a, w, B, R);
    w.total = a.off;
    w.ok = a.ok;
    return w;
}

extern "C" size_t imcui_hip_imp_workspace_bytes(int B, int ncap) {
    const int R = (int)align_up((size_t)(ncap > 0 ? ncap : 1), 128);
    return imp_carve(nullptr, 0, B, R).total;
}

// ------------------------------------------------------------------ kernels
// outputs preset to -1 / 0, scalings u = v = 1 (R + 1 entries: index n is the dust-bin)
__global__ __launch_bounds__(256) void imp_reset_kernel(int ncap, int R, float* __restrict__ u, float* __restrict__ v,
                                                        int* __restrict__ matches0, int* __restrict__ matches1,
                                                        float* __restrict__ ms0, float* __restrict__ ms1) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > R) return;
    u[(size_t)b * (R + 64) + i] = 1.0f;
    v[(size_t)b * (R + 64) + i] = 1.0f;
    if (i < ncap) {
        const size_t o = (size_t)b * ncap + i;
        matches0[o] = -1, matches1[o] = -1;
        ms0[o] = 0.0f, ms1[o] = 0.0f;
    }
}

// one wave per token row: descriptor -> d128 (padded rows cleared), key-point normalisation and the first encoder layer
// relu(W0' [kx, ky, score] + b0') -> e32, identity rotation tables for the shared QKV epilogue
__global__ __launch_bounds__(256) void imp_init_kernel(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                       const float* __restrict__ sc0, const float* __restrict__ sc1,
                                                       const float* __restrict__ d0, const float* __restrict__ d1,
                                                       const int* __restrict__ cnt, int ncap, int R, float w0, float h0, float w1,
                                                       float h1, const float* __restrict__ k0w, float* __restrict__ d128,
                                                       float* __restrict__ e32, float* __restrict__ one, float* __restrict__ zero) {
    const int lane = threadIdx.x & 63;
    const int seq = blockIdx.y, b = seq >> 1, img = seq & 1;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= R) return;
    const int n = cnt[seq];
    const size_t row = (size_t)seq * R + i;
    if (lane >= 32) {
        one[row * 32 + lane - 32] = 1.0f;
        zero[row * 32 + lane - 32] = 0.0f;
        return;
    }
    if (i >= n) {
        *reinterpret_cast<float4*>(d128 + row * IMP_DESC + lane * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        e32[row * 32 + lane] = 0.0f;
        return;
    }
    const float* d = (img ? d1 : d0) + ((size_t)b * ncap + i) * IMP_DESC;
    *reinterpret_cast<float4*>(d128 + row * IMP_DESC + lane * 4) = *reinterpret_cast<const float4*>(d + lane * 4);
    const float* kp = (img ? kp1 : kp0) + ((size_t)b * ncap + i) * 2;
    const float s = (img ? sc1 : sc0)[(size_t)b * ncap + i];
    e32[row * 32 + lane] = glue_kenc0(kp, s, img ? w1 : w0, img ? h1 : h0, *reinterpret_cast<const float4*>(k0w + lane * 4));
}

// probe only: scores [B, ncap, ncap] -> the R-strided matrix
__global__ __launch_bounds__(256) void imp_stage_kernel(const float* __restrict__ src, const int* __restrict__ cnt, int ncap, int R,
                                                        float* __restrict__ sim) {
    const int b = blockIdx.z, i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt[2 * b] || j >= cnt[2 * b + 1]) return;
    sim[((size_t)b * R + i) * R + j] = src[((size_t)b * ncap + i) * ncap + j];
}

__global__ __launch_bounds__(256) void imp_copy_kernel(const float* __restrict__ src, int sstride, int n, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[(size_t)blockIdx.y * n + i] = src[(size_t)blockIdx.y * sstride + i];
}

// the 64 lane values folded as a tree, every lane ends with the same bits: t = s[l] + s[l ^ 32], then ^ 16, ... ^ 1
__device__ __forceinline__ float imp_wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
    return s;
}

// a row of the matrix in registers: lane holds columns k * 256 + lane * 4 .. + 3, k < IMP_NK; entries outside the n1 real
// columns (and rows that do not exist) are 0.  Padding of the matrix is never read as a value: it may hold anything.
__device__ __forceinline__ void imp_load_row(float4 (&z)[IMP_NK], const float* __restrict__ row, bool ok, int lane, int n1) {
    const int nch = (n1 + 255) >> 8;
#pragma unroll
    for (int k = 0; k < IMP_NK; ++k) {
        const int j = k * 256 + lane * 4;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && k < nch && j < n1) t = *reinterpret_cast<const float4*>(row + j);
        if (j + 1 >= n1) t.y = 0.0f;
        if (j + 2 >= n1) t.z = 0.0f;
        if (j + 3 >= n1) t.w = 0.0f;
        z[k] = t;
    }
}

// Row soft-max with the dust-bin column, one wave per row: p_ij = exp(M_ij - max) / sum over the n1 columns and the
// dust-bin entry bin_score; replaces M by p, the dust-bin entry p[i][n1] goes to binc.
// Sum order: per lane k-major then x, y, z, w; lanes as a tree (imp_wave_sum); the dust-bin term last.
__global__ __launch_bounds__(256) void imp_softmax_kernel(float* __restrict__ sim, const int* __restrict__ cnt,
                                                          const int* __restrict__ active, int R, const float* __restrict__ binp,
                                                          float binv, float* __restrict__ binc) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    if (i >= n0) return;
    const float alpha = binp ? binp[0] : binv;
    float* row = sim + ((size_t)b * R + i) * R;
    float4 z[IMP_NK];
    imp_load_row(z, row, true, lane, n1);
    float mx = alpha;
#pragma unroll
    for (int k = 0; k < IMP_NK; ++k) {
        const int j = k * 256 + lane * 4;
        if (j < n1) mx = fmaxf(mx, z[k].x);
        if (j + 1 < n1) mx = fmaxf(mx, z[k].y);
        if (j + 2 < n1) mx = fmaxf(mx, z[k].z);
        if (j + 3 < n1) mx = fmaxf(mx, z[k].w);
    }
    mx = wave_max(mx);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < IMP_NK; ++k) {
        const int j = k * 256 + lane * 4;
        z[k].x = (j < n1) ? expf(z[k].x - mx) : 0.0f;
        z[k].y = (j + 1 < n1) ? expf(z[k].y - mx) : 0.0f;
        z[k].z = (j + 2 < n1) ? expf(z[k].z - mx) : 0.0f;
        z[k].w = (j + 3 < n1) ? expf(z[k].w - mx) : 0.0f;
        s = s + z[k].x;
        s = s + z[k].y;
        s = s + z[k].z;
        s = s + z[k].w;
    }
    const float eb = expf(alpha - mx);
    const float tot = imp_wave_sum(s) + eb;
#pragma unroll
    for (int k = 0; k < IMP_NK; ++k) {
        const int j = k * 256 + lane * 4;
        if (j < n1) *reinterpret_cast<float4*>(row + j) = make_float4(z[k].x / tot, z[k].y / tot, z[k].z / tot, z[k].w / tot);
    }
    if (lane == 0) binc[(size_t)b * R + i] = eb / tot;
}

// One Sinkhorn round, first half: workgroup = IMP_BAND rows of one pair (wave w: rows 2w, 2w + 1 of the band), a row lives
// in registers (IMP_NK float4 per lane = 4096 columns, so one regime serves every ncap the call accepts).
//   u_i = 1 / ((sum_j p_ij v_j + p_i,bin v_bin) + eps)          sum order as in the soft-max, v staged in LDS
//   part[band][j] = fold over waves 0..7 of (p_ij u_i + p_i'j u_i')   with the NEW u: the matrix is read once per round
// Block index == number of bands: the dust-bin row, u_bin = n1 / (sum_{j <= n1} v_j / (n1 + 1) + eps).
__global__ __launch_bounds__(512) void imp_round_kernel(const float* __restrict__ sim, const int* __restrict__ cnt,
                                                        const int* __restrict__ active, int R, const float* __restrict__ binc,
                                                        const float* __restrict__ v, float* __restrict__ u, float* __restrict__ part) {
    __shared__ float4 lds4[(8 * IMP_HALF + IMP_COLS + 64) / 4];
    float* lm = reinterpret_cast<float*>(lds4);  // [8 waves][2048]: a wave's column sums, one half of the columns at a time
    float* lv = lm + 8 * IMP_HALF;               // [4096 + 64]: staged v, 0 beyond the dust-bin entry
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    const int nbands = (n0 + IMP_BAND - 1) / IMP_BAND;
    const int band = blockIdx.x;
    if (band > nbands) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* vb = v + (size_t)b * (R + 64);
    float* ub = u + (size_t)b * (R + 64);
    for (int j = tid; j < IMP_COLS + 64; j += 512) lv[j] = (j <= n1) ? vb[j] : 0.0f;
    __syncthreads();
    if (band == nbands) {
        const float dbrow = 1.0f / (float)(n1 + 1);
        float s = 0.0f;
        for (int j = tid; j <= n1; j += 512) s = s + dbrow * lv[j];
        s = imp_wave_sum(s);
        if (lane == 0) lm[w] = s;
        __syncthreads();
        if (tid == 0) {
            float S = lm[0];
            for (int k = 1; k < 8; ++k) S = S + lm[k];
            ub[n0] = IMP_ROW_BIN_MASS(n0, n1) / (S + IMP_EPS);
        }
        return;
    }
    const float* simb = sim + (size_t)b * R * R;
    const float* bincb = binc + (size_t)b * R;
    const float vbin = lv[n1];
    float4 acc[IMP_NK];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int i = band * IMP_BAND + 2 * w + rr;
        const bool ok = i < n0;  // wave-uniform
        float4 z[IMP_NK];
        imp_load_row(z, simb + (size_t)i * R, ok, lane, n1);
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < IMP_NK; ++k) {
            const float4 vj = *reinterpret_cast<const float4*>(lv + k * 256 + lane * 4);
            s = s + z[k].x * vj.x;
            s = s + z[k].y * vj.y;
            s = s + z[k].z * vj.z;
            s = s + z[k].w * vj.w;
        }
        s = imp_wave_sum(s);
        float ui = 0.0f;
        if (ok) {
            ui = 1.0f / ((s + bincb[i] * vbin) + IMP_EPS);
            if (lane == 0) ub[i] = ui;
        }
#pragma unroll
        for (int k = 0; k < IMP_NK; ++k) {
            if (rr == 0)
                acc[k] = make_float4(z[k].x * ui, z[k].y * ui, z[k].z * ui, z[k].w * ui);
            else
                acc[k] = make_float4(acc[k].x + z[k].x * ui, acc[k].y + z[k].y * ui, acc[k].z + z[k].z * ui, acc[k].w + z[k].w * ui);
        }
    }
    const int nch = (n1 + 255) >> 8;
    float* pb = part + ((size_t)b * (R / IMP_BAND) + band) * R;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half * 8 >= nch) break;  // block-uniform
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<float4*>(lm + w * IMP_HALF + k * 256 + lane * 4) = acc[half * 8 + k];
        __syncthreads();
        float4 S = *reinterpret_cast<const float4*>(lm + 4 * tid);
#pragma unroll
        for (int ww = 1; ww < 8; ++ww) {
            const float4 t = *reinterpret_cast<const float4*>(lm + ww * IMP_HALF + 4 * tid);
            S = make_float4(S.x + t.x, S.y + t.y, S.z + t.z, S.w + t.w);
        }
        const int col = half * IMP_HALF + 4 * tid;
        if (col < R) *reinterpret_cast<float4*>(pb + col) = S;
        __syncthreads();
    }
}

// Second half of the round: v_j = 1 / ((sum over bands + u_bin / (n1 + 1)) + eps).  Block = 256 columns x IMP_MG groups; group g
// folds bands 16 g .. 16 g + 15 in order, then the groups are folded in order.  The last block is the dust-bin column:
// v_bin = n0 / ((sum_i p_i,bin u_i + u_bin / (n1 + 1)) + eps), thread-strided partial sums, wave tree, waves in order.
__global__ __launch_bounds__(64 * IMP_MG) void imp_merge_kernel(const int* __restrict__ cnt, const int* __restrict__ active, int R,
                                                                const float* __restrict__ binc, const float* __restrict__ u,
                                                                const float* __restrict__ part, float* __restrict__ v) {
    __shared__ float sm[IMP_MG][256];
    const int b = blockIdx.y;
    if (!active[b]) return;
    const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const float* ub = u + (size_t)b * (R + 64);
    const float dbrow = 1.0f / (float)(n1 + 1);
    const float rowterm = dbrow * ub[n0];
    if (blockIdx.x == gridDim.x - 1) {
        const float* bincb = binc + (size_t)b * R;
        float s = 0.0f;
        for (int i = threadIdx.x; i < n0; i += 64 * IMP_MG) s = s + bincb[i] * ub[i];
        s = imp_wave_sum(s);
        if (c == 0) sm[g][0] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            float S = sm[0][0];
            for (int gg = 1; gg < IMP_MG; ++gg) S = S + sm[gg][0];
            v[(size_t)b * (R + 64) + n1] = IMP_COL_BIN_MASS(n0, n1) / ((S + rowterm) + IMP_EPS);
        }
        return;
    }
    if ((int)blockIdx.x * 256 >= n1) return;
    const int nbands = (n0 + IMP_BAND - 1) / IMP_BAND;
    const int j = blockIdx.x * 256 + c * 4;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < n1) {
        const int k1 = min(nbands, (g + 1) * IMP_MG);
        const float* p = part + (size_t)b * (R / IMP_BAND) * R + j;
#pragma unroll 4
        for (int k = g * IMP_MG; k < k1; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(p + (size_t)k * R);
            t = make_float4(t.x + a.x, t.y + a.y, t.z + a.z, t.w + a.w);
        }
    }
    *reinterpret_cast<float4*>(&sm[g][c * 4]) = t;
    __syncthreads();
    const int jj = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < 256 && jj < n1) {
        float r = sm[0][threadIdx.x];
        for (int gg = 1; gg * IMP_MG < nbands; ++gg) r = r + sm[gg][threadIdx.x];
        v[(size_t)b * (R + 64) + jj] = 1.0f / ((r + rowterm) + IMP_EPS);
    }
}

// the assignment stage on w.sim: soft-max, `iterations` rounds, arg-maxima, filter
static int imp_assign(imcui_hip_t* h, const ImpWs& w, int B, int ncap, int R, const float* binp, float binv, int iterations, float thr,
                      int* matches0, int* matches1, float* mscores0, float* mscores1, hipStream_t stream) {
    const dim3 blk(256);
    hipLaunchKernelGGL(imp_softmax_kernel, dim3(R / 4, B), blk, 0, stream, w.sim, w.cnt, w.active, R, binp, binv, w.binc);
    const dim3 rg(R / IMP_BAND + 1, B), mg(cdiv(R, 256) + 1, B);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(imp_round_kernel, rg, dim3(512), 0, stream, w.sim, w.cnt, w.active, R, w.binc, w.vv, w.u, w.part);
        hipLaunchKernelGGL(imp_merge_kernel, mg, dim3(64 * IMP_MG), 0, stream, w.cnt, w.active, R, w.binc, w.u, w.part, w.vv);
    }
    glue_match<ImpScore, false>(w, w.u, w.vv, w.max0, B, ncap, R, thr, matches0, matches1, mscores0, mscores1, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ probe: the assignment stage alone
extern "C" int imcui_hip_imp_ot_probe(imcui_hip_t* h, const float* scores, int B, int ncap, const int* n0, const int* n1, float bin_score,
                                      int iterations, double p, int* matches0, int* matches1, float* mscores0, float* mscores1,
                                      float* u_out, float* v_out, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (ncap <= 0 || ncap > IMP_COLS) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: ncap=%d outside 1..%d", ncap, IMP_COLS);
    if (iterations < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: iterations=%d", iterations);
    if (!scores || !n0 || !n1 || !matches0 || !matches1 || !mscores0 || !mscores1) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: null argument");
    const int R = (int)align_up((size_t)ncap, 128);
    ImpWs w = imp_carve(ws, ws_bytes, B, R);
    if (!ws || !w.ok) return imcui_set_err(h, IMCUI_ERR_WS, "imp: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipLaunchKernelGGL(glue_pairs_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, n0, n1, B, w.cnt, w.active);
    hipLaunchKernelGGL(imp_reset_kernel, dim3(cdiv(R + 1, 256), B), dim3(256), 0, stream, ncap, R, w.u, w.vv, matches0, matches1, mscores0,
                       mscores1);
    hipLaunchKernelGGL(imp_stage_kernel, dim3(cdiv(ncap, 256), ncap, B), dim3(256), 0, stream, scores, w.cnt, ncap, R, w.sim);
    int rc;
    IMCUI_RUN(imp_assign(h, w, B, ncap, R, nullptr, bin_score, iterations, (float)p, matches0, matches1, mscores0, mscores1, stream));
    // u, v [B, ncap + 1]: entry n0 / n1 of a pair is its dust-bin (entries beyond it are 1)
    if (u_out) hipLaunchKernelGGL(imp_copy_kernel, dim3(cdiv(ncap + 1, 256), B), dim3(256), 0, stream, w.u, R + 64, ncap + 1, u_out);
    if (v_out) hipLaunchKernelGGL(imp_copy_kernel, dim3(cdiv(ncap + 1, 256), B), dim3(256), 0, stream, w.vv, R + 64, ncap + 1, v_out);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ forward
extern "C" int imcui_hip_imp_forward(imcui_hip_t* h, const float* packed, int B, int ncap, const float* keypoints0, const float* keypoints1,
                                     const float* scores0, const float* scores1, const float* descriptors0, const float* descriptors1,
                                     const int* n0, const int* n1, float w0, float h0, float w1, float h1, int sinkhorn_iterations,
                                     double match_threshold, int* matches0, int* matches1, float* mscores0, float* mscores1, void* ws,
                                     size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (ncap <= 0 || ncap > IMP_COLS) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: ncap=%d outside 1..%d", ncap, IMP_COLS);
    if (sinkhorn_iterations < 0) return imcui_set_err(h, IMCUI_ERR_ARG, "imp: sinkhorn_iterations=%d", sinkhorn_iterations);
    if (!packed || !keypoints0 || !keypoints1 || !scores0 || !scores1 || !descriptors0 || !descriptors1 || !n0 || !n1 || !matches0 ||
        !matches1 || !mscores0 || !mscores1)
        return imcui_set_err(h, IMCUI_ERR_ARG, "imp: null argument");
    const int R = (int)align_up((size_t)ncap, 128);
    ImpWs w = imp_carve(ws, ws_bytes, B, R);
    if (!ws || !w.ok) return imcui_set_err(h, IMCUI_ERR_WS, "imp: workspace too small (%zu < %zu)", ws_bytes, w.total);
    const GlueLayout l = glue_layout(true);
    const float* P = packed;
    int rc;

    hipLaunchKernelGGL(glue_pairs_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, n0, n1, B, w.cnt, w.active);
    hipLaunchKernelGGL(imp_reset_kernel, dim3(cdiv(R + 1, 256), B), dim3(256), 0, stream, ncap, R, w.u, w.vv, matches0, matches1, mscores0,
                       mscores1);
    hipLaunchKernelGGL(imp_init_kernel, dim3(R / 4, 2 * B), dim3(256), 0, stream, keypoints0, keypoints1, scores0, scores1, descriptors0,
                       descriptors1, w.cnt, ncap, R, w0, h0, w1, h1, P + l.k0, w.d128, w.ctx, w.one, w.zero);
    IMCUI_CHECK_LAUNCH(h);

    IMCUI_RUN(glue_trunk(h, P, l, w, B, R, GLUE_HEADS, false, stream));  // (no IMCUI_LG_FFN_UNFUSED switch here)
    return imp_assign(h, w, B, ncap, R, P + l.bin, 0.0f, sinkhorn_iterations, (float)match_threshold, matches0, matches1, mscores0,
                      mscores1, stream);
}
