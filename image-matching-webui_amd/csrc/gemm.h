// MFMA GEMM with fused epilogues:  C = epi(A[M,K] * W[N,K]^T + bias).
// Both operands are K-contiguous (nn.Linear weight layout / NHWC activations).
// Two arithmetic modes (imcui_hip_s::precision):
//   0  exact f32 on v_mfma_f32_32x32x2_f32
//   1  3 x f16 split (hi/lo) on v_mfma_f32_32x32x16_f16, f32 accumulate (~fp32 accuracy, ~5x rate)
#pragma once
#include "common.h"

enum GemmEpi {
    EPI_BIAS = 0,   // C = (acc + bias) * alpha          (bias may be null)
    EPI_RELU = 1,   // C = relu(acc + bias)
    EPI_RESID = 2,  // C += acc + bias                  (in-place residual)
    EPI_QKV = 3,    // LightGlue SelfBlock: bias, RoPE on q/k, q *= alpha, head-major split
    EPI_CROSS = 4,  // LightGlue CrossBlock: [qk | v] = bias, qk *= alpha, head-major split
    EPI_CONV = 5,   // C = act(acc + bias + resid): act 0 none / 1 ReLU / 2 LeakyReLU(0.01) / 3 GELU (erf)
    // (6 was EPI_SIMSTAT, rounds 3-4: the similarity stored AND reduced to soft-max partials -- replaced by simred.hip, which stores nothing)
    // ViT blocks of the DUSt3R / MASt3R networks (gemm_wreg_kernel only): the output features are `heads` x 64 wide blocks of
    // q / k / v in that order starting at block `role0` (0: q, 1: k, 2: v -- self attention [q | k | v]: role0 = 0, N = 3 C; the
    // cross-attention key / value projection [k | v]: role0 = 1, N = 2 C; its query projection: role0 = 0, N = C).  q and k get
    // CroCo's RoPE2D from the tables rope_cos / rope_sin [rows_per_seq][32] (entry 16 half + i = angle of the y (half 0) / x
    // (half 1) position of the token times inv_freq[i]; inside a 32-feature half feature i < 16 pairs with i + 16), q *= alpha;
    // everything leaves as f16 hi / lo planes, q / k [seq][head][row][64], v transposed [seq][head][64][row].
    EPI_QKV_VIT = 7,
    // NO matrix output: the similarity tile of two activation matrices (batched) is reduced while it is parked in LDS to the
    // nearest-neighbour partials of the mutual-NN matcher -- per row (best value, its column, second best value) over the tile's
    // 128 columns -> st_rpm / st_rpi / st_rps [batch][st_nct][st_rpitch], per column over each 64-row half -> st_cpm / st_cpi /
    // st_cps [batch][st_nrh][st_cpitch]; ties keep the lowest index (split mode, f32 B operand; nn.hip)
    EPI_NNSTAT = 8,
};

struct GemmP {
    int epi = EPI_BIAS;
    const float* A = nullptr;   // [M, K1] (or [M, K] when A2 == nullptr)
    long lda = 0;
    const float* A2 = nullptr;  // optional second K-slab: k >= K1 comes from A2[:, k - K1]
    long lda2 = 0;
    int K1 = 0;
    const float* W = nullptr;  // [N, K] f32
    long ldw = 0;
    // pre-split weights for precision 1 (optional; when null W is split on the fly): f16 planes of
    // W * 2^e in FRAGMENT-MAJOR order [ceil(N/32)][K/16][64 lanes][8 halves] (split_weights_frag_host),
    // wscale -> 2^-e
    const unsigned short* Wh = nullptr;
    const unsigned short* Wl = nullptr;
    const float* wscale = nullptr;
    const float* bias = nullptr;  // [N] or null
    float* C = nullptr;           // [M, N] (EPI_BIAS / RELU / RESID)
    long ldc = 0;
    int M = 0, N = 0, K = 0;
    float alpha = 1.0f;
    int group_rows = 0;  // > 1: tile order in groups of this many 128-row panels (L2 re-use when both operands are large)
    // ragged sequences: row tile r0 belongs to sequence r0 / rows_per_seq; tiles whose first
    // row is >= cnt[seq] (or whose pair active[seq >> 1] == 0) are skipped.
    const int* cnt = nullptr;
    const int* active = nullptr;
    int rows_per_seq = 0;
    // per-pair weight selection: W += (wsel[seq >> 1] + wsel_off) * w_stride, bias likewise
    const int* wsel = nullptr;
    int wsel_off = 0;
    long w_stride = 0, b_stride = 0;
    // batched mode (blockIdx.z = batch): per-batch strides and dynamic M/N
    int batch = 1;
    long a_bs = 0, a2_bs = 0, w_bs = 0, c_bs = 0;
    const int* mcnt = nullptr;  // M for batch z = mcnt[z * cnt_stride]
    const int* ncnt = nullptr;  // N for batch z = ncnt[z * cnt_stride]
    int cnt_stride = 1;
    // EPI_QKV / EPI_CROSS outputs, head-major [seq][head][row_in_seq][64]
    float* Q = nullptr;
    float* Kt = nullptr;
    float* V = nullptr;
    int v_transposed = 0;  // 1: V is written as V^T [seq][head][64][rows_per_seq] (split attention)
    int split_out = 0;     // 1: Q / K / V^T are written as f16 hi / lo planes (lo plane at +plane_halves)
    size_t plane_halves = 0;
    // implicit im2col (enabled when conv_k > 0): A is an NHWC image [B, hin, win, cin], row m of the
    // GEMM is output pixel m of a conv_k x conv_k convolution (stride, zero padding), K = conv_k^2 * cin
    // ordered (tap, channel) -- the layout of pack_conv_gemm(); cin % 32 == 0
    int conv_k = 0, conv_stride = 1, conv_pad = 0, conv_hin = 0, conv_win = 0, conv_hout = 0, conv_wout = 0, conv_cin = 0;
    const float* resid = nullptr;  // EPI_CONV: [M, N] added before the activation (may alias C)
    long ldr = 0;
    // EPI_CONV, split kernels: the residual is the bilinear x2 up-sampling of the NHWC map `resid` [images, rup_h, rup_w, ldr]
    // (rows of the GEMM = pixels of the 2 rup_h x 2 rup_w maps), evaluated in the epilogue instead of being materialised;
    // rup_align = align_corners of the interpolation (LoFTR: 1, EfficientLoFTR: 0).  0 = plain [M, N] residual.
    int rup_h = 0, rup_w = 0, rup_align = 1;
    int act = 0;
    // 1: ONE f16 product per element pair (hi planes only, f32 accumulate) instead of the three of the split arithmetic: 11-bit
    // operands, the class of a bf16 / fp16 autocast run.  EPI_CONV with pre-split weight planes only.
    int single = 0;
    float *st_rpm = nullptr, *st_rps = nullptr, *st_cpm = nullptr, *st_cps = nullptr;  // EPI_NNSTAT partials: best / second best
    int st_nct = 0, st_nrh = 0;                                                         // partial slots per row / per column
    int *st_rpi = nullptr, *st_cpi = nullptr;                                           // EPI_NNSTAT: arg-best partials
    long st_rpitch = 0, st_cpitch = 0;                                                  // EPI_NNSTAT: entries per partial slot (>= M rows / >= N columns)
    const float* rope_cos = nullptr;  // [rows, 32]
    const float* rope_sin = nullptr;
    int heads = 4;
    int role0 = 0;  // EPI_QKV_VIT: role (0 q, 1 k, 2 v) of the first heads x 64 block of output features
    // EPI_QKV_VIT with sequences on token grids of different shapes: first table row of each sequence's grid (device, per sequence);
    // nullptr: every sequence reads the table from row 0
    const int* rope_seq_row0 = nullptr;
    // LayerNorm folded into the layer (DUSt3R; gemm_wreg_kernel, EPI_CONV and EPI_QKV_VIT only): A holds the RAW rows x, the weights carry
    // gamma and the bias carries W beta (pack time); the kernel centres every row while it stages it (x - mean_row) and the epilogue
    // applies  out = rstd_row acc + bias[n]  where the plain layer computes acc + bias[n].  ln_stats [M][2] = (mean, rstd) of every row
    // of A.  ln_rowsum [N] = sum_k W[n][k] of the packed weights (+ ln_stride floats per weight set) served the uncentred fold,
    // rstd (acc - mean rowsum), and is no longer read: the packed DUSt3R format still carries it
    const float* ln_stats = nullptr;
    const float* ln_rowsum = nullptr;
    long ln_stride = 0;
    // implicit im2col with dilated taps (conv_k > 0): tap (ky, kx) reads input pixel (oy stride - pad + ky conv_dil, ox stride - pad +
    // kx conv_dil).  0 / 1 = no dilation: the launch is the undilated one, instantiation and bits.  > 1 selects the ASRC = 2
    // instantiations (GR_EXACT_DIL / GR_CONVD_*); the single-product arithmetic is not built for them
    // Dilated launches with K >= 2048 sum in two levels (gemm.hip, GEMM_CHUNK_MIN_K): the exact kernel in place, the split arithmetic (pre-split planes) on the 128-column kernel's CHUNK instantiation, route GR_CONVD_128 whatever N
    int conv_dil = 0;
};

// Route of a launch: which kernel instantiation gemm_launch chose, GEMM_ROUTE(kind, epilogue).  The launch sites store it in the
// handle (imcui_hip_gemm_last_route / _route_counts), so the report cannot disagree with what ran.  Values are part of the test
// ABI (tests/test_gpu_gemm_variants.py mirrors them; a CPU test compares the two).
enum GemmRouteKind {
    GR_NONE = 0,
    GR_EXACT = 1,            // gemm_kernel<EPI>
    GR_SPLIT_F32B = 2,       // gemm_split_kernel<EPI, 0, false, 2>: f32 B operand split on the fly
    GR_SPLIT_128 = 3,        // gemm_split_kernel<EPI, 0, true, 2>
    GR_SPLIT_256 = 4,        // gemm_split_kernel<EPI, 0, true, 4>
    GR_SPLIT_128_SINGLE = 5, // gemm_split_kernel<EPI_CONV, 0, true, 2, true>
    GR_SPLIT_256_SINGLE = 6, // gemm_split_kernel<EPI_CONV, 0, true, 4, true>
    GR_CONV_F32B = 7,        // gemm_split_kernel<EPI_CONV, 1, false, 2>
    GR_CONV_128 = 8,         // gemm_split_kernel<EPI_CONV, 1, true, 2>
    GR_CONV_256 = 9,         // gemm_split_kernel<EPI_CONV, 1, true, 4>
    GR_CONV_128_SINGLE = 10, // gemm_split_kernel<EPI_CONV, 1, true, 2, true>
    GR_CONV_256_SINGLE = 11, // gemm_split_kernel<EPI_CONV, 1, true, 4, true>
    GR_WREG_ROLLED = 12,     // gemm_wreg_kernel<EPI, false, false, 4>
    GR_WREG_PIPE = 13,       // gemm_wreg_kernel<EPI, false, true, 4>
    GR_WREG_ROLLED_SINGLE = 14,  // gemm_wreg_kernel<EPI_CONV, true, false, 4>
    GR_WREG_PIPE_SINGLE = 15,    // gemm_wreg_kernel<EPI_CONV, true, true, 4>
    GR_WREG_MT2 = 16,        // gemm_wreg_kernel<EPI, false, true, 2>
    GR_WREG_MT1 = 17,        // gemm_wreg_kernel<EPI, false, true, 1>
    GR_EXACT_DIL = 18,       // gemm_kernel<EPI_CONV, true>: dilated taps (GemmP.conv_dil > 1)
    GR_CONVD_F32B = 19,      // gemm_split_kernel<EPI_CONV, 2, false, 2>
    GR_CONVD_128 = 20,       // gemm_split_kernel<EPI_CONV, 2, true, 2> (K >= 2048: <EPI_CONV, 2, true, 2, false, true>)
    GR_CONVD_256 = 21,       // gemm_split_kernel<EPI_CONV, 2, true, 4>
    GR_NKIND = 22
};
#define GEMM_ROUTE(kind, epi) ((kind) * 16 + (epi))
static_assert(GR_NKIND * 16 <= IMCUI_GEMM_ROUTE_SLOTS, "route table of imcui_hip_s too small");
#define GEMM_CHUNK_MIN_K 2048  // dilated launches (the exact kernel; the split kernel on pre-split planes) sum in two levels from this K on (gemm.hip)
// undilated launches of the exact kernel take its two-level instantiation from this K on: one chain holds the 2e-6 bar of the exact mode
// at K = 2048 .. 2400 and misses it at K = 4608 (tests/test_gpu_gemm_variants.py, the longk_* cases), and that instantiation runs at a
// third of the occupancy, so nothing below gets it
#define GEMM_EXACT_CHUNK_MIN_K 4096

// What a launch ran with besides its route: the route names the kernel instantiation, but most of the hand-written index arithmetic
// (tap walk, borders, device-side counts, output strides, residuals) is chosen by the parameters.  gemm_features derives the mask from
// the parameters of the launch and every gemm_route_note call passes it, so the mask cannot disagree with what ran; the handle keeps
// the OR per route (imcui_hip_gemm_route_features).  Host code only, O(1).  Values are part of the test interface
// (imcui_hip/backend.py GEMM_FEATURES; a CPU test compares the two).
enum GemmFeature {
    GF_CONV_K1 = 1,             // implicit im2col, conv_k == 1
    GF_CONV_K3 = 2,             // ... conv_k == 3
    GF_CONV_K5 = 4,             // ... conv_k == 5
    GF_CONV_KOTHER = 8,         // ... any other conv_k (2: R2D2's last layers)
    GF_STRIDE2 = 16,            // conv_stride == 2
    GF_STRIDE_OTHER = 32,       // conv_stride > 2 (own bit: the tests of stride 2 say nothing about a larger step between output pixels)
    GF_PAD_NOT_SAME = 64,       // conv_pad != ((conv_k - 1) dilation) / 2: valid convolutions and every other pad
    GF_DILATED = 128,           // conv_dil > 1
    GF_CHUNK = 256,             // the two-level sum (dilated, K >= GEMM_CHUNK_MIN_K, exact kernel or pre-split planes; undilated exact kernel, K >= GEMM_EXACT_CHUNK_MIN_K)
    GF_LONG_K = 512,            // K >= GEMM_CHUNK_MIN_K summed in ONE level: every other launch
    GF_RESID = 1024,            // plain residual (EPI_CONV with resid, EPI_RESID)
    GF_RUP = 2048,              // bilinear x2 up-sampled residual (rup_h > 0)
    GF_ACT1 = 4096,             // EPI_CONV activation 1 (ReLU)
    GF_ACT2 = 8192,             // ... 2 (LeakyReLU)
    GF_ACT3 = 16384,            // ... 3 (GELU)
    GF_LDC = 32768,             // ldc != N (row-major epilogues)
    GF_N_MOD32 = 65536,         // N % 32 != 0: a partial weight fragment, scalar stores
    GF_N_MOD_TILE = 131072,     // N % (column tile of the route: 256 on the *_256 and wreg kinds, else 128) != 0
    GF_M_SMALL = 262144,        // M < 128: a single partial row tile
    GF_A2 = 524288,             // second K slab
    GF_BATCH = 1048576,         // batch > 1
    GF_MCNT = 2097152,          // device-side row counts
    GF_NCNT = 4194304,          // device-side column counts
    GF_CONV_BATCHED = 8388608,  // implicit im2col together with (batch > 1 or mcnt): the pixel decode runs on per-item row counts
    GF_CNT = 16777216,          // ragged sequences (cnt)
    GF_ACTIVE = 33554432,       // per-pair active flags
    GF_WSEL = 67108864,         // per-pair weight selection
    GF_LN = 134217728,          // folded LayerNorm (ln_stats)
    GF_ALPHA = 268435456,       // alpha != 1 on an epilogue that reads it (EPI_BIAS and the attention layouts)
    GF_NO_BIAS = 536870912,     // null bias
    GF_GROUP_ROWS = 1073741824  // group_rows > 1: the tiles are walked in another order (gemm_tile.h), own bit since the row / column decode differs
};
static inline int gemm_features(const GemmP& p, int kind) {
    int f = 0;
    const bool row_major = p.epi == EPI_BIAS || p.epi == EPI_RELU || p.epi == EPI_RESID || p.epi == EPI_CONV;
    if (p.conv_k > 0) {
        const int dil = p.conv_dil > 1 ? p.conv_dil : 1;
        f |= p.conv_k == 1 ? GF_CONV_K1 : p.conv_k == 3 ? GF_CONV_K3 : p.conv_k == 5 ? GF_CONV_K5 : GF_CONV_KOTHER;
        f |= p.conv_stride == 2 ? GF_STRIDE2 : p.conv_stride > 2 ? GF_STRIDE_OTHER : 0;
        f |= p.conv_pad != (p.conv_k - 1) * dil / 2 ? GF_PAD_NOT_SAME : 0;
        f |= dil > 1 ? GF_DILATED : 0;
        f |= p.batch > 1 || p.mcnt ? GF_CONV_BATCHED : 0;
    }
    const bool chunk = (kind == GR_EXACT && p.K >= GEMM_EXACT_CHUNK_MIN_K) || ((kind == GR_EXACT_DIL || kind == GR_CONVD_128) && p.K >= GEMM_CHUNK_MIN_K);
    f |= chunk ? GF_CHUNK : p.K >= GEMM_CHUNK_MIN_K ? GF_LONG_K : 0;
    if (p.rup_h > 0)
        f |= GF_RUP;
    else if (p.epi == EPI_RESID || (p.epi == EPI_CONV && p.resid))
        f |= GF_RESID;
    if (p.epi == EPI_CONV) f |= p.act == 1 ? GF_ACT1 : p.act == 2 ? GF_ACT2 : p.act == 3 ? GF_ACT3 : 0;
    f |= row_major && p.ldc != p.N ? GF_LDC : 0;
    f |= p.N % 32 ? GF_N_MOD32 : 0;
    const bool wide = kind == GR_SPLIT_256 || kind == GR_SPLIT_256_SINGLE || kind == GR_CONV_256 || kind == GR_CONV_256_SINGLE || kind == GR_CONVD_256 ||
                      (kind >= GR_WREG_ROLLED && kind <= GR_WREG_MT1);
    f |= p.N % (wide ? 256 : 128) ? GF_N_MOD_TILE : 0;
    f |= p.M < 128 ? GF_M_SMALL : 0;
    f |= p.A2 ? GF_A2 : 0;
    f |= p.batch > 1 ? GF_BATCH : 0;
    f |= p.mcnt ? GF_MCNT : 0;
    f |= p.ncnt ? GF_NCNT : 0;
    f |= p.cnt ? GF_CNT : 0;
    f |= p.active ? GF_ACTIVE : 0;
    f |= p.wsel ? GF_WSEL : 0;
    f |= p.ln_stats ? GF_LN : 0;
    f |= p.alpha != 1.0f && (p.epi == EPI_BIAS || p.epi == EPI_QKV || p.epi == EPI_CROSS || p.epi == EPI_QKV_VIT) ? GF_ALPHA : 0;
    f |= p.bias == nullptr ? GF_NO_BIAS : 0;
    f |= p.group_rows > 1 ? GF_GROUP_ROWS : 0;
    return f;
}
static inline void gemm_route_note(imcui_hip_s* h, const GemmP& p, int kind, int epi) {
    const int r = GEMM_ROUTE(kind, epi);
    h->gemm_last_route = r;
    ++h->gemm_route_count[r];
    h->gemm_route_features[r] |= gemm_features(p, kind);
}

int gemm_launch(imcui_hip_s* h, const GemmP& p, hipStream_t stream);
// gemm_wreg.hip: the weights-in-registers kernel for projection layers (split mode, pre-split weight planes); gemm_launch
// routes eligible launches to it
bool gemm_wreg_ok(const imcui_hip_s* h, const GemmP& p);
void gemm_wreg_launch(imcui_hip_s* h, const GemmP& p, hipStream_t stream);

// host: OIHW conv weight -> GEMM weight [Cout][tap][Cin] (K order of the implicit im2col)
void pack_conv_gemm(const float* w_oihw, int Cout, int Cin, int ksize, int Cin_pad, float* dst);
// host: split an [n] f32 array into f16 hi / lo planes of w * 2^e; returns 2^-e
float split_weights_host(const float* w, size_t n, unsigned short* hi, unsigned short* lo);
// host: the same for a GEMM weight [N][K], planes written fragment-major with rows padded to 32
float split_weights_frag_host(const float* w, int N, int K, unsigned short* hi, unsigned short* lo);
