// Fused transformer FFN of the LightGlue / SuperGlue blocks (3 x f16 split mode):
//   x <- x + W2 * GELU(LayerNorm(W1 * [x | ctx] + b1)) + b2          (512 hidden features, 256-wide residual stream)
//   x <- x + W2 * ReLU(W1 * [x | ctx] + b1) + b2                     (act = 1: SuperGlue's MLP, BatchNorm folded)
//   x <- x + LayerNorm(W2 * act(W1 * [x | ctx]))                    (act = 2 / 3: the dense matchers' MLPs)
// one kernel per block instead of GEMM -> LayerNorm/GELU -> GEMM: the 512-wide hidden row never leaves the CU.
#pragma once
#include "common.h"

struct FfnP {
    const float* x = nullptr;    // [M, 256] residual stream (read as the first K slab and as the residual)
    const float* ctx = nullptr;  // [M, 256] attention context (second K slab; out_proj is folded into W1)
    float* out = nullptr;        // [M, 256], may alias x
    // fragment-major f16 hi / lo planes (split_weights_frag_host): W1 [512][512]; W2 [256][512] with its K axis in
    // the order ffn_permute_k() produces (the order GEMM 1's accumulators hand their features to GEMM 2)
    const unsigned short *w1h = nullptr, *w1l = nullptr, *w2h = nullptr, *w2l = nullptr;
    const float *s1 = nullptr, *s2 = nullptr;  // 2^-e scales of the planes (device)
    const float *b1 = nullptr, *gamma = nullptr, *beta = nullptr;  // [512]
    const float* b2 = nullptr;                                     // [256]
    // 0: LayerNorm(512) + GELU between the GEMMs (LightGlue); 1: ReLU (SuperGlue, BatchNorm folded into W1);
    // 2 / 3: LeakyReLU(0.01) / ReLU between the GEMMs and LayerNorm(256) (gamma, beta [256]) after the second, before the
    // residual (EfficientLoFTR / LoFTR coarse MLPs: x + LN(fc2(act(fc1([x | message])))), no biases: b1 = b2 = nullptr)
    int act = 0;
    int M = 0;
    // ragged sequences, as in GemmP (rows_per_seq % 128 == 0, sequence = row / rows_per_seq, pair = sequence >> 1): the unit that is
    // skipped is the launch's TOKEN TILE (128, 64 or 32 rows, see ffn_launch) -- a tile whose first row is >= cnt[seq], or whose pair
    // has active[pair] == 0, neither reads nor writes.  A live tile is computed and stored whole: its rows past cnt[seq] (up to
    // roundup(cnt[seq], tile)) are written with whatever the padding rows of x / ctx give; they never feed a live row.
    const int* cnt = nullptr;
    const int* active = nullptr;
    int rows_per_seq = 0;
    long long* dbg = nullptr;  // lab only: 8 wall-clock stamps per workgroup (phase boundaries, wave 0)
};

// Limit of the opt-in range check (imcui_hip_set_range_check): ffn_launch scans the two operands it can see, x and ctx.  The hidden
// activations are re-split into f16 planes INSIDE the kernel (between the two GEMMs) and are not scanned: in the LayerNorm + GELU mode
// they are bounded by |gamma| sqrt(512) + |beta|, in the ReLU / LeakyReLU modes (act 1, 2, 3) they are unbounded, and a hidden value
// beyond 65504 saturates its hi plane without raising the flag.

// Route of a launch: which kernel instantiation ffn_launch chose, FFN_ROUTE(kind, act); 0 = none (a refused or empty call).  The launch
// site stores it in the handle (imcui_hip_ffn_last_route / _route_counts), so the report cannot disagree with what ran; host code only.
// The kinds are the rows of ffn_launch's kernel table.  Values are part of the test ABI (imcui_hip/backend.py mirrors them; a CPU test
// compares the two).
enum FfnRouteKind {
    FR_T128_ROLLED = 0,  // lg_ffn_kernel<0, ACT, 4>: 128-token tile, rolled K loop (lab: IMCUI_FFN_VARIANT=0)
    FR_T128 = 1,         // lg_ffn_kernel<1, ACT, 4>
    FR_T64 = 2,          // lg_ffn_kernel<1, ACT, 2>
    FR_T32 = 3,          // lg_ffn_kernel<1, ACT, 1>
    FR_NKIND = 4
};
#define FFN_ROUTE(kind, act) (1 + (kind) * 4 + (act))
static_assert(FFN_ROUTE(FR_NKIND - 1, 3) < IMCUI_FFN_ROUTE_SLOTS, "route table of imcui_hip_s too small");
static inline void ffn_route_note(imcui_hip_s* h, int kind, int act) {
    const int r = FFN_ROUTE(kind, act);
    h->ffn_last_route = r;
    ++h->ffn_route_count[r];
}

int ffn_launch(imcui_hip_s* h, const FfnP& p, hipStream_t stream);

// host: dst[n][c] = src[n][ffn_k_source(c)] -- the K order of W2 the kernel expects (K = 512)
void ffn_permute_k(const float* src, int N, int K, float* dst);
