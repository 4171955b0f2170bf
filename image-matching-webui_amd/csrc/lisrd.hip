// LISRD's matcher (imcui/hloc/matchers/lisrd.py:122-149): the meta-weighted mutual nearest neighbour rule and the confidence of the
// matched pairs.  Every key-point carries four local descriptors (128-d, one per invariance) and four meta descriptors (Dm-d); the
// similarity of a pair is
//     sim(i, j) = sum_v softmax_v(<meta0[i][v], meta1[j][v]>) * <desc0[i][v], desc1[j][v]>,
// and the matcher only ever REDUCES it: row and column arg-maxima, the mutual check, a confidence per match.  Upstream materialises two
// [N, 4, M] tensors (2 x 67 MB at N = M = 2048); here neither they nor the N x M matrix exist.
//
// lisrd_match_kernel: a workgroup (4 waves) owns 128 rows of image 0 and walks the 64-column tiles of its column chunk; wave w owns rows
// 32 w .. + 31 of the block and both 32-column fragments of the tile.  For the variances v = 0 .. 3 in order the meta product (K = Dm)
// and the local product (K = 128) run on the matrix cores out of simred_pack()'s fragments (exact f32, or the three-product f16 split, in
// gemm_split_kernel's product order), and are folded into a running soft-max over v: per element a maximum, a denominator and a
// weighted numerator.  Two product accumulators and those three values per element are all that is live (2 x 32 + 3 x 32 registers).
// Accumulators hold sim^T as in simred.hip: a lane owns ONE row of sim per fragment, so everything per row is lane-local and carried
// across the tiles; per column the tile is parked in LDS column-major and reduced by four adjacent lanes.
//
// What this first version does NOT do (README, "LISRD matcher"): the fragments are read straight from global memory / L2 by every wave
// (no LDS ring, no LDS-DMA as in simred.hip), and image 0's fragments are re-read per column tile -- at Dm = 1024 they do not fit the
// register file.  The kernel is bound by L2 traffic, not by the matrix pipe; that is the first thing to rewrite.
//
// Equal similarities: the FIRST column (row) attaining the maximum wins, everywhere (tile, chunk and block merges ascend).  `torch.max`
// leaves the index among equal values open; this is the intended divergence.
#include <math.h>

#include "imcui_hip.h"
#include "simred.h"

#define LM_ROWS 128  // rows of image 0 per workgroup (= SR_TILE: the fragments of simred_pack cover multiples of it)
#define LM_CT 64     // columns per tile: two 32-column fragments
#define LM_PLD 132   // floats per parked column of 128 rows
#define LM_NV 4      // variances
#define LM_DESC 128  // width of a local descriptor

struct LisrdMatchP {
    // fragments of simred_pack(): [variance][batch][32-row fragment][K / 16][2 pieces][64 lanes] x 16 bytes
    const uint4 *Ad, *Am, *Bd, *Bm;
    long ad_s, am_s, bd_s, bm_s;  // uint4 per (variance, batch)
    int N, M, KSm, B;             // static maxima; KSm = Dm / 16
    const int *cnt0, *cnt1;       // [B] live rows / columns (device) or null
    int nchunk;
    float* r0;  // [B][nchunk][N] row best of the chunk and its first column
    int* ri;
    float* c0;  // [B][ceil(N / 128)][M] column best of the row block and its first row
    int* ci;
};

// acc[n] += B fragment n (columns) x A fragment (rows) over KS k-steps of 16
template <bool F32>
__device__ __forceinline__ void lm_product(const uint4* __restrict__ ap, const uint4* __restrict__ bp0, const uint4* __restrict__ bp1, int KS, f32x16 (&acc)[2]) {
    for (int ks = 0; ks < KS; ++ks) {
        const uint4 a0 = ap[ks * 128], a1 = ap[ks * 128 + 64];
        const uint4 b0[2] = {bp0[ks * 128], bp1[ks * 128]};
        const uint4 b1[2] = {bp0[ks * 128 + 64], bp1[ks * 128 + 64]};
        if constexpr (!F32) {
            // pieces = f16 hi / lo planes; per accumulator b_hi a_lo, b_lo a_hi, b_hi a_hi (gemm_split_kernel's order)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[n] = mfma16(b0[n], a1, acc[n]);
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[n] = mfma16(b1[n], a0, acc[n]);
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[n] = mfma16(b0[n], a0, acc[n]);
        } else {
            // pieces = the lane's two k-quads; step j pairs k = 16 ks + j (lanes hi = 0) with k = 16 ks + 8 + j (hi = 1)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 fa = __builtin_bit_cast(float4, j < 4 ? a0 : a1);
                const float av4[4] = {fa.x, fa.y, fa.z, fa.w};
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const float4 fb = __builtin_bit_cast(float4, j < 4 ? b0[n] : b1[n]);
                    const float bv4[4] = {fb.x, fb.y, fb.z, fb.w};
                    acc[n] = mfma32(bv4[j & 3], av4[j & 3], acc[n]);
                }
            }
        }
    }
}

template <bool F32>
__global__ __launch_bounds__(256, 2) void lisrd_match_kernel(LisrdMatchP p) {
    __shared__ float park[LM_CT * LM_PLD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, lo = lane & 31, hi = lane >> 5;
    const int nrb = (p.N + LM_ROWS - 1) / LM_ROWS, nct_s = (p.M + LM_CT - 1) / LM_CT;
    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int rb = t % nrb;
    t /= nrb;
    const int chunk = t % p.nchunk, b = t / p.nchunk;
    const int Nb = p.cnt0 ? max(min(p.cnt0[b], p.N), 0) : p.N;
    const int Mb = p.cnt1 ? max(min(p.cnt1[b], p.M), 0) : p.M;
    if (rb * LM_ROWS >= Nb) return;  // (the whole workgroup: no barrier is passed by a part of it)
    const int rowsv = min(LM_ROWS, Nb - rb * LM_ROWS);
    const int tpc = (nct_s + p.nchunk - 1) / p.nchunk;
    const int ct0 = chunk * tpc, ct1 = min(ct0 + tpc, (Mb + LM_CT - 1) / LM_CT);

    const int fa = rb * 4 + wid;  // the wave's row fragment
    float q0 = -INFINITY;         // the row's best over the lane's columns (4 hi .. + 3 of every 8) and its first column
    int qi = 0x7fffffff;

    for (int ct = ct0; ct < ct1; ++ct) {
        // running soft-max over the variances: maximum, denominator, weighted numerator.  From (-inf, 0, 0) the first variance gives
        // (meta_0, 1, desc_0) exactly: exp(-inf) = 0, exp(0) = 1
        f32x16 sm[2], sd[2], sn[2];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) sm[n][r] = -INFINITY, sd[n][r] = 0.0f, sn[n][r] = 0.0f;
#pragma unroll 1
        for (int v = 0; v < LM_NV; ++v) {
            f32x16 am[2], ad[2];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) am[n][r] = 0.0f, ad[n][r] = 0.0f;
            const size_t vb = (size_t)v * p.B + b;
            {
                const uint4* ap = p.Am + vb * p.am_s + ((size_t)fa * p.KSm) * 128 + lane;
                const uint4* bp = p.Bm + vb * p.bm_s + ((size_t)(ct * 2) * p.KSm) * 128 + lane;
                lm_product<F32>(ap, bp, bp + (size_t)p.KSm * 128, p.KSm, am);
            }
            {
                constexpr int KSD = LM_DESC / 16;
                const uint4* ap = p.Ad + vb * p.ad_s + ((size_t)fa * KSD) * 128 + lane;
                const uint4* bp = p.Bd + vb * p.bd_s + ((size_t)(ct * 2) * KSD) * 128 + lane;
                lm_product<F32>(ap, bp, bp + KSD * 128, KSD, ad);
            }
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float mn = fmaxf(sm[n][r], am[n][r]);
                    const float so = __expf(sm[n][r] - mn), e = __expf(am[n][r] - mn);  // (one of the two is exp(0) = 1)
                    sd[n][r] = sd[n][r] * so + e;
                    sn[n][r] = sn[n][r] * so + e * ad[n][r];
                    sm[n][r] = mn;
                }
        }
        // similarity of the lane's 32 elements (row lo of the wave's fragment; column n * 32 + 8 (r >> 2) + (r & 3) + 4 hi of the tile);
        // columns past the image's count are -inf
        const int jb = ct * LM_CT + 4 * hi, jlim = Mb - jb;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = sn[n][r] / sd[n][r];
                sn[n][r] = (n * 32 + 8 * (r >> 2) + (r & 3) < jlim) ? s : -INFINITY;
            }
        // (1) per row: the tile's maximum, its FIRST column by equality walking downwards; tiles ascend, so a later one wins only when larger
        {
            float tm = sn[0][0];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) tm = fmaxf(tm, sn[n][r]);
            int tc = 0;
#pragma unroll
            for (int n = 1; n >= 0; --n)
#pragma unroll
                for (int r = 15; r >= 0; --r) tc = (sn[n][r] == tm) ? n * 32 + 8 * (r >> 2) + (r & 3) : tc;
            const bool up = tm > q0;
            qi = up ? jb + tc : qi;
            q0 = up ? tm : q0;
        }
        // (2) per column: park the tile column-major, four adjacent lanes reduce a column (32 contiguous rows each), folded by two exchanges
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) park[(n * 32 + 8 * (r >> 2) + (r & 3) + 4 * hi) * LM_PLD + wid * 32 + lo] = sn[n][r];
        __syncthreads();
        {
            const int jl = tid >> 2, part = tid & 3;
            const float4* col = reinterpret_cast<const float4*>(park + jl * LM_PLD + 32 * part);
            float v[32];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 t4 = col[k];
                v[4 * k + 0] = t4.x, v[4 * k + 1] = t4.y, v[4 * k + 2] = t4.z, v[4 * k + 3] = t4.w;
            }
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = (32 * part + u < rowsv) ? v[u] : -INFINITY;  // rows past the image's count
            float tm = v[0];
#pragma unroll
            for (int u = 1; u < 32; ++u) tm = fmaxf(tm, v[u]);
            int ti = 0;
#pragma unroll
            for (int u = 31; u >= 0; --u) ti = (v[u] == tm) ? u : ti;
            ti += rb * LM_ROWS + 32 * part;
#pragma unroll
            for (int st = 1; st <= 2; st <<= 1) {
                const float om = __shfl_xor(tm, st, 64);
                const int oi = __shfl_xor(ti, st, 64);
                const bool up = om > tm || (om == tm && oi < ti);
                ti = up ? oi : ti;
                tm = up ? om : tm;
            }
            const int j = ct * LM_CT + jl;
            if (part == 0 && j < Mb) {
                const size_t o = ((size_t)b * nrb + rb) * p.M + j;
                p.c0[o] = tm;
                p.ci[o] = ti;
            }
        }
        __syncthreads();  // (the parked tile is dead before the next one is written)
    }
    // rows: fold the two half-waves (interleaved column sets: lowest column among equal values)
    {
        const float o0 = __shfl_xor(q0, 32, 64);
        const int oi = __shfl_xor(qi, 32, 64);
        const bool up = o0 > q0 || (o0 == q0 && oi < qi);
        qi = up ? oi : qi;
        q0 = up ? o0 : q0;
    }
    if (hi == 0 && wid * 32 + lo < rowsv) {
        const size_t o = ((size_t)b * p.nchunk + chunk) * p.N + rb * LM_ROWS + wid * 32 + lo;
        p.r0[o] = q0;
        p.ri[o] = qi;
    }
}

// fold the partials of one direction in ascending slot order (larger value, lowest index among equal values); items past the image's
// count, and items without any partner, get index -1 and value 0.  Columns: only the row blocks that hold live rows were written.
__global__ __launch_bounds__(256) void lisrd_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int nslots, int slot_rows, int n,
                                                          const int* __restrict__ cnt_self, const int* __restrict__ cnt_other, int n_other, float* __restrict__ best,
                                                          int* __restrict__ idx) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int live = cnt_self ? max(min(cnt_self[b], n), 0) : n;
    const int other = cnt_other ? max(min(cnt_other[b], n_other), 0) : n_other;
    const int ns = slot_rows > 0 ? min(nslots, (other + slot_rows - 1) / slot_rows) : nslots;  // (columns: slots = row blocks of `other`)
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (i < live && other > 0)
        for (int s = 0; s < ns; ++s) {
            const size_t o = ((size_t)b * nslots + s) * n + i;
            const float v = pv[o];
            const int k = pi[o];
            if (v > bv || (v == bv && k < bi)) bv = v, bi = k;
        }
    const bool ok = bi != 0x7fffffff;
    if (best) best[(size_t)b * n + i] = ok ? bv : 0.0f;
    idx[(size_t)b * n + i] = ok ? bi : -1;
}

// the mutual rule `ids1 == nn21[nn12]` (lisrd.py:130-134) and `_compute_confidence` (lisrd.py:137-149) of the surviving pairs, in the
// wrapper's own order: every vector re-normalised (x / max(|x|, 1e-12)), four dots of each kind, soft-max, weighted sum.  One wave per row.
__device__ __forceinline__ float lm_norm_dot(const float* __restrict__ a, const float* __restrict__ c, int D, int lane) {
    float sa = 0.0f, sc = 0.0f;
    for (int k = lane; k < D; k += 64) sa += a[k] * a[k], sc += c[k] * c[k];
    const float na = fmaxf(sqrtf(wave_sum(sa)), 1e-12f), nc = fmaxf(sqrtf(wave_sum(sc)), 1e-12f);
    float d = 0.0f;
    for (int k = lane; k < D; k += 64) d += (a[k] / na) * (c[k] / nc);
    return wave_sum(d);
}
__global__ __launch_bounds__(256) void lisrd_mutual_conf_kernel(const float* __restrict__ desc0, const float* __restrict__ meta0, const float* __restrict__ desc1,
                                                                const float* __restrict__ meta1, const int* __restrict__ nn12, const int* __restrict__ nn21, int N, int M,
                                                                int Dm, int* __restrict__ matches0, float* __restrict__ mconf) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    int j = nn12[(size_t)b * N + i];
    if (j >= 0 && j < M) {
        if (nn21[(size_t)b * M + j] != i) j = -1;
    } else {
        j = -1;
    }
    float conf = 0.0f;
    if (j >= 0) {  // (wave-uniform)
        float ds[LM_NV], ms[LM_NV];
#pragma unroll
        for (int v = 0; v < LM_NV; ++v) {
            ds[v] = lm_norm_dot(desc0 + (((size_t)b * N + i) * LM_NV + v) * LM_DESC, desc1 + (((size_t)b * M + j) * LM_NV + v) * LM_DESC, LM_DESC, lane);
            ms[v] = lm_norm_dot(meta0 + (((size_t)b * N + i) * LM_NV + v) * Dm, meta1 + (((size_t)b * M + j) * LM_NV + v) * Dm, Dm, lane);
        }
        const float mx = fmaxf(fmaxf(ms[0], ms[1]), fmaxf(ms[2], ms[3]));
        float e[LM_NV], den = 0.0f;
#pragma unroll
        for (int v = 0; v < LM_NV; ++v) e[v] = expf(ms[v] - mx), den += e[v];
#pragma unroll
        for (int v = 0; v < LM_NV; ++v) conf += ds[v] * (e[v] / den);
    }
    if (lane == 0) {
        matches0[(size_t)b * N + i] = j;
        if (mconf) mconf[(size_t)b * N + i] = conf;
    }
}

// ------------------------------------------------------------------ host side
// column chunks per row block: about two workgroups per CU of the target part (a function of the sizes alone: the workspace and the
// launch agree without a handle).  At 2048 x 2048, B = 1: 16 row blocks x 32 chunks = 512 workgroups of ONE 64-column tile each -- the
// walk over several tiles per workgroup starts where 512 workgroups cover fewer than the tiles there are (4096 columns at 2048 rows)
static int lm_chunks(int B, int N, int M) {
    const int nrb = (N + LM_ROWS - 1) / LM_ROWS, nct = (M + LM_CT - 1) / LM_CT;
    int nchunk = (512 + B * nrb - 1) / (B * nrb);
    if (nchunk > nct) nchunk = nct;
    return nchunk < 1 ? 1 : nchunk;
}

struct LisrdMatchWs {
    uint4 *ad, *am, *bd, *bm;
    float *r0, *c0;
    int *ri, *ci, *nn12, *nn21;
    int nchunk, nrb;
    bool ok;
    size_t total;
};
static LisrdMatchWs lm_carve(void* ws, size_t ws_bytes, int B, int N, int M, int Dm) {
    LisrdMatchWs w;
    WsAlloc a(ws, ws_bytes);
    w.nchunk = lm_chunks(B, N, M);
    w.nrb = (N + LM_ROWS - 1) / LM_ROWS;
    w.ad = a.get<uint4>((size_t)LM_NV * B * simred_packed_uint4(N, LM_DESC));
    w.am = a.get<uint4>((size_t)LM_NV * B * simred_packed_uint4(N, Dm));
    w.bd = a.get<uint4>((size_t)LM_NV * B * simred_packed_uint4(M, LM_DESC));
    w.bm = a.get<uint4>((size_t)LM_NV * B * simred_packed_uint4(M, Dm));
    w.r0 = a.get<float>((size_t)B * w.nchunk * N);
    w.ri = a.get<int>((size_t)B * w.nchunk * N);
    w.c0 = a.get<float>((size_t)B * w.nrb * M);
    w.ci = a.get<int>((size_t)B * w.nrb * M);
    w.nn12 = a.get<int>((size_t)B * N);
    w.nn21 = a.get<int>((size_t)B * M);
    w.ok = a.ok;
    w.total = a.off;
    return w;
}
static bool lm_shape_ok(int B, int N, int M, int Dm) { return B > 0 && N > 0 && M > 0 && Dm >= 128 && Dm <= 1024 && Dm % 128 == 0; }

extern "C" size_t imcui_hip_lisrd_match_workspace_bytes(int B, int N, int M, int Dm) {
    if (!lm_shape_ok(B, N, M, Dm)) return 0;
    return lm_carve(nullptr, 0, B, N, M, Dm).total;
}

extern "C" int imcui_hip_lisrd_match(imcui_hip_t* h, const float* desc0, const float* meta0, const int* cnt0, const float* desc1, const float* meta1, const int* cnt1,
                                     int B, int N, int M, int Dm, int* matches0, float* best0, float* mconf, int* nn12, int* nn21, float* best1, void* ws,
                                     size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (!desc0 || !meta0 || !desc1 || !meta1 || !matches0) return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd_match: null descriptors or matches0");
    if (!lm_shape_ok(B, N, M, Dm))
        return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "lisrd_match: B=%d N=%d M=%d must be positive and the meta width %d a multiple of 128 up to 1024", B, N, M, Dm);
    const LisrdMatchWs w = lm_carve(ws, ws_bytes, B, N, M, Dm);
    if (!ws || !w.ok) return imcui_set_err(h, IMCUI_ERR_WS, "lisrd_match: workspace too small (%zu < %zu)", ws_bytes, w.total);
    // both sets, once, into matrix-core fragments: per variance one strided view of [B, K, 4, D]
    for (int v = 0; v < LM_NV; ++v) {
        simred_pack(h, desc0 + v * LM_DESC, LM_NV * LM_DESC, 1, (long)N * LM_NV * LM_DESC, N, LM_DESC, B, cnt0, 1, w.ad + (size_t)v * B * simred_packed_uint4(N, LM_DESC), stream);
        simred_pack(h, meta0 + (size_t)v * Dm, (long)LM_NV * Dm, 1, (long)N * LM_NV * Dm, N, Dm, B, cnt0, 1, w.am + (size_t)v * B * simred_packed_uint4(N, Dm), stream);
        simred_pack(h, desc1 + v * LM_DESC, LM_NV * LM_DESC, 1, (long)M * LM_NV * LM_DESC, M, LM_DESC, B, cnt1, 1, w.bd + (size_t)v * B * simred_packed_uint4(M, LM_DESC), stream);
        simred_pack(h, meta1 + (size_t)v * Dm, (long)LM_NV * Dm, 1, (long)M * LM_NV * Dm, M, Dm, B, cnt1, 1, w.bm + (size_t)v * B * simred_packed_uint4(M, Dm), stream);
    }
    LisrdMatchP p;
    p.Ad = w.ad, p.Am = w.am, p.Bd = w.bd, p.Bm = w.bm;
    p.ad_s = (long)simred_packed_uint4(N, LM_DESC), p.am_s = (long)simred_packed_uint4(N, Dm);
    p.bd_s = (long)simred_packed_uint4(M, LM_DESC), p.bm_s = (long)simred_packed_uint4(M, Dm);
    p.N = N, p.M = M, p.KSm = Dm / 16, p.B = B;
    p.cnt0 = cnt0, p.cnt1 = cnt1;
    p.nchunk = w.nchunk;
    p.r0 = w.r0, p.ri = w.ri, p.c0 = w.c0, p.ci = w.ci;
    const dim3 grid((unsigned)(B * w.nchunk * w.nrb));
    imcui_prof_begin(h, PROF_GEMM, stream);
    if (h->precision == 1)
        hipLaunchKernelGGL(lisrd_match_kernel<false>, grid, dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL(lisrd_match_kernel<true>, grid, dim3(256), 0, stream, p);
    imcui_prof_end(h, PROF_GEMM, stream);
    IMCUI_CHECK_LAUNCH(h);
    int* o12 = nn12 ? nn12 : w.nn12;
    int* o21 = nn21 ? nn21 : w.nn21;
    hipLaunchKernelGGL(lisrd_merge_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, stream, w.r0, w.ri, w.nchunk, 0, N, cnt0, cnt1, M, best0, o12);
    hipLaunchKernelGGL(lisrd_merge_kernel, dim3(cdiv(M, 256), B), dim3(256), 0, stream, w.c0, w.ci, w.nrb, LM_ROWS, M, cnt1, cnt0, N, best1, o21);
    hipLaunchKernelGGL(lisrd_mutual_conf_kernel, dim3(cdiv(N, 4), B), dim3(256), 0, stream, desc0, meta0, desc1, meta1, o12, o21, N, M, Dm, matches0, mconf);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// =====================================================================================================================================
// The LISRD network (`self.net._forward(inputs, Mode.EXPORT, LISRD_CONFIG)`, lisrd.py:259-268) and `_extract_descriptors`
// (lisrd.py:90-119) as one call per image batch.  third_party/LISRD is not part of the reference checkout: the network is restated in
// tests/lisrd_reference.py, and that file is the definition this one is tested against ("LISRD: what is pinned").
//
//   image     [B, 3, H, W] in [0, 1]; the wrapper's `* 255` (lisrd.py:209-210) and the network's `/ 255` are applied where layer 0 READS
//             the image (LisrdStemLoad: two float32 roundings)
//   block     conv 3x3 (pad 1, bias) -> ReLU -> BatchNorm2d on running statistics.  The BatchNorm sits BEHIND the ReLU, so it folds
//             neither into its own convolution nor exactly into the next (the next layer's zero padding is zero AFTER the shift): it
//             stays an affine pass y = x a + b with a, b folded in double and rounded once -- lisrd_affine_kernel in place, or
//             lisrd_pool_affine_kernel where AvgPool2d(2, 2) follows (pooling and the affine commute: one pass reads 4 C floats and
//             writes C).  Folding it into the next layer with a per-border-class bias is NOT built.
//   backbone  LISRD_LAYERS: layer 0 on the VALU (stem3x3_kernel<64>), the others on the shared implicit GEMM with ReLU in the epilogue
//   heads     the eight hidden 3x3 layers (descriptor and meta head of each of the four variances) read the same map: ONE launch with
//             N = 2048, rows concatenated at pack time; the eight 1x1 layers are plain GEMMs with lda = 2048
//   NetVLAD   per variance, on each of the 3 x 3 regions of Hc / 3 x Wc / 3 cells of the meta map (remainder rows / columns dropped):
//             lisrd_vlad_assign_kernel (one wave per cell: L2-normalise, 8 assignment logits, soft-max), lisrd_vlad_agg_kernel (fixed
//             chunks of 64 cells per region), lisrd_vlad_fold_kernel (chunks in ascending order, intra-normalisation, flatten k * 128 + d,
//             L2-normalise).  No float atomics: bits do not depend on batch or replay.
//   sampling  lisrd_sample_kernel, one wave per key-point: grid_sample(align_corners=False, zero padding) of the four 128-channel maps
//             and of the four 3 x 3 meta maps in the wrapper's float32 order, v / max(|v|, 1e-12)
#include <string.h>

#include <string>
#include <vector>

#include <algorithm>

#include "net_kernels.h"
#include "netpack.h"
#include "select.h"

#define LR_NV 4
#define LR_DESC 128    // desc_size
#define LR_META 128    // meta_desc_dim
#define LR_NCLU 8      // n_clusters
#define LR_TILE 3      // tile
#define LR_DM (LR_NCLU * LR_META)
#define LR_HID 256     // hidden width of a head
#define LR_NHID (2 * LR_NV * LR_HID)
#define LR_MIN_SIDE (8 * LR_TILE)
#define LR_CHUNK 64    // cells per aggregation chunk
#define LR_MAGIC 19538.0f  // "LR"

static const char* const LR_VAR[LR_NV] = {"rot_var_illum_var", "rot_invar_illum_var", "rot_var_illum_invar", "rot_invar_illum_invar"};

// ------------------------------------------------------------------ the layer table (the ONE place that states the network's launches)
// kind: 0 layer 0 on the VALU, 1 3x3 on the implicit GEMM, 2 the eight hidden head layers as one launch, 3 a head's 1x1 layer (plain GEMM
// on `in_off` .. + 255 of the 2048-channel hidden map).  pool: AvgPool2d(2, 2) behind the block.
enum { LR_STEM = 0, LR_CONV3 = 1, LR_HEADS = 2, LR_PW = 3 };
struct LrRow {
    const char* name;
    int kind, cin, cout, pool, in_off;
};
static const LrRow LISRD_LAYERS[] = {
    {"conv1_1", LR_STEM, 3, 64, 0, 0},     {"conv1_2", LR_CONV3, 64, 64, 1, 0},    {"conv2_1", LR_CONV3, 64, 64, 0, 0},    {"conv2_2", LR_CONV3, 64, 64, 1, 0},
    {"conv3_1", LR_CONV3, 64, 128, 0, 0},  {"conv3_2", LR_CONV3, 128, 128, 1, 0},  {"conv4_1", LR_CONV3, 128, 256, 0, 0},  {"conv4_2", LR_CONV3, 256, 256, 0, 0},
    {"heads_1", LR_HEADS, 256, LR_NHID, 0, 0},
    {"desc_2.0", LR_PW, LR_HID, LR_DESC, 0, 0 * LR_HID}, {"desc_2.1", LR_PW, LR_HID, LR_DESC, 0, 1 * LR_HID}, {"desc_2.2", LR_PW, LR_HID, LR_DESC, 0, 2 * LR_HID},
    {"desc_2.3", LR_PW, LR_HID, LR_DESC, 0, 3 * LR_HID}, {"meta_2.0", LR_PW, LR_HID, LR_META, 0, 4 * LR_HID}, {"meta_2.1", LR_PW, LR_HID, LR_META, 0, 5 * LR_HID},
    {"meta_2.2", LR_PW, LR_HID, LR_META, 0, 6 * LR_HID}, {"meta_2.3", LR_PW, LR_HID, LR_META, 0, 7 * LR_HID},
};
#define LR_NLAYER ((int)(sizeof(LISRD_LAYERS) / sizeof(LISRD_LAYERS[0])))
#define LR_NBLOCK 9  // layers followed by ReLU + BatchNorm (the backbone's eight and the fused head launch)

extern "C" int imcui_hip_lisrd_num_layers(void) { return LR_NLAYER; }
// out5 = kind, cin, cout, pool, in_off
extern "C" const char* imcui_hip_lisrd_layer(int i, int* out5) {
    if (i < 0 || i >= LR_NLAYER) return nullptr;
    const LrRow& r = LISRD_LAYERS[i];
    if (out5) out5[0] = r.kind, out5[1] = r.cin, out5[2] = r.cout, out5[3] = r.pool, out5[4] = r.in_off;
    return r.name;
}

// state-dict prefixes: the convolution and the BatchNorm of block i < 8; head (meta ? meta : descriptor) of variance v
static std::string lr_conv(int i) { return std::string("_backbone._") + LISRD_LAYERS[i].name; }
static std::string lr_bn(int i) { return std::string("_backbone._bn") + (LISRD_LAYERS[i].name + 4); }
static std::string lr_head(int meta, int v, const char* what, int n) {
    return std::string(what) + (meta ? "_meta_" : "_") + LR_VAR[v] + "_" + std::to_string(n);
}
static const char* const LR_BN_KEYS[4] = {"weight", "bias", "running_mean", "running_var"};
// the tensors the packer takes, in order, and (when asked) the shape of each: the ONE statement of both, read by the binding
struct LrShape {
    int nd, d[4];
};
static TensorTable lr_tensors(std::vector<LrShape>* shapes = nullptr) {
    TensorTable t;
    const auto add = [&](const std::string& name, int nd, int d0, int d1 = 1, int d2 = 1, int d3 = 1) {
        t.add(name, (size_t)d0 * d1 * d2 * d3);
        if (shapes) shapes->push_back({nd, {d0, d1, d2, d3}});
    };
    for (int i = 0; i < 8; ++i) {
        const LrRow& r = LISRD_LAYERS[i];
        add(lr_conv(i) + ".weight", 4, r.cout, r.cin, 3, 3);
        add(lr_conv(i) + ".bias", 1, r.cout);
        for (const char* s : LR_BN_KEYS) add(lr_bn(i) + "." + s, 1, r.cout);
    }
    for (int meta = 0; meta < 2; ++meta)
        for (int v = 0; v < LR_NV; ++v) {
            add(lr_head(meta, v, "conv", 1) + ".weight", 4, LR_HID, 256, 3, 3);
            add(lr_head(meta, v, "conv", 1) + ".bias", 1, LR_HID);
            for (const char* s : LR_BN_KEYS) add(lr_head(meta, v, "bn", 1) + "." + s, 1, LR_HID);
            add(lr_head(meta, v, "conv", 2) + ".weight", 4, 128, LR_HID, 1, 1);
            add(lr_head(meta, v, "conv", 2) + ".bias", 1, 128);
        }
    for (int v = 0; v < LR_NV; ++v) {
        add(std::string("vlad_") + LR_VAR[v] + ".conv.weight", 4, LR_NCLU, LR_META, 1, 1);
        add(std::string("vlad_") + LR_VAR[v] + ".centroids", 2, LR_NCLU, LR_META);
    }
    return t;
}
extern "C" const char* imcui_hip_lisrd_variance(int v) { return (v < 0 || v >= LR_NV) ? nullptr : LR_VAR[v]; }
// number of dimensions of tensor i (0: no such tensor), the dimensions in out4
extern "C" int imcui_hip_lisrd_tensor_shape(int i, int* out4) {
    std::vector<LrShape> s;
    lr_tensors(&s);
    if (i < 0 || i >= (int)s.size()) return 0;
    if (out4)
        for (int k = 0; k < 4; ++k) out4[k] = s[i].d[k];
    return s[i].nd;
}
extern "C" int imcui_hip_lisrd_num_tensors(void) { return lr_tensors().size(); }
extern "C" const char* imcui_hip_lisrd_tensor_name(int i) {
    static thread_local std::string name;
    const TensorTable t = lr_tensors();
    if (i < 0 || i >= t.size()) return nullptr;
    name = t.t[i].name;
    return name.c_str();
}

// ------------------------------------------------------------------ packed layout
// hdr [64]: magic.  w0 / b0: layer 0 for the VALU kernel [tap][cin 3][64] + [64] (no fold: the BatchNorm is behind the ReLU).  g[i]: GEMM layer i
// ([cout][tap][cin] or [cout][cin]) with its bias.  aa[i] / ab[i]: the affine behind block i < 9.  va / vc [v]: assignment weights and
// centroids [8][128].
struct LrLayout {
    size_t hdr, w0, b0;
    GemmLayerOff g[LR_NLAYER];
    size_t aa[LR_NBLOCK], ab[LR_NBLOCK], va[LR_NV], vc[LR_NV];
    size_t total;
};
static LrLayout lr_layout() {
    LrLayout l;
    PackCursor p;
    l.hdr = p.get(64);
    l.w0 = p.get(27 * 64);
    l.b0 = p.get(64);
    for (int i = 1; i < LR_NLAYER; ++i) l.g[i].place(p, LISRD_LAYERS[i].cout, (LISRD_LAYERS[i].kind == LR_PW ? 1 : 9) * LISRD_LAYERS[i].cin);
    for (int i = 0; i < LR_NBLOCK; ++i) l.aa[i] = p.get(LISRD_LAYERS[i].cout), l.ab[i] = p.get(LISRD_LAYERS[i].cout);
    for (int v = 0; v < LR_NV; ++v) l.va[v] = p.get(LR_NCLU * LR_META), l.vc[v] = p.get(LR_NCLU * LR_META);
    l.total = p.off;
    return l;
}
extern "C" size_t imcui_hip_lisrd_packed_floats(void) { return lr_layout().total; }

// BatchNorm2d (eval, eps 1e-5) as y = x a + b: folded in double, rounded once
static void lr_affine(const float* const* bn, int n, float* a, float* b) {
    for (int c = 0; c < n; ++c) {
        const double s = (double)bn[0][c] / sqrt((double)bn[3][c] + 1e-5);
        a[c] = (float)s;
        b[c] = (float)((double)bn[1][c] - (double)bn[2][c] * s);
    }
}
// t: host pointers of the tensors in imcui_hip_lisrd_tensor_name order (shapes checked by the caller)
extern "C" int imcui_hip_lisrd_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    const TensorTable names = lr_tensors();
    for (int i = 0; i < names.size(); ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const LrLayout l = lr_layout();
    memset(packed, 0, l.total * sizeof(float));
    packed[l.hdr] = LR_MAGIC;
    auto T = [&](const std::string& name) { return t[names.find(name)]; };
    for (int i = 0; i < 8; ++i) {
        const LrRow& r = LISRD_LAYERS[i];
        const float *w = T(lr_conv(i) + ".weight"), *b = T(lr_conv(i) + ".bias");
        if (r.kind == LR_STEM) {
            for (int co = 0; co < 64; ++co)
                for (int ci = 0; ci < 3; ++ci)
                    for (int k = 0; k < 9; ++k) packed[l.w0 + ((size_t)k * 3 + ci) * 64 + co] = w[((size_t)co * 3 + ci) * 9 + k];
            memcpy(packed + l.b0, b, 64 * sizeof(float));
        } else {
            pack_conv_gemm(w, r.cout, r.cin, 3, r.cin, packed + l.g[i].w);
            memcpy(packed + l.g[i].b, b, r.cout * sizeof(float));
            l.g[i].split_planes(packed, r.cout, 9 * r.cin);
        }
        lr_affine(t + names.find(lr_bn(i) + ".weight"), r.cout, packed + l.aa[i], packed + l.ab[i]);
    }
    for (int meta = 0; meta < 2; ++meta)
        for (int v = 0; v < LR_NV; ++v) {
            const int j = meta * LR_NV + v;  // row block of the fused launch = 1x1 layer 9 + j
            pack_conv_gemm(T(lr_head(meta, v, "conv", 1) + ".weight"), LR_HID, 256, 3, 256, packed + l.g[8].w + (size_t)j * LR_HID * 9 * 256);
            memcpy(packed + l.g[8].b + j * LR_HID, T(lr_head(meta, v, "conv", 1) + ".bias"), LR_HID * sizeof(float));
            lr_affine(t + names.find(lr_head(meta, v, "bn", 1) + ".weight"), LR_HID, packed + l.aa[8] + j * LR_HID, packed + l.ab[8] + j * LR_HID);
            memcpy(packed + l.g[9 + j].w, T(lr_head(meta, v, "conv", 2) + ".weight"), (size_t)128 * LR_HID * sizeof(float));
            memcpy(packed + l.g[9 + j].b, T(lr_head(meta, v, "conv", 2) + ".bias"), 128 * sizeof(float));
            l.g[9 + j].split_planes(packed, 128, LR_HID);
        }
    l.g[8].split_planes(packed, LR_NHID, 9 * 256);
    for (int v = 0; v < LR_NV; ++v) {
        memcpy(packed + l.va[v], T(std::string("vlad_") + LR_VAR[v] + ".conv.weight"), LR_NCLU * LR_META * sizeof(float));
        memcpy(packed + l.vc[v], T(std::string("vlad_") + LR_VAR[v] + ".centroids"), LR_NCLU * LR_META * sizeof(float));
    }
    return IMCUI_OK;
}

namespace {

// the wrapper's `image * 255` and the network's `/ 255`: one rounding each
struct LisrdStemLoad {
    __device__ float operator()(const float* __restrict__ img, long b, int c, int h, int w, int yy, int xx) const {
        return __fdiv_rn(__fmul_rn(img[((b * 3 + c) * h + yy) * (long)w + xx], 255.0f), 255.0f);
    }
};

// y = x a[c] + b[c] in place on an NHWC map, 16 bytes per access; n4 = float4s of the map.  Reads C, writes C floats per pixel.
__global__ __launch_bounds__(256) void lisrd_affine_kernel(float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b, int C, long n4) {
    const int C4 = C >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const float4 v = reinterpret_cast<const float4*>(x)[i], s = *reinterpret_cast<const float4*>(a + c), t = *reinterpret_cast<const float4*>(b + c);
        reinterpret_cast<float4*>(x)[i] = make_float4(v.x * s.x + t.x, v.y * s.y + t.y, v.z * s.z + t.z, v.w * s.w + t.w);
    }
}
// AvgPool2d(2, 2) (flooring: the last row / column of an odd map is not read) of the affine = the affine of the pool: the four pixels
// summed row-major, x 0.25, then x a + b.  [B, hi, wi, C] -> [B, hi / 2, wi / 2, C]; reads 4 C, writes C floats per output pixel.
__global__ __launch_bounds__(256) void lisrd_pool_affine_kernel(const float* __restrict__ src, const float* __restrict__ a, const float* __restrict__ b,
                                                                float* __restrict__ dst, int hi, int wi, int ho, int wo, int C, long n4) {
    const int C4 = C >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        long t = i / C4;
        const int x = (int)(t % wo);
        t /= wo;
        const int y = (int)(t % ho);
        const long bb = t / ho;
        const float* s = src + ((bb * hi + 2L * y) * wi + 2L * x) * C + c;
        const float4 v00 = *reinterpret_cast<const float4*>(s), v01 = *reinterpret_cast<const float4*>(s + C),
                     v10 = *reinterpret_cast<const float4*>(s + (long)wi * C), v11 = *reinterpret_cast<const float4*>(s + (long)wi * C + C);
        const float4 o = add4(add4(add4(v00, v01), v10), v11);
        const float4 sc = *reinterpret_cast<const float4*>(a + c), sh = *reinterpret_cast<const float4*>(b + c);
        reinterpret_cast<float4*>(dst)[i] = make_float4((o.x * 0.25f) * sc.x + sh.x, (o.y * 0.25f) * sc.y + sh.y, (o.z * 0.25f) * sc.z + sh.z, (o.w * 0.25f) * sc.w + sh.w);
    }
}

// ------------------------------------------------------------------ regional NetVLAD
// One wave per cell of the 3 x 3 regions of th x tw cells of map [B, hc, wc, 128] (cells outside the regions are never read): the
// L2-normalised vector -> xn [B, 9, th tw, 128], the soft-max over the 8 assignment logits <xn, aw[k]> -> asg [B, 9, th tw, 8].
// Lane l owns channels 2 l, 2 l + 1.
__global__ __launch_bounds__(256) void lisrd_vlad_assign_kernel(const float* __restrict__ map, const float* __restrict__ aw, int hc, int wc, int th, int tw,
                                                                float* __restrict__ xn, float* __restrict__ asg, long ncell) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= ncell) return;  // (wave-uniform)
    const int ncr = th * tw, n = (int)(g % ncr), reg = (int)((g / ncr) % (LR_TILE * LR_TILE));
    const long b = g / ((long)ncr * LR_TILE * LR_TILE);
    const int y = (reg / LR_TILE) * th + n / tw, x = (reg % LR_TILE) * tw + n % tw;
    const float2 v = *reinterpret_cast<const float2*>(map + ((b * hc + y) * wc + x) * LR_META + 2 * lane);
    const float nrm = fmaxf(sqrtf(wave_sum(v.x * v.x + v.y * v.y)), 1e-12f);
    const float2 u = make_float2(v.x / nrm, v.y / nrm);
    *reinterpret_cast<float2*>(xn + g * LR_META + 2 * lane) = u;
    float lg[LR_NCLU], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < LR_NCLU; ++k) {
        const float2 w = *reinterpret_cast<const float2*>(aw + k * LR_META + 2 * lane);
        lg[k] = wave_sum(u.x * w.x + u.y * w.y);
        mx = fmaxf(mx, lg[k]);
    }
    float den = 0.0f, mine = 0.0f;
#pragma unroll
    for (int k = 0; k < LR_NCLU; ++k) {
        lg[k] = expf(lg[k] - mx);
        den += lg[k];
    }
#pragma unroll
    for (int k = 0; k < LR_NCLU; ++k) mine = lane == k ? lg[k] : mine;
    if (lane < LR_NCLU) asg[g * LR_NCLU + lane] = mine / den;
}
// V[k][d] = sum_n a[n][k] (x[n][d] - c[k][d]) over ONE chunk of LR_CHUNK cells of a region, cells ascending.  grid (chunks, 9, B), 256
// threads: thread (d = t & 127, half = t >> 7) owns channel d of clusters 4 half .. + 3.  part [B, 9, chunks, 8, 128].
__global__ __launch_bounds__(256) void lisrd_vlad_agg_kernel(const float* __restrict__ xn, const float* __restrict__ asg, const float* __restrict__ cent, int ncr,
                                                             float* __restrict__ part) {
    const int chunk = blockIdx.x, nchunk = gridDim.x, d = threadIdx.x & 127, k0 = (threadIdx.x >> 7) * 4;
    const long rg = (long)blockIdx.z * (LR_TILE * LR_TILE) + blockIdx.y, base = rg * ncr;
    const int n0 = chunk * LR_CHUNK, n1 = min(n0 + LR_CHUNK, ncr);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = cent[(k0 + j) * LR_META + d];
    for (int n = n0; n < n1; ++n) {
        const float x = xn[(base + n) * LR_META + d];
        const float4 a = *reinterpret_cast<const float4*>(asg + (base + n) * LR_NCLU + k0);
        acc[0] += a.x * (x - c[0]);
        acc[1] += a.y * (x - c[1]);
        acc[2] += a.z * (x - c[2]);
        acc[3] += a.w * (x - c[3]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) part[((rg * nchunk + chunk) * LR_NCLU + k0 + j) * LR_META + d] = acc[j];
}
// the chunks of a region in ascending order, intra-normalisation over d, flatten k * 128 + d, L2-normalise.  grid (9, B), 128 threads (d).
// out [B, 9, out_stride] at + out_off: the caller's [B, 4, 3, 3, 1024] with out_stride = 4 * 9 * 1024 per image (variance v at v * 9 * 1024)
__global__ __launch_bounds__(128) void lisrd_vlad_fold_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ out, long out_bs) {
    __shared__ float red[2][LR_NCLU + 1];
    const int d = threadIdx.x, wv = d >> 6;
    const long rg = (long)blockIdx.y * (LR_TILE * LR_TILE) + blockIdx.x;
    float v[LR_NCLU];
#pragma unroll
    for (int k = 0; k < LR_NCLU; ++k) {
        float s = 0.0f;
        for (int q = 0; q < nchunk; ++q) s += part[((rg * nchunk + q) * LR_NCLU + k) * LR_META + d];
        v[k] = s;
        const float w = wave_sum(s * s);
        if ((d & 63) == 0) red[wv][k] = w;
    }
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int k = 0; k < LR_NCLU; ++k) {
        v[k] = v[k] / fmaxf(sqrtf(red[0][k] + red[1][k]), 1e-12f);
        tot += v[k] * v[k];
    }
    tot = wave_sum(tot);
    if ((d & 63) == 0) red[wv][LR_NCLU] = tot;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(red[0][LR_NCLU] + red[1][LR_NCLU]), 1e-12f);
    float* o = out + (long)blockIdx.y * out_bs + (long)blockIdx.x * LR_DM;
#pragma unroll
    for (int k = 0; k < LR_NCLU; ++k) o[k * LR_META + d] = v[k] / nrm;
}

// ------------------------------------------------------------------ sparse sampling
// `_keypoints_to_grid` (lisrd.py:77-87) and grid_sample(align_corners=False, zeros): g = k * 2 / size - 1 (the IMAGE's size), i = ((g + 1) *
// n - 1) / 2 (the MAP's size n), corners floor(i), floor(i) + 1 with ATen's weights, a corner outside the map contributes nothing; the sum
// runs nw, ne, sw, se; every product, sum and quotient rounded once.
struct LrTap {
    int x0, y0;
    float wnw, wne, wsw, wse;
};
__device__ __forceinline__ LrTap lr_tap(float gx, float gy, int w, int h) {
    const float ix = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.0f), (float)w), 1.0f), 2.0f);
    const float iy = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.0f), (float)h), 1.0f), 2.0f);
    const float fx = floorf(ix), fy = floorf(iy);
    const float ax = __fsub_rn(__fadd_rn(fx, 1.0f), ix), bx = __fsub_rn(ix, fx), ay = __fsub_rn(__fadd_rn(fy, 1.0f), iy), by = __fsub_rn(iy, fy);
    return LrTap{(int)fx, (int)fy, __fmul_rn(ax, ay), __fmul_rn(bx, ay), __fmul_rn(ax, by), __fmul_rn(bx, by)};
}
// NQ float2 per lane (channels 2 lane + 128 q .. + 1) of map [h, w, 128 NQ] at tap t, then v / max(|v|, 1e-12) -> o
template <int NQ>
__device__ __forceinline__ void lr_sample(const float* __restrict__ map, int h, int w, const LrTap& t, int lane, float* __restrict__ o) {
    constexpr int C = 128 * NQ;
    float2 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = make_float2(0.0f, 0.0f);
    const int xs[4] = {t.x0, t.x0 + 1, t.x0, t.x0 + 1}, ys[4] = {t.y0, t.y0, t.y0 + 1, t.y0 + 1};
    const float ws[4] = {t.wnw, t.wne, t.wsw, t.wse};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (xs[c] < 0 || xs[c] >= w || ys[c] < 0 || ys[c] >= h) continue;  // (wave-uniform)
        const float* p = map + ((long)ys[c] * w + xs[c]) * C + 2 * lane;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float2 v = *reinterpret_cast<const float2*>(p + 128 * q);
            acc[q].x = __fadd_rn(acc[q].x, __fmul_rn(v.x, ws[c]));
            acc[q].y = __fadd_rn(acc[q].y, __fmul_rn(v.y, ws[c]));
        }
    }
    float ss = 0.0f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) ss += acc[q].x * acc[q].x + acc[q].y * acc[q].y;
    const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
    for (int q = 0; q < NQ; ++q) *reinterpret_cast<float2*>(o + 2 * lane + 128 * q) = make_float2(__fdiv_rn(acc[q].x, nrm), __fdiv_rn(acc[q].y, nrm));
}
// One wave per key-point row (grid (cdiv(K, 4), B)).  dmaps [4][B, hc, wc, 128] (variance v at + v * dmap_vs), vlad [B, 4, 3, 3, 1024];
// kpts [B, K, 2] (x, y) in pixels of the H x W image, cnt [B].  desc [B, K, 4, 128], meta [B, K, 4, 1024]; rows past the count are zero.
__global__ __launch_bounds__(256) void lisrd_sample_kernel(const float* __restrict__ dmaps, long dmap_vs, const float* __restrict__ vlad, int hc, int wc, int H,
                                                           int W, const float* __restrict__ kpts, const int* __restrict__ cnt, int K, float* __restrict__ desc,
                                                           float* __restrict__ meta) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= K) return;  // (wave-uniform)
    float* od = desc + ((long)b * K + i) * LR_NV * LR_DESC;
    float* om = meta + ((long)b * K + i) * LR_NV * LR_DM;
    if (i >= min(cnt[b], K)) {
        for (int c = lane; c < LR_NV * LR_DESC; c += 64) od[c] = 0.0f;
        for (int c = lane; c < LR_NV * LR_DM; c += 64) om[c] = 0.0f;
        return;
    }
    const float kx = kpts[((long)b * K + i) * 2], ky = kpts[((long)b * K + i) * 2 + 1];
    const float gx = __fsub_rn(__fdiv_rn(__fmul_rn(kx, 2.0f), (float)W), 1.0f), gy = __fsub_rn(__fdiv_rn(__fmul_rn(ky, 2.0f), (float)H), 1.0f);
    const LrTap td = lr_tap(gx, gy, wc, hc), tm = lr_tap(gx, gy, LR_TILE, LR_TILE);
#pragma unroll 1
    for (int v = 0; v < LR_NV; ++v) {
        lr_sample<1>(dmaps + v * dmap_vs + (long)b * hc * wc * LR_DESC, hc, wc, td, lane, od + v * LR_DESC);
        lr_sample<LR_DM / 128>(vlad + ((long)b * LR_NV + v) * LR_TILE * LR_TILE * LR_DM, LR_TILE, LR_TILE, tm, lane, om + v * LR_DM);
    }
}

}  // namespace

// ------------------------------------------------------------------ host: launches
static int lr_gemm(imcui_hip_t* h, const float* P, const GemmLayerOff& o, const float* in, long lda, float* out, int B, int hh, int ww, int cin, int cout, int k, int act,
                   hipStream_t stream) {
    GemmP g;
    g.epi = EPI_CONV;
    g.A = in;
    g.lda = lda;
    gemm_set_weights(g, P, o, cout, k * k * cin, h->precision == 1);
    if (k == 3) gemm_set_conv(g, 3, 1, 1, hh, ww, hh, ww, cin);
    g.M = B * hh * ww;
    g.C = out;
    g.ldc = cout;
    g.act = act;
    return gemm_launch(h, g, stream);
}
static void lr_affine_launch(float* x, const float* a, const float* b, long npix, int C, hipStream_t stream) {
    const long n4 = npix * C / 4;
    hipLaunchKernelGGL(lisrd_affine_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, x, a, b, C, n4);
}
static void lr_pool_affine_launch(const float* src, const float* a, const float* b, float* dst, int B, int hi, int wi, int C, hipStream_t stream) {
    const long n4 = (long)B * (hi / 2) * (wi / 2) * C / 4;
    if (n4 > 0) hipLaunchKernelGGL(lisrd_pool_affine_kernel, dim3(grid_stride_blocks(n4)), dim3(256), 0, stream, src, a, b, dst, hi, wi, hi / 2, wi / 2, C, n4);
}

// blocks [first, last] (< LR_NBLOCK) of the launch list on `in` (the planar image when first == 0, else the NHWC map of hh x ww): every block
// writes the one of buf[0..1] that is not its input; a pooled block goes through the other one.  -> the last block's map, *hh / *ww its size
static int lr_run(imcui_hip_t* h, const LrLayout& l, const float* P, int first, int last, const float* in, int B, int* hh, int* ww, float* const buf[2],
                  const float** result, hipStream_t stream) {
    const float* cur = in;
    int rc;
    for (int i = first; i <= last; ++i) {
        const LrRow& r = LISRD_LAYERS[i];
        float* dst = cur == buf[0] ? buf[1] : buf[0];
        const long npix = (long)B * *hh * *ww;
        if (r.kind == LR_STEM) {
            hipLaunchKernelGGL((stem3x3_kernel<64, LisrdStemLoad>), dim3(blocks_256(npix)), dim3(256), 0, stream, cur, P + l.w0, P + l.b0, dst, *hh, *ww, LisrdStemLoad{}, npix);
            IMCUI_CHECK_LAUNCH(h);
        } else {
            IMCUI_RUN(lr_gemm(h, P, l.g[i], cur, r.cin, dst, B, *hh, *ww, r.cin, r.cout, 3, 1, stream));
        }
        if (r.pool) {
            float* pooled = dst == buf[0] ? buf[1] : buf[0];  // (the block's input is dead)
            lr_pool_affine_launch(dst, P + l.aa[i], P + l.ab[i], pooled, B, *hh, *ww, r.cout, stream);
            *hh /= 2, *ww /= 2;
            cur = pooled;
        } else {
            lr_affine_launch(dst, P + l.aa[i], P + l.ab[i], npix, r.cout, stream);
            cur = dst;
        }
        IMCUI_CHECK_LAUNCH(h);
    }
    *result = cur;
    return IMCUI_OK;
}
// the floats of the largest map blocks [first, last] write for B maps of hin x win
static size_t lr_run_floats(int first, int last, int B, int hin, int win) {
    size_t m = 0;
    int hh = hin, ww = win;
    for (int i = first; i <= last; ++i) {
        m = std::max(m, (size_t)B * hh * ww * LISRD_LAYERS[i].cout);
        if (LISRD_LAYERS[i].pool) hh /= 2, ww /= 2;
    }
    return m;
}

struct LrVladWs {
    float *xn, *asg, *part;
    int th, tw, nchunk;
};
static void lr_carve_vlad(WsAlloc& a, LrVladWs& w, int B, int hc, int wc) {
    w.th = hc / LR_TILE, w.tw = wc / LR_TILE;
    w.nchunk = cdiv(w.th * w.tw, LR_CHUNK);
    const size_t ncell = (size_t)B * LR_TILE * LR_TILE * w.th * w.tw;
    w.xn = a.get<float>(ncell * LR_META);
    w.asg = a.get<float>(ncell * LR_NCLU);
    w.part = a.get<float>((size_t)B * LR_TILE * LR_TILE * w.nchunk * LR_DM);
}
// regional NetVLAD of map [B, hc, wc, 128] with the weights of variance v -> out + b * out_bs: [3, 3, 1024]
static int lr_vlad(imcui_hip_t* h, const LrLayout& l, const float* P, int v, const float* map, int B, int hc, int wc, const LrVladWs& w, float* out, long out_bs,
                   hipStream_t stream) {
    const long ncell = (long)B * LR_TILE * LR_TILE * w.th * w.tw;
    hipLaunchKernelGGL(lisrd_vlad_assign_kernel, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, stream, map, P + l.va[v], hc, wc, w.th, w.tw, w.xn, w.asg, ncell);
    hipLaunchKernelGGL(lisrd_vlad_agg_kernel, dim3(w.nchunk, LR_TILE * LR_TILE, B), dim3(256), 0, stream, w.xn, w.asg, P + l.vc[v], w.th * w.tw, w.part);
    hipLaunchKernelGGL(lisrd_vlad_fold_kernel, dim3(LR_TILE * LR_TILE, B), dim3(128), 0, stream, w.part, w.nchunk, out, out_bs);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

struct LrWs {
    float *buf[2], *hid, *dense, *vlad;  // dense: [8][B, Hc, Wc, 128] (descriptor maps of the four variances, then the raw meta maps)
    LrVladWs vw;
    size_t total;
    bool ok;
};
static LrWs lr_carve(void* ws, size_t bytes, int B, int H, int W) {
    WsAlloc a(ws, bytes);
    LrWs s;
    const int Hc = H / 8, Wc = W / 8;
    const size_t run = lr_run_floats(0, 7, B, H, W), nc = (size_t)B * Hc * Wc;
    for (int k = 0; k < 2; ++k) s.buf[k] = a.get<float>(run);
    s.hid = a.get<float>(nc * LR_NHID);
    s.dense = a.get<float>(nc * 128 * 8);
    s.vlad = a.get<float>((size_t)B * LR_NV * LR_TILE * LR_TILE * LR_DM);
    lr_carve_vlad(a, s.vw, B, Hc, Wc);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}
static int lr_check(imcui_hip_t* h, int B, int C, int H, int W) {
    if (C != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd: %d image channels; the network reads 3", C);
    if (B < 1 || B > 1024) return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd: B=%d outside 1 .. 1024", B);
    if (H < LR_MIN_SIDE || W < LR_MIN_SIDE)
        return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd: H=%d W=%d: every side needs at least %d pixels (a %d x %d region of the 1/8-resolution map without cells)", H, W,
                             LR_MIN_SIDE, LR_TILE, LR_TILE);
    if (((long)H + 3) * ((long)W + 3) * 64 > 0x7fffffffL / B) return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd: B=%d images of %dx%d exceed the 2^31 index range of one call", B, H, W);
    return IMCUI_OK;
}
extern "C" size_t imcui_hip_lisrd_describe_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 1024 || H < LR_MIN_SIDE || W < LR_MIN_SIDE) return 0;
    return lr_carve(nullptr, 0, B, H, W).total;
}

// entry 8 of the table: the eight hidden head layers of feat [B, hh, ww, 256] as one launch and the affine behind them -> hid [B, hh, ww, 2048]
static int lr_heads_hidden(imcui_hip_t* h, const LrLayout& l, const float* P, const float* feat, int B, int hh, int ww, float* hid, hipStream_t stream) {
    int rc;
    IMCUI_RUN(lr_gemm(h, P, l.g[8], feat, 256, hid, B, hh, ww, 256, LR_NHID, 3, 1, stream));
    lr_affine_launch(hid, P + l.aa[8], P + l.ab[8], (long)B * hh * ww, LR_NHID, stream);
    return IMCUI_OK;
}
// entry i >= 9 of the table: a head's 1x1 layer on its 256 channels of hid [B, hh, ww, 2048] -> out [B, hh, ww, 128]
static int lr_head_pw(imcui_hip_t* h, const LrLayout& l, const float* P, int i, const float* hid, int B, int hh, int ww, float* out, hipStream_t stream) {
    return lr_gemm(h, P, l.g[i], hid + LISRD_LAYERS[i].in_off, LR_NHID, out, B, hh, ww, LR_HID, LISRD_LAYERS[i].cout, 1, 0, stream);
}

// the network up to the eight dense maps and the four 3 x 3 meta maps, in the workspace
static int lr_dense(imcui_hip_t* h, const LrLayout& l, const float* P, const float* image, int B, int H, int W, const LrWs& s, hipStream_t stream) {
    int hh = H, ww = W, rc;
    const float* feat = nullptr;
    IMCUI_RUN(lr_run(h, l, P, 0, 7, image, B, &hh, &ww, s.buf, &feat, stream));
    const long nc = (long)B * hh * ww;
    IMCUI_RUN(lr_heads_hidden(h, l, P, feat, B, hh, ww, s.hid, stream));
    for (int j = 0; j < 8; ++j) IMCUI_RUN(lr_head_pw(h, l, P, 9 + j, s.hid, B, hh, ww, s.dense + (size_t)j * nc * 128, stream));
    for (int v = 0; v < LR_NV; ++v)
        IMCUI_RUN(lr_vlad(h, l, P, v, s.dense + (size_t)(LR_NV + v) * nc * 128, B, hh, ww, s.vw, s.vlad + (size_t)v * LR_TILE * LR_TILE * LR_DM,
                          (long)LR_NV * LR_TILE * LR_TILE * LR_DM, stream));
    return IMCUI_OK;
}
static void lr_sample_launch(const float* dmaps, long dmap_vs, const float* vlad, int B, int hc, int wc, int H, int W, const float* kpts, const int* cnt, int K,
                             float* desc, float* meta, hipStream_t stream) {
    hipLaunchKernelGGL(lisrd_sample_kernel, dim3(cdiv(K, 4), B), dim3(256), 0, stream, dmaps, dmap_vs, vlad, hc, wc, H, W, kpts, cnt, K, desc, meta);
}

extern "C" int imcui_hip_lisrd_describe(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, const float* keypoints, const int* counts,
                                        int K, float* desc, float* meta, int* status, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    int rc;
    IMCUI_RUN(lr_check(h, B, C, H, W));
    if (K < 1 || K > 65535 * 4) return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd: K=%d key-point rows", K);
    if (!packed || !image || !keypoints || !counts || !desc || !meta) return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd: null argument");
    const LrWs s = lr_carve(ws, ws_bytes, B, H, W);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "lisrd: workspace too small (%zu < %zu)", ws_bytes, s.total);
    if (status) hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, status, 1);
    const LrLayout l = lr_layout();
    IMCUI_RUN(lr_dense(h, l, packed, image, B, H, W, s, stream));
    const int Hc = H / 8, Wc = W / 8;
    lr_sample_launch(s.dense, (long)B * Hc * Wc * 128, s.vlad, B, Hc, Wc, H, W, keypoints, counts, K, desc, meta, stream);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// ------------------------------------------------------------------ test entries
// the eight dense maps [8][B, Hc, Wc, 128] (descriptor maps of the four variances, then the raw meta maps) and the meta maps [B, 4, 3, 3, 1024]
extern "C" int imcui_hip_lisrd_dense(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, float* dense, float* vlad, void* ws,
                                     size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    int rc;
    IMCUI_RUN(lr_check(h, B, C, H, W));
    if (!packed || !image) return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd dense: null argument");
    const LrWs s = lr_carve(ws, ws_bytes, B, H, W);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "lisrd dense: workspace too small (%zu < %zu)", ws_bytes, s.total);
    IMCUI_RUN(lr_dense(h, lr_layout(), packed, image, B, H, W, s, stream));
    copy_if(dense, s.dense, (size_t)B * (H / 8) * (W / 8) * 128 * 8 * sizeof(float), stream);
    copy_if(vlad, s.vlad, (size_t)B * LR_NV * LR_TILE * LR_TILE * LR_DM * sizeof(float), stream);
    return IMCUI_OK;
}
static bool lr_probe_shape(int B, int H, int W, int C) { return B >= 1 && B <= 1024 && H >= 1 && W >= 1 && C >= 1 && ((long)H + 3) * ((long)W + 3) * C <= 0x7fffffffL / B; }

// entries [first, last] of LISRD_LAYERS on `in`: blocks (< 9) through the forward's own launch list (the planar image [B, 3, H, W] when first
// == 0, else the NHWC map [B, H, W, cin]); first == last == 8: the fused head launch and its affine; first == last >= 9: that 1x1 layer on
// the 2048-channel hidden map `in` -> out (the last entry's NHWC map)
extern "C" size_t imcui_hip_lisrd_layers_workspace_bytes(int first, int last, int B, int H, int W) {
    if (first < 0 || last < first || last >= LR_NLAYER || B < 1 || H < 1 || W < 1) return 0;
    WsAlloc a(nullptr, 0);
    const size_t run = last < 8 ? lr_run_floats(first, last, B, H, W) : (size_t)B * H * W * LISRD_LAYERS[last].cout;
    a.get<float>(run), a.get<float>(run);
    return a.off;
}
extern "C" int imcui_hip_lisrd_layers_probe(imcui_hip_t* h, const float* packed, const float* in, int first, int last, int B, int H, int W, float* out, void* ws,
                                            size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (first < 0 || last < first || last >= LR_NLAYER || (last >= 8 && first != last) || !lr_probe_shape(B, H, W, LR_NHID) || !packed || !in || !out)
        return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd layers probe: entries [%d, %d] of %d (the head entries one at a time), shape or null argument", first, last, LR_NLAYER);
    WsAlloc a(ws, ws_bytes);
    const size_t run = last < 8 ? lr_run_floats(first, last, B, H, W) : (size_t)B * H * W * LISRD_LAYERS[last].cout;
    float* buf[2] = {a.get<float>(run), a.get<float>(run)};
    if (!ws || !a.ok) return imcui_set_err(h, IMCUI_ERR_WS, "lisrd layers probe: workspace too small (%zu < %zu)", ws_bytes, a.off);
    const LrLayout l = lr_layout();
    int hh = H, ww = W, rc;
    if (last < 8) {
        const float* res = nullptr;
        IMCUI_RUN(lr_run(h, l, packed, first, last, in, B, &hh, &ww, buf, &res, stream));
        copy_if(out, res, (size_t)B * hh * ww * LISRD_LAYERS[last].cout * sizeof(float), stream);
    } else if (last == 8) {
        IMCUI_RUN(lr_heads_hidden(h, l, packed, in, B, H, W, out, stream));
    } else {
        IMCUI_RUN(lr_head_pw(h, l, packed, last, in, B, H, W, out, stream));
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
// the affine pass alone on x [B, H, W, C] (C a multiple of 4): pool = 0: y = x a + b -> out [B, H, W, C]; pool = 1: the pooled pass -> out [B, H / 2, W / 2, C]
extern "C" int imcui_hip_lisrd_affine_probe(imcui_hip_t* h, const float* x, const float* a, const float* b, int B, int H, int W, int C, int pool, float* out,
                                            void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (!lr_probe_shape(B, H, W, C) || C % 4 || !x || !a || !b || !out) return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd affine probe: shape, C %% 4 or null argument");
    if (pool) {
        lr_pool_affine_launch(x, a, b, out, B, H, W, C, stream);
    } else {
        hipMemcpyAsync(out, x, (size_t)B * H * W * C * sizeof(float), hipMemcpyDeviceToDevice, stream);
        lr_affine_launch(out, a, b, (long)B * H * W, C, stream);
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
// regional NetVLAD with the weights of variance v on a given map [B, hc, wc, 128] (hc, wc >= 3) -> out [B, 3, 3, 1024]
extern "C" size_t imcui_hip_lisrd_vlad_workspace_bytes(int B, int hc, int wc) {
    if (B < 1 || hc < LR_TILE || wc < LR_TILE) return 0;
    WsAlloc a(nullptr, 0);
    LrVladWs w;
    lr_carve_vlad(a, w, B, hc, wc);
    return a.off;
}
extern "C" int imcui_hip_lisrd_vlad_probe(imcui_hip_t* h, const float* packed, int v, const float* map, int B, int hc, int wc, float* out, void* ws, size_t ws_bytes,
                                          void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    if (v < 0 || v >= LR_NV || !lr_probe_shape(B, hc, wc, LR_META) || B > 65535 || hc < LR_TILE || wc < LR_TILE || !packed || !map || !out)
        return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd vlad probe: variance, shape (at least 3 x 3 cells) or null argument");
    WsAlloc a(ws, ws_bytes);
    LrVladWs w;
    lr_carve_vlad(a, w, B, hc, wc);
    if (!ws || !a.ok) return imcui_set_err(h, IMCUI_ERR_WS, "lisrd vlad probe: workspace too small (%zu < %zu)", ws_bytes, a.off);
    return lr_vlad(h, lr_layout(), packed, v, map, B, hc, wc, w, out, (long)LR_TILE * LR_TILE * LR_DM, (hipStream_t)stream_);
}
// the sparse sampling alone: dmaps [4][B, hc, wc, 128], vlad [B, 4, 3, 3, 1024], keypoints [B, K, 2] (x, y) of H x W images, counts [B]
extern "C" int imcui_hip_lisrd_sample_probe(imcui_hip_t* h, const float* dmaps, const float* vlad, int B, int hc, int wc, int H, int W, const float* keypoints,
                                            const int* counts, int K, float* desc, float* meta, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    if (!lr_probe_shape(B, hc, wc, 4 * LR_DESC) || B > 65535 || H < 1 || W < 1 || K < 1 || K > 65535 * 4 || !dmaps || !vlad || !keypoints || !counts || !desc || !meta)
        return imcui_set_err(h, IMCUI_ERR_ARG, "lisrd sample probe: shape or null argument");
    lr_sample_launch(dmaps, (long)B * hc * wc * LR_DESC, vlad, B, hc, wc, H, W, keypoints, counts, K, desc, meta, (hipStream_t)stream_);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
