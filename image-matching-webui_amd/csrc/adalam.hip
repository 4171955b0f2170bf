// AdaLAM (`adalam` of the zoo: imcui/hloc/matchers/adalam.py:39-68 -> kornia.feature.adalam.AdalamFilter.match_and_filter), the
// hand-crafted outlier filter over putative nearest-neighbour matches, for B ragged pairs in one graph-capturable call.
//
// The rule is stated stage by stage (A .. G) in INTEGRATION.md, "AdaLAM: what is pinned", and restated in numpy by
// tests/adalam_reference.py, whose float32 mode follows the operation order of this file (compiled with -ffp-contract=off: every
// multiply and every add rounds on its own).
//   A  putative matches: squared distances of unnormalised descriptors on the matrix cores (simred.hip, SR_NND: the n0 x n1 matrix
//      never exists), folded over the column chunks / row blocks here: nn, ratio score, mutual flag
//   B  seeds: one thread per key-point against every key-point of its image (LDS tiles of 256)
//   -  one LDS bitonic sort per pair: the key-points by (score, index); a neighbourhood compacted in that order is in score order
//   C .. G  one workgroup per seed (grid = ncap x B, a workgroup without a seed leaves at once: no count is read back): ordered
//      compaction of the members, local coordinates in LDS, duplicates, then per hypothesis an LDS bitonic sort of (r^2, position)
//      keys and a block scan of the weights; the best hypothesis again (and its refit) to mark the accepted members.
// Determinism: no atomics, every sum is a fixed tree or an integer; matches0 is written with plain stores of nn[i], the same value
// whichever neighbourhood writes it.
#include <math.h>

#include "imcui_hip.h"
#include "simred.h"

#define AL_MAXN 4096   // key-points per image (the LDS sorts hold 4096 keys of 8 bytes)
#define AL_T 256       // threads of the per-pair sort and of a neighbourhood workgroup
#define AL_MINP 64     // narrowest sort / tree width
#define AL_NCONF 10    // doubles of the conf array (imcui_hip.h)

struct AlP {
    float seed_ratio;  // 0.8^2
    float r0sq;        // seed suppression radius^2 (image 0)
    float nb0sq, nb1sq, rs0, rs1;  // neighbourhood radii^2, local-coordinate scales (R * search_expansion)
    int iters, min_inl;
    float min_conf;
    int use_ori, use_sc, use_dt, refit, force_mnn;
    float ori_thr, sc_lo, sc_hi, dt_lo, dt_hi;
};

struct AlWs {
    uint4 *pk0, *pk1;
    float *rn, *cn;                // squared norms
    float *rb1, *rb2, *cb1, *cb2;  // SR_NND partials
    int *ri1, *ci1;
    int* nn21;
    int *nn, *mnn, *seed;
    float* score;
    float2* p;         // k1[nn[i]]
    float *relo, *rels;
    int* valid;
    int* order;        // [B][P2]: key-point of rank r by (score, index), -1 past the valid ones
    int nchunk, nrb, P2;
    size_t total;
    bool ok;
};

static int al_pow2(int n) {
    int p = AL_MINP;
    while (p < n) p <<= 1;
    return p;
}

static AlWs al_carve(void* ws, size_t bytes, int B, int ncap, int D) {
    WsAlloc a(ws, bytes);
    AlWs w{};
    const size_t bn = (size_t)B * ncap;
    w.P2 = al_pow2(ncap);
    if (D > 0) {
        w.nchunk = simred_chunks(B, ncap, ncap);
        w.nrb = cdiv(ncap, SR_TILE);
        w.pk0 = a.get<uint4>((size_t)B * simred_packed_uint4(ncap, D));
        w.pk1 = a.get<uint4>((size_t)B * simred_packed_uint4(ncap, D));
        w.rn = a.get<float>(bn);
        w.cn = a.get<float>(bn);
        w.rb1 = a.get<float>(bn * w.nchunk);
        w.rb2 = a.get<float>(bn * w.nchunk);
        w.ri1 = a.get<int>(bn * w.nchunk);
        w.cb1 = a.get<float>(bn * w.nrb);
        w.cb2 = a.get<float>(bn * w.nrb);
        w.ci1 = a.get<int>(bn * w.nrb);
        w.nn21 = a.get<int>(bn);
    }
    w.nn = a.get<int>(bn);
    w.mnn = a.get<int>(bn);
    w.score = a.get<float>(bn);
    w.seed = a.get<int>(bn);
    w.p = a.get<float2>(bn);
    w.relo = a.get<float>(bn);
    w.rels = a.get<float>(bn);
    w.valid = a.get<int>(bn);
    w.order = a.get<int>((size_t)B * w.P2);
    w.total = a.off;
    w.ok = a.ok;
    return w;
}

__device__ __forceinline__ bool al_live(const int* n0, const int* n1, int b, int ncap, int& m0, int& m1) {
    m0 = min(max(n0[b], 0), ncap);
    m1 = min(max(n1[b], 0), ncap);
    return m0 >= 2 && m1 >= 2;  // adalam.py:41-44
}
// v into [-180, 180)
__device__ __forceinline__ float al_wrap(float v) { return v - 360.0f * floorf((v + 180.0f) / 360.0f); }

// -x with a zero of either sign made +0, on the bits: hipcc turns `0.0f - x` into a negated operand, which keeps the sign of a zero
// distance (seen in the ISA and as a score of -0 on the card)
__device__ __forceinline__ float al_neg(float x) {
    const unsigned u = __float_as_uint(x) ^ 0x80000000u;
    return __uint_as_float((u << 1) == 0u ? 0u : u);
}

// ------------------------------------------------------------------ stage A
// squared norms, k ascending; grid (ceil(ncap / 256), B, 2)
__global__ __launch_bounds__(256) void adalam_norm_kernel(const float* __restrict__ d0, const float* __restrict__ d1, int ncap, int D, const int* __restrict__ n0,
                                                          const int* __restrict__ n1, float* __restrict__ rn, float* __restrict__ cn) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncap) return;
    const int side = blockIdx.z;
    const int n = min(max((side ? n1 : n0)[b], 0), ncap);
    float s = 0.0f;
    if (i < n) {
        const float4* x = reinterpret_cast<const float4*>((side ? d1 : d0) + ((size_t)b * ncap + i) * D);
        for (int k = 0; k < D / 4; ++k) {
            const float4 v = x[k];
            s += v.x * v.x;
            s += v.y * v.y;
            s += v.z * v.z;
            s += v.w * v.w;
        }
    }
    (side ? cn : rn)[(size_t)b * ncap + i] = s;
}
// column direction: nn21[j] over the live row blocks (ascending rows: lowest index on equal values)
__global__ __launch_bounds__(256) void adalam_colmerge_kernel(const float* __restrict__ cb1, const int* __restrict__ ci1, int nrb, int ncap, const int* __restrict__ n0,
                                                              const int* __restrict__ n1, int* __restrict__ nn21) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ncap) return;
    int m0, m1, best = -1;
    if (al_live(n0, n1, b, ncap, m0, m1) && j < m1) {
        float b1 = -INFINITY;
        int i1 = 0x7fffffff;
        const int live = (m0 + SR_TILE - 1) / SR_TILE;  // (row blocks past the pair's rows wrote nothing)
        for (int s = 0; s < live; ++s) {
            const size_t o = ((size_t)b * nrb + s) * ncap + j;
            const float v = cb1[o];
            const int vi = ci1[o];
            if (v > b1 || (v == b1 && vi < i1)) b1 = v, i1 = vi;
        }
        best = (i1 >= 0 && i1 < m0) ? i1 : -1;
    }
    nn21[(size_t)b * ncap + j] = best;
}
// row direction over the column chunks: nn, score = dist / max(second, 1e-3), mutual flag
__global__ __launch_bounds__(256) void adalam_rowmerge_kernel(const float* __restrict__ rb1, const float* __restrict__ rb2, const int* __restrict__ ri1, int nchunk,
                                                              int ncap, const int* __restrict__ n0, const int* __restrict__ n1, const int* __restrict__ nn21,
                                                              int* __restrict__ nn, float* __restrict__ score, int* __restrict__ mnn) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncap) return;
    int m0, m1, j = -1, mu = 0;
    float sc = 0.0f;
    if (al_live(n0, n1, b, ncap, m0, m1) && i < m0) {
        float b1 = -INFINITY, b2 = -INFINITY;
        int i1 = 0x7fffffff;
        for (int s = 0; s < nchunk; ++s) {
            const size_t o = ((size_t)b * nchunk + s) * ncap + i;
            const float ob1 = rb1[o], ob2 = rb2[o];
            const int oi1 = ri1[o];
            if (ob1 > b1 || (ob1 == b1 && oi1 < i1)) {
                b2 = fmaxf(b1, ob2);
                b1 = ob1;
                i1 = oi1;
            } else {
                b2 = fmaxf(b2, ob1);
            }
        }
        if (i1 >= 0 && i1 < m1) {
            j = i1;
            sc = al_neg(b1) / fmaxf(al_neg(b2), 1e-3f);  // (the kernel's value is minus the squared distance)
            mu = nn21[(size_t)b * ncap + j] == i;
        }
    }
    const size_t o = (size_t)b * ncap + i;
    nn[o] = j;
    score[o] = sc;
    mnn[o] = mu;
}

// ------------------------------------------------------------------ per key-point quantities of stage C; outputs cleared
__global__ __launch_bounds__(256) void adalam_prep_kernel(int ncap, const int* __restrict__ n0, const int* __restrict__ n1, const float2* __restrict__ k1,
                                                          const float* __restrict__ s0, const float* __restrict__ s1, const float* __restrict__ o0,
                                                          const float* __restrict__ o1, const int* __restrict__ nn, float2* __restrict__ p, float* __restrict__ relo,
                                                          float* __restrict__ rels, int* __restrict__ valid, int* __restrict__ matches0, float* __restrict__ mscores0,
                                                          int* __restrict__ info, float* __restrict__ sconf) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncap) return;
    const size_t o = (size_t)b * ncap + i;
    int m0, m1, ok = 0;
    float2 pp = make_float2(0.0f, 0.0f);
    float ro = 0.0f, rs = 1.0f;
    if (al_live(n0, n1, b, ncap, m0, m1) && i < m0) {
        const int j = nn[o];
        if (j >= 0 && j < m1) {
            ok = 1;
            const size_t oj = (size_t)b * ncap + j;
            pp = k1[oj];
            if (o0) ro = al_wrap(o1[oj] - o0[o]);
            if (s0) rs = s1[oj] / s0[o];
        }
    }
    p[o] = pp, relo[o] = ro, rels[o] = rs, valid[o] = ok;
    matches0[o] = -1;
    mscores0[o] = 0.0f;
    if (info) *reinterpret_cast<int4*>(info + 4 * o) = make_int4(0, -1, 0, 0);
    if (sconf) sconf[o] = 0.0f;
}

// ------------------------------------------------------------------ stage B: seeds.  grid (ceil(ncap / 256), B)
__global__ __launch_bounds__(256) void adalam_seed_kernel(int ncap, const int* __restrict__ n0, const int* __restrict__ n1, const float2* __restrict__ k0,
                                                          const float* __restrict__ score, const int* __restrict__ mnn, const int* __restrict__ valid, AlP c,
                                                          int* __restrict__ seed) {
    __shared__ float4 tile[256];  // x, y, score, eligible
    const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    int m0, m1;
    const bool live = al_live(n0, n1, b, ncap, m0, m1);
    const size_t base = (size_t)b * ncap;
    float2 ki = make_float2(0.0f, 0.0f);
    float si = 0.0f;
    bool cand = false;
    if (live && i < m0) {
        ki = k0[base + i];
        si = score[base + i];
        cand = valid[base + i] && si < c.seed_ratio && (!c.force_mnn || mnn[base + i]);
    }
    const int nj = live ? m0 : 0;
    for (int j0 = 0; j0 < nj; j0 += 256) {  // (nj is uniform over the workgroup)
        const int j = j0 + tid;
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < nj) {
            const float2 kj = k0[base + j];
            t = make_float4(kj.x, kj.y, score[base + j], (valid[base + j] && (!c.force_mnn || mnn[base + j])) ? 1.0f : 0.0f);
        }
        __syncthreads();
        tile[tid] = t;
        __syncthreads();
        const int cnt = min(256, nj - j0);
        if (cand)
            for (int u = 0; u < cnt; ++u) {
                const float4 q = tile[u];
                const float dx = ki.x - q.x, dy = ki.y - q.y;
                const float d2 = dx * dx + dy * dy;
                if (q.w != 0.0f && d2 < c.r0sq && si > q.z) cand = false;
            }
    }
    if (i < ncap) seed[base + i] = cand ? 1 : 0;
}

// ------------------------------------------------------------------ LDS bitonic sort of P 64-bit keys (P a power of two >= 64), ascending
__device__ __forceinline__ void al_sort(unsigned long long* keys, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < (P >> 1); t += AL_T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = keys[i], z = keys[l];
                const bool up = (i & k) == 0;
                if ((a > z) == up) keys[i] = z, keys[l] = a;
            }
        }
    __syncthreads();
}

// the key-points of a pair by (score, index): grid (B), AL_T threads, P2 * 8 bytes of dynamic LDS
__global__ __launch_bounds__(AL_T) void adalam_order_kernel(int ncap, int P2, const int* __restrict__ n0, const int* __restrict__ n1, const float* __restrict__ score,
                                                            const int* __restrict__ valid, int* __restrict__ order) {
    extern __shared__ unsigned long long al_keys[];
    const int b = blockIdx.x, tid = threadIdx.x;
    int m0, m1;
    const bool live = al_live(n0, n1, b, ncap, m0, m1);
    for (int i = tid; i < P2; i += AL_T) {
        unsigned long long key = ~0ull;
        if (live && i < m0 && valid[(size_t)b * ncap + i]) {
            const float s = score[(size_t)b * ncap + i];
            unsigned u = (s == 0.0f) ? 0u : __float_as_uint(s);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving
            key = ((unsigned long long)u << 32) | (unsigned)i;
        }
        al_keys[i] = key;
    }
    al_sort(al_keys, P2, tid);
    for (int r = tid; r < P2; r += AL_T) order[(size_t)b * P2 + r] = (al_keys[r] == ~0ull) ? -1 : (int)(unsigned)(al_keys[r] & 0xffffffffull);
}

// ------------------------------------------------------------------ stages C .. G: one workgroup per seed
struct AlAff {
    float a00, a01, a10, a11;
};
struct AlSel {
    int count, tot;
    float maxr2;
};

__device__ __forceinline__ int al_wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// stage E for one map: sort (r^2, position), scan the weights, accept per member.  acc (when given): bit 0 = accepted, bit 1 = with weight 1
__device__ __forceinline__ AlSel al_select(const AlAff& A, int n, int P, const float4* xy, const unsigned char* wdup, unsigned long long* keys, unsigned char* acc,
                                           int* red, float min_conf, int tid) {
    const int lane = tid & 63, wid = tid >> 6;
    for (int m = tid; m < P; m += AL_T) {
        unsigned long long key = ~0ull;
        if (m < n) {
            const float4 v = xy[m];
            const float ex = (A.a00 * v.x + A.a01 * v.y) - v.z, ey = (A.a10 * v.x + A.a11 * v.y) - v.w;
            const float r2 = ex * ex + ey * ey;
            key = ((unsigned long long)__float_as_uint(r2) << 32) | (unsigned)m;
        }
        keys[m] = key;
    }
    al_sort(keys, P, tid);
    // thread t owns the sorted elements [t E, (t + 1) E)
    const int E = P >= AL_T ? P / AL_T : 1;
    const int e0 = tid * E;
    int wsum = 0;
    if (e0 < P)
        for (int e = 0; e < E; ++e) {
            const unsigned long long key = keys[e0 + e];
            if (key != ~0ull) {
                const float r2 = __uint_as_float((unsigned)(key >> 32));
                wsum += (wdup[(unsigned)(key & 0xffffffffull)] && !(r2 <= 1e-8f)) ? 1 : 0;
            }
        }
    const int incl = al_wave_incl_scan(wsum, lane);
    if (lane == 63) red[wid] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < AL_T / 64; ++w) {
        off += (w < wid) ? red[w] : 0;
        tot += red[w];
    }
    int cum = off + incl - wsum, cnt = 0;
    float mx = 0.0f;
    const float ftot = (float)tot;
    if (e0 < P)
        for (int e = 0; e < E; ++e) {
            const unsigned long long key = keys[e0 + e];
            if (key == ~0ull) continue;
            const float r2 = __uint_as_float((unsigned)(key >> 32));
            const unsigned m = (unsigned)(key & 0xffffffffull);
            const bool tp = r2 <= 1e-8f;
            const int w = (wdup[m] && !tp) ? 1 : 0;
            cum += w;
            const bool ok = tp || (tot > 0 && r2 * min_conf <= (float)cum / ftot);
            if (ok && w) {
                ++cnt;
                mx = fmaxf(mx, r2);
            }
            if (acc) acc[m] = (unsigned char)((ok ? 1 : 0) | ((ok && w) ? 2 : 0));
        }
    cnt = wave_sum_i(cnt);
    mx = wave_max(mx);
    __syncthreads();  // (every wave has read the scan's partials)
    if (lane == 0) red[wid] = cnt, red[4 + wid] = __float_as_int(mx);
    __syncthreads();
    AlSel s;
    s.tot = tot;
    s.count = 0;
    s.maxr2 = 0.0f;
#pragma unroll
    for (int w = 0; w < AL_T / 64; ++w) {
        s.count += red[w];
        s.maxr2 = fmaxf(s.maxr2, __int_as_float(red[4 + w]));
    }
    __syncthreads();  // (`red` is free again)
    return s;
}

// the map through members a, b of couple `it` (enumerated b-major, indices modulo n); false = void
__device__ __forceinline__ bool al_hypothesis(int it, int n, const float4* xy, const AlP& c, AlAff& A) {
    int cb = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)it)) * 0.5f);
    while (cb * (cb - 1) / 2 > it) --cb;
    while (cb * (cb + 1) / 2 <= it) ++cb;
    const int a = (it - cb * (cb - 1) / 2) % n, b = cb % n;
    if (a == b) return false;
    const float4 pa = xy[a], pb = xy[b];
    const float det = pa.x * pb.y - pb.x * pa.y;
    if (fabsf(det) < 1e-8f) return false;
    A.a00 = (pa.z * pb.y - pb.z * pa.y) / det;
    A.a01 = (pb.z * pa.x - pa.z * pb.x) / det;
    A.a10 = (pa.w * pb.y - pb.w * pa.y) / det;
    A.a11 = (pb.w * pa.x - pa.w * pb.x) / det;
    if (c.use_dt) {
        const float da = A.a00 * A.a11 - A.a01 * A.a10;
        if (!(da >= c.dt_lo && da <= c.dt_hi)) return false;
    }
    return true;
}

// sum over the accepted weight-1 members of term(m), as a fixed tree over P slots: f[t] += f[t + s], s = P / 2 .. 1
template <typename F>
__device__ __forceinline__ float al_tree_sum(float* f, int n, int P, const unsigned char* acc, int tid, F term) {
    __syncthreads();
    for (int m = tid; m < P; m += AL_T) f[m] = (m < n && (acc[m] & 2)) ? term(m) : 0.0f;
    for (int s = P >> 1; s > 0; s >>= 1) {
        __syncthreads();
        for (int t = tid; t < s; t += AL_T) f[t] += f[t + s];
    }
    __syncthreads();
    return f[0];
}

// LDS of a neighbourhood workgroup: xy 16 P2, keys 8 P2, members 2 P2, wdup P2, acc P2
static size_t al_nbh_lds(int P2) { return (size_t)P2 * 28; }

__global__ __launch_bounds__(AL_T) void adalam_nbh_kernel(int ncap, int P2, const int* __restrict__ n0, const int* __restrict__ n1, const float2* __restrict__ k0,
                                                          const int* __restrict__ nn, const float2* __restrict__ pq, const float* __restrict__ relo,
                                                          const float* __restrict__ rels, const int* __restrict__ seed, const int* __restrict__ order, AlP c,
                                                          int* __restrict__ matches0, int* __restrict__ members, int* __restrict__ info, float* __restrict__ sconf) {
    extern __shared__ float4 al_smem[];
    __shared__ int red[8];
    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int m0, m1;
    if (!al_live(n0, n1, b, ncap, m0, m1) || s >= m0) return;
    const size_t base = (size_t)b * ncap;
    if (!seed[base + s]) return;
    float4* xy = al_smem;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(xy + P2);
    unsigned short* mem = reinterpret_cast<unsigned short*>(keys + P2);
    unsigned char* wdup = reinterpret_cast<unsigned char*>(mem + P2);
    unsigned char* acc = wdup + P2;

    // ---- C: the members, in (score, index) order
    const float2 ks = k0[base + s], ps = pq[base + s];
    const float ros = relo[base + s], rss = rels[base + s];
    int n = 0;
    for (int r0 = 0; r0 < P2; r0 += AL_T) {
        const int i = (r0 + tid < P2) ? order[(size_t)b * P2 + r0 + tid] : -1;
        bool in = false;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i >= 0) {
            const float2 ki = k0[base + i], pi = pq[base + i];
            const float dx = ki.x - ks.x, dy = ki.y - ks.y, ex = pi.x - ps.x, ey = pi.y - ps.y;
            in = (dx * dx + dy * dy < c.nb0sq) && (ex * ex + ey * ey < c.nb1sq);
            if (c.use_ori) in = in && (fabsf(al_wrap(relo[base + i] - ros)) < c.ori_thr);
            if (c.use_sc) {
                const float q = rss / rels[base + i];
                in = in && (q > c.sc_lo && q < c.sc_hi);
            }
            v = make_float4(dx / c.rs0, dy / c.rs0, ex / c.rs1, ey / c.rs1);
        }
        const unsigned long long bal = __ballot(in);
        if (lane == 0) red[wid] = __popcll(bal);
        __syncthreads();
        int off = n;
#pragma unroll
        for (int w = 0; w < AL_T / 64; ++w) {
            off += (w < wid) ? red[w] : 0;
            n += red[w];
        }
        if (in) {
            const int at = off + __popcll(bal & ((1ull << lane) - 1ull));
            mem[at] = (unsigned short)i;
            xy[at] = v;
        }
        __syncthreads();
    }
    const size_t so = base + s;
    if (members)
        for (int m = tid; m < n; m += AL_T) members[so * ncap + m] = mem[m];
    if (n < c.min_inl) {
        if (tid == 0 && info) *reinterpret_cast<int4*>(info + 4 * so) = make_int4(n, -1, 0, 0);
        return;
    }
    const int P = max(AL_MINP, 1 << (32 - __clz(n - 1)));  // (n >= 1: the seed itself)

    // duplicates: the four local coordinates bit-equal to an earlier member's
    for (int m = tid; m < n; m += AL_T) {
        const uint4 a = __builtin_bit_cast(uint4, xy[m]);
        bool dup = false;
        for (int u = 0; u < m && !dup; ++u) {
            const uint4 z = __builtin_bit_cast(uint4, xy[u]);
            dup = a.x == z.x && a.y == z.y && a.z == z.z && a.w == z.w;
        }
        wdup[m] = dup ? 0 : 1;
    }
    __syncthreads();

    // ---- D, E: the hypotheses
    int best_it = -1, best_cnt = 0;
    for (int it = 0; it < c.iters; ++it) {
        AlAff A;
        if (!al_hypothesis(it, n, xy, c, A)) continue;  // (the same LDS values in every thread: uniform)
        const AlSel r = al_select(A, n, P, xy, wdup, keys, nullptr, red, c.min_conf, tid);
        if (r.count > best_cnt) best_cnt = r.count, best_it = it;
    }
    int4 out = make_int4(n, best_it, 0, 0);
    float conf = 0.0f;
    bool passed = false;
    if (best_it >= 0) {
        AlAff A;
        al_hypothesis(best_it, n, xy, c, A);
        AlSel r = al_select(A, n, P, xy, wdup, keys, acc, red, c.min_conf, tid);
        bool ok = true;
        if (c.refit) {
            // ---- F
            float* f = reinterpret_cast<float*>(keys);
            const float sxx = al_tree_sum(f, n, P, acc, tid, [&](int m) { return xy[m].x * xy[m].x; });
            const float sxy = al_tree_sum(f, n, P, acc, tid, [&](int m) { return xy[m].x * xy[m].y; });
            const float syy = al_tree_sum(f, n, P, acc, tid, [&](int m) { return xy[m].y * xy[m].y; });
            const float c00 = al_tree_sum(f, n, P, acc, tid, [&](int m) { return xy[m].z * xy[m].x; });
            const float c01 = al_tree_sum(f, n, P, acc, tid, [&](int m) { return xy[m].z * xy[m].y; });
            const float c10 = al_tree_sum(f, n, P, acc, tid, [&](int m) { return xy[m].w * xy[m].x; });
            const float c11 = al_tree_sum(f, n, P, acc, tid, [&](int m) { return xy[m].w * xy[m].y; });
            __syncthreads();
            const float det = sxx * syy - sxy * sxy;
            ok = r.count >= 2 && det >= 1e-12f;
            if (ok) {
                A.a00 = (c00 * syy - c01 * sxy) / det;
                A.a01 = (c01 * sxx - c00 * sxy) / det;
                A.a10 = (c10 * syy - c11 * sxy) / det;
                A.a11 = (c11 * sxx - c10 * sxy) / det;
                r = al_select(A, n, P, xy, wdup, keys, acc, red, c.min_conf, tid);
            }
        }
        // ---- G
        if (ok && r.count > 0) {
            conf = (float)r.count / ((float)r.tot * r.maxr2);
            passed = conf >= c.min_conf && (float)r.count * (1.0f - 1.0f / conf) >= (float)c.min_inl;
            out.z = r.count;
            out.w = passed ? 1 : 0;
        }
    }
    if (tid == 0) {
        if (info) *reinterpret_cast<int4*>(info + 4 * so) = out;
        if (sconf) sconf[so] = conf;
    }
    if (passed) {
        __syncthreads();
        for (int m = tid; m < n; m += AL_T)
            if (acc[m] & 1) {
                const int i = mem[m];
                matches0[base + i] = nn[base + i];
            }
    }
}

// ------------------------------------------------------------------ host
static int al_conf(imcui_hip_s* h, const double* conf, int h0, int w0, int h1, int w1, bool have_ori, bool have_scale, AlP& c) {
    if (!conf) return imcui_set_err(h, IMCUI_ERR_ARG, "adalam: null conf");
    const double area_ratio = conf[0], se = conf[1], ot = conf[5], st = conf[6], dt = conf[7];
    if (!(area_ratio > 0.0) || !(se > 0.0) || conf[2] < 1.0 || conf[3] < 1.0 || !(conf[4] > 0.0) || h0 <= 0 || w0 <= 0 || h1 <= 0 || w1 <= 0)
        return imcui_set_err(h, IMCUI_ERR_ARG, "adalam: area_ratio, search_expansion, min_confidence and the image sizes must be positive, ransac_iters and min_inliers >= 1");
    const double R0 = sqrt((double)h0 * (double)w0 / area_ratio / M_PI), R1 = sqrt((double)h1 * (double)w1 / area_ratio / M_PI);
    c.seed_ratio = (float)(0.8 * 0.8);
    c.r0sq = (float)(R0 * R0);
    const double rs0 = R0 * se, rs1 = R1 * se;
    c.rs0 = (float)rs0, c.rs1 = (float)rs1;
    c.nb0sq = (float)(rs0 * rs0), c.nb1sq = (float)(rs1 * rs1);
    c.iters = (int)conf[2], c.min_inl = (int)conf[3];
    c.min_conf = (float)conf[4];
    c.use_ori = ot >= 0.0 && ot < 180.0;
    c.ori_thr = (float)ot;
    c.use_sc = st >= 0.0 && st < 10.0;
    c.sc_lo = c.use_sc ? (float)(1.0 / st) : 0.0f, c.sc_hi = (float)st;
    c.use_dt = dt >= 0.0;
    c.dt_lo = c.use_dt ? (float)(1.0 / dt) : 0.0f, c.dt_hi = (float)dt;
    if ((c.use_sc && !(st > 0.0)) || (c.use_dt && !(dt > 0.0))) return imcui_set_err(h, IMCUI_ERR_ARG, "adalam: a rate threshold must be positive (negative = off)");
    c.refit = conf[8] != 0.0, c.force_mnn = conf[9] != 0.0;
    if (c.use_ori && !have_ori) return imcui_set_err(h, IMCUI_ERR_ARG, "adalam: orientation_difference_threshold is active but oris0 / oris1 are missing");
    if (c.use_sc && !have_scale) return imcui_set_err(h, IMCUI_ERR_ARG, "adalam: scale_rate_threshold is active but scales0 / scales1 are missing");
    return IMCUI_OK;
}

static int al_check(imcui_hip_s* h, int B, int ncap, const void* k0, const void* k1, const void* n0, const void* n1, const void* m0, const void* ms0) {
    if (B <= 0 || ncap <= 0) return imcui_set_err(h, IMCUI_ERR_ARG, "adalam: B=%d, ncap=%d", B, ncap);
    if (ncap > AL_MAXN) return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "adalam: ncap=%d (at most %d key-points per image)", ncap, AL_MAXN);
    if (B > 65535) return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "adalam: B=%d (at most 65535 pairs per call)", B);
    if (!k0 || !k1 || !n0 || !n1 || !m0 || !ms0) return imcui_set_err(h, IMCUI_ERR_ARG, "adalam: null key-points, counts or outputs");
    return IMCUI_OK;
}

// stages B .. G on nn / score / mnn
static int al_filter(imcui_hip_s* h, const AlWs& w, const AlP& c, int B, int ncap, const float* k0, const float* k1, const float* s0, const float* s1, const float* o0,
                     const float* o1, const int* n0, const int* n1, const int* nn, const float* score, const int* mnn, int* matches0, float* mscores0, int* seed,
                     int* members, int* info, float* sconf, hipStream_t stream) {
    static std::atomic<unsigned long long> optin{0};
    const size_t lds = al_nbh_lds(w.P2);
    if (lds > 65536 && !imcui_lds_optin(optin, reinterpret_cast<const void*>(adalam_nbh_kernel), (int)al_nbh_lds(AL_MAXN)))
        return imcui_set_err(h, IMCUI_ERR_HIP, "adalam: cannot reserve %zu bytes of LDS", lds);
    const dim3 g1(cdiv(ncap, 256), B), blk(256);
    // (scales / orientations are read only by the test that is on)
    hipLaunchKernelGGL(adalam_prep_kernel, g1, blk, 0, stream, ncap, n0, n1, reinterpret_cast<const float2*>(k1), c.use_sc ? s0 : nullptr, s1, c.use_ori ? o0 : nullptr, o1,
                       nn, w.p, w.relo, w.rels, w.valid, matches0, mscores0, info, sconf);
    int* sd = seed ? seed : w.seed;
    hipLaunchKernelGGL(adalam_seed_kernel, g1, blk, 0, stream, ncap, n0, n1, reinterpret_cast<const float2*>(k0), score, mnn, w.valid, c, sd);
    hipLaunchKernelGGL(adalam_order_kernel, dim3(B), dim3(AL_T), (size_t)w.P2 * 8, stream, ncap, w.P2, n0, n1, score, w.valid, w.order);
    hipLaunchKernelGGL(adalam_nbh_kernel, dim3(ncap, B), dim3(AL_T), lds, stream, ncap, w.P2, n0, n1, reinterpret_cast<const float2*>(k0), nn, w.p, w.relo, w.rels, sd,
                       w.order, c, matches0, members, info, sconf);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

extern "C" size_t imcui_hip_adalam_workspace_bytes(imcui_hip_t* h, int B, int ncap, int D) {
    (void)h;
    if (B <= 0 || ncap <= 0 || ncap > AL_MAXN) return 0;
    return al_carve(nullptr, 0, B, ncap, D > 0 ? D : 0).total;
}

extern "C" int imcui_hip_adalam_filter(imcui_hip_t* h, int B, int ncap, const float* keypoints0, const float* keypoints1, const float* scales0, const float* scales1,
                                       const float* oris0, const float* oris1, const int* n0, const int* n1, int h0, int w0, int h1, int w1, const double* conf,
                                       const int* nn, const float* score, const int* mnn, int* matches0, float* matching_scores0, int* seed, int* seed_members,
                                       int* seed_info, float* seed_conf, void* ws, size_t ws_bytes, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    int rc;
    IMCUI_RUN(al_check(h, B, ncap, keypoints0, keypoints1, n0, n1, matches0, matching_scores0));
    if (!nn || !score || !mnn) return imcui_set_err(h, IMCUI_ERR_ARG, "adalam_filter: null nn / score / mnn");
    AlP c{};
    IMCUI_RUN(al_conf(h, conf, h0, w0, h1, w1, oris0 && oris1, scales0 && scales1, c));
    const AlWs w = al_carve(ws, ws_bytes, B, ncap, 0);
    if (!ws || !w.ok) return imcui_set_err(h, IMCUI_ERR_WS, "adalam_filter: workspace too small (%zu < %zu)", ws_bytes, w.total);
    return al_filter(h, w, c, B, ncap, keypoints0, keypoints1, scales0, scales1, oris0, oris1, n0, n1, nn, score, mnn, matches0, matching_scores0, seed, seed_members,
                     seed_info, seed_conf, (hipStream_t)stream_);
}

extern "C" int imcui_hip_adalam_forward(imcui_hip_t* h, int B, int ncap, int D, const float* descriptors0, const float* descriptors1, const float* keypoints0,
                                        const float* keypoints1, const float* scales0, const float* scales1, const float* oris0, const float* oris1, const int* n0,
                                        const int* n1, int h0, int w0, int h1, int w1, const double* conf, int* matches0, float* matching_scores0, int* nn, float* score,
                                        int* mnn, int* seed, int* seed_members, int* seed_info, float* seed_conf, void* ws, size_t ws_bytes, void* stream_) {
    if (!h) return IMCUI_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    int rc;
    IMCUI_RUN(al_check(h, B, ncap, keypoints0, keypoints1, n0, n1, matches0, matching_scores0));
    if (!simred_ok(D)) return imcui_set_err(h, IMCUI_ERR_UNSUPPORTED, "adalam: descriptor width %d (64, 128 or 256)", D);
    if (!descriptors0 || !descriptors1) return imcui_set_err(h, IMCUI_ERR_ARG, "adalam: null descriptors");
    AlP c{};
    IMCUI_RUN(al_conf(h, conf, h0, w0, h1, w1, oris0 && oris1, scales0 && scales1, c));
    const AlWs w = al_carve(ws, ws_bytes, B, ncap, D);
    if (!ws || !w.ok) return imcui_set_err(h, IMCUI_ERR_WS, "adalam: workspace too small (%zu < %zu)", ws_bytes, w.total);
    // ---- A
    hipLaunchKernelGGL(adalam_norm_kernel, dim3(cdiv(ncap, 256), B, 2), dim3(256), 0, stream, descriptors0, descriptors1, ncap, D, n0, n1, w.rn, w.cn);
    simred_pack(h, descriptors0, D, 1, (long)ncap * D, ncap, D, B, n0, 1, w.pk0, stream);
    simred_pack(h, descriptors1, D, 1, (long)ncap * D, ncap, D, B, n1, 1, w.pk1, stream);
    SimRedP p;
    p.mode = SR_NND;
    p.Ap = w.pk0, p.Bp = w.pk1;
    p.ap_bs = p.bp_bs = (long)simred_packed_uint4(ncap, D);
    p.M = ncap, p.N = ncap, p.K = D, p.batch = B;
    p.mcnt = n0, p.ncnt = n1, p.cnt_stride = 1;
    p.nchunk = w.nchunk;
    p.r0 = w.rb1, p.r1 = w.rb2, p.ri = w.ri1, p.r_pitch = ncap;
    p.c0 = w.cb1, p.c1 = w.cb2, p.ci = w.ci1, p.c_pitch = ncap;
    p.rnorm = w.rn, p.cnorm = w.cn, p.rn_bs = p.cn_bs = ncap;
    IMCUI_RUN(simred_launch(h, p, stream));
    int* nn_ = nn ? nn : w.nn;
    float* sc_ = score ? score : w.score;
    int* mu_ = mnn ? mnn : w.mnn;
    const dim3 g1(cdiv(ncap, 256), B), blk(256);
    hipLaunchKernelGGL(adalam_colmerge_kernel, g1, blk, 0, stream, w.cb1, w.ci1, w.nrb, ncap, n0, n1, w.nn21);
    hipLaunchKernelGGL(adalam_rowmerge_kernel, g1, blk, 0, stream, w.rb1, w.rb2, w.ri1, w.nchunk, ncap, n0, n1, w.nn21, nn_, sc_, mu_);
    return al_filter(h, w, c, B, ncap, keypoints0, keypoints1, scales0, scales1, oris0, oris1, n0, n1, nn_, sc_, mu_, matches0, matching_scores0, seed, seed_members, seed_info,
                     seed_conf, stream);
}
