// List-building blocks shared by the extractors and matchers: ordered candidate compaction over a score map, an exclusive scan, the
// order-preserving float key, the radix select of the k-th largest key, the rank of a flagged thread inside its workgroup, the loop
// that keeps the keys >= the k-th in list order, and the candidate list of the multi-scale extractors (zero, advance, cut, rank, the
// ranked rows).  Below the kernels, the host side of the same blocks: cand_chunks, the scratch they index (CandScan, ScoreIndexList,
// CutList, each with its carve) and their launches (cand_count_scan, cand_compact, cand_list, cand_cut, ranked_rows).
// The RULES stay with their owners (sp_topk_kernel, dk_select_kernel, ak_select_kernel, xf_rank_kernel, al_cut_kernel, dd_cut_kernel,
// the Row functors of ranked_rows_kernel, ...): which candidates a network keeps, in which order and how ties fall differs per network,
// and none of that is decided here; R2D2, D2-Net, LANet and DarkFeat share one rule (a stable argsort of (score, list index)) and hence
// one cut and one rank.
#pragma once
#include "common.h"

namespace {  // internal linkage: several translation units include these kernels

// ------------------------------------------------------------------ rank of a flagged thread, in thread order
// rank inside the wave (flagged lanes below this one) and the wave's count
__device__ __forceinline__ int wave_ordered_rank(bool flag, int* count) {
    const unsigned long long bal = __ballot(flag);
    *count = __popcll(bal);
    return __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// rank inside a workgroup of NWAVES waves and the workgroup's count (*total, the same in every thread: a caller that walks a list in
// batches carries its running base in a register).  Every thread of the workgroup calls it.  lds_counts[NWAVES] may be handed to the
// next call straight away: the second barrier keeps a fast wave's next counts away from a slow wave's reads.
template <int NWAVES>
__device__ __forceinline__ int block_ordered_rank(bool flag, int* lds_counts, int* total) {
    const int wid = threadIdx.x >> 6;
    int wcount;
    const int before = wave_ordered_rank(flag, &wcount);
    if ((threadIdx.x & 63) == 0) lds_counts[wid] = wcount;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < NWAVES; ++q) {
        const int c = lds_counts[q];
        if (q < wid) off += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return off + before;
}

// ------------------------------------------------------------------ ordered candidate compaction over a score map
// count -> exclusive scan of the per-chunk counts -> compact: the candidates of image b leave in row-major order, no sort and no atomics.
// Grid (nchunk, B) with nchunk = cdiv(npix, SEL_CHUNK), 256 threads.
//   Pred: void bind(int b)                                   -- once per thread, ahead of its pixels: what the predicate reads per image
//         bool operator()(const float* img, int idx) const   -- img = image b's map, idx < npix its flat pixel index
//   Emit: void operator()(int b, int pos, int idx, float v) const   -- candidate number pos of image b is pixel idx with value v
#define SEL_CHUNK 4096  // pixels per block (16 consecutive per thread)

template <class Pred>
__global__ __launch_bounds__(256) void cand_count_kernel(const float* __restrict__ map, int npix, Pred pred, int* __restrict__ blkcnt, int nchunk) {
    __shared__ int wsum[4];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* img = map + (long)b * npix;
    const int base = chunk * SEL_CHUNK + threadIdx.x * 16;
    pred.bind(b);
    int c = 0;
    for (int j = 0; j < 16; ++j) {
        const int idx = base + j;
        if (idx < npix && pred(img, idx)) ++c;  // (the last chunk is partial)
    }
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blkcnt[b * nchunk + chunk] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// the candidate list DISK and ALIKED keep: cscore [b][ccap] = map value, cidx [b][ccap] = flat pixel index
struct EmitScoreIndex {
    float* cscore;
    int* cidx;
    int ccap;
    __device__ void operator()(int b, int pos, int idx, float v) const {
        cscore[(long)b * ccap + pos] = v;
        cidx[(long)b * ccap + pos] = idx;
    }
};

// blkoff = the exclusive scan of cand_count_kernel's counts.  Positions past `cap` are counted and not written, so that the total (the
// scan's) still tells the owner of the list that it overflowed.
template <class Pred, class Emit>
__global__ __launch_bounds__(256) void cand_compact_kernel(const float* __restrict__ map, int npix, Pred pred, const int* __restrict__ blkoff, int nchunk,
                                                           int cap, Emit emit) {
    __shared__ int tcnt[256];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* img = map + (long)b * npix;
    const int base = chunk * SEL_CHUNK + threadIdx.x * 16;
    pred.bind(b);
    unsigned flags = 0;
    int c = 0;
    for (int j = 0; j < 16; ++j) {
        const int idx = base + j;
        if (idx < npix && pred(img, idx)) {
            flags |= 1u << j;
            ++c;
        }
    }
    tcnt[threadIdx.x] = c;
    __syncthreads();
    // exclusive prefix over the 256 per-thread counts (Hillis-Steele)
    for (int o = 1; o < 256; o <<= 1) {
        const int add = (threadIdx.x >= o) ? tcnt[threadIdx.x - o] : 0;
        __syncthreads();
        tcnt[threadIdx.x] += add;
        __syncthreads();
    }
    int pos = blkoff[b * nchunk + chunk] + tcnt[threadIdx.x] - c;
    for (int j = 0; j < 16; ++j)
        if (flags & (1u << j)) {
            if (pos < cap) emit(b, pos, base + j, img[base + j]);
            ++pos;
        }
}

// exclusive scan of in[b][0..n) (n = min(*n_dev[b], n_cap) when n_dev, else n_cap) -> out[b][.], total[b]; one workgroup of 1024 per
// row; in place (out == in) or out of place.  (A template so that only the translation units that launch it carry a copy.)
template <class T>
__global__ __launch_bounds__(1024) void exclusive_scan_kernel(const T* in, T* out, T* total, const int* n_dev, int n_cap, long stride) {
    __shared__ T s[1024];
    const int b = blockIdx.x;
    int n = n_cap;
    if (n_dev) n = min(n_dev[b], n_cap);
    const T* ib = in + (long)b * stride;
    T* ob = out + (long)b * stride;
    T carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const T v = i < n ? ib[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const T t = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n) ob[i] = carry + s[threadIdx.x] - v;
        carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[b] = carry;
}

// ------------------------------------------------------------------ k-th largest key
// order-preserving key of a float: a < b <=> order_key(a) < order_key(b)
__device__ __forceinline__ unsigned order_key(float f) {
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;  // -0 == +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The k-th largest of the n keys load(0) .. load(n - 1), Key = unsigned (4 rounds of an 8-bit histogram) or unsigned long long (8
// rounds).  *n_equal (when asked for) = how many of the keys EQUAL to it belong to the k largest: k minus the count of strictly
// larger keys.  Every thread of the workgroup of NTHREADS calls it, with 1 <= k <= n.
template <int NTHREADS, class Key, class Load>
__device__ __forceinline__ Key radix_select_kth(Load load, int n, int k, int* n_equal = nullptr) {
    __shared__ int hist[256];
    __shared__ Key s_prefix;
    __shared__ int s_k;
    const int tid = threadIdx.x;
    constexpr int TOP = (int)sizeof(Key) - 1;
    if (tid == 0) {
        s_prefix = 0;
        s_k = k;
    }
    __syncthreads();
    for (int byte = TOP; byte >= 0; --byte) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const Key prefix = s_prefix;
        const Key himask = (byte == TOP) ? (Key)0 : (Key)(~(Key)0 << (8 * (byte + 1)));
        for (int i = tid; i < n; i += NTHREADS) {
            const Key key = load(i);
            if ((key & himask) == prefix) atomicAdd(&hist[(int)((key >> (8 * byte)) & 0xFF)], 1);
        }
        __syncthreads();
        // the digit of the k-th key: walk the bins downwards until the running count reaches k.  One wave does it in parallel (lane l owns
        // bins 255 - 4 l .. 252 - 4 l, inclusive scan over the lanes, the first lane that reaches k finishes inside its four bins); one
        // thread walking 255 dependent LDS reads, eight times, was most of sp_topk_kernel's 84 us
        if (tid < 64) {
            const int d0 = 255 - 4 * tid;
            const int h0 = hist[d0], h1 = hist[d0 - 1], h2 = hist[d0 - 2], h3 = hist[d0 - 3];
            const int mine = h0 + h1 + h2 + h3;
            int inc = mine;
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(inc, o, 64);
                if (tid >= o) inc += up;
            }
            const int kk = s_k;
            const unsigned long long reach = __ballot(inc >= kk);
            const int L = reach ? __ffsll((long long)reach) - 1 : 63;  // (never empty: at least k keys carry the prefix; 63 = bin 0 all the same)
            if (tid == L) {
                int k2 = kk - (inc - mine), d;
                if (h0 >= k2)
                    d = d0;
                else if (h0 + h1 >= k2)
                    d = d0 - 1, k2 -= h0;
                else if (h0 + h1 + h2 >= k2)
                    d = d0 - 2, k2 -= h0 + h1;
                else
                    d = d0 - 3, k2 -= h0 + h1 + h2;  // (lane 63: bin 0 takes what is left, as the sequential walk did)
                s_prefix = prefix | ((Key)d << (8 * byte));
                s_k = k2;
            }
        }
        __syncthreads();
    }
    if (n_equal) *n_equal = s_k;
    return s_prefix;
}

// ------------------------------------------------------------------ keeping the k largest of a list, in list order
// Entries i of 0 .. n - 1 with key_at(i) >= kth (every entry when !filter) go to out[0 .. limit) in list order.  Returns how many
// qualified (it may exceed limit).  Every thread of the workgroup of 1024 calls it.
template <class KeyAt>
__device__ __forceinline__ int keep_kth_in_order(KeyAt key_at, int n, bool filter, unsigned long long kth, int limit, int* __restrict__ out) {
    __shared__ int wcnt[16];
    int run = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const bool keep = i < n && (!filter || key_at(i) >= kth);
        int tot;
        const int pos = run + block_ordered_rank<16>(keep, wcnt, &tot);
        if (keep && pos < limit) out[pos] = i;
        run += tot;
    }
    return run;
}

// ------------------------------------------------------------------ the candidate list of a multi-scale extractor (R2D2, D2-Net)
// Every level appends its candidates to the image's list at base[b]; after the last level the list is cut and the emit kernel of the
// network ranks what is left.  (The three kernels are templates -- launched as name<> -- so that only the translation units that launch
// them carry a copy.)
template <class = void>
__global__ void zero_i32_kernel(int* __restrict__ p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}
template <class = void>
__global__ void advance_base_kernel(int* __restrict__ base, const int* __restrict__ nlev, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) base[b] += nlev[b];  // (the true count: an overflow stays visible)
}

// (score, candidate index) as one ordered key: a stable argsort puts equal scores in list order
__device__ __forceinline__ unsigned long long score_index_key(float s, int i) { return ((unsigned long long)order_key(s) << 32) | (unsigned)i; }

// The cut.  One workgroup of 1024 per image: more than `limit` candidates -> the `limit` largest keys stay; the kept slots leave in
// candidate order (kslot), the emit kernel ranks them.  status bit 1: more candidates than the list holds.
template <class = void>
__global__ __launch_bounds__(1024) void cand_cut_kernel(const float* __restrict__ cscore, const int* __restrict__ ntotal, int kcap, int limit_,
                                                        int* __restrict__ kslot, int* __restrict__ nkept, int* __restrict__ status) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* cs = cscore + (long)b * kcap;
    const int n = min(ntotal[b], kcap);
    if (tid == 0 && ntotal[b] > kcap) atomicOr(status, 2);  // candidate capacity too small
    const auto key_at = [&](int i) { return score_index_key(cs[i], i); };
    bool filter = false;
    unsigned long long kth = 0;
    int limit = n;
    if (limit_ > 0 && n > limit_) {
        filter = true;
        limit = limit_;
        kth = radix_select_kth<1024, unsigned long long>(key_at, n, limit_);
    }
    const int run = keep_kth_in_order(key_at, n, filter, kth, limit, kslot + (long)b * kcap);
    if (tid == 0) nkept[b] = min(run, limit);
}

// The rank of kept candidate i (this thread's; any value when i >= n) among the n kept ones ks[0 .. n) in ascending (score, position)
// order; the kept list is in slot order, so equal scores keep it.  Every thread of the workgroup of 256 calls it.
__device__ __forceinline__ int kept_rank_ascending(const float* __restrict__ cs, const int* __restrict__ ks, int n, int i) {
    __shared__ float tile[256];
    const int tid = threadIdx.x;
    const float mine = i < n ? cs[ks[i]] : 0.0f;
    int rank = 0;
    for (int base = 0; base < n; base += 256) {
        __syncthreads();
        tile[tid] = base + tid < n ? cs[ks[base + tid]] : INFINITY;
        __syncthreads();
        const int m = min(256, n - base);
        for (int j = 0; j < m; ++j) {
            const float o = tile[j];
            rank += (o < mine || (o == mine && base + j < i)) ? 1 : 0;
        }
    }
    return rank;
}

// The ranked rows of a cut list.  Grid (cdiv(kout, 256), B), 256 threads: one workgroup = 256 kept candidates of image b; n =
// min(nkept[b], kout) rows leave, nkpts[b] = n (when asked for).  The rank needs every thread of the workgroup (it has barriers), so
// a workgroup leaves only as a whole.  Every thread calls both members of Row, which shares the rows out (a thread or a wave each):
//   void clear(int b, int lo, int hi) const   -- output rows [lo, hi) of this workgroup lie past the count
//   void emit(int b, int i0, int m, const int* ks, const int* rank, const float* cs) const
//        -- kept candidate i0 + j (j < m) sits in slot ks[i0 + j] with score cs[slot] and goes to output row rank[j] (LDS)
template <class Row>
__global__ __launch_bounds__(256) void ranked_rows_kernel(const float* __restrict__ cscore, const int* __restrict__ kslot, const int* __restrict__ nkept, int cap,
                                                          int kout, int* __restrict__ nkpts, Row row) {
    __shared__ int rank_s[256];
    const int b = blockIdx.y, i0 = blockIdx.x * 256;
    const float* cs = cscore + (long)b * cap;
    const int* ks = kslot + (long)b * cap;
    const int n = min(nkept[b], kout);
    if (nkpts && blockIdx.x == 0 && threadIdx.x == 0) nkpts[b] = n;
    row.clear(b, max(i0, n), min(i0 + 256, kout));
    if (i0 >= n) return;  // (uniform)
    rank_s[threadIdx.x] = kept_rank_ascending(cs, ks, n, i0 + threadIdx.x);
    __syncthreads();
    row.emit(b, i0, min(256, n - i0), ks, rank_s, cs);
}

// ------------------------------------------------------------------ host side: the scratch of the blocks above and their launches
// One place that sizes, carves and passes what the kernels index with, so that the chunk count, the row stride and the capacity cannot
// differ between a launch and its scratch.  The caller checks the launches (IMCUI_CHECK_LAUNCH), where the handle is.
static inline int cand_chunks(long domain) { return (int)((domain + SEL_CHUNK - 1) / SEL_CHUNK); }

// per-chunk counts, their exclusive scan and the per-image total, sized for the largest domain the owner scans
struct CandScan {
    int *blkcnt, *blkoff, *total;
    void carve(WsAlloc& a, int B, size_t domain_max) {
        const size_t n = (size_t)B * cand_chunks((long)domain_max);
        blkcnt = a.get<int>(n);
        blkoff = a.get<int>(n);
        total = a.get<int>(B);
    }
};

template <class Pred>
static void cand_count_scan(hipStream_t stream, const float* map, int domain, int B, Pred pred, const CandScan& s) {
    const int nchunk = cand_chunks(domain);
    hipLaunchKernelGGL(cand_count_kernel<Pred>, dim3(nchunk, B), dim3(256), 0, stream, map, domain, pred, s.blkcnt, nchunk);
    hipLaunchKernelGGL(exclusive_scan_kernel<int>, dim3(B), dim3(1024), 0, stream, s.blkcnt, s.blkoff, s.total, (const int*)nullptr, nchunk, (long)nchunk);
}
template <class Pred, class Emit>
static void cand_compact(hipStream_t stream, const float* map, int domain, int B, Pred pred, const CandScan& s, int cap, Emit emit) {
    const int nchunk = cand_chunks(domain);
    hipLaunchKernelGGL((cand_compact_kernel<Pred, Emit>), dim3(nchunk, B), dim3(256), 0, stream, map, domain, pred, s.blkoff, nchunk, cap, emit);
}
template <class Pred, class Emit>
static void cand_list(hipStream_t stream, const float* map, int domain, int B, Pred pred, const CandScan& s, int cap, Emit emit) {
    cand_count_scan(stream, map, domain, B, pred, s);
    cand_compact(stream, map, domain, B, pred, s, cap, emit);
}

// the list EmitScoreIndex fills, [B][cap] each
struct ScoreIndexList {
    float* cscore;
    int* cidx;
    int cap;
    void carve(WsAlloc& a, int B, int cap_) {
        cap = cap_;
        cscore = a.get<float>((size_t)B * cap);
        cidx = a.get<int>((size_t)B * cap);
    }
    EmitScoreIndex emit() const { return EmitScoreIndex{cscore, cidx, cap}; }
};

// what cand_cut_kernel leaves: kslot [B][cap], nkept [B]
struct CutList {
    int *kslot, *nkept;
    void carve(WsAlloc& a, int B, int cap) {
        kslot = a.get<int>((size_t)B * cap);
        nkept = a.get<int>(B);
    }
};
template <class = void>  // (as the kernel: only the translation units that call it carry a copy)
static void cand_cut(hipStream_t stream, const float* cscore, const int* ntotal, int cap, int limit, const CutList& cut, int* status, int B) {
    hipLaunchKernelGGL(cand_cut_kernel<>, dim3(B), dim3(1024), 0, stream, cscore, ntotal, cap, limit, cut.kslot, cut.nkept, status);
}
template <class Row>
static void ranked_rows(hipStream_t stream, const float* cscore, int cap, const CutList& cut, int kout, int* nkpts, Row row, int B) {
    hipLaunchKernelGGL(ranked_rows_kernel<Row>, dim3(cdiv(kout, 256), B), dim3(256), 0, stream, cscore, cut.kslot, cut.nkept, cap, kout, nkpts, row);
}

}  // namespace
