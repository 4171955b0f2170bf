// Test entry into the list-building blocks of select.h (imcui_hip_select_probe, tests/test_gpu_select.py): every op wraps one block, or
// the chain its callers launch together, with the template arguments the tree uses, on arrays given by the caller.
//
// The blocks are templates in an anonymous namespace, so this translation unit carries its OWN compiled copy of each: the probe tests
// the SOURCE of select.h.  It does not test the copies compiled into each owner (superpoint.hip, disk.hip, aliked.hip, ...); those are
// reached by the stage probes (imcui_hip_superpoint_select_probe, imcui_hip_disk_select_probe) and by the network tests.
//
// Everything a launch indexes with is checked on the host (imcui_hip_select_desc_check) before anything is launched.
#include "imcui_hip.h"
#include "select.h"

enum SelOp { SEL_COMPACT = 0, SEL_SCAN, SEL_ORDER_KEY, SEL_KTH32, SEL_KTH64, SEL_RANK4, SEL_RANK16, SEL_KEEP, SEL_CUT, SEL_NOP };

// per-row lengths and ranks, by value
struct SelRows {
    int n[IMCUI_SELECT_MAXB], k[IMCUI_SELECT_MAXB];
};

// COMPACT's predicate: above the image's own threshold, which bind(b) fetches once per thread
struct SelAboveThr {
    const float* thr;  // [B]
    float t;
    __device__ void bind(int b) { t = thr[b]; }
    __device__ bool operator()(const float* img, int idx) const { return img[idx] > t; }
};

__global__ void sel_order_key_kernel(const float* __restrict__ in, unsigned* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = order_key(in[i]);
}

__global__ __launch_bounds__(1024) void sel_kth32_kernel(const float* __restrict__ score, long stride, SelRows r, unsigned* __restrict__ key, int* __restrict__ n_equal) {
    const int b = blockIdx.x;
    const float* s = score + b * stride;
    int ne;
    const unsigned kth = radix_select_kth<1024, unsigned>([&](int i) { return order_key(s[i]); }, r.n[b], r.k[b], &ne);
    if (threadIdx.x == 0) key[b] = kth, n_equal[b] = ne;
}

__global__ __launch_bounds__(1024) void sel_kth64_kernel(const unsigned long long* __restrict__ keys, long stride, SelRows r, unsigned long long* __restrict__ key,
                                                         int* __restrict__ n_equal) {
    const int b = blockIdx.x;
    const unsigned long long* s = keys + b * stride;
    int ne;
    const unsigned long long kth = radix_select_kth<1024, unsigned long long>([&](int i) { return s[i]; }, r.n[b], r.k[b], &ne);
    if (threadIdx.x == 0) key[b] = kth, n_equal[b] = ne;
}

template <int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void sel_rank_kernel(const int* __restrict__ flags, long stride, SelRows r, int* __restrict__ pos, int* __restrict__ total) {
    __shared__ int wcnt[NWAVES];
    const int b = blockIdx.x, n = r.n[b];
    int run = 0;
    for (int base = 0; base < n; base += NWAVES * 64) {
        const int i = base + threadIdx.x;
        const bool flag = i < n && flags[b * stride + i] != 0;
        int tot;
        const int p = run + block_ordered_rank<NWAVES>(flag, wcnt, &tot);
        if (flag) pos[b * stride + i] = p;
        run += tot;
    }
    if (threadIdx.x == 0) total[b] = run;
}

__global__ __launch_bounds__(1024) void sel_keep_kernel(const unsigned long long* __restrict__ keys, long stride, SelRows r, int filter, unsigned long long kth, int limit,
                                                        int* __restrict__ out, int* __restrict__ count) {
    const int b = blockIdx.x;
    const unsigned long long* s = keys + b * stride;
    const int run = keep_kth_in_order([&](int i) { return s[i]; }, r.n[b], filter != 0, kth, limit, out + b * stride);
    if (threadIdx.x == 0) count[b] = run;
}

// CUT's rows of ranked_rows_kernel: entry i of the output holds the rank of kept candidate i; entries past the count keep what the
// caller put there
struct SelRankRow {
    int* rank;  // [B][kcap]
    int kcap;
    __device__ void clear(int, int, int) const {}
    __device__ void emit(int b, int i0, int m, const int*, const int* rank_s, const float*) const {
        if ((int)threadIdx.x < m) rank[(long)b * kcap + i0 + threadIdx.x] = rank_s[threadIdx.x];
    }
};

extern "C" size_t imcui_hip_select_desc_bytes(void) { return sizeof(imcui_hip_select_desc); }

extern "C" int imcui_hip_select_desc_check(const imcui_hip_select_desc* d) {
    if (!d) return 6;
    if (d->op < 0 || d->op >= SEL_NOP) return 1;
    if (d->B < 1 || d->B > IMCUI_SELECT_MAXB) return 2;
    const int MAXN = 1 << 24;
    if (d->capacity < 1 || d->capacity > MAXN) return 3;
    const bool rows = d->op == SEL_KTH32 || d->op == SEL_KTH64 || d->op == SEL_RANK4 || d->op == SEL_RANK16 || d->op == SEL_KEEP;
    if (d->op == SEL_COMPACT) {
        if (d->n < 1 || d->n > MAXN) return 3;
    } else if (d->op == SEL_SCAN || d->op == SEL_ORDER_KEY) {
        if (d->n < 0 || d->n > d->capacity) return 3;
    }
    if (rows)
        for (int b = 0; b < d->B; ++b)
            if (d->n_row[b] < 0 || d->n_row[b] > d->capacity) return 3;
    if (d->op == SEL_KTH32 || d->op == SEL_KTH64)
        for (int b = 0; b < d->B; ++b)
            if (d->k_row[b] < 1 || d->k_row[b] > d->n_row[b]) return 4;
    if (d->op == SEL_COMPACT && (d->cap < 0 || d->cap > d->capacity)) return 5;
    if ((d->op == SEL_KEEP || d->op == SEL_CUT) && d->limit < 0) return 5;
    bool ptrs = true;
    switch (d->op) {
        case SEL_COMPACT: ptrs = d->score && d->thr && d->out_score && d->out_idx && d->out_count && d->out_i32 && d->out_aux; break;
        case SEL_SCAN: ptrs = d->in_i32 && d->out_i32 && d->out_count; break;
        case SEL_ORDER_KEY: ptrs = d->score && d->out_key32; break;
        case SEL_KTH32: ptrs = d->score && d->out_key32 && d->out_count; break;
        case SEL_KTH64: ptrs = d->key64 && d->out_key64 && d->out_count; break;
        case SEL_RANK4:
        case SEL_RANK16: ptrs = d->in_i32 && d->out_idx && d->out_count; break;
        case SEL_KEEP: ptrs = d->key64 && d->out_idx && d->out_count; break;
        case SEL_CUT: ptrs = d->score && d->in_i32 && d->out_idx && d->out_count && d->out_i32 && d->out_aux && d->status; break;
    }
    if (!ptrs) return 6;
    if (d->op == SEL_CUT && (d->nlev < 2 || d->nlev > 16)) return 7;
    return 0;
}

extern "C" int imcui_hip_select_probe(imcui_hip_t* h, const imcui_hip_select_desc* d, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    const int rule = imcui_hip_select_desc_check(d);
    if (rule) return imcui_set_err(h, IMCUI_ERR_ARG, "select_probe: descriptor rule %d (include/imcui_hip.h)", rule);
    const int B = d->B, cap = d->capacity;
    SelRows r;
    for (int b = 0; b < IMCUI_SELECT_MAXB; ++b) r.n[b] = b < B ? d->n_row[b] : 0, r.k[b] = b < B ? d->k_row[b] : 1;
    switch (d->op) {
        case SEL_COMPACT:  // (the list's rows are `capacity` apart; positions past d->cap are counted only)
            cand_list(stream, d->score, d->n, B, SelAboveThr{d->thr, 0.0f}, CandScan{d->out_aux, d->out_i32, d->out_count}, d->cap,
                      EmitScoreIndex{d->out_score, d->out_idx, cap});
            break;
        case SEL_SCAN:
            hipLaunchKernelGGL(exclusive_scan_kernel<int>, dim3(B), dim3(1024), 0, stream, d->in_i32, d->out_i32, d->out_count, d->n_dev, d->n, (long)cap);
            break;
        case SEL_ORDER_KEY:
            if (d->n > 0) hipLaunchKernelGGL(sel_order_key_kernel, dim3(cdiv(d->n, 256)), dim3(256), 0, stream, d->score, d->out_key32, d->n);
            break;
        case SEL_KTH32:
            hipLaunchKernelGGL(sel_kth32_kernel, dim3(B), dim3(1024), 0, stream, d->score, (long)cap, r, d->out_key32, d->out_count);
            break;
        case SEL_KTH64:
            hipLaunchKernelGGL(sel_kth64_kernel, dim3(B), dim3(1024), 0, stream, d->key64, (long)cap, r, d->out_key64, d->out_count);
            break;
        case SEL_RANK4:
            hipLaunchKernelGGL(sel_rank_kernel<4>, dim3(B), dim3(256), 0, stream, d->in_i32, (long)cap, r, d->out_idx, d->out_count);
            break;
        case SEL_RANK16:
            hipLaunchKernelGGL(sel_rank_kernel<16>, dim3(B), dim3(1024), 0, stream, d->in_i32, (long)cap, r, d->out_idx, d->out_count);
            break;
        case SEL_KEEP:
            hipLaunchKernelGGL(sel_keep_kernel, dim3(B), dim3(1024), 0, stream, d->key64, (long)cap, r, d->filter, d->kth, d->limit, d->out_idx, d->out_count);
            break;
        case SEL_CUT: {
            int* base = d->out_aux;
            hipLaunchKernelGGL(zero_i32_kernel<>, dim3(cdiv(B, 256)), dim3(256), 0, stream, base, B);
            hipLaunchKernelGGL(zero_i32_kernel<>, dim3(1), dim3(64), 0, stream, d->status, 1);
            for (int l = 0; l < d->nlev; ++l)
                hipLaunchKernelGGL(advance_base_kernel<>, dim3(cdiv(B, 256)), dim3(256), 0, stream, base, d->in_i32 + (long)l * B, B);
            const CutList cut{d->out_idx, d->out_count};
            cand_cut(stream, d->score, base, cap, d->limit, cut, d->status, B);
            ranked_rows(stream, d->score, cap, cut, cap, (int*)nullptr, SelRankRow{d->out_i32, cap}, B);
            break;
        }
    }
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
