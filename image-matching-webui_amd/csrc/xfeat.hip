// XFeat sparse extraction on MI355X: XFeatModel (verlab/accelerated_features) + XFeat.detectAndCompute, the call behind
// imcui/hloc/extractors/xfeat.py:26-34 (`self.net.detectAndCompute(data["image"], top_k=max_keypoints)[0]`).
//
// Data flow (NHWC maps; Hr x Wr = the image resized to multiples of 32, level l = 1/2^l):
//   gray   = bilinear resize (ATen, align_corners=False) of every channel, channel mean                     [B, Hr, Wr]
//   stats  = per-image mean / biased variance of gray (InstanceNorm2d(1), eps 1e-5), fixed order
//   block1 = 1->4, 4->8 s2, 8->8, 8->24 s2 on the VALU, the normalisation applied while the first layer loads; the last layer adds
//            skip1 (4x4 average of the normalised image, 1x1 convolution to 24) and stores 32 channels (24..31 zero)
//   block2, block3.0 : channels stored as 32, implicit 3x3 GEMM (gemm.h);  block3.1 .. block5, block_fusion: implicit 3x3 GEMM
//            (stride 1 / 2) and plain GEMM for the 1x1 layers, BatchNorm folded into weights and bias at pack time
//   fuse   = x3 + up2(x4) + up4(x5) in one kernel (nothing up-sampled is stored)
//   heads  = heatmap_head.0 / .1 (GEMM), then ONE epilogue kernel: 64 -> 1 + sigmoid (reliability) and the channel L2 norm of feats
//            keypoint_head on the 8x8 cells of the normalised image (xf_unfold_kernel), 65-way soft-max, dustbin dropped, written
//            straight to the pixel grid (K1h)
//   select = 5x5 NMS (== max and > threshold, plateaus keep every member) -> candidate list (select.h) -> score = nearest(K1h) x
//            bilinear(reliability) with the reference's float32 grid arithmetic, (0, 0) -> -1 -> rank by (score descending, flat index
//            ascending) -> cut at top_k -> score > 0
//   desc   = bicubic grid_sample (A = -0.75, zeros) of the normalised 64-channel map at the key-point, L2 norm; one wave per key-point
// InstanceNorm statistics are reduced in a fixed order and every grid is sized by shapes or capacities: an image's outputs do not depend
// on the batch it is in and nothing synchronises with the host.
// The layer table, the kernels and the trunk's launch sequence live in xf_shared.h (LiftFeat runs the same trunk); this file keeps the
// packing, XFeat's heads and selection rule, and the entry points.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "xf_shared.h"

extern "C" size_t imcui_hip_xfeat_packed_floats(void) { return xf_layout().total; }
extern "C" int imcui_hip_xfeat_num_tensors(void) { return xf_num_tensors(); }

extern "C" const char* imcui_hip_xfeat_tensor_name(int i) {
    static thread_local char buf[64];
    if (i < 0 || i >= xf_num_tensors()) return nullptr;
    if (i < 2) return i == 0 ? "skip1.1.weight" : "skip1.1.bias";
    int t = 2;
    for (int l = 0; l < XF_NL; ++l) {
        const int n = XF_LAYERS[l].bn ? 3 : 2;
        if (i < t + n) {
            static const char* const bn[3] = {"layer.0.weight", "layer.1.running_mean", "layer.1.running_var"};
            static const char* const pl[2] = {"weight", "bias"};
            snprintf(buf, sizeof buf, "%s.%s", XF_LAYERS[l].name, XF_LAYERS[l].bn ? bn[i - t] : pl[i - t]);
            return buf;
        }
        t += n;
    }
    return nullptr;
}

// t: host pointers of the tensors in imcui_hip_xfeat_tensor_name order (shapes checked by the caller).  BatchNorm2d(affine=False) in
// eval mode is folded: w' = w / sqrt(var + eps), b' = -mean / sqrt(var + eps).
extern "C" int imcui_hip_xfeat_pack_weights(const float* const* t, float* packed) {
    if (!t || !packed) return IMCUI_ERR_ARG;
    const int nt = xf_num_tensors();
    for (int i = 0; i < nt; ++i)
        if (!t[i]) return IMCUI_ERR_ARG;
    const XfLayout l = xf_layout();
    memset(packed, 0, l.total * sizeof(float));
    memcpy(packed + l.skw, t[0], 24 * sizeof(float));
    memcpy(packed + l.skb, t[1], 24 * sizeof(float));
    for (int i = 0; i < XF_NL; ++i) {
        const XfLayer& L = XF_LAYERS[i];
        const int t0 = xf_tensor_of_layer(i), kk = L.k * L.k;
        const float* w = t[t0];  // OIHW
        std::vector<float> wf((size_t)L.cout * L.cin * kk), bf(L.cout);
        for (int co = 0; co < L.cout; ++co) {
            const double sd = L.bn ? sqrt((double)t[t0 + 2][co] + XF_BN_EPS) : 1.0;  // (double, rounded once: within 1 ulp of the float32 fold)
            bf[co] = L.bn ? (float)(-(double)t[t0 + 1][co] / sd) : t[t0 + 1][co];
            for (int j = 0; j < L.cin * kk; ++j) {
                const float v = w[(size_t)co * L.cin * kk + j];
                wf[(size_t)co * L.cin * kk + j] = L.bn ? (float)((double)v / sd) : v;
            }
        }
        if (!xf_is_gemm(i)) {  // [tap][cin][cout]
            for (int co = 0; co < L.cout; ++co)
                for (int ci = 0; ci < L.cin; ++ci)
                    for (int tap = 0; tap < kk; ++tap) packed[l.g[i].w + ((size_t)tap * L.cin + ci) * L.cout + co] = wf[((size_t)co * L.cin + ci) * kk + tap];
            memcpy(packed + l.g[i].b, bf.data(), L.cout * sizeof(float));
        } else {  // rows cout .. npad - 1 (the zero channels of the 24-channel maps) stay zero
            const int K = kk * L.cpad;
            pack_conv_gemm(wf.data(), L.cout, L.cin, L.k, L.cpad, packed + l.g[i].w);
            memcpy(packed + l.g[i].b, bf.data(), L.cout * sizeof(float));
            l.g[i].split_planes(packed, L.npad, K);
        }
    }
    return IMCUI_OK;
}

// ------------------------------------------------------------------ workspace
struct XfWs : XfTrunkBufs {
    float *k1h, *rel, *m1, *cfinal;
    CandScan scan;
    ScoreIndexList cand;
    int *npos, *crank, *status;
    size_t total;
    bool ok;
};

static XfWs xf_carve(void* ws, size_t bytes, int B, int Hr, int Wr) {
    WsAlloc a(ws, bytes);
    XfWs s;
    const size_t P = (size_t)B * Hr * Wr;
    s.XfTrunkBufs::carve(a, B, Hr, Wr);
    s.k1h = a.get<float>(P);
    s.rel = a.get<float>(P / 64);
    s.m1 = a.get<float>(P / 64 * 64);
    s.scan.carve(a, B, (size_t)Hr * Wr);
    s.npos = a.get<int>(B);
    s.cand.carve(a, B, Hr * Wr);  // a constant map is one plateau: every pixel can be a candidate
    s.cfinal = a.get<float>(P);
    s.crank = a.get<int>(P);
    s.status = a.get<int>(1);
    s.total = a.off;
    s.ok = a.ok;
    return s;
}

extern "C" size_t imcui_hip_xfeat_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H < 32 || W < 32) return 0;
    return xf_carve(nullptr, 0, B, H / 32 * 32, W / 32 * 32).total;
}

// NMS survivors whose scores do not tie exactly are more than 2 apart (Chebyshev)
extern "C" int imcui_hip_xfeat_max_keypoints_bound(int H, int W) {
    if (H < 32 || W < 32) return 0;
    return cdiv(H / 32 * 32, 3) * cdiv(W / 32 * 32, 3);
}

extern "C" int imcui_hip_xfeat_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, float threshold, int top_k,
                                       int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, float* kpt_heat,
                                       float* reliability, float* feats_norm, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (B <= 0) return IMCUI_OK;
    if (C != 1 && C != 3) return imcui_set_err(h, IMCUI_ERR_ARG, "xfeat: C=%d must be 1 or 3", C);
    if (H < 32 || W < 32 || (long)H * W > (1l << 30)) return imcui_set_err(h, IMCUI_ERR_ARG, "xfeat: H=%d W=%d must be at least 32", H, W);
    if (kcap <= 0 || !packed || !image || !keypoints || !scores || !descriptors || !num_keypoints)
        return imcui_set_err(h, IMCUI_ERR_ARG, "xfeat: null argument or kcap<=0");
    const int Hr = H / 32 * 32, Wr = W / 32 * 32;
    XfWs s = xf_carve(ws, ws_bytes, B, Hr, Wr);
    if (!ws || !s.ok) return imcui_set_err(h, IMCUI_ERR_WS, "xfeat: workspace too small (%zu < %zu)", ws_bytes, s.total);
    const XfLayout l = xf_layout();
    const float* P = packed;
    int rc;
    // ---- input stage
    const long np0 = (long)B * Hr * Wr;
    hipLaunchKernelGGL(xf_gray_kernel, dim3(blocks_256(np0)), dim3(256), 0, stream, image, s.gray, C, H, W, Hr, Wr, (float)H / (float)Hr, (float)W / (float)Wr,
                       np0);
    xf_stats(stream, s.gray, (long)Hr * Wr, B, s.part, s.norm);
    IMCUI_CHECK_LAUNCH(h);
    // ---- block1 .. block5, fusion (xf_shared.h), heads
    IMCUI_RUN(xf_trunk_feats(h, P, l, s, B, Hr, Wr, stream));
    const long np3 = (long)B * (Hr / 8) * (Wr / 8);
    IMCUI_RUN(xf_layer(h, P, l, 19, s.e3, 3, s.e1, 64, B, Hr, Wr, stream));
    IMCUI_RUN(xf_layer(h, P, l, 20, s.e1, 3, s.e2, 64, B, Hr, Wr, stream));
    float* m1 = feats_norm ? feats_norm : s.m1;
    float* rel = reliability ? reliability : s.rel;
    float* k1h = kpt_heat ? kpt_heat : s.k1h;
    hipLaunchKernelGGL(xf_heads_kernel, dim3((unsigned)((np3 + 3) / 4)), dim3(256), 0, stream, s.e3, s.e2, P + l.g[XF_L_HEAT].w, P + l.g[XF_L_HEAT].b, m1, rel,
                       np3);
    IMCUI_CHECK_LAUNCH(h);
    IMCUI_RUN(xf_trunk_kpts(h, P, l, s, B, Hr, Wr, k1h, stream));
    // ---- selection
    int* st = status ? status : s.status;
    hipMemsetAsync(st, 0, sizeof(int), stream);
    hipMemsetAsync(s.npos, 0, sizeof(int) * B, stream);
    const int ccap = s.cand.cap, *cidx = s.cand.cidx, *ncand = s.scan.total;
    cand_list(stream, k1h, Hr * Wr, B, XfKeep{Hr, Wr, threshold}, s.scan, ccap, s.cand.emit());
    const dim3 cgrid(cdiv(ccap, 256), B);
    hipLaunchKernelGGL(xf_score_kernel, cgrid, dim3(256), 0, stream, k1h, rel, cidx, ncand, ccap, Hr, Wr, s.cfinal, s.npos);
    hipLaunchKernelGGL(xf_rank_kernel, cgrid, dim3(256), 0, stream, s.cfinal, cidx, ncand, s.npos, ccap, top_k, kcap, Wr,
                       (float)((double)W / (double)Wr), (float)((double)H / (double)Hr), keypoints, scores, s.crank);
    hipLaunchKernelGGL(xf_finish_kernel, dim3(cdiv(kcap, 4), B), dim3(256), 0, stream, ncand, s.npos, ccap, top_k, kcap, keypoints, scores, descriptors,
                       num_keypoints, st);
    hipLaunchKernelGGL(xf_desc_kernel, dim3(min(cdiv(ccap, 4), 1024), B), dim3(256), 0, stream, m1, cidx, s.crank, ncand, ccap, kcap, Hr, Wr, descriptors);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}

// Test entry: the kernel's nearest / bilinear / bicubic sampling rules at n integer pixels (xy [n][2] int32 = x, y) of an H x W image
// (multiples of 8): kpt_heat [H, W], reliability [H/8, W/8], feats [H/8, W/8, 64] -> nearest [n], bilinear [n], bicubic [n, 64] (not
// normalised).  Device pointers.
extern "C" int imcui_hip_xfeat_sample_probe(imcui_hip_t* h, const float* kpt_heat, const float* reliability, const float* feats, int H, int W, const int* xy,
                                            int n, float* nearest, float* bilinear, float* bicubic, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return IMCUI_ERR_ARG;
    if (n <= 0) return IMCUI_OK;
    if (H < 8 || W < 8 || H % 8 || W % 8 || !kpt_heat || !reliability || !feats || !xy || !nearest || !bilinear || !bicubic)
        return imcui_set_err(h, IMCUI_ERR_ARG, "xfeat probe: H=%d W=%d must be multiples of 8 and no pointer null", H, W);
    hipLaunchKernelGGL(xf_probe_kernel, dim3(cdiv(n, 4)), dim3(256), 0, stream, kpt_heat, reliability, feats, H, W, xy, n, nearest, bilinear, bicubic);
    IMCUI_CHECK_LAUNCH(h);
    return IMCUI_OK;
}
