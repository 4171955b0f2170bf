/* libimcui_hip -- C ABI of the MI355X (gfx950) extract/match backend for imcui.
 *
 * Drop-in boundary.  The reference has no FFI for this path: its hot path
 * is the `_forward(data: dict) -> dict` of three `imcui.hloc` plugins, which delegate to
 * PyTorch modules.  Each entry point below replaces the arithmetic behind one of those calls
 * and is what a host-side binding (ctypes today) binds:
 *
 *   imcui_hip_superpoint_forward  <- imcui/hloc/extractors/superpoint.py:56-57  `self.net(data, self.conf)`
 *   imcui_hip_lightglue_forward   <- imcui/hloc/matchers/lightglue.py:54-75     `self.net(input)`
 *   imcui_hip_mutual_nn           <- imcui/hloc/matchers/nearest_neighbor.py:38-66 `_forward`
 *   imcui_hip_loftr_forward       <- imcui/hloc/matchers/loftr.py:54            `self.net(data_)`
 *   imcui_hip_dual_softmax        <- imcui/hloc/matchers/dual_softmax.py:62-75  `dual_softmax_matcher(...)`
 *   imcui_hip_superglue_forward   <- imcui/hloc/matchers/superglue.py:42-43     `self.net(data)`
 *   imcui_hip_imp_forward         <- imcui/hloc/matchers/imp.py:51              `self.net.produce_matches(data, p=0.2)`
 *   imcui_hip_adalam_forward      <- imcui/hloc/matchers/adalam.py:46-57        `self.adalam.match_and_filter(...)`
 *   *_pack_weights                <- the `_init` weight loading (superpoint.py:48-53, lightglue.py:39-51)
 *
 * Conventions
 *   - every pointer marked [dev] is a device pointer owned by the caller (PyTorch-ROCm tensor
 *     storage); the library never allocates or frees caller-visible memory.  Scratch comes from
 *     a caller-provided workspace sized by the matching *_workspace_bytes() query.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *     All work is enqueued on it; calls return without synchronising unless stated.
 *   - return value: 0 = ok, < 0 = error (IMCUI_HIP_ERR_*); imcui_hip_last_error(h) has the text.
 *     No exceptions cross the boundary.  The library is re-entrant per (handle, stream) and
 *     holds no global mutable state.
 *   - all tensors are float32 / int32, C-contiguous, batch-major.
 */
#ifndef IMCUI_HIP_H
#define IMCUI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMCUI_HIP_OK 0
#define IMCUI_HIP_ERR_ARG -1         /* bad argument */
#define IMCUI_HIP_ERR_WS -2          /* workspace missing / too small */
#define IMCUI_HIP_ERR_HIP -3         /* HIP runtime error */
#define IMCUI_HIP_ERR_UNSUPPORTED -4 /* configuration outside what the kernels support */

typedef struct imcui_hip_s imcui_hip_t;

/* ---- handle ------------------------------------------------------------------------- */
int imcui_hip_create(int device, imcui_hip_t** out);
void imcui_hip_destroy(imcui_hip_t* h);
const char* imcui_hip_last_error(const imcui_hip_t* h);
/* 400 since round 4: imcui_hip_dust3r_forward[_sizes] take the size of the packed buffer (a blob of another layout is rejected),
 * the packed DUSt3R buffer ends in a format trailer, imcui_hip_set_option / _get_option exist.  (100: rounds 1-3.) */
int imcui_hip_version(void);

/* A/B switches of the kernel routing (profiling and the bitwise old-vs-new kernel tests).  The IMCUI_<NAME> environment variables
 * are read ONCE, by imcui_hip_create; afterwards a switch changes only through this call -- set it BETWEEN forward passes, never while
 * another thread runs a call on the same handle.  Names / values: "gemm_wreg" 0 | 1 | 2 (default 2: every eligible projection on
 * the weights-in-registers GEMM), "wreg_pipe" 0 | 1 (default 1), "attn_variant" 8 (default: three f16 products in both contractions; the retired schedules 0 .. 3 and 5 map onto it) | 7 (the two-product P.V; 6 maps
 * onto it; NOT fp32-grade on its own) | 9 (round 6, opt-in: P.V corrections on the block-scaled fp6 matrix instruction, csrc/attention_mx.hip; callers without the
 * fp6 scratch -- SuperGlue, DUSt3R -- fall back to 8), "attn_split" 0 | 1 | 2 (key-split attention launches, csrc/attention.hip: 0 never, 1 = default: when the grid
 * has fewer than two workgroups per CU -- one pair per call --, 2 whenever the caller gave scratch; the geometries are bitwise equal),
 * "attn_variant_self" / "attn_variant_cross" (-1 = attn_variant; else the variant of LightGlue's self / cross blocks in the layers whose bit is set in
 * "attn_mix_layers", default 0x1ff.  Default cross = -2: variant 7 -- the two-product P.V in the CROSS blocks only, audited per block: layer error <= 7.1e-6 and
 * score error <= 4.7e-5 at N = M = 2048 on three weight sets, half the parity bar -- WHILE "attn_variant" is left at 8; an explicit "attn_variant" governs every
 * block; -1 restores three products everywhere), "simred"
 * 1 | 0 (default 1: the mutual-NN matcher on the persistent similarity-and-reduce kernel; 0: the round-4 tile GEMM with the reducing
 * epilogue, kept for A/B and for descriptor widths other than 64 / 128 / 256), "ffn_tile" / "wreg_tile" 0 | 128 | 64 | 32 (tokens per workgroup of the
 * fused FFN / of the weights-in-registers projection GEMM; default 0 = by token count, the largest tile that still gives every CU a workgroup; bitwise equal results), "conv_tall"
 * 0 | 1 | 2 and "conv_narrow" 0 | 1 | 2 (convolution tile shapes; conv_narrow 0 = 64-channel tiles where 128-channel tiles would give fewer than 256
 * workgroups, 1 = always, 2 = never).  Unknown name: IMCUI_HIP_ERR_ARG. */
int imcui_hip_set_option(imcui_hip_t* h, const char* name, int value);
int imcui_hip_get_option(imcui_hip_t* h, const char* name, int* value);

/* Arithmetic mode of the matrix-core kernels (default 1):
 *   0  exact f32: v_mfma_f32_32x32x2_f32, bitwise an fmaf chain
 *   1  3 x f16 split: every f32 operand is split into f16 (hi, lo) and a product is evaluated as
 *      ah*bh + ah*bl + al*bh on v_mfma_f32_32x32x16_f16 with f32 accumulation (~fp32 accuracy,
 *      ~5x the f32 matrix rate).  Attention then consumes V transposed (internal detail).
 * For imcui_hip_attention_f32 in mode 1 the caller passes pre-split operands: each of Q, K
 * [S][heads][rows][64] and V^T [S][heads][64][rows] as two f16 planes (hi, then lo). */
int imcui_hip_set_precision(imcui_hip_t* h, int mode);
int imcui_hip_get_precision(const imcui_hip_t* h);

/* Optional HIP-event timing of the three heavy kernel classes on the launch stream
 * (0 = attention, 1 = conv3x3, 2 = gemm): enable, run, then read (synchronises the events;
 * returns the summed kernel time in ms and the number of launches, and resets the counters). */
int imcui_hip_profile_enable(imcui_hip_t* h, int on);
int imcui_hip_profile_read(imcui_hip_t* h, int kernel_class, double* total_ms, int* count);

/* ---- SuperPoint --------------------------------------------- */
/* Weight packing runs on the HOST: `w[i]`, `b[i]` are the 12 conv weights (OIHW) / biases in the
 * order conv1a conv1b conv2a conv2b conv3a conv3b conv4a conv4b convPa convPb convDa convDb
 * (upstream state-dict keys `<name>.weight` / `<name>.bias`); `packed` receives
 * imcui_hip_superpoint_packed_floats() floats which the caller uploads once. */
size_t imcui_hip_superpoint_packed_floats(void);
int imcui_hip_superpoint_pack_weights(const float* const* w, const float* const* b, float* packed);

size_t imcui_hip_superpoint_workspace_bytes(int B, int H, int W, int nms_radius);
/* Key-points a non-degenerate HxW image can yield after NMS (sizes `kcap` when max_keypoints < 0). */
int imcui_hip_superpoint_max_keypoints_bound(int H, int W, int nms_radius);

/* image [dev, B,1,H,W] in [0,1]; H, W multiples of 8.  Runtime conf (read per call, like the
 * reference re-reads self.conf): nms_radius (0..4), keypoint_threshold, remove_borders,
 * max_keypoints (-1 = all), fix_sampling (imcui/hloc/extractors/superpoint.py:16-30).
 * Outputs, fixed stride `kcap` per image, first num_keypoints[b] entries valid:
 *   keypoints   [dev, B,kcap,2]   (x, y) float pixel coordinates
 *   scores      [dev, B,kcap]
 *   descriptors [dev, B,kcap,256] row per key-point (the reference's [256,N] is its transpose view)
 *   num_keypoints [dev, B] int32
 *   status      [dev, 1] int32 optional (may be NULL): selection status word of this call, 0 = fine, bit 1 = `kcap`
 *               too small (only possible with max_keypoints = -1 and exactly tied scores; the first kcap are
 *               returned), bit 0 = candidate overflow.  Reading it is the caller's business (no sync here).
 *   score_map   [dev, B,H,W] optional (may be NULL): dense pre-NMS detector scores
 * max_keypoints above 16384 (the on-chip sorter; the UI slider ends at 10000) is rejected with
 * IMCUI_HIP_ERR_UNSUPPORTED before anything is launched; -1 (all) has no such limit.
 * Order: score-descending (ties: lower flat index first) when top-k applies, row-major otherwise. */
int imcui_hip_superpoint_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W,
                                 int nms_radius, float keypoint_threshold, int remove_borders, int max_keypoints,
                                 int fix_sampling, int kcap, float* keypoints, float* scores, float* descriptors,
                                 int* num_keypoints, int* status, float* score_map, void* ws, size_t ws_bytes, void* stream);
/* Synchronises `stream` and reports selection overflow of the last forward on `ws`
 * (IMCUI_HIP_ERR_UNSUPPORTED + message) -- e.g. kcap too small for a max_keypoints = -1 call. */
int imcui_hip_superpoint_status(imcui_hip_t* h, int B, int H, int W, int nms_radius, void* ws, size_t ws_bytes,
                                void* stream);
/* upstream `simple_nms` alone: scores/out [dev, B,H,W] */
int imcui_hip_simple_nms(imcui_hip_t* h, const float* scores, float* out, int B, int H, int W, int nms_radius,
                         void* stream);

/* ---- DISK (zoo entries disk, disk+lightglue, disk+dualsoftmax; imcui/hloc/extractors/disk.py:18-36) ------------------ */
/* Weight packing runs on the HOST (imcui/hloc/extractors/disk.py:18-36 -> kornia DISK.from_pretrained): tensor i is the kornia
 * state-dict entry named imcui_hip_disk_tensor_name(i) (unet.path_down.*, unet.path_up.*: 26 tensors); `packed` receives
 * imcui_hip_disk_packed_floats() floats which the caller uploads once. */
size_t imcui_hip_disk_packed_floats(void);
int imcui_hip_disk_num_tensors(void);
const char* imcui_hip_disk_tensor_name(int i);
int imcui_hip_disk_pack_weights(const float* const* tensors, float* packed);
/* Scratch of imcui_hip_disk_forward for B images of H x W (independent of the window, the threshold and kcap). */
size_t imcui_hip_disk_workspace_bytes(int B, int H, int W);
/* Exact bound on the key-points of an H x W image: NMS survivors are pairwise >= window / 2 + 1 apart (Chebyshev). */
int imcui_hip_disk_max_keypoints_bound(int H, int W, int window);
/* imcui/hloc/extractors/disk.py:18-36 `self.model(image, n=max_keypoints, window_size=nms_window_size,
 * score_threshold=detection_threshold, pad_if_not_divisible=...)`.
 * image [dev, B,3,H,W] RGB in [0,1].  pad_if_not_divisible: zero-pad right / bottom to multiples of 16 (else H, W must be
 * multiples of 16); window: odd NMS window; threshold: strict; max_keypoints -1 = None.
 * Outputs, fixed stride `kcap` per image, first num_keypoints[b] entries valid, the rest zero:
 *   keypoints [dev, B,kcap,2] (x, y) integer pixels as float, ROW-MAJOR order (not sorted by score)
 *   scores [dev, B,kcap] raw heatmap values;  descriptors [dev, B,kcap,128] L2-normalised rows;  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: 0 = fine, bit 1 = more key-points than kcap (the first kcap are returned)
 *   heatmap [dev, B,H,W] optional: the dense detection logits (cropped)
 * One intended divergence: zero candidates give zero key-points (kornia raises inside kthvalue).  No host synchronisation. */
int imcui_hip_disk_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, int pad_if_not_divisible, int window,
                           float threshold, int max_keypoints, int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints,
                           int* status, float* heatmap, void* ws, size_t ws_bytes, void* stream);

/* ---- ALIKED (zoo entry aliked+lightglue; imcui/hloc/extractors/aliked.py:24-32 -> LightGlue's ALIKED.forward) -------- */
/* aliked-n16 / aliked-n16rot: (c1,c2,c3,c4,dim,K,M) = (16,32,64,128,128,3,16).  Weight packing runs on the HOST (replaces the
 * `ALIKED(**conf)` construction and `load_state_dict` of imcui/hloc/extractors/aliked.py:19-22): tensor i is the upstream state-dict
 * entry named imcui_hip_aliked_tensor_name(i), in upstream's order without the `num_batches_tracked` counters; BatchNorm (eval) is
 * folded into the convolution before it.  `packed` receives imcui_hip_aliked_packed_floats() floats; it begins with block1.conv1
 * folded with block1.bn1 as [9 taps][3][16] floats followed (from float 448) by the 16 folded biases. */
size_t imcui_hip_aliked_packed_floats(void);
int imcui_hip_aliked_num_tensors(void);
const char* imcui_hip_aliked_tensor_name(int i);
int imcui_hip_aliked_pack_weights(const float* const* tensors, float* packed);
/* Scratch of imcui_hip_aliked_forward for B images of H x W (independent of the radius, the threshold and kcap): less than ONE dense
 * 128-channel map of the padded images, B * Hp * Wp * 128 * 4 bytes. */
size_t imcui_hip_aliked_workspace_bytes(int B, int H, int W);
/* Bound on the key-points of an H x W image whose scores do not tie exactly: simple_nms survivors are more than nms_radius apart. */
int imcui_hip_aliked_max_keypoints_bound(int H, int W, int nms_radius);
/* imcui/hloc/extractors/aliked.py:24-32 `self.model(data)`: InputPadder (replicate, multiples of 32), encoder, score head, DKD, SDDH.
 * image [dev, B,3,H,W] RGB in [0,1], H, W >= 32.  nms_radius 1..4.  threshold > 0: candidates are nms > threshold, or nms > mean(score
 * map) when an image has none (decided per image); more than n_limit (max_keypoints if > 0, else 20000): the n_limit highest scores
 * stay, ties to the lower flat index.  threshold <= 0 and max_keypoints > 0: the max_keypoints highest positive NMS scores.
 * threshold <= 0 and max_keypoints <= 0: nms > mean.
 * Outputs, fixed stride `kcap` per image, first num_keypoints[b] entries valid, the rest zero, ROW-MAJOR order of the integer
 * candidate (not sorted by score):
 *   keypoints [dev, B,kcap,2] (x, y) refined, in pixels;  scores [dev, B,kcap] score map sampled there
 *   descriptors [dev, B,kcap,128] L2-normalised rows;  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: 0 = fine, bit 1 = more key-points than kcap (the first kcap are returned)
 *   score_map [dev, B,H,W] optional;  keypoints_norm [dev, B,kcap,2] optional: the key-points in [-1, 1] as DKD hands them to SDDH
 *   dbg_x3 [dev, B,Hp/8,Wp/8,64], dbg_x4 [dev, B,Hp/32,Wp/32,128] optional: outputs of the two deformable blocks (NHWC, padded size)
 * The descriptor head runs in two launches per batch whatever kcap is; while it runs, floats 0..31 of a key-point's descriptor row hold
 * its sample offsets.  No host synchronisation. */
int imcui_hip_aliked_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, int nms_radius, float threshold,
                             int max_keypoints, int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status,
                             float* score_map, float* keypoints_norm, float* dbg_x3, float* dbg_x4, void* ws, size_t ws_bytes, void* stream);

/* ---- ALIKE (zoo entry alike = `feature: alike` + NN-mutual; imcui/hloc/extractors/alike.py) ------------------------------- */
/* variant: 0 alike-t (c1..c4, dim = 8,16,32,64, 64), 1 alike-s (8,16,48,96, 96), 2 alike-n (16,32,64,128, 128); DKD radius 2.  alike-l
 * (a second head layer behind a ReLU) is not served: every entry refuses other values (0 / NULL / IMCUI_ERR_UNSUPPORTED).
 * Weight packing runs on the HOST (replaces the `ALike(**configs[...])` construction of alike.py:31-45): tensor i is the state-dict
 * entry named imcui_hip_alike_tensor_name(variant, i) (block{1..4}.conv{1,2}.weight, .bn{1,2}.{weight,bias,running_mean,running_var},
 * block{2..4}.downsample.{weight,bias}, conv{1..4}.weight, convhead2.weight; no `num_batches_tracked` counters); BatchNorm (eval,
 * eps 1e-5) is folded into the convolution before it.  `packed` receives imcui_hip_alike_packed_floats(variant) floats; it begins with
 * block1.conv1 folded with block1.bn1 as [9 taps][3][c1] floats followed (from the next multiple of 64 floats) by the c1 folded biases. */
size_t imcui_hip_alike_packed_floats(int variant);
int imcui_hip_alike_num_tensors(int variant);
const char* imcui_hip_alike_tensor_name(int variant, int i);
int imcui_hip_alike_pack_weights(int variant, const float* const* tensors, float* packed);
/* Scratch of imcui_hip_alike_forward for B images of H x W (independent of the selection arguments and kcap). */
size_t imcui_hip_alike_workspace_bytes(int variant, int B, int H, int W);
/* Bound on the key-points of an H x W image whose scores do not tie exactly: simple_nms survivors are more than 2 pixels apart. */
int imcui_hip_alike_max_keypoints_bound(int H, int W);
/* alike.py:47-61 `self.net(image, sub_pixel)`: image [dev, B,3,H,W] RGB in [0,1], H, W >= 32, read as (x * 255) / 255 in float32 (the
 * wrapper's and upstream's scaling), zero-padded at the bottom and right to multiples of 32; encoder, head, DKD (radius 2):
 * simple_nms, rows / columns [0, 2] and the last 2 zeroed; top_k > 0: the top_k highest positive NMS scores in descending order; else
 * threshold > 0: nms > threshold, or nms > mean(score map) when an image has none (per image); else nms > mean; survivors in row-major
 * order; more than n_limit (> 0) of them: the n_limit highest scores, then in DESCENDING score order.  Ties go to the lower flat index.
 * sub_pixel == 0: n = idx / (W - 1, H - 1) * 2 - 1 in float32, score = bilinear sample of the score map at n, descriptor = the head at
 * pixel trunc((n + 1) / 2 * (W - 1, H - 1)) (upstream's round trip: sometimes the pixel before), key-point = (n + 1) / 2 * (W - 1, H - 1).
 * sub_pixel != 0: n from the soft-argmax (temperature 0.1, 5x5 patch of the raw score map), descriptor = bilinear sample of the
 * normalised descriptor map at n.  Descriptors are normalised again.
 * Outputs, fixed stride `kcap` per image, first num_keypoints[b] entries valid, the rest zero:
 *   keypoints [dev, B,kcap,2] (x, y) in pixels;  scores [dev, B,kcap];  descriptors [dev, B,kcap,dim];  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: 0 = fine, bit 1 = more key-points than kcap (the first kcap of the output order are returned)
 *   score_map [dev, B,H,W] optional;  dbg_x4 [dev, B,Hp/32,Wp/32,c4 stored as a multiple of 32] optional: block 4's output (NHWC);
 *   dbg_f2 / dbg_f3 / dbg_f4 [dev, B,Hp/2^s,Wp/2^s,dim/4] (s = 1, 3, 5) optional: the branch maps ReLU(conv_i x_i) before up-sampling
 * Zero key-points is a valid result.  No host synchronisation. */
int imcui_hip_alike_forward(imcui_hip_t* h, int variant, const float* packed, const float* image, int B, int H, int W, float threshold, int top_k,
                            int n_limit, int sub_pixel, int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints,
                            int* status, float* score_map, float* dbg_x4, float* dbg_f2, float* dbg_f3, float* dbg_f4, void* ws, size_t ws_bytes,
                            void* stream);
/* Test entry: the sparse descriptor head at n integer pixels xy [dev, n,2] int32 (x, y) of ONE image [dev, 3,H,W] -> descriptors
 * [dev, n,dim] = F.normalize(descriptor_map)[:, y, x].  ws: imcui_hip_alike_workspace_bytes(variant, 1, H, W). */
int imcui_hip_alike_desc_probe(imcui_hip_t* h, int variant, const float* packed, const float* image, int H, int W, const int* xy, int n,
                               float* descriptors, void* ws, size_t ws_bytes, void* stream);

/* ---- R2D2 (zoo entry r2d2: `feature: r2d2` + NN-mutual; imcui/hloc/extractors/r2d2.py) ----------------------------------- */
/* Packed weights of naver/r2d2's Quad_L2Net_ConfCFS (r2d2_WASF_N16 / r2d2_WASF_N8 / r2d2_WAF_N16 share it; replaces `load_network`,
 * r2d2.py:41): tensors in imcui_hip_r2d2_tensor_name order (`ops.N.weight` / `.bias`, the running statistics of the affine-free
 * BatchNorms `ops.N+1`, `clf`, `sal`); BatchNorm (eval, eps 1e-5) is folded into the convolution before it in float32.  The network is
 * restated from its description (tests/r2d2_reference.py): parity with upstream's code is NOT pinned. */
size_t imcui_hip_r2d2_packed_floats(void);
int imcui_hip_r2d2_num_tensors(void);
const char* imcui_hip_r2d2_tensor_name(int i);
int imcui_hip_r2d2_pack_weights(const float* const* tensors, float* packed);
/* Scratch of imcui_hip_r2d2_forward for B images and the level list (nh, nw) [host, nlev] with room for kcap candidates per image (the
 * feature maps are sized for the largest level, the parked candidate vectors are 512 bytes each). */
size_t imcui_hip_r2d2_workspace_bytes(int B, int nlev, const int* nh, const int* nw, int kcap);
/* r2d2.py:49-73 `_forward` (norm_rgb, extract_multiscale with NonMaxSuppression, the argsort cut): image [dev, B,3,H,W] RGB in [0,1].
 * Levels [host, nlev]: level 0 = (H, W), level l + 1 = ATen bilinear (align_corners=False) of level l to (nh, nw)[l + 1]; the network
 * and the detector run on the levels with run[l] != 0.  The BINDING evaluates upstream's float64 schedule (s /= scale_factor, round);
 * nlev <= 32, every level inside the image (upstream asserts max_scale <= 1).  Per level: (x - mean) / std, nine convolutions (3x3 and
 * 2x2, dilations 1 .. 16, every map nh x nw), reliability = softmax(clf(x^2))[1], repeatability = softplus(sal(x^2)) / (1 + softplus),
 * candidates = (rep == 3x3 max) & (rep >= rep_thr) & (rel >= rel_thr) in row-major order, key-point = ((x * W) / nw, (y * H) / nh) in
 * float32, score = rel * rep, descriptor = F.normalize of the 128-vector at the pixel.  Candidates are concatenated level-major; more
 * than max_keypoints (> 0; 0 = all): the highest scores stay, among equal scores the later candidates; output in ASCENDING (score,
 * candidate) order, i.e. scores.argsort(stable)[-max_keypoints:].
 * kcap = room for candidates per image (<= the pixels of the running levels); kout = rows per image of the outputs = kcap when
 * max_keypoints == 0, else min(max_keypoints, kcap).  Outputs, first num_keypoints[b] rows valid, the rest zero:
 *   keypoints [dev, B,kout,2] (x, y);  scores [dev, B,kout];  descriptors [dev, B,kout,128];  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: 0 = fine, bit 1 = an image had more candidates than kcap (a flat map: every pixel of a plateau is
 *   a 3x3 maximum); the result is then that of the first kcap candidates
 *   dbg_rel / dbg_rep optional: [dev] the maps of the running levels one after another, each [B, nh, nw]; dbg_map likewise, the final
 *   128-channel map [B, nh, nw, 128]
 * Zero key-points is a valid result.  No host synchronisation. */
int imcui_hip_r2d2_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, int nlev, const int* nh, const int* nw,
                           const int* run, float rel_thr, float rep_thr, int max_keypoints, int kcap, int kout, float* keypoints, float* scores,
                           float* descriptors, int* num_keypoints, int* status, float* dbg_rel, float* dbg_rep, float* dbg_map, void* ws,
                           size_t ws_bytes, void* stream);
/* Test entry: the network on ONE image [dev, 3,H,W] at full resolution and F.normalize of its final map at n integer pixels xy
 * [dev, n,2] int32 (x, y) -> descriptors [dev, n,128] (what the emit stage computes from a parked vector; extract.py: `descriptors[0, :, y,
 * x]`).  ws: imcui_hip_r2d2_workspace_bytes(1, 1, &H, &W, 1). */
int imcui_hip_r2d2_desc_probe(imcui_hip_t* h, const float* packed, const float* image, int H, int W, const int* xy, int n, float* descriptors,
                              void* ws, size_t ws_bytes, void* stream);

/* ---- D2-Net / RoRD (zoo entries d2net, rord: `feature: d2net-ss` / `rord` + NN-mutual; imcui/hloc/extractors/d2net.py, rord.py) ---- */
/* Packed weights of mihaidusmanu/d2-net's DenseFeatureExtractionModule (VGG-16 cut at conv4_3; replaces `_D2Net(model_file=...)`,
 * d2net.py:32-34): tensors in imcui_hip_d2net_tensor_name order (`dense_feature_extraction.model.N.weight` / `.bias`, N = 0, 2, 5, 7, 10,
 * 12, 14, 17, 19, 21).  The network, detector and pyramid are restated from their description (tests/d2net_reference.py): parity with
 * upstream's code is NOT pinned; RoRD's lib/model_test.py is taken to be D2-Net's. */
size_t imcui_hip_d2net_packed_floats(void);
int imcui_hip_d2net_num_tensors(void);
const char* imcui_hip_d2net_tensor_name(int i);
int imcui_hip_d2net_pack_weights(const float* const* tensors, float* packed);
/* Scratch of imcui_hip_d2net_forward for B images and the level list (lh, lw) [host, nlev] (IMAGE sizes of the levels) with room for kcap
 * candidates per image; every level's 512-channel map stays in it until the descriptors are gathered. */
size_t imcui_hip_d2net_workspace_bytes(int B, int nlev, const int* lh, const int* lw, int kcap);
/* d2net.py:37-60 `_forward` (flip to BGR, x * 255 - mean, process_multiscale, the column swap, the argsort cut): image [dev, B,3,H,W] RGB
 * in [0,1].  Levels [host, nlev <= 8]: the image sizes floor(H s) x floor(W s) in list order, evaluated by the BINDING in float64 (a
 * level equal to (H, W) is the image itself, any other ATen's bilinear resize with align_corners=True of the normalised image).  Per
 * level: the trunk -> f [h, w, 512] with (h, w) = (lh / 4 - 1, lw / 4 - 1), every one at least 1 or the call is refused; f += bilinear
 * (align_corners=True) of the previous level's f; HardDetectionModule (channel-wise maximum, 3x3 maximum, edge test 7.2, det > 0)
 * minus the pixels banned by earlier levels (nearest), HandcraftedLocalizationModule's step with |step| < 0.5, the four bilinear corners
 * inside the map; candidates in (level, channel, row, column) order; key-point = ((p * 2 + 0.5) * 2 + 0.5) * (H / lh, W / lw) in
 * float32, returned as (x, y); score = f[c, i, j] / (level index + 1); descriptor = F.normalize of the bilinear 512-vector at p.  More
 * than max_keypoints (> 0; 0 = all): the highest scores stay, among equal scores the later candidates; output in ASCENDING (score,
 * candidate) order, i.e. a STABLE argsort of upstream's concatenation (upstream's numpy argsort leaves ties open).
 * use_relu: F.relu after conv4_3.  kcap = room for candidates per image; kout = rows per image of the outputs = kcap when
 * max_keypoints == 0, else min(max_keypoints, kcap).  Outputs, first num_keypoints[b] rows valid, the rest zero:
 *   keypoints [dev, B,kout,2] (x, y);  scores [dev, B,kout];  descriptors [dev, B,kout,512];  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: 0 = fine, bit 1 = an image had more candidates than kcap (channels tied for the maximum); the
 *   result is then that of the first kcap candidates
 *   dbg_feat optional: [dev] the levels' maps after the sum, one after another, each [B, h, w, 512]
 * Zero key-points is a valid result.  No host synchronisation. */
int imcui_hip_d2net_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, int nlev, const int* lh, const int* lw,
                            int use_relu, int max_keypoints, int kcap, int kout, float* keypoints, float* scores, float* descriptors,
                            int* num_keypoints, int* status, float* dbg_feat, void* ws, size_t ws_bytes, void* stream);
/* Test entry: detector, localization, candidate list, cut and descriptors (lib/model_test.py HardDetectionModule,
 * HandcraftedLocalizationModule; lib/pyramid.py from `detections` on) on maps GIVEN by the caller, feat [dev, B,fh,fw,C] with C a
 * multiple of 64 up to 512, as one level that is its own image (factors 1): descriptors [dev, B,kout,C], the rest as above. */
/* Test entry: one small kernel of the trunk alone (the matrix layers have imcui_hip_conv_probe / imcui_hip_gemm_probe_f32).  op 0: layer 0
 * with d2net.py:39-41 applied as the image is read, in = image [dev, B,3,H,W] -> out [dev, B,H,W,64] (model.0 + ReLU); op 1: model.4 / .9
 * nn.MaxPool2d(2, 2), flooring, in [dev, B,H,W,C] -> out [dev, B,H/2,W/2,C]; op 2: model.16 nn.AvgPool2d(2, stride=1) -> [dev, B,H-1,W-1,C]. */
int imcui_hip_d2net_layer_probe(imcui_hip_t* h, int op, const float* packed, const float* in, int B, int H, int W, int C, float* out, void* stream);
size_t imcui_hip_d2net_probe_workspace_bytes(int B, int fh, int fw, int C, int kcap);
int imcui_hip_d2net_detect_probe(imcui_hip_t* h, const float* feat, int B, int fh, int fw, int C, int max_keypoints, int kcap, int kout,
                                 float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, void* ws, size_t ws_bytes,
                                 void* stream);

/* ---- LANet (zoo entry lanet: `feature: lanet` + NN-mutual; imcui/hloc/extractors/lanet.py) ------------------------------ */
/* lanet.network_v0.model.PointModel(is_test=True) (replaces lanet.py:34-36) is not part of the reference checkout: the network is
 * restated from its description (tests/lanet_reference.py) and parity with upstream's code is NOT pinned.  What the
 * checkpoint decides is READ from it by the binding and handed over as cfg [host, 12 ints]:
 *   c1, c2, c3, c4 (multiples of 32; c4 = 256), k of des_conv2 and of des_conv3 (1 or 3), bias present on des_conv2 / des_conv3,
 *   BatchNorm present behind des_conv2 / des_conv3, activation (1 ReLU, 2 LeakyReLU(0.01)), bias on the convolutions in front of a
 *   BatchNorm.
 * The packed buffer starts with a 64-float header: magic, the 12 values, Normalize's mean (0.5) and std (0.225).  Tensors in
 * imcui_hip_lanet_tensor_name order, under this library's own names (conv1a .. conv4b / bn1a .. bn4b, convDa / bnDa / convDb: the score
 * head, convPa / bnPa / convPb: the location head, des_conv2 / des_bn2, des_conv3 / des_bn3); the plugin maps a checkpoint's keys. */
size_t imcui_hip_lanet_packed_floats(const int* cfg);
int imcui_hip_lanet_num_tensors(const int* cfg);
const char* imcui_hip_lanet_tensor_name(const int* cfg, int i);
int imcui_hip_lanet_pack_weights(const int* cfg, const float* const* tensors, float* packed);
/* Scratch of imcui_hip_lanet_forward: B images of H x W (H, W >= 8), kout output rows per image. */
size_t imcui_hip_lanet_workspace_bytes(const int* cfg, int B, int H, int W, int kout);
/* lanet.py:39-63 `_forward` around `self.net(image)`: image [dev, B,3,H,W] RGB in [0,1].  Cells of 8 x 8 pixels, Hc x Wc = H/8 x W/8 in
 * row-major order; per cell score = sigmoid (0 on the first / last row and column), position = (c * 8 + 3.5) + tanh * 7.0 clamped to
 * the image, level weights = soft-max of three channels.  A cell is kept when score > threshold (:49-50, strict); more than
 * max_keypoints (> 0; 0 = all, :54 `or None`; negative refused): the highest scores stay, among equal scores the later cells; output
 * in ASCENDING (score, cell) order, a STABLE form of :54's argsort (torch.argsort leaves ties open).  descriptor = the three levels
 * des_conv2(x2), des_conv3(x3), x4 sampled bilinearly at the key-point (F.grid_sample defaults), weighted, divided by the norm -- the two
 * level convolutions are evaluated at the key-points only.  kout >= min(max_keypoints or all cells, Hc Wc).  Outputs, first
 * num_keypoints[b] rows valid, the rest zero:
 *   keypoints [dev, B,kout,2] (x, y);  scores [dev, B,kout];  descriptors [dev, B,kout,256];  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: always 0 (the candidate list holds every cell)
 *   optional debug outputs: dbg_x2 [B,H/2,W/2,c2], dbg_x3 [B,H/4,W/4,c3], dbg_x4 [B,Hc,Wc,256], dbg_score [B,Hc Wc], dbg_coord and
 *   dbg_tanh [B,Hc Wc,2], dbg_aware [B,Hc Wc,3]
 * Zero key-points is a valid result.  No host synchronisation; a row's bits do not depend on the batch. */
int imcui_hip_lanet_forward(imcui_hip_t* h, const int* cfg, const float* packed, const float* image, int B, int H, int W, float threshold,
                            int max_keypoints, int kout, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status,
                            float* dbg_x2, float* dbg_x3, float* dbg_x4, float* dbg_score, float* dbg_coord, float* dbg_aware, float* dbg_tanh,
                            void* ws, size_t ws_bytes, void* stream);
/* Test entries.  stem_probe: conv1a with the normalisation, image [dev, B,3,H,W] -> out [dev, B,H,W,c1]; scratch [dev, B,H,W,32] is
 * needed when the layer runs on the GEMM (LeakyReLU, or c1 other than 32 / 64).  tail_probe: the two tails and the decode on given
 * hidden maps s1, p1 [dev, B,Hc,Wc,256].  select_probe: decode and selection from given head outputs raw [dev, B,Hc Wc,6] (score head
 * 0..3, location head 4..5); ws: imcui_hip_lanet_select_workspace_bytes.  desc_probe: the sparse descriptor head of ONE image at n
 * given positions coords [dev, n,2] (pixels of the H x W image) and level weights aw [dev, n,3] from given maps -> [dev, n,256].
 * dense_levels: des_conv2(x2) -> d2 [dev, B,h2,w2,256] and des_conv3(x3) -> d3 on the shared GEMM, the form the forward never runs. */
int imcui_hip_lanet_stem_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* image, int B, int H, int W, float* out, float* scratch,
                               void* stream);
int imcui_hip_lanet_tail_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* s1, const float* p1, int B, int Hc, int Wc, int H, int W,
                               float* score, float* coord, float* tanhv, float* aware, void* stream);
size_t imcui_hip_lanet_select_workspace_bytes(int B, int Hc, int Wc, int kout);
int imcui_hip_lanet_select_probe(imcui_hip_t* h, const float* raw, int B, int Hc, int Wc, int H, int W, float threshold, int max_keypoints, int kout,
                                 float* keypoints, float* scores, int* num_keypoints, int* status, float* dbg_score, float* dbg_coord, float* dbg_aware,
                                 float* dbg_tanh, void* ws, size_t ws_bytes, void* stream);
int imcui_hip_lanet_desc_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* x2, int h2, int w2, const float* x3, int h3, int w3,
                               const float* x4, int h4, int w4, int H, int W, const float* coords, const float* aw, int n, float* descriptors, void* stream);
int imcui_hip_lanet_dense_levels(imcui_hip_t* h, const int* cfg, const float* packed, const float* x2, int B, int h2, int w2, const float* x3, int h3, int w3,
                                 float* d2, float* d3, void* stream);

/* ---- DarkFeat (zoo entry darkfeat: `feature: darkfeat` + NN-mutual; imcui/hloc/extractors/darkfeat.py) -------------------- */
/* darkfeat.DarkFeat(model_path) (replaces darkfeat.py:28) is not part of the reference checkout (third_party/DarkFeat is an empty
 * submodule): the network is restated from its description (tests/darkfeat_reference.py) and parity with upstream's code is NOT pinned
 * ("DarkFeat: what is pinned").  The backbone is ONE table in csrc/darkfeat.hip (DF_LAYERS), readable through
 * imcui_hip_darkfeat_layer: name, and out5 = cin, cout, stride, InstanceNorm + ReLU behind it, score level its RAW output feeds (-1 none).
 * Tensors in imcui_hip_darkfeat_tensor_name order: `<layer>.0.weight` [cout,cin,3,3], `<layer>.0.bias` [cout] (zeros when the checkpoint
 * has none), clf.weight [2,128,1,1], clf.bias [2], moving_avg_params.0..2 [1]. */
int imcui_hip_darkfeat_num_layers(void);
const char* imcui_hip_darkfeat_layer(int i, int* out5);
int imcui_hip_darkfeat_num_tensors(void);
const char* imcui_hip_darkfeat_tensor_name(int i);
size_t imcui_hip_darkfeat_packed_floats(void);
int imcui_hip_darkfeat_pack_weights(const float* const* tensors, float* packed);
/* Scratch of imcui_hip_darkfeat_forward: B images of H x W (H, W >= 16). */
size_t imcui_hip_darkfeat_workspace_bytes(int B, int H, int W);
/* darkfeat.py:31-44 `_forward` around `self.net({"image": image})` (:32): image [dev, B,C,H,W] with C == 3 (anything else is refused),
 * H, W >= 16.  Per image (x - mean) / std over its 3 H W values (std unbiased); 3x3 convolutions with a non-affine InstanceNorm
 * (eps 1e-5, biased variance) and ReLU; per score level max_c softplus(x - box3x3_d(x)) softplus(x - mean_c(x)) of the raw map divided by
 * its moving average (d = 3, 2, 1, reflect padding); score = (sum_l (l + 1) / 6 up(s_l)) up(soft-max(clf(desc^2))[1]), up = bilinear,
 * align_corners=True.  Detector: score > score_thld (strict), 3x3 maximum (nms_size 3; 0 = off), not within eof_mask pixels of the
 * border, det > 0 and tr^2 / det <= (edge_thld + 1)^2 / edge_thld of the dilation-3 Hessian (zero padding), every operation rounded
 * once.  Candidates in row-major order; the min(kpt_n, max_keypoints or all) highest scores stay (:36 `[-max_keypoints or None:]`; a
 * negative max_keypoints is refused), among equal scores the later pixels; output in ASCENDING (score, pixel) order, a STABLE form of
 * :36's argsort.  descriptor = the last layer's 1/4-resolution map at (y, x) / 4 (floor / ceil corners clamped, weights from the
 * unclamped fractions) / max(norm, 1e-12).  kout >= min(kpt_n, max_keypoints or all, H W).  Outputs, first num_keypoints[b] rows valid,
 * the rest zero:
 *   keypoints [dev, B,kout,2] (x, y), integer-valued;  scores [dev, B,kout];  descriptors [dev, B,kout,128];  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: bit 4 = an image of the batch is flat (std == 0: NaN upstream; here that image has zero key-points).
 *   The candidate list holds every pixel, so it cannot overflow (bit 2 never shows).
 *   optional debug outputs: dbg_score [B,H,W], dbg_desc [B,h4,w4,128], dbg_peak0 [B,H,W], dbg_peak1 [B,h2,w2], dbg_peak2 and dbg_prob
 *   [B,h4,w4] (h2 = (H-1)/2+1, h4 = (h2-1)/2+1); dbg_raw / dbg_norm: the output of layer dbg_layer before / behind its InstanceNorm
 * No host synchronisation; a row's bits do not depend on the batch. */
int imcui_hip_darkfeat_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, float score_thld, float edge_thld,
                               int nms_size, int eof_mask, int kpt_n, int max_keypoints, int kout, float* keypoints, float* scores, float* descriptors,
                               int* num_keypoints, int* status, float* dbg_score, float* dbg_desc, float* dbg_peak0, float* dbg_peak1, float* dbg_peak2,
                               float* dbg_prob, int dbg_layer, float* dbg_raw, float* dbg_norm, void* ws, size_t ws_bytes, void* stream);
/* Test entries; ws: imcui_hip_darkfeat_probe_workspace_bytes(B, H, W) of the map the probe is given.  stem_probe: the image statistics
 * and layer 0, image [dev, B,3,H,W] -> out [dev, B,H,W,32] RAW, imstat [dev, B,2] = mean, std (1 when flat), status OR-ed with bit 4
 * (the caller zeroes it).  inorm_probe: InstanceNorm + ReLU of x [dev, B,H,W,C], C = 32 / 64 / 128 -> out, stat [dev, B,C,2] = mean,
 * 1 / sqrt(var + eps) (optional).  peak_probe: the peakiness pass, (C, d) = (32, 3), (64, 2), (128, 1), H, W >= d + 1, mavg [dev, 1].
 * score_probe: the assembly from given level maps pk0 [B,H,W], pk1 [B,h2,w2], pk2 [B,h4,w4] and dmap [B,h4,w4,128].  detect_probe: the
 * detector, the cut and the ranked rows on a given score map [dev, B,H,W]; num_candidates [dev, B] and det_map [dev, B,H,W] (the score
 * at candidates, -inf elsewhere) optional.  describe_probe: descriptors at keypoints [dev, B,K,2] (nkpts [dev, B] valid rows) of a
 * given map dmap [dev, B,h4,w4,128]. */
size_t imcui_hip_darkfeat_probe_workspace_bytes(int B, int H, int W);
int imcui_hip_darkfeat_stem_probe(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, float* out, float* imstat, int* status,
                                  void* ws, size_t ws_bytes, void* stream);
int imcui_hip_darkfeat_inorm_probe(imcui_hip_t* h, const float* x, int B, int H, int W, int C, float* out, float* stat, void* ws, size_t ws_bytes,
                                   void* stream);
int imcui_hip_darkfeat_peak_probe(imcui_hip_t* h, const float* x, const float* mavg, int B, int H, int W, int C, int d, float* out, void* stream);
int imcui_hip_darkfeat_score_probe(imcui_hip_t* h, const float* packed, const float* pk0, const float* pk1, const float* pk2, const float* dmap, int B, int H,
                                   int W, float* score, void* ws, size_t ws_bytes, void* stream);
int imcui_hip_darkfeat_detect_probe(imcui_hip_t* h, const float* score, int B, int H, int W, float score_thld, float edge_thld, int nms_size, int eof_mask,
                                    int kpt_n, int max_keypoints, int kout, float* keypoints, float* scores, int* num_keypoints, int* num_candidates,
                                    int* status, float* det_map, void* ws, size_t ws_bytes, void* stream);
int imcui_hip_darkfeat_describe_probe(imcui_hip_t* h, const float* dmap, int B, int h4, int w4, const float* keypoints, const int* nkpts, int K,
                                      float* descriptors, void* stream);

/* ---- SFD2 (zoo entry sfd2+mnn: `feature: sfd2` + NN-mutual; imcui/hloc/extractors/sfd2.py) ------------------------------- */
/* pram.nets.sfd2.load_sfd2(weight_path) (replaces sfd2.py:31) is not part of the reference checkout (third_party is empty): the ResNet4x
 * network is restated from its description (tests/sfd2_reference.py) and parity with upstream's code is NOT pinned (INTEGRATION.md,
 * "SFD2: what is pinned").  cfg [host, 12 ints], read from the checkpoint's shapes by the binding: c1 (64), c2, c3 (trunk widths,
 * multiples of 32 up to 512), bottlenecks of conv4 (0..8), channels per group of their 3x3 (4 / 8 / 16), hidden width of either head,
 * kernel size of convPb and of convDb (1 or 3), BatchNorm behind the convolutions (0 / 1), bias on the trunk / head convolutions,
 * bias on the bottleneck convolutions, 0.  The backbone is ONE table in csrc/sfd2.hip (SFD2_LAYERS), readable through
 * imcui_hip_sfd2_layer: launch name, and out5 = kind (0 layer 0 on the VALU, 1 3x3 implicit GEMM, 2 1x1 GEMM, 3 grouped 3x3, 4 the two
 * heads' hidden layers as one launch), cin, cout, stride, place in a bottleneck (0 none, 1 first, 2 middle, 3 last: + identity).
 * Tensors in imcui_hip_sfd2_tensor_name order, upstream's state-dict keys: `conv1a.0.weight` .. (`.0.bias`, `.1.{weight, bias,
 * running_mean, running_var}`), `conv4.{i}.conv{1,2,3}.weight` / `conv4.{i}.bn{1,2,3}.*`, `convPa.0` / `convPa.1`, `convDa.0` /
 * `convDa.1`, `convPb.{weight, bias}`, `convDb.{weight, bias}`. */
int imcui_hip_sfd2_num_layers(const int* cfg);
const char* imcui_hip_sfd2_layer(const int* cfg, int i, int* out5);
int imcui_hip_sfd2_num_tensors(const int* cfg);
const char* imcui_hip_sfd2_tensor_name(const int* cfg, int i);
size_t imcui_hip_sfd2_packed_floats(const int* cfg);
/* BatchNorm (eval, eps 1e-5) is folded in float32; tvf.Normalize's mean / std (sfd2.py:24-26) go into the packed header. */
int imcui_hip_sfd2_pack_weights(const int* cfg, const float* const* tensors, float* packed);
/* Scratch of imcui_hip_sfd2_forward: B images of H x W (H, W >= 16). */
size_t imcui_hip_sfd2_workspace_bytes(const int* cfg, int B, int H, int W);
/* sfd2.py:35-44 `_forward`: `self.norm_rgb(data["image"])` (:37) and `self.net.extract_local_global(data, config=self.conf)` (:36).
 * image [dev, B,C,H,W] RGB in [0, 1] with C == 3 (anything else is refused), H, W >= 16.  (x - mean_c) / std_c where layer 0 reads the
 * image; trunk to 1/4 resolution (Hc = ceil(ceil(H / 2) / 2)); score = sigmoid(convPb(relu(convPa(x)))) through a 4 x 4 depth-to-space
 * (channel 4 dy + dx) -> [4 Hc, 4 Wc]; descriptors = F.normalize(convDb(relu(convDa(x)))) at 1/4 resolution.  Selection: simple_nms radius
 * 4; score > conf_th (strict) and not within remove_borders pixels of the IMAGE's border (the map may exceed the image by up to 3 rows /
 * columns: nothing outside the image is kept); an image with fewer than min_keypoints such candidates is selected again with threshold 0
 * (decided on the device); the max_keypoints highest scores stay (0: all; negative: refused).  Output in DESCENDING score order, equal
 * scores by ascending pixel index (torch.topk leaves that open).  descriptor = sample_descriptors with s = 4 (grid_sample bilinear,
 * align_corners=True, zero padding) / max(norm, 1e-12).  kout >= min(max_keypoints or all, 16 Hc Wc).  Outputs, first num_keypoints[b]
 * rows valid, the rest zero:
 *   keypoints [dev, B,kout,2] (x, y), integer-valued;  scores [dev, B,kout];  descriptors [dev, B,kout,128];  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: always 0 (the candidate list holds every score-map pixel, so it cannot overflow)
 *   optional debug outputs: dbg_score [B,4 Hc,4 Wc], dbg_desc [B,Hc,Wc,128] (normalised), dbg_map: the NHWC output of launch dbg_layer
 * No host synchronisation; a row's bits do not depend on the batch. */
int imcui_hip_sfd2_forward(imcui_hip_t* h, const int* cfg, const float* packed, const float* image, int B, int C, int H, int W, float conf_th,
                           int remove_borders, int min_keypoints, int max_keypoints, int kout, float* keypoints, float* scores, float* descriptors,
                           int* num_keypoints, int* status, float* dbg_score, float* dbg_desc, int dbg_layer, float* dbg_map, void* ws, size_t ws_bytes,
                           void* stream);
/* Test entries.  gconv_probe: the grouped 3x3 convolution (F.conv2d(groups=C / cg), pad 1) of x [dev, B,H,W,C] with weights in the packed
 * order [group][tap][ci][co] and shift [C] as the start of every sum, optional ReLU.  layers_probe: launches [first, last] of the
 * forward's own list on the planar image (first == 0) or an NHWC map [dev, B,H,W,cin] -> the last launch's NHWC map; ws:
 * imcui_hip_sfd2_layers_workspace_bytes.  score_probe: logits [dev, B,Hc,Wc,16] -> score [dev, B,4 Hc,4 Wc].  select_probe: the selection on
 * a given score map [dev, B,Hs,Ws] of H x W images (H <= Hs, W <= Ws); num_candidates [dev, B], eff [dev, B] (the per-image threshold)
 * and nms_map optional; ws: imcui_hip_sfd2_select_workspace_bytes.  describe_probe: descriptors at keypoints [dev, B,K,2] (nkpts [dev, B]
 * valid rows) of a map dmap [dev, B,h4,w4,128], normalised into dmap_out first when `normalise`. */
int imcui_hip_sfd2_gconv_probe(imcui_hip_t* h, const float* x, const float* w_packed, const float* shift, int B, int H, int W, int C, int cg, int relu,
                               float* out, void* stream);
size_t imcui_hip_sfd2_layers_workspace_bytes(const int* cfg, int first, int last, int B, int H, int W);
int imcui_hip_sfd2_layers_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* in, int first, int last, int B, int H, int W, float* out,
                                void* ws, size_t ws_bytes, void* stream);
int imcui_hip_sfd2_score_probe(imcui_hip_t* h, const float* logits, int B, int Hc, int Wc, float* score, void* stream);
size_t imcui_hip_sfd2_select_workspace_bytes(int B, int Hs, int Ws);
int imcui_hip_sfd2_select_probe(imcui_hip_t* h, const float* score, int B, int Hs, int Ws, int H, int W, float conf_th, int remove_borders, int min_keypoints,
                                int max_keypoints, int kout, float* keypoints, float* scores, int* num_keypoints, int* num_candidates, float* eff, int* status,
                                float* nms_map, void* ws, size_t ws_bytes, void* stream);
int imcui_hip_sfd2_describe_probe(imcui_hip_t* h, const float* dmap, int B, int h4, int w4, int normalise, float* dmap_out, const float* keypoints,
                                  const int* nkpts, int K, float* descriptors, void* stream);

/* ---- DeDoDe (zoo entry dedode: `feature: dedode` + Dual-Softmax; imcui/hloc/extractors/dedode.py) ----------------------- */
/* dedode_detector_L (vgg19_bn encoder) and dedode_descriptor_B (vgg11_bn encoder) of Parskatt/DeDoDe, each with a decoder of four
 * ConvRefiners (scales 8, 4, 2, 1).  The refiners' shapes are READ from the checkpoint by the binding and handed over as
 * dims [host, 2 models (detector, descriptor)][4 scales (8, 4, 2, 1)][in, hidden, out, hidden blocks]: hidden a multiple of 32 up to
 * 512, 1..16 hidden blocks, in = feature channels (512, 256, 128, 64) + the context the coarser scale hands down (out - P there, a
 * multiple of 32), P = 1 key-point logit (detector) or 256 description channels (descriptor).  imcui_hip_dedode_dims_error says why a
 * dims table is refused (empty string: served).  Tensors in imcui_hip_dedode_tensor_name order: both state dicts under the prefixes
 * `detector.` / `descriptor.` (`encoder.layers.N.*`, `decoder.layers.S.block1.{0,1,3}.*`, `.hidden_blocks.I.{0,1,3}.*`, `.out_conv.*`;
 * BatchNorm as weight, bias, running_mean, running_var and folded here in float32), then `density_taps` [51] =
 * exp(-linspace(-2, 2, 51)^2) as the binding's float32 evaluates it.  The networks are restated from their description
 * (tests/dedode_reference.py): parity with upstream's code is NOT pinned. */
size_t imcui_hip_dedode_packed_floats(const int* dims);
int imcui_hip_dedode_num_tensors(const int* dims);
const char* imcui_hip_dedode_tensor_name(const int* dims, int i);
const char* imcui_hip_dedode_dims_error(const int* dims);
int imcui_hip_dedode_pack_weights(const int* dims, const float* const* tensors, float* packed);
size_t imcui_hip_dedode_workspace_bytes(const int* dims, int B, int H, int W, int k);
/* dedode.py:55-86 `_forward`: image [dev, B,3,H,W] RGB in [0,1], H and W multiples of 8 (every dedode conf resizes with dfactor 8) ->
 * transforms.Normalize, detector.detect(num_keypoints = k): p = soft-max of the logits over the image, density = the separable 51-tap
 * filter of (p + 1e-6) * 10000 (rows, then columns, zero padding), score = p * (density + 1e-8)^-1/2, the k highest scores (1 <= k <=
 * H W; equal scores: the lower flat index first), key-points at the pixel centres x = (2 j + 1) / W - 1; descriptor.describe_keypoints:
 * bilinear grid_sample (align_corners=False) of the 256-channel description grid there, NOT normalised; to_pixel_coords.  Outputs, rows
 * in descending score, the first k valid and rows k .. kout zero:
 *   keypoints [dev, B,kout,2] (x, y in pixels);  scores [dev, B,kout];  descriptors [dev, B,kout,256];  num_keypoints [dev, B] int32 (= k)
 *   status [dev, 1] int32 optional: 0 (every pixel is a candidate, no list can overflow)
 *   dbg_logits optional [dev]: the detector's accumulated logits of the scales 8, 4, 2, 1, one after another, each [B, h, w]
 *   dbg_logp / dbg_score optional [dev, B,H,W];  dbg_desc2 optional [dev, B,H/2,W/2,256]: the description grid accumulated down to 1/2
 *   dbg_dense optional [dev, B,H,W,256]: the full-resolution description grid, which the call otherwise never forms (tests)
 * No host synchronisation. */
int imcui_hip_dedode_forward(imcui_hip_t* h, const float* packed, const int* dims, const float* image, int B, int H, int W, int k, int kout,
                             float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, float* dbg_logits, float* dbg_logp,
                             float* dbg_score, float* dbg_desc2, float* dbg_dense, void* ws, size_t ws_bytes, void* stream);
/* Test entry: one of the new kernels alone (the matrix layers have imcui_hip_conv_probe / imcui_hip_gemm_probe_f32).  op 0: layer 0 of
 * `model` (0 detector, 1 descriptor) with Normalize applied as the image is read, in = image [dev, B,3,H,W] -> out [dev, B,H,W,64]
 * (needs packed and dims); op 1: depth-wise 5x5 (pad 2) + bias + ReLU, in [dev, B,H,W,C], C a multiple of 32, wts [dev] = [25 taps][C]
 * then [C] bias; op 2: bilinear x2 (align_corners=False), in [dev, B,H,W,C] -> [dev, B,2H,2W,C]; op 3: bicubic x2 of the planes
 * in [dev, B,H,W]; op 4: soft-max statistics of in [dev, B,H*W] -> out [dev, 2 B + 2 B chunks]: (max, log sum exp(l - max)) per image,
 * then scratch; op 5: the separable 51-tap filter of the planes in [dev, B,H,W], wts = the taps, out [dev, 2,B,H,W]: the result, then
 * the row pass. */
int imcui_hip_dedode_layer_probe(imcui_hip_t* h, int op, const float* packed, const int* dims, int model, const float* wts, const float* in, int B, int H,
                                 int W, int C, float* out, void* stream);
/* Test entry: the selection code on maps GIVEN by the caller.  mode 0: map = log p [dev, B,H,W] -> p = exp(log p), filter, score, cut,
 * rows; mode 1: map = the score map itself -> cut and rows (crafted equal scores).  score_out optional [dev, B,H,W]. */
size_t imcui_hip_dedode_select_probe_workspace_bytes(int B, int H, int W, int k);
int imcui_hip_dedode_select_probe(imcui_hip_t* h, int mode, const float* taps, const float* map, int B, int H, int W, int k, int kout, float* keypoints,
                                  float* scores, int* num_keypoints, float* score_out, void* ws, size_t ws_bytes, void* stream);

/* ---- NetVLAD (retrieval_zoo entry netvlad; imcui/hloc/extractors/netvlad.py, imcui/hloc/pairs_from_retrieval.py) ---------------------- */
/* Packed weights of the reference's `NetVLAD` module (replaces the MATLAB parsing of netvlad.py:76-120 as far as the device is
 * concerned: the plugin parses the .mat, this packs the result): tensors in imcui_hip_netvlad_tensor_name order -- `backbone.N.weight` /
 * `.bias` (N = 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28 of torchvision's vgg16().features), `netvlad.score_proj.weight` [64,512,1],
 * `netvlad.centers` [512,64], `preprocess.mean` [3] (netvlad.py:118) and, with whiten != 0, `whiten.weight` [4096,32768] / `whiten.bias`.
 * The whitening matrix stays float32 (no f16 planes); without whitening it is neither packed nor launched. */
size_t imcui_hip_netvlad_packed_floats(int whiten);
int imcui_hip_netvlad_num_tensors(int whiten);
const char* imcui_hip_netvlad_tensor_name(int whiten, int i);
int imcui_hip_netvlad_pack_weights(int whiten, const float* const* tensors, float* packed);
size_t imcui_hip_netvlad_workspace_bytes(int B, int H, int W, int whiten);
/* netvlad.py:122-146 `_forward`: image [dev, B,C,H,W] RGB in [0,1] -> descriptor [dev, B,4096] (whiten) or [dev, B,32768], unit norm.
 * clamp(x * 255, 0, 255) - mean as the image is read, VGG-16 to conv5_3 without its ReLU and pool (:66-68), F.normalize per pixel (:138),
 * NetVLADLayer.forward (:27-38), `self.whiten` and the final F.normalize (:143-144).  Refused with a message: C != 3, a side below 16
 * (empty conv5_3 map).  dbg_feat optional: [dev, B,H/16,W/16,512] the conv5_3 map (NHWC).  Every image is computed independently of the
 * batch (bitwise); no float atomics; no host synchronisation, graph-capturable. */
int imcui_hip_netvlad_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, int whiten, float* descriptor,
                              float* dbg_feat, void* ws, size_t ws_bytes, void* stream);
/* Test entry: one stage alone.  op 0: layer 0 with netvlad.py:126-129 applied as the image is read, in = image [dev, B,3,H,W] -> out
 * [dev, B,H,W,64]; op 1: nn.MaxPool2d(2, 2), flooring, in [dev, B,H,W,C] -> out [dev, B,H/2,W/2,C]; op 2: netvlad.py:138 + NetVLADLayer
 * on maps in [dev, B,H,W,512] -> out [dev, B,32768]; op 3: backbone.28 (conv5_3, no ReLU) as the forward launches it -- the 512 input
 * channels in 8 groups of 64, each a launch of the patch-staging kernels, summed in group order -- in the handle's arithmetic mode, in / out
 * [dev, B,H,W,512].  Ops 2 and 3 take the workspace of imcui_hip_netvlad_probe_workspace_bytes(B, H * W). */
size_t imcui_hip_netvlad_probe_workspace_bytes(int B, int N);
int imcui_hip_netvlad_layer_probe(imcui_hip_t* h, int op, const float* packed, const float* in, int B, int H, int W, int C, float* out, void* ws,
                                  size_t ws_bytes, void* stream);
/* Test entry: the whitening's split-K skinny GEMM, its fold and the normalisation at a free shape: out [dev, B,out_dim] =
 * normalize(weight [dev, out_dim,in_dim] x [dev, B,in_dim] + bias), in_dim a multiple of 4. */
size_t imcui_hip_netvlad_whiten_workspace_bytes(int B, int in_dim, int out_dim);
int imcui_hip_netvlad_whiten_probe(imcui_hip_t* h, const float* weight, const float* bias, const float* x, int B, int in_dim, int out_dim, float* out, void* ws,
                                   size_t ws_bytes, void* stream);
/* pairs_from_retrieval.py:109 `einsum("id,jd->ij")` and :56-66 `pairs_from_score_matrix` up to the top-k, on the device: query [dev, Q,D],
 * db [dev, N,D] float32; invalid optional [dev, Q,N] bytes; an entry that is invalid, or below min_score when has_min_score != 0, counts
 * as -inf.  indices [dev, Q,num_select] int32 / scores [dev, Q,num_select]: the num_select highest of every row in descending score,
 * equal scores by ascending database index (torch.topk leaves that order open); slots past N hold -1 / -inf.  The score matrix lives in
 * the workspace only. */
size_t imcui_hip_retrieval_topk_workspace_bytes(int Q, int N);
int imcui_hip_retrieval_topk(imcui_hip_t* h, const float* query, const float* db, int Q, int N, int D, const unsigned char* invalid, int has_min_score,
                             float min_score, int num_select, int* indices, float* scores, void* ws, size_t ws_bytes, void* stream);

/* ---- CosPlace / EigenPlaces (retrieval_zoo entry cosplace; imcui/hloc/extractors/cosplace.py, eigenplaces.py) ------------------------- */
/* Packed weights of the model that cosplace.py:28-34 / eigenplaces.py:41-47 fetch with torch.hub.load("gmberton/...", "get_trained_model",
 * backbone=, fc_output_dim=): backbone = 18 / 50 / 101 / 152 (torchvision ResNet without avgpool and fc), tensors in
 * imcui_hip_places_tensor_name order -- `backbone.0.weight`, `backbone.1.{weight,bias,running_mean,running_var}`,
 * `backbone.{4..7}.<block>.conv{1,2,3}.weight` / `.bn{1,2,3}.*` / `.downsample.0.weight` / `.downsample.1.*`, `aggregation.1.p` [1],
 * `aggregation.3.weight` [fc_output_dim, F] / `.bias` (F = 512 for ResNet-18, else 2048).  Every BatchNorm (eps 1e-5) is folded into its
 * convolution in float32.  The network is restated, not in the reference checkout: the names are as recalled from upstream, unverified. */
size_t imcui_hip_places_packed_floats(int backbone, int fc_output_dim);
int imcui_hip_places_num_tensors(int backbone, int fc_output_dim);
const char* imcui_hip_places_tensor_name(int backbone, int fc_output_dim, int i);
int imcui_hip_places_pack_weights(int backbone, int fc_output_dim, const float* const* tensors, float* packed);
size_t imcui_hip_places_workspace_bytes(int backbone, int fc_output_dim, int B, int H, int W);
/* cosplace.py:40-45 / eigenplaces.py:53-58 `_forward`: image [dev, B,C,H,W] RGB in [0,1] -> descriptor [dev, B,fc_output_dim], unit norm.
 * tvf.Normalize (:36-38, :41) as the image is read, conv1 + bn1 + ReLU + max-pool in one kernel, layer1 .. layer4 on the shared GEMM,
 * L2Norm, GeM (p from the packed buffer), Linear, L2Norm.  Any H, W >= 1.  Refused with a message: C != 3, an unknown backbone.  map
 * optional: [dev, B,h4,w4,F] the layer4 map (NHWC), every stage's size (n - 1) / 2 + 1 of the one before, five times from H, W.  Every
 * image is computed independently of the batch (bitwise); no float atomics; no host synchronisation, graph-capturable. */
int imcui_hip_places_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, int backbone, int fc_output_dim,
                             float* descriptor, float* map, void* ws, size_t ws_bytes, void* stream);
/* Test entry: one stage alone, through the forward's own launch code.  op 0: tvf.Normalize + conv1 + bn1 + ReLU + max-pool, in = image
 * [dev, B,3,H,W] -> out [dev, B,Hp,Wp,64]; op 1: block `block` of layer 1 .. 4 in the handle's arithmetic mode, in [dev, B,H,W,cin] -> out
 * [dev, B,Ho,Wo,cout]; op 2: L2Norm + GeM, in [dev, B,H,W,F] -> out [dev, B,F]; op 3: Linear + L2Norm, in [dev, B,F] (H = W = 1) -> out
 * [dev, B,fc_output_dim].  Ops 1 and 2 take the workspace of imcui_hip_places_probe_workspace_bytes. */
size_t imcui_hip_places_probe_workspace_bytes(int backbone, int fc_output_dim, int op, int B, int H, int W, int layer, int block);
int imcui_hip_places_layer_probe(imcui_hip_t* h, int op, int backbone, int fc_output_dim, const float* packed, const float* in, int B, int H, int W, int layer,
                                 int block, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- DoG + HardNet / SOSNet patch descriptors (extractor confs `hardnet` / `sosnet`; imcui/hloc/extractors/dog.py:87-105) ------------ */
/* model 0 = kornia.feature.HardNet (state dict `features.N.*`), 1 = kornia.feature.SOSNet (`layers.N.*`): seven bias-free convolutions,
 * each with the running_mean / running_var of its BatchNorm2d(affine=False); tensors in imcui_hip_patchdesc_tensor_name order.  The
 * BatchNorms are folded in float32 at pack time; both networks share one packed layout. */
size_t imcui_hip_patchdesc_packed_floats(void);
int imcui_hip_patchdesc_num_tensors(int model);
const char* imcui_hip_patchdesc_tensor_name(int model, int i);
int imcui_hip_patchdesc_pack_weights(int model, const float* const* tensors, float* packed);
/* levels of the pyramid the call builds for an H x W image (level 0 = the image) */
int imcui_hip_patchdesc_num_levels(int H, int W);
/* the activations are sized by `chunk`; kcap only sizes the table of per-chunk row counts */
size_t imcui_hip_patchdesc_workspace_bytes(int B, int H, int W, int kcap, int chunk);
/* dog.py:87-105 on key-points given by the caller: image [dev, B,1,H,W] in [0,1]; keypoints [dev, B,kcap,2] (x, y as the detector returns
 * them: the call adds 0.5), scales [dev, B,kcap] (sigma), oris_deg [dev, B,kcap] (degrees; the LAF angle is -ori), num_keypoints [dev, B]
 * -> descriptors [dev, B,kcap,128], unit rows; rows past num_keypoints[b] are not written.  LAF scale = sigma mr_size / 2; pyramid =
 * kornia pyrdown (5x5 binomial blur, reflect; bilinear halving) while min(h, w) >= 32; level floor(log2(2 laf_scale / 32)) clamped to
 * [0, max(0, min(H, W) / 32 - 1)]; 32x32 affine grid, bilinear, border padding, align_corners=False.  Patches are processed per image in
 * chunks of `chunk` rows (the reference's max_batch_size is 1024); the launches are fixed by (B, kcap, chunk) and a chunk past an image's
 * count exits on the device.  A descriptor does not depend (bitwise) on B, on the other counts or on `chunk`.  status optional [dev, 1]:
 * bit 1 = a count above kcap (clipped), bit 2 = a non-finite key-point, scale or orientation (its row is zero).  dbg_patches optional
 * [dev, B,kcap,1024].  No float atomics, no host synchronisation, graph-capturable. */
int imcui_hip_patchdesc_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int H, int W, const float* keypoints, const float* scales,
                                const float* oris_deg, const int* num_keypoints, int kcap, int model, float mr_size, int chunk, float* descriptors, int* status,
                                float* dbg_patches, void* ws, size_t ws_bytes, void* stream);
/* Test entry: pyramid + sampling alone on ONE image [dev, H,W]: n key-points -> patches [dev, n,1024]; status [dev, 1] as above. */
size_t imcui_hip_patchdesc_patch_probe_workspace_bytes(int H, int W);
int imcui_hip_patchdesc_patch_probe(imcui_hip_t* h, const float* image, int H, int W, const float* keypoints, const float* scales, const float* oris_deg, int n,
                                    float mr_size, float* patches, int* status, void* ws, size_t ws_bytes, void* stream);
/* Test entry: one launch alone on n rows, as the forward launches it (row counts read on the device).  op 0: pyrdown, in [dev, n,H,W] ->
 * out [dev, n,H/2,W/2]; op 1: the input normalisation [n,1024] -> [n,1024]; op 2: normalisation + layer 1 -> NHWC [n,32,32,32]; ops 3..7:
 * layers 2..6, NHWC in -> NHWC out; op 8: layer 7 (8 partial products over 1024 of K each, folded in group order, then the BatchNorm
 * shift) [n,8192] -> [n,128]; op 9: the output
 * normalisation [n,128] -> [n,128].  H, W are read by op 0 only. */
size_t imcui_hip_patchdesc_probe_workspace_bytes(int n, int H, int W);
int imcui_hip_patchdesc_layer_probe(imcui_hip_t* h, int op, int model, const float* packed, const float* in, int n, int H, int W, float* out, void* ws,
                                    size_t ws_bytes, void* stream);

/* ---- SIFT(zoo entry sift-lightglue, and `sift` + NN; imcui/hloc/extractors/sift.py, backend "opencv") ------------------- */
/* OpenCV 4.x SIFT_create(contrastThreshold, nfeatures, edgeThreshold, nOctaveLayers = `layers`; sigma 1.6, first octave -1, float
 * pipeline) -> detectAndCompute (sift.py:61-78), then `filter_dog_point` (:19-52), the score top-k (:188-193) and
 * `sift_to_rootsift` (:55-58).  No weights.  OpenCV's sources are restated from its documentation (tests/sift_reference.py is the
 * written definition); the angle of a gradient is atan2, not cv2's fastAtan2 polynomial.
 * Octaves of an H x W image: cvRound(log2(min(2W, 2H)) - 2) + 1; octave o is (2H >> o) x (2W >> o) with layers + 3 levels. */
int imcui_hip_sift_num_octaves(int H, int W);
/* Floats of the Gaussian pyramid of B images: octave after octave, each a block [B][layers + 3][h_o][w_o]. */
size_t imcui_hip_sift_pyramid_floats(int B, int H, int W, int layers);
/* Scratch of imcui_hip_sift_forward: the pyramid, one 2H x 2W plane and the candidate lists (ccap entries per image). */
size_t imcui_hip_sift_workspace_bytes(int B, int H, int W, int layers, int ccap, int kcap);
/* image [dev, B,C,H,W] float in [0,1], C = 1 or 3 (gray = 0.299 R + 0.587 G + 0.114 B in float, kornia's rgb_to_grayscale), then
 * `(x * 255.0)` truncated to uint8 (sift.py:158).  layers 3..5; H, W >= 8.
 * nfeatures > 0: OpenCV's retainBest (ties stay); nms_radius < 0 skips `filter_dog_point` (the wrapper's `nms_radius: None`), 0 keeps
 * the highest score and then the lowest |angle| of a pixel, > 0 adds the max-pool NMS; max_keypoints > 0: the max_keypoints highest
 * scores (ties to the earlier key-point).  rootsift != 0: RootSIFT rows, else the 0..255 integers as float.
 * Order of the outputs: detection order (octave, layer, row, column, orientation bin) of the survivors, NOT sorted by score.
 * Outputs (device; capacity kcap per image, rows beyond num_keypoints[b] are not written):
 *   keypoints [B,kcap,2] (x, y) pixels;  scores (|contrast|), scales (KeyPoint.size), oris (radians) [B,kcap];
 *   descriptors [B,kcap,128];  num_keypoints [B];  status [1]: bit 1 = more survivors than kcap, bit 2 = more extrema or more
 *   oriented key-points than ccap (call again with larger capacities; `counts` tells how large)
 *   counts [B,3] optional: extrema found, table rows (oriented key-points), survivors -- the true numbers, not clipped
 * Optional outputs for the tests:
 *   dbg_pyramid [imcui_hip_sift_pyramid_floats];  dbg_extrema [B,ccap] int: index (octave, layer - 1, row, column) of each extremum
 *   in the image's search space;  dbg_refined [B,ccap,16]: valid, octave, layer, r, c, xc, xr, xi, contrast (signed), size, x, y,
 *   edge quantity tr^2 e - (e+1)^2 det, det, 0, 0;  dbg_hist [B,ccap,36]: smoothed orientation histogram of every valid candidate
 *   dbg_table [B,ccap,12]: the key-point table before removeDuplicated / retainBest / halving and the wrapper stages: octave, layer,
 *   r, c, xc, xr, xi, response, size, angle (degrees), x, y (size, x, y in the doubled image's units)
 *   dbg_desc_raw [B,kcap,128]: the descriptor after x 512 / norm, before saturate_cast
 * No float atomics and no host synchronisation: results are bitwise reproducible and the call is graph-capturable. */
int imcui_hip_sift_forward(imcui_hip_t* h, const float* image, int B, int C, int H, int W, int layers, float contrast_threshold,
                           float edge_threshold, int nfeatures, int nms_radius, int max_keypoints, int rootsift, int ccap, int kcap,
                           float* keypoints, float* scores, float* scales, float* oris, float* descriptors, int* num_keypoints, int* status,
                           int* counts, float* dbg_pyramid, int* dbg_extrema, float* dbg_refined, float* dbg_hist, float* dbg_table,
                           float* dbg_desc_raw, void* ws, size_t ws_bytes, void* stream);

/* ---- XFeat (zoo entry xfeat(sparse) = `feature: xfeat` + NN-mutual; imcui/hloc/extractors/xfeat.py:8-34) ---------------- */
/* Weight packing runs on the HOST (replaces the `torch.hub.load("verlab/accelerated_features", "XFeat")` of xfeat.py:17-21): tensor i
 * is the XFeatModel state-dict entry named imcui_hip_xfeat_tensor_name(i) (skip1.1.*, then block1 .. keypoint_head in module order,
 * without the `num_batches_tracked` counters and without `fine_matcher.*`); BatchNorm2d(affine=False) in eval mode is folded into the
 * convolution before it: w / sqrt(var + 1e-5), bias -mean / sqrt(var + 1e-5).  `packed` receives imcui_hip_xfeat_packed_floats()
 * floats; it begins with block1.0 folded as [9 taps][4] floats followed (from float 64) by its 4 folded biases. */
size_t imcui_hip_xfeat_packed_floats(void);
int imcui_hip_xfeat_num_tensors(void);
const char* imcui_hip_xfeat_tensor_name(int i);
int imcui_hip_xfeat_pack_weights(const float* const* tensors, float* packed);
/* Scratch of imcui_hip_xfeat_forward for B images of H x W (independent of the threshold, top_k and kcap). */
size_t imcui_hip_xfeat_workspace_bytes(int B, int H, int W);
/* Bound on the key-points of an H x W image whose scores do not tie exactly: survivors of the 5x5 NMS are more than 2 pixels apart.
 * An exact plateau (a constant image) keeps every member and can exceed it, up to (H / 32 * 32) * (W / 32 * 32). */
int imcui_hip_xfeat_max_keypoints_bound(int H, int W);
/* imcui/hloc/extractors/xfeat.py:26-34 `self.net.detectAndCompute(data["image"], top_k=max_keypoints)[0]`.
 * image [dev, B,C,H,W] in [0,1], C = 1 or 3, H, W >= 32: resized (bilinear, align_corners=False) to Hr x Wr = multiples of 32, channel
 * mean, InstanceNorm, XFeatModel, then NMS (5x5, `==` max and > threshold), score = nearest(key-point map) x bilinear(reliability), a
 * key-point at (0, 0) scores -1, order by descending score (ties: lower flat index first), Python's `[:top_k]` per image (-1 drops the
 * lowest), bicubic descriptors, key-points x (W / Wr, H / Hr), score > 0.  threshold: xfeat.py never passes its `keypoint_threshold`,
 * so the reference runs at upstream's 0.05.
 * Outputs, fixed stride `kcap` per image, first num_keypoints[b] entries valid, the rest zero, in descending score order:
 *   keypoints [dev, B,kcap,2] (x, y) in pixels of the H x W image;  scores [dev, B,kcap]
 *   descriptors [dev, B,kcap,64] L2-normalised rows;  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: 0 = fine, bit 1 = more key-points than kcap (the first kcap are returned)
 *   kpt_heat [dev, B,Hr,Wr], reliability [dev, B,Hr/8,Wr/8], feats_norm [dev, B,Hr/8,Wr/8,64] (NHWC) optional: the dense maps
 * Zero key-points is a valid result.  No host synchronisation. */
int imcui_hip_xfeat_forward(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, float threshold, int top_k, int kcap,
                            float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, float* kpt_heat, float* reliability,
                            float* feats_norm, void* ws, size_t ws_bytes, void* stream);
/* Test entry: the sampling rules of the selection (xfeat.py:30 -> InterpolateSparse2d: F.grid_sample at 2 * (xy / (W - 1, H - 1)) - 1,
 * align_corners=False) at n integer pixels xy [dev, n,2] int32 of an H x W image (multiples of 8): kpt_heat [dev, H,W] sampled nearest,
 * reliability [dev, H/8,W/8] bilinear, feats [dev, H/8,W/8,64] bicubic (not normalised) -> nearest [n], bilinear [n], bicubic [n,64]. */
int imcui_hip_xfeat_sample_probe(imcui_hip_t* h, const float* kpt_heat, const float* reliability, const float* feats, int H, int W, const int* xy, int n,
                                 float* nearest, float* bilinear, float* bicubic, void* stream);

/* ---- LiftFeat (zoo entry liftfeat(sparse) = `feature: liftfeat` + NN-mutual; imcui/hloc/extractors/liftfeat.py) ------------ */
/* `models.liftfeat_wrapper.LiftFeat` (liftfeat.py:9, :27-31) is not part of the reference checkout (third_party is empty): the network is
 * restated from its description (tests/liftfeat_reference.py) and parity with upstream's code is NOT pinned ("LiftFeat:
 * what is pinned").  cfg [8] int32, read from the checkpoint's shapes and keys: {kenc present, FFN hidden width, denc hidden, nenc hidden
 * 1, nenc hidden 2, kenc hidden 1, kenc hidden 2, AFT layers}; first hidden widths and the FFN: multiples of 32 up to 128, second hidden
 * widths 32 or 64, 1 .. 8 layers; an unsupported cfg gives 0 / NULL / IMCUI_ERR_ARG.  Weight packing runs on the HOST (replaces the
 * checkpoint load of liftfeat.py:27): tensor i is the state-dict entry named imcui_hip_liftfeat_tensor_name(cfg, i): XFeat's trunk
 * without heatmap_head.*, normal_head.{0,1,2}.{conv,bn}.* and normal_head.3.*, feature_boost.*.  BatchNorm is folded in float32. */
size_t imcui_hip_liftfeat_packed_floats(const int* cfg);
int imcui_hip_liftfeat_num_tensors(const int* cfg);
const char* imcui_hip_liftfeat_tensor_name(const int* cfg, int i);
int imcui_hip_liftfeat_pack_weights(const int* cfg, const float* const* tensors, float* packed);
/* Scratch of imcui_hip_liftfeat_forward for B images of H x W (independent of the threshold, max_keypoints and kcap). */
size_t imcui_hip_liftfeat_workspace_bytes(int B, int H, int W);
/* Bound on the key-points of an image whose scores do not tie exactly (5x5 NMS over the padded map); a plateau can exceed it. */
int imcui_hip_liftfeat_max_keypoints_bound(int H, int W);
/* liftfeat.py:34-53 `_forward`: `self.net.extract(image)` (:37) and the wrapper's cut (:42-46).
 * image [dev, B,3,H,W] in [0,1] (the `* 255` of :35 and extract's `/ 255` are applied as two float32 roundings): zero-padded at the bottom
 * and right to Hp x Wp = multiples of 32, channel mean, InstanceNorm over the padded image, XFeat's trunk, the normal head, the lifting
 * network over all (Hp/8)(Wp/8) cells, then 5x5 NMS over the padded map (`==` max and > threshold), x < W and y < H, score = nearest
 * sample of the heat map, bicubic descriptors of the boosted map.  Order (:42-46): count <= max_keypoints: row-major; otherwise ascending
 * score (equal scores by row-major index: stable), the last max_keypoints entries (0: all; -k: all but the k lowest).
 * Outputs, fixed stride `kcap` per image, first num_keypoints[b] entries valid, the rest zero:
 *   keypoints [dev, B,kcap,2] (x, y);  scores [dev, B,kcap];  descriptors [dev, B,kcap,64] unit rows;  num_keypoints [dev, B] int32
 *   status [dev, 1] int32 optional: 0 = fine, bit 1 = more key-points than kcap
 *   kpt_heat [dev, B,Hp,Wp], normals [dev, B,Hp/8,Wp/8,192] (channel c * 64 + dy * 8 + dx), boosted [dev, B,Hp/8,Wp/8,64] optional
 * Zero key-points is a valid result.  No host synchronisation. */
int imcui_hip_liftfeat_forward(imcui_hip_t* h, const int* cfg, const float* packed, const float* image, int B, int C, int H, int W, float threshold,
                               int max_keypoints, int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status,
                               float* kpt_heat, float* normals, float* boosted, void* ws, size_t ws_bytes, void* stream);
/* Test entries (device pointers), each a stage of liftfeat.py:37 alone.  input_probe: image [B,3,H,W] -> gray [B,Hp,Wp], norm [B,2] =
 * (invstd, -mean * invstd); ws: B * cdiv(Hp Wp, 4096) * 16 bytes.  upconv_probe: up-conv stage 0 / 1 / 2 on x [B,hh,ww,cin] (NHWC) -> out
 * [B,2hh,2ww,cin/2], or with fused = 1 (stage 2, 2hh and 2ww multiples of 8) the unfolded unit normals [B,2hh/8,2ww/8,192].  booster_probe:
 * d [B,N,64], k [B,N,65], n [B,N,192] -> out [B,N,64] (unit rows), x_enc optional [B,N,64] = the encoders' sum.  aft_probe: AFT layer
 * `layer` on x [B,N,64] -> out, kv optional [B,64]; both with ws of imcui_hip_liftfeat_tokens_workspace_bytes.  select_probe: the selection
 * on heat [B,Hp,Wp] and boosted [B,Hp/8,Wp/8,64] (Hp, Wp multiples of 8), outputs as imcui_hip_liftfeat_forward. */
int imcui_hip_liftfeat_input_probe(imcui_hip_t* h, const float* image, int B, int H, int W, float* gray, float* norm, void* ws, size_t ws_bytes, void* stream);
int imcui_hip_liftfeat_upconv_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* x, int stage, int fused, int B, int hh, int ww,
                                    int align_corners, float slope, float* out, void* stream);
size_t imcui_hip_liftfeat_tokens_workspace_bytes(int B, int N);
int imcui_hip_liftfeat_booster_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* d, const float* k, const float* n, int B, int N,
                                     float* out, float* x_enc, void* ws, size_t ws_bytes, void* stream);
int imcui_hip_liftfeat_aft_probe(imcui_hip_t* h, const int* cfg, const float* packed, const float* x, int layer, int B, int N, float* out, float* kv, void* ws,
                                 size_t ws_bytes, void* stream);
size_t imcui_hip_liftfeat_select_workspace_bytes(int B, int Hp, int Wp);
int imcui_hip_liftfeat_select_probe(imcui_hip_t* h, const float* heat, const float* boosted, int B, int H, int W, int Hp, int Wp, float threshold,
                                    int max_keypoints, int kcap, float* keypoints, float* scores, float* descriptors, int* num_keypoints, int* status, void* ws,
                                    size_t ws_bytes, void* stream);

/* ---- LightGlue --------------------------------------------- */
/* Host-side packing of the upstream state dict (9 layers, dim 256, 4 heads).  `tensors` holds the
 * host pointers of imcui_hip_lightglue_num_tensors() tensors; tensor i is the upstream state-dict
 * entry named imcui_hip_lightglue_tensor_name(i) (posenc.Wr.weight, transformers.{l}.*,
 * log_assignment.{l}.*, token_confidence.{l}.token.0.*);
 * `packed` receives imcui_hip_lightglue_packed_floats() floats. */
size_t imcui_hip_lightglue_packed_floats(void);
int imcui_hip_lightglue_num_tensors(void);
const char* imcui_hip_lightglue_tensor_name(int i); /* upstream state-dict key of tensor i */
int imcui_hip_lightglue_pack_weights(const float* const* tensors, float* packed);
/* Variants of upstream's `features` table (imcui/hloc/configs/matchers.py:51-83,140-150: disk- / aliked- / raco- /
 * sift-lightglue).  Call after imcui_hip_lightglue_pack_weights on the same host buffer:
 *   wr [32][wr_cols]: posenc.Wr.weight, wr_cols = 2, or 4 with add_scale_ori (sift, doghardnet: (x, y, scale, orientation));
 *   w_input_proj [256][input_dim], b_input_proj [256]: `input_proj` when input_dim != 256 (128 for disk / aliked / sift);
 *   input_dim: descriptor size, a multiple of 32 and at most 256. */
int imcui_hip_lightglue_pack_input(const float* wr, int wr_cols, const float* w_input_proj, const float* b_input_proj, int input_dim,
                                   float* packed);

size_t imcui_hip_lightglue_workspace_bytes(int B, int ncap);

/* B pairs.  keypoints0/1 [dev, B,ncap,2] pixel (x,y); descriptors0/1 [dev, B,ncap,input_dim] (256 for SuperPoint);
 * scales0/1, oris0/1 [dev, B,ncap] or all NULL: only for weights with add_scale_ori (lightglue.py:62-73 passes them on);
 * n0/n1 [dev, B] int32 valid counts (<= ncap).  size0/size1: (W,H) of the images the key-points
 * live in (only used to normalise key-points, lightglue.py passes `image.shape`).
 * depth_confidence / width_confidence <= 0 disable early stopping / point pruning;
 * pruning_threshold: a side is pruned only while it holds MORE than this many points -- upstream's
 * pruning_keypoint_thresholds[device] (cpu / mps -1 = always, cuda 1024, flash 1536); -1 reproduces the
 * reference's PyTorch-CPU path, which is what the parity tests pin;
 * filter_threshold is conf["match_threshold"] (imcui/hloc/matchers/lightglue.py:50).  The three
 * thresholds are doubles because the reference compares fp32 tensors against Python floats
 * (e.g. `1 - width_confidence` is formed in double before the fp32 cast).
 * Outputs [dev]: matches0/1 [B,ncap] int32 (-1 = unmatched), matching_scores0/1 [B,ncap],
 * stop [B] int32 (layers run), prune0/1 [B,ncap] int32.  Entries >= n are -1 / 0. */
int imcui_hip_lightglue_forward(imcui_hip_t* h, const float* packed, int B, int ncap, int input_dim, const float* keypoints0,
                                const float* keypoints1, const float* descriptors0, const float* descriptors1,
                                const float* scales0, const float* oris0, const float* scales1, const float* oris1,
                                const int* n0, const int* n1, float w0, float h0, float w1, float h1,
                                double depth_confidence, double width_confidence, int pruning_threshold,
                                double filter_threshold, int* matches0, int* matches1, float* matching_scores0,
                                float* matching_scores1, int* stop, int* prune0, int* prune1, void* ws, size_t ws_bytes,
                                void* stream);
/* Parity-test hook (the oracle exposes the same intermediates): while `dump` [dev] is non-NULL every
 * imcui_hip_lightglue_forward on this handle copies the token states x [2B, R, 256] (R = roundup(ncap, 128),
 * row (2*pair + image)*R + i, rows in their current -- pruned -- order) after each of the 9 layers to
 * dump + layer * 2B*R*256; `floats` = capacity of `dump`.  NULL switches it off. */
int imcui_hip_lightglue_set_layer_dump(imcui_hip_t* h, float* dump, size_t floats);

/* ---- SuperGlue (imcui/hloc/matchers/superglue.py:42-43 `self.net(data)`) ---------- */
/* Host-side packing of the upstream state dict (Vincentqyw/SuperGluePretrainedNetwork models/superglue.py:
 * kenc.encoder.*, gnn.layers.{0..17}.{attn.proj.{0,1,2},attn.merge,mlp.{0,1,3}}, final_proj, bin_score).
 * `tensors` holds the host pointers of imcui_hip_superglue_num_tensors() tensors, tensor i being the state-dict entry
 * imcui_hip_superglue_tensor_name(i) (Conv1d weights [out,in,1] are passed as [out,in]).  Eval-mode BatchNorm and
 * attn.merge are folded into the neighbouring layers; heads are de-interleaved. */
size_t imcui_hip_superglue_packed_floats(void);
int imcui_hip_superglue_num_tensors(void);
const char* imcui_hip_superglue_tensor_name(int i);
int imcui_hip_superglue_pack_weights(const float* const* tensors, float* packed);
size_t imcui_hip_superglue_workspace_bytes(int B, int ncap);
/* B pairs.  keypoints0/1 [dev, B,ncap,2] pixel (x,y); scores0/1 [dev, B,ncap] detector scores; descriptors0/1
 * [dev, B,ncap,256] (row per key-point); n0/n1 [dev, B] int32 valid counts (<= ncap); (w0,h0)/(w1,h1): size of the
 * images (superglue.py passes `data["image0"].shape`, only used to normalise key-points).
 * sinkhorn_iterations / match_threshold = conf (superglue.py:17-18; configs/matchers.py:15-16,30-31).
 * Outputs [dev]: matches0/1 [B,ncap] int32 (-1 = unmatched), matching_scores0/1 [B,ncap]; a pair with an empty
 * image gets all -1 / 0 (upstream early return).  Entries >= n are -1 / 0. */
int imcui_hip_superglue_forward(imcui_hip_t* h, const float* packed, int B, int ncap, const float* keypoints0,
                                const float* keypoints1, const float* scores0, const float* scores1, const float* descriptors0,
                                const float* descriptors1, const int* n0, const int* n1, float w0, float h0, float w1, float h1,
                                int sinkhorn_iterations, double match_threshold, int* matches0, int* matches1,
                                float* matching_scores0, float* matching_scores1, void* ws, size_t ws_bytes, void* stream);

/* ---- IMP (`sfd2+imp`; imcui/hloc/matchers/imp.py:51 `self.net.produce_matches(data, p=0.2)`, pram.nets.gml.GML) ---------- */
/* The state dict in ONE table (csrc/imp.hip): imcui_hip_imp_num_tensors() entries, entry i named imcui_hip_imp_tensor_name(i)
 * with the shape imcui_hip_imp_tensor_shape(i, dims) (returns the number of dimensions, at most 3; 0 = scalar; -1 = bad index).
 * imp.py:41-44 loads exactly these names strictly.  Packing (imp.py:40-44 `GML(conf)` + `load_state_dict`): `tensors` holds the
 * host pointers in table order; eval-mode BatchNorm and attn.merge are folded into the neighbouring layers, heads are
 * de-interleaved, of the nine final projections only final_proj.8 is packed (inference reads no other). */
size_t imcui_hip_imp_packed_floats(void);
int imcui_hip_imp_num_tensors(void);
const char* imcui_hip_imp_tensor_name(int i);
int imcui_hip_imp_tensor_shape(int i, int* dims);
int imcui_hip_imp_pack_weights(const float* const* tensors, float* packed);
size_t imcui_hip_imp_workspace_bytes(int B, int ncap);
/* imp.py:51 for B pairs.  keypoints0/1 [dev, B,ncap,2] pixel (x,y); scores0/1 [dev, B,ncap]; descriptors0/1 [dev, B,ncap,128]
 * (row per key-point: what imp.py:48-49 hands over); n0/n1 [dev, B] int32 valid counts (<= ncap <= 4096); (w0,h0)/(w1,h1): image
 * sizes, used to normalise key-points only.  sinkhorn_iterations = conf (imp.py:19); match_threshold = the `p` of imp.py:51.
 * Outputs [dev]: matches0/1 [B,ncap] int32 (-1 = unmatched), matching_scores0/1 [B,ncap] (probabilities); a pair with an empty
 * side gets all -1 / 0, entries >= n are -1 / 0.  No host synchronisation; graph-capturable. */
int imcui_hip_imp_forward(imcui_hip_t* h, const float* packed, int B, int ncap, const float* keypoints0, const float* keypoints1,
                          const float* scores0, const float* scores1, const float* descriptors0, const float* descriptors1,
                          const int* n0, const int* n1, float w0, float h0, float w1, float h1, int sinkhorn_iterations,
                          double match_threshold, int* matches0, int* matches1, float* matching_scores0, float* matching_scores1,
                          void* ws, size_t ws_bytes, void* stream);
/* Test hook: the assignment stage of imp.py:51 alone (dust-bin soft-max, `iterations` probability-domain Sinkhorn rounds, mutual
 * arg-max, strict threshold `p`) on given scores [dev, B,ncap,ncap] (pair b uses its top-left n0[b] x n1[b]).  u / v [dev, B,ncap+1]
 * (may be NULL): the row / column scalings, entry n0[b] / n1[b] = the dust-bin's.  Workspace: imcui_hip_imp_workspace_bytes. */
int imcui_hip_imp_ot_probe(imcui_hip_t* h, const float* scores, int B, int ncap, const int* n0, const int* n1, float bin_score,
                           int iterations, double p, int* matches0, int* matches1, float* matching_scores0, float* matching_scores1,
                           float* u, float* v, void* ws, size_t ws_bytes, void* stream);

/* ---- AdaLAM (`adalam`; imcui/hloc/matchers/adalam.py:46-57 `self.adalam.match_and_filter(...)`, kornia.feature.adalam.AdalamFilter) ---- */
/* No weights.  The rule (stages A .. G) is stated in INTEGRATION.md, "AdaLAM: what is pinned"; csrc/adalam.hip.
 * conf [host, 10 doubles], the keys of adalam.py:10-21 in this order: area_ratio, search_expansion, ransac_iters, min_inliers,
 * min_confidence, orientation_difference_threshold, scale_rate_threshold, detected_scale_rate_threshold, refit, force_seed_mnn;
 * a threshold that is None in Python is passed as a negative number; the two flags as 0 / 1.  It is read during the call.
 * D = 0: the workspace of imcui_hip_adalam_filter. */
size_t imcui_hip_adalam_workspace_bytes(imcui_hip_t* h, int B, int ncap, int D);
/* adalam.py:39-68 for B pairs.  descriptors0/1 [dev, B,ncap,D] (row per key-point, not assumed normalised; D = 64, 128 or 256,
 * another width is IMCUI_HIP_ERR_UNSUPPORTED); keypoints0/1 [dev, B,ncap,2] pixel (x,y); scales0/1, oris0/1 [dev, B,ncap] (oris in
 * degrees; a pair of them may be NULL while its threshold is off, otherwise IMCUI_HIP_ERR_ARG); n0/n1 [dev, B] int32 valid counts
 * (<= ncap <= 4096); (h0,w0)/(h1,w1): image sizes (adalam.py:51-52).  Outputs [dev]: matches0 [B,ncap] int32 (-1 = unmatched;
 * a pair with fewer than two key-points on a side is all -1, adalam.py:41-44), matching_scores0 [B,ncap] (zeros, adalam.py:67).
 * Optional outputs (NULL allowed): nn / score / mnn [B,ncap] (nearest neighbour, ratio of the squared distances, mutual flag),
 * seed [B,ncap] int32 (1 = key-point is a seed), and per seed slot (= the seed's key-point index) seed_members [B,ncap,ncap] int32
 * (the first seed_info[.,.,0] entries of a slot: its members in (score, index) order), seed_info [B,ncap,4] int32 {members, best
 * iteration or -1, accepted count, passed}, seed_conf [B,ncap].  No host synchronisation; graph-capturable; the same input gives
 * the same bits alone, in a batch and under replay. */
int imcui_hip_adalam_forward(imcui_hip_t* h, int B, int ncap, int D, const float* descriptors0, const float* descriptors1,
                             const float* keypoints0, const float* keypoints1, const float* scales0, const float* scales1,
                             const float* oris0, const float* oris1, const int* n0, const int* n1, int h0, int w0, int h1, int w1,
                             const double* conf, int* matches0, float* matching_scores0, int* nn, float* score, int* mnn, int* seed,
                             int* seed_members, int* seed_info, float* seed_conf, void* ws, size_t ws_bytes, void* stream);
/* kornia's `AdalamFilter.filter_matches`: the same from given nn / score / mnn [dev, B,ncap] (an nn outside [0, n1) takes its
 * key-point out of every stage).  Doubles as the probe of stages B .. G. */
int imcui_hip_adalam_filter(imcui_hip_t* h, int B, int ncap, const float* keypoints0, const float* keypoints1, const float* scales0,
                            const float* scales1, const float* oris0, const float* oris1, const int* n0, const int* n1, int h0, int w0,
                            int h1, int w1, const double* conf, const int* nn, const float* score, const int* mnn, int* matches0,
                            float* matching_scores0, int* seed, int* seed_members, int* seed_info, float* seed_conf, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- LoFTR (kornia.feature.LoFTR behind imcui/hloc/matchers/loftr.py:54) ---- */
/* Host-side packing.  Every convolution / Linear is one layer W[N][K] (+ bias[N], may be NULL) in GEMM
 * layout: imcui_hip_loftr_num_layers() layers of imcui_hip_loftr_layer_shape(i); convolutions as
 * [Cout][tap][Cin] with BatchNorm folded and the 196-channel stage zero-padded to 256 channels (the
 * Python host layer imcui_hip/backend.py:pack_loftr builds them from the kornia state dict).
 * conv1_w [49][128] / conv1_b [128]: the first 7x7 convolution (BN folded).  norms: LayerNorm weight /
 * bias vectors, imcui_hip_loftr_num_norms() of imcui_hip_loftr_norm_dim(i) floats. */
size_t imcui_hip_loftr_packed_floats(void);
int imcui_hip_loftr_num_layers(void);
int imcui_hip_loftr_layer_shape(int i, int* N, int* K);
int imcui_hip_loftr_num_norms(void);
int imcui_hip_loftr_norm_dim(int i);
int imcui_hip_loftr_pack_weights(const float* conv1_w, const float* conv1_b, const float* const* w, const float* const* b,
                                 const float* const* norms, float* packed);
size_t imcui_hip_loftr_workspace_bytes(int B, int H0, int W0, int H1, int W1);
/* kornia LoFTR.forward on B pairs: image0 [dev, B,1,H0,W0], image1 [dev, B,1,H1,W1] (multiples of 8, >= 32; the two
 * sizes may differ -- `minima_loftr` keeps each image's aspect ratio, configs/matchers.py:283 -- kornia then runs the
 * backbone per image instead of on the concatenated batch, which gives the same values).
 * Outputs with capacity B*(H0/8)*(W0/8) rows, first num_matches[0] valid, ordered like torch.where
 * (batch-major, coarse cell of image0 ascending): keypoints0/1 [dev, cap,2] pixel (x,y),
 * confidence [dev, cap], batch_indexes [dev, cap] int32, num_matches [dev, 1] int32.
 * match_threshold = conf["match_threshold"] (loftr.py:23); temp_bug_fix = 1 only for MINIMA weights (:28). */
int imcui_hip_loftr_forward(imcui_hip_t* h, const float* packed, const float* image0, const float* image1, int B, int H0,
                            int W0, int H1, int W1, double match_threshold, int temp_bug_fix, float* keypoints0,
                            float* keypoints1, float* confidence, int* batch_indexes, int* num_matches, void* ws,
                            size_t ws_bytes, void* stream);

/* The last FPN stage (1/2 resolution: layer1_outconv + layer1_outconv2, kornia ResNetFPN_8_2 behind loftr.py:54) produces the fine map that is
 * only ever read through the 5x5 windows of the matched cells.  Option "loftr_fine_sparse" (imcui_hip_set_option; default 1): the stage is
 * deferred until the matches are known and evaluated on those windows alone when that is cheaper than the dense maps -- for that decision
 * imcui_hip_loftr_forward reads the 4-byte match count back and SYNCHRONISES THE STREAM ONCE per call (not while the stream is being captured
 * into a graph: dense then); 2 = always on the windows, 0 = dense maps, no read-back (the call does not synchronise).  Same matches either way;
 * window features agree to round-off (tests/test_gpu_loftr.py).  Returns how the last forward on this handle did it: 0 dense, 1 windows;
 * *matches (may be NULL) = the count it read back, -1 without a read-back. */
int imcui_hip_loftr_last_fine_mode(imcui_hip_t* h, int* matches);

/* byte offset inside the LoFTR workspace of: 0 coarse features after the transformer [B*L0 + B*L1, 256] (side 0 first),
 * 1 fine features [B*H0/2*W0/2 + B*H1/2*W1/2, 128], 2 sim [B,L0,L1], 3 fine windows [2,B*L0,25,128]  (parity tests) */
size_t imcui_hip_loftr_debug_offset(int which, int B, int H0, int W0, int H1, int W1);

/* ---- EfficientLoFTR (upstream zju3dv/EfficientLoFTR `LoFTR` behind
 * imcui/hloc/matchers/eloftr.py:79, 'full' model, fp32) ------------------------------------------------------ */
/* Host-side packing, as for LoFTR: imcui_hip_eloftr_num_layers() layers W[N][K] (+ bias, may be NULL) of
 * imcui_hip_eloftr_layer_shape(i) in GEMM layout -- 20 re-parameterised RepVGG blocks ([Cout][tap][Cin]; 3x3 + 1x1 +
 * identity branches and their BatchNorms folded, what the reference's `reparameter()` does, eloftr.py:61), 8 attention
 * blocks x {q, k, v, o, fc1, fc2}, 7 fine-fusion convolutions (BatchNorm folded, the 1/16 coarse-feature scale folded
 * into the first) -- built from the state dict by imcui_hip/backend.py:pack_eloftr.  conv0_w [9][64] / conv0_b [64]: the
 * first block (1 -> 64, stride 2).  dw: 8 depth-wise 4x4 query-aggregation kernels [256][16] (block = layer * 2 +
 * {self, cross}).  norms: 32 vectors of 256 (per block: aggregation norm w, b; mlp LayerNorm w, b).  inv_freq [64]:
 * rotary frequencies 1 / 10000^(2t/128). */
size_t imcui_hip_eloftr_packed_floats(void);
int imcui_hip_eloftr_num_layers(void);
int imcui_hip_eloftr_layer_shape(int i, int* N, int* K);
int imcui_hip_eloftr_pack_weights(const float* conv0_w, const float* conv0_b, const float* const* w, const float* const* b,
                                  const float* const* dw, const float* const* norms, const float* inv_freq, float* packed);
size_t imcui_hip_eloftr_workspace_bytes(int B, int H0, int W0, int H1, int W1, int debug_windows);
/* Upstream LoFTR.forward on B pairs: image0 [dev, B,1,H0,W0], image1 [dev, B,1,H1,W1] (multiples of 32, >= 64; the UI path
 * resizes both images to width x height, configs/matchers.py:296-303, the batch path of match_dense.py does not, so the two
 * sizes may differ: the backbone then runs side by side and the attention is between token sets of different length).
 * Outputs with capacity B*(H0/8)*(W0/8) rows, first num_matches[0] valid, ordered batch-major by the coarse cell of image0: keypoints0/1
 * [dev, cap,2] pixel (x,y) after the two-stage fine refinement, confidence [dev, cap], batch_indexes [dev, cap] int32,
 * num_matches [dev, 1] int32.  match_threshold = conf["match_threshold"] (eloftr.py:54).  debug_windows != 0 also
 * writes the unfolded fine windows to the workspace (parity tests; size it with the same flag). */
int imcui_hip_eloftr_forward(imcui_hip_t* h, const float* packed, const float* image0, const float* image1, int B, int H0, int W0,
                             int H1, int W1, double match_threshold, float* keypoints0, float* keypoints1, float* confidence,
                             int* batch_indexes, int* num_matches, int debug_windows, void* ws, size_t ws_bytes, void* stream);
/* The same with the arithmetic of the reference wrapper's `precision` switch (imcui/hloc/matchers/eloftr.py:32-33,43-47,63-64):
 * arith 0 = the call above ("fp32": 3 x f16 split products, fp32-grade); arith 1 = "fp16" / "mp": one f16 product per element pair
 * (f32 accumulate) in the backbone and fine-fusion convolutions, everything that decides a match in the split arithmetic. */
int imcui_hip_eloftr_forward_ex(imcui_hip_t* h, const float* packed, const float* image0, const float* image1, int B, int H0, int W0,
                                int H1, int W1, double match_threshold, int arith, float* keypoints0, float* keypoints1,
                                float* confidence, int* batch_indexes, int* num_matches, int debug_windows, void* ws, size_t ws_bytes,
                                void* stream);
/* byte offset inside the workspace of (per-image buffers: the B maps of image 0, then the B maps of image 1): 0 backbone 1/2
 * features [.,H/2,W/2,64], 1 1/4 features [.,H/4,W/4,128], 2 coarse features after the transformer [.,L,256], 3 sim [B,L0,L1],
 * 4 fused 1/2-resolution fine map [.,H/2,W/2,64], 5 fine windows [B*L0][64 + 100][64] (debug_windows)  (parity tests) */
size_t imcui_hip_eloftr_debug_offset(int which, int B, int H0, int W0, int H1, int W1);

/* ---- nearest neighbour by dot product (the primitive of MASt3R's `fast_reciprocal_NNs(..., dist="dot")`,
 * imcui/hloc/matchers/mast3r.py:68-75 -> upstream mast3r/fast_nn.py `cdistMatcher.query`) --------------------------------- */
/* idx [dev, Q] int32 = FIRST arg-max over n of <queries[q], db[n]>, best [dev, Q] (may be NULL) the maximum; queries [dev, Q,D], db [dev,
 * N,D] f32 rows, D in {16, 24, 32}.  Exact-f32 MFMA, similarity and running arg-max fused (no Q x N matrix). */
size_t imcui_hip_nn_argmax_workspace_bytes(int Q, int N);
int imcui_hip_nn_argmax_f32(imcui_hip_t* h, const float* queries, const float* db, int Q, int N, int D, int* idx, float* best, void* ws,
                            size_t ws_bytes, void* stream);
/* The same search in the 3 x f16 split arithmetic (rows scaled by 2^8, split into f16 hi / lo planes, three products per pair,
 * f32 accumulate; D <= 32): a quarter of the matrix cycles.  fp32-grade values, but not the exact-f32 instruction's fmaf chain:
 * between candidates closer than ~3e-7 the arg-max may differ from imcui_hip_nn_argmax_f32's (opt-in, conf "matcher_arithmetic"). */
size_t imcui_hip_nn_argmax_split_workspace_bytes(int Q, int N);
int imcui_hip_nn_argmax_split_f32(imcui_hip_t* h, const float* queries, const float* db, int Q, int N, int D, int* idx, float* best, void* ws,
                                  size_t ws_bytes, void* stream);

/* ---- DUSt3R pair network (BASELINE config 5; what `dust3r.inference.inference(pairs, self.net, ...)`
 * computes at imcui/hloc/matchers/duster.py:73 with self.net = AsymmetricCroCo3DStereo (duster.py:37): ViT encoder with 2-D rotary
 * embedding, two-stream cross-attention decoder, DPT point-map head; the un-vendored `third_party/dust3r` submodule) -------- */
/* The architecture is given by (enc_dim, enc_depth, dec_dim, dec_depth): 1024, 24, 768, 12 for `duster_vit_large.pth`; dims are
 * multiples of 64 (head_dim 64) up to 1024, dec_depth a multiple of 4 (DPT hooks at 0, dec_depth/2, 3 dec_depth/4, dec_depth).
 * Host-side packing: imcui_hip_dust3r_num_layers() matrices W[N][K] of imcui_hip_dust3r_layer_shape(i) (+ bias [N] or NULL):
 * patch_embed.proj as [E][3*16*16]; per encoder block qkv, proj, fc1, fc2; decoder_embed; per decoder block of dec_blocks then
 * dec_blocks2: qkv, proj, cross projq, [projk ; projv], cross proj, fc1, fc2; per head (downstream_head1, 2): act_postprocess
 * 1x1 convolutions, the kernel = stride transposed convolutions as [(dy, dx, cout)][cin] with the bias tiled, the 3x3
 * convolutions in implicit-GEMM order [cout][tap][cin] (act_postprocess.3.1, layer_rn, refinenet 4..1 residual units + out_conv,
 * head.0, head.2).  imcui_hip_dust3r_num_vectors() f32 vectors of imcui_hip_dust3r_vector_len(i): the LayerNorm weights / biases in
 * module order, head.4 weight [4][128] and bias [4] per head, the 16 rotary frequencies 100^(-i/16).  Built from the upstream
 * state dict by imcui_hip/backend.py:pack_dust3r.  CONTRACT since round 3: the q / k / v projections (attn.qkv, cross_attn.projq,
 * [projk ; projv]) and mlp.fc1 are handed over with the affine part of the LayerNorm in front of them folded in -- W * gamma (per input
 * column) and b + W beta for norm1 / norm2 / norm_y / norm3 -- because the device normalises those inputs WITHOUT gamma / beta (one
 * pass serves several consumers); their LayerNorm vectors are still passed (layout unchanged) and ignored.  enc_norm and dec_norm
 * are applied as they are. */
/* desc_dim: 0 = DUSt3R; > 0 = MASt3R (`AsymmetricMASt3R`, imcui/hloc/matchers/mast3r.py:41 with the 'catmlp+dpt' head of
 * `MASt3R_ViTLarge_BaseDecoder_512_catmlpdpt_metric.pth`, desc_dim = 24): two more matrices per head, head_local_features.fc1
 * [4 (E + D)][E + D] and .fc2 [(desc_dim + 1) * 256][4 (E + D)], after head.2. */
size_t imcui_hip_dust3r_packed_floats(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim);
int imcui_hip_dust3r_num_layers(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim);
int imcui_hip_dust3r_num_vectors(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim);
int imcui_hip_dust3r_layer_shape(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, int i, int* N, int* K);
int imcui_hip_dust3r_vector_len(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, int i);
/* float offsets of layer i inside the packed buffer (inspection / tests): bias, f16 hi / lo planes, 2^-e scale; kind 0 = fragment-major
 * GEMM planes, 1 = 3x3 convolution planes */
int imcui_hip_dust3r_layer_offsets(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, int i, size_t* bias, size_t* plane_hi,
                                   size_t* plane_lo, size_t* scale, int* kind);
int imcui_hip_dust3r_pack_weights(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, const float* const* w,
                                  const float* const* b, const float* const* vec, float* packed);
/* Format of the packed buffer (round 4).  Its CONTENT is a contract with the packer: the LayerNorm gamma / beta of every block must
 * already be folded into the matrices that consume the normalised rows (qkv, the cross-attention projections, fc1: what
 * imcui_hip/backend.py:dust3r_matrices does before it calls imcui_hip_dust3r_pack_weights) -- the device only normalises -- and the
 * row sums of the folded matrices sit behind the vectors.  The buffer ends in a 64-word trailer (magic 'IMDU', format number, total
 * size, the five configuration integers).  `packed_floats` of the forward entry points = the size of the caller's buffer: anything but
 * imcui_hip_dust3r_packed_floats() of the configuration is refused with IMCUI_HIP_ERR_ARG (a blob cached from an older library would
 * otherwise run with its affine parts dropped and return plausible but wrong point maps); imcui_hip_dust3r_check_packed verifies
 * size AND trailer of a HOST copy (0 = fine) -- call it once when a cached blob is loaded. */
int imcui_hip_dust3r_format_version(void);
int imcui_hip_dust3r_check_packed(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, const float* packed_host, size_t packed_floats);
size_t imcui_hip_dust3r_workspace_bytes(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, int NI, int P, int H, int W);
size_t imcui_hip_dust3r_dump_floats(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, int NI, int P, int H, int W);
/* `AsymmetricCroCo3DStereo.forward(view1, view2)` for P directed pairs over NI images: images [dev, NI,3,H,W] in [0,1] (the
 * wrapper's mean = std = 0.5 normalisation, duster.py:60-64, is applied inside), H and W multiples of 16 (the patch size); pairs [dev, P,2] int32 =
 * (view-1 image, view-2 image) -- duster.py:70-72 asks for (1,0) then (0,1) (`make_pairs`' order).  Every image is encoded once.  Outputs, view-major:
 * pts3d [dev, 2,P,H,W,3] (view 1: `pts3d`; view 2: `pts3d_in_other_view`, i.e. in view 1's frame), conf [dev, 2,P,H,W]; with
 * desc_dim > 0 also desc [dev, 2,P,H,W,desc_dim] (unit-norm local descriptors: MLP on [encoder | decoder] tokens, pixel shuffle
 * 16, `desc / |desc|`) and desc_conf [dev, 2,P,H,W] = exp(.) (mast3r.py:61-64 reads `pred1["desc"]`, `pred2["desc"]`); NULL otherwise.
 * dump (may be NULL; parity tests): imcui_hip_dust3r_dump_floats() floats of intermediate token states and head maps.
 * arith: 0 = 3 x f16 split products (fp32-grade results, the parity mode), 1 = one f16 product per element pair in the GEMMs and
 * convolutions with f32 accumulation (the class of the bf16 run the reference's configuration names; since round 3 attention too: hi planes of Q / K / V, P rounded to f16).
 * The handle must be in the split mode (IMCUI_ERR_UNSUPPORTED in precision 0). */
int imcui_hip_dust3r_forward(imcui_hip_t* h, int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, const float* packed,
                             size_t packed_floats, const float* images, int NI, int H, int W, const int* pairs, int P, int arith, float* pts3d, float* conf,
                             float* desc, float* desc_conf, float* dump, size_t dump_floats, void* ws, size_t ws_bytes, void* stream);

/* The same network on images of SEVERAL sizes.  imcui/hloc/match_dense.py:match_images and ImagePairDataset.preprocess resize
 * each image of a pair on its own (resize_max 512, dfactor 16), so two photos of different aspect ratio reach duster.py:73 at two
 * sizes; upstream's `inference` then encodes the two views separately and runs one pair per batch (dust3r/inference.py).
 * sizes [host, NI,2] = (H, W) of every image, multiples of 16, at most 4 distinct sizes per call; images [dev]: the NI images
 * [3,H_i,W_i] one behind the other; pairs_host [host, P,2] and pairs [dev, P,2]: the same table twice (the host copy lays out the
 * sequences, the device copy drives the gathers).  Outputs are ragged, map after map in (view, pair) order: the map of
 * (view v, pair p) has the size of image pairs[p][v] and starts at pixel map_pixel_offsets[v P + p] -- pts3d at 3 x that offset,
 * conf at it, desc at desc_dim x it; map_pixel_offsets [host, 2 P + 1] (may be NULL) is filled by the call, the last entry is the
 * total number of pixels the output buffers must hold.  With one size this is exactly imcui_hip_dust3r_forward's layout.
 * dump (may be NULL): imcui_hip_dust3r_token_dump_floats() floats -- the token states only ((enc_depth + 2) x [NI,R,E], (dec_depth + 2) x
 * [2P,R,D], R = tokens of the largest image rounded up to 128; rows past a sequence's own token count are undefined). */
size_t imcui_hip_dust3r_workspace_bytes_sizes(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, int NI, const int* sizes, int P);
size_t imcui_hip_dust3r_token_dump_floats(int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, int NI, const int* sizes, int P);
int imcui_hip_dust3r_forward_sizes(imcui_hip_t* h, int enc_dim, int enc_depth, int dec_dim, int dec_depth, int desc_dim, const float* packed,
                                   size_t packed_floats, const float* images, int NI, const int* sizes, const int* pairs_host, const int* pairs, int P, int arith,
                                   float* pts3d, float* conf, float* desc, float* desc_conf, size_t* map_pixel_offsets, float* dump,
                                   size_t dump_floats, void* ws, size_t ws_bytes, void* stream);

/* ---- baseline-JPEG decode (the step before the path) ----------------------------------------------
 * imcui/hloc/utils/io.py:11-21 `read_image` = cv2.imread(IMREAD_GRAYSCALE | IMREAD_COLOR), called per image by
 * imcui/hloc/extract_features.py:120-156 and match_dense.py.  Split where the format splits (csrc/jpeg.hip): the Huffman bit stream is
 * decoded on HOST threads (imcui_hip_jpeg_info / _entropy_decode: re-entrant, no state, no handle), dequantisation + 8x8 inverse DCT +
 * chroma up-sampling + YCbCr -> RGB run on the DEVICE (imcui_hip_jpeg_reconstruct).  The device arithmetic restates libjpeg's default
 * path (jpeg_idct_islow, fancy up-sampling, ycc_rgb_convert) integer for integer: outputs equal PIL's / cv2's decode BIT FOR BIT
 * (oracle/jpeg.py is pinned to PIL on every JPEG of the reference repository).
 * info [host, 24 ints]: 0 width, 1 height, 2 components (1 | 3), 3 hmax, 4 vmax, 5 MCUs per row, 6 MCU rows, 7 restart interval,
 * 8 EXIF orientation (1 = upright or absent; 2..8: imcui_hip_orient_u8 after the reconstruction), 9 + 4c .. 11 + 4c: h, v, quantisation
 * table of component c.  Supported: SOF0 / SOF1 Huffman, 8 bit, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, restart intervals,
 * interleaved or per-component scans, and -- round 5 -- progressive Huffman frames (SOF2: every scan up to EOI is accumulated into the same
 * coefficient planes); everything else (arithmetic coding, CMYK, 12 bit, 4:4:0) returns IMCUI_HIP_ERR_UNSUPPORTED. */
int imcui_hip_jpeg_info(const unsigned char* data, size_t n, int* info);
/* number of int16 coefficients of all components (every component padded to whole MCUs) */
size_t imcui_hip_jpeg_coef_count(const int* info);
/* coef [host, imcui_hip_jpeg_coef_count() int16]: quantised DCT coefficients in natural order, [component][block row][block column][64];
 * qt [host, 3 x 64 uint16]: the quantisation table of every component, natural order */
int imcui_hip_jpeg_entropy_decode(const unsigned char* data, size_t n, short* coef, unsigned short* qt);
/* `count` files on `threads` host threads OF THE LIBRARY (no interpreter lock, no per-file allocation): planes [3 * count] = where
 * component c of file i goes (planes[3 i + c]; unused components may be NULL) -- typically slices of one pinned staging buffer laid out
 * plane-major, so the luma coefficients of a batch cross PCIe in one transfer; qt [count][3 * 64]; status [count] per-file codes */
int imcui_hip_jpeg_entropy_decode_batch(const unsigned char* const* data, const size_t* sizes, int count, short* const* planes, unsigned short* qt,
                                        int* status, int threads);
size_t imcui_hip_jpeg_workspace_bytes(const int* info, int gray);
size_t imcui_hip_jpeg_workspace_bytes_batch(const int* info, int gray, int n);
/* n files of ONE geometry (equal info records) in three launches: coef_y / coef_cb / coef_cr [dev, n x plane coefficients] (chroma may be
 * NULL for gray output / one-component files), qt [dev, n x 192], out [dev]: [n,H,W] uint8 (gray) or [n,H,W,3] */
/* EXIF orientation 1..8 applied to a decoded image (cv2.imread does this inside the decoder): src [dev, H,W,C] uint8 -> dst [dev, H*W*C
 * bytes] = [H,W,C] for 1..4, [W,H,C] for 5..8 (5 transpose, 6 rotate 90 clockwise, 7 transverse, 8 rotate 90 counter-clockwise) */
int imcui_hip_orient_u8(imcui_hip_t* h, const unsigned char* src, int H, int W, int C, int orientation, unsigned char* dst, void* stream);
int imcui_hip_jpeg_reconstruct_batch(imcui_hip_t* h, const short* coef_y, const short* coef_cb, const short* coef_cr, const unsigned short* qt, const int* info,
                                     int n, int gray, unsigned char* out, void* ws, size_t ws_bytes, void* stream);
/* coef / qt [dev]: copies of the two buffers above; info [host]; out [dev]: gray != 0 -> [H][W] uint8 = the luma plane (what
 * cv2.IMREAD_GRAYSCALE returns for a YCbCr file), else [H][W][3] RGB (a one-component file replicated, as IMREAD_COLOR does) */
int imcui_hip_jpeg_reconstruct(imcui_hip_t* h, const short* coef, const unsigned short* qt, const int* info, int gray, unsigned char* out,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- batched geometric verification (the step after the path) ------------------------------------------------
 * imcui/ui/utils.py:424-456 `proc_ransac_matches` (cv2.findHomography / findFundamentalMat per pair on the host, called twice per pair by
 * `compute_geometry` :532-610).  An ADDITIONAL method for the reference's `ransac_zoo` ("HIP_RANSAC"), not a re-implementation of cv2's
 * USAC samplers: plain RANSAC with local optimisation for B pairs at once, every step specified in csrc/geometry.hip and restated on the
 * CPU in oracle/geometry.py (parity unpinned with respect to cv2).
 * pts0 / pts1 [dev, B,N,2] float32 matched key-points in pixels (row i of pair b is one correspondence), counts [dev, B] valid rows;
 * geometry 0 = homography (x1 ~ H x0, forward transfer error), 1 = fundamental matrix (x1^T F x0 = 0, Sampson error);
 * reproj_threshold [px], confidence, max_iter as in the reference's call (at most 16384 hypotheses are drawn), seed: the sampler is a
 * counter-based generator, results are a pure function of (inputs, seed).
 * model [dev, B,9] float64 row-major (H with h33 = 1; F with unit Frobenius norm), mask [dev, B,N] uint8 inliers, info [dev, B,4] int32 =
 * (inliers, hypotheses consumed by the sequential stopping rule, index of the winning hypothesis, ok). */
size_t imcui_hip_ransac_workspace_bytes(int B, int N, int max_iter);
int imcui_hip_ransac(imcui_hip_t* h, const float* pts0, const float* pts1, const int* counts, int B, int N, int geometry, double reproj_threshold,
                     double confidence, int max_iter, unsigned long long seed, double* model, unsigned char* mask, int* info, void* ws, size_t ws_bytes,
                     void* stream);

/* ---- mutual nearest neighbour (row a12) --------------------------------------------------- */
/* Round 5: descriptors of width 64 / 128 / 256 (SIFT, DISK, SuperPoint ...) run on the persistent similarity-and-reduce kernel
 * (csrc/simred.hip) in EITHER arithmetic: both sets are packed once into matrix-core fragments (4 bytes per element), a workgroup keeps
 * 128 descriptors of image 0 in registers and streams image 1 past them; per row (best, index, second best) live in registers, per
 * column and 128-row block 12 bytes go to memory.  The similarity matrix never exists.  Other widths keep the round-4 paths: the tile
 * GEMM with the reducing epilogue (3 x f16 split) or the materialised B x N x M matrix (exact f32: 4 B N M bytes).
 * Workspace: ..._bytes(B, N, M) serves every path (sized for D <= 256); ..._bytes_for(h, ...) what THIS handle needs for D <= 256;
 * ..._bytes_d(h, ..., D) what this handle needs for descriptors of width D. */
size_t imcui_hip_mutual_nn_workspace_bytes(int B, int N, int M);
size_t imcui_hip_mutual_nn_workspace_bytes_for(imcui_hip_t* h, int B, int N, int M);
size_t imcui_hip_mutual_nn_workspace_bytes_d(imcui_hip_t* h, int B, int N, int M, int D);
/* desc0 [dev, B,N,D], desc1 [dev, B,M,D] row per descriptor (D % 32 == 0); ratio_threshold /
 * distance_threshold <= 0 mean "None"; matches0 [dev, B,N] int32, scores0 [dev, B,N]. */
int imcui_hip_mutual_nn(imcui_hip_t* h, const float* desc0, const float* desc1, int B, int N, int M, int D,
                        double ratio_threshold, double distance_threshold, int do_mutual_check, int* matches0,
                        float* scores0, void* ws, size_t ws_bytes, void* stream);
/* The same matcher on the layout `NearestNeighbor._forward` receives (nearest_neighbor.py:38-66): descriptors0 [dev, B,D,N], descriptors1
 * [dev, B,D,M], one column per descriptor.  D = 64 / 128 / 256: the fragment packer reads that layout directly (no transposed copy);
 * other widths: transposed on the device into the workspace (tiled through LDS), then the call above. */
size_t imcui_hip_mutual_nn_dn_workspace_bytes_for(imcui_hip_t* h, int B, int N, int M, int D);
int imcui_hip_mutual_nn_dn(imcui_hip_t* h, const float* desc0_dn, const float* desc1_dm, int B, int N, int M, int D, double ratio_threshold,
                           double distance_threshold, int do_mutual_check, int* matches0, float* scores0, void* ws, size_t ws_bytes, void* stream);

/* ---- PNG decode (row f-3; `read_image` = cv2.imread, imcui/hloc/utils/io.py:11-21; the reference's WxBS / EVD fixtures are PNG) ----
 * Host: chunk walk + zlib inflate of the IDAT stream into the FILTERED scan lines (re-entrant; the batch call runs on the library's own host
 * threads into caller-provided, typically pinned, staging).  Device: the scan-line filters undone as a wavefront (one workgroup per image,
 * one thread per row) and the pixels written as the host reader returns them: [H][W] for gray / gray + alpha files, [H][W][3] RGB for RGB /
 * RGBA / palette files (alpha dropped).  Bit-exact (checker: PIL).  8-bit, non-interlaced files; everything else: IMCUI_HIP_ERR_UNSUPPORTED
 * (the caller keeps its host reader).  info: 8 ints = width, height, colour type, samples per pixel, decoded channels (1 | 3), bytes per
 * pixel, palette entries, 0. */
int imcui_hip_png_info(const unsigned char* data, size_t n, int* info);
size_t imcui_hip_png_raw_bytes(const int* info);
int imcui_hip_png_inflate(const unsigned char* data, size_t n, unsigned char* raw, size_t raw_bytes, unsigned char* palette);
int imcui_hip_png_inflate_batch(const unsigned char* const* data, const size_t* sizes, int count, unsigned char* const* raw, const size_t* raw_bytes,
                                unsigned char* palettes, int* status, int threads);
size_t imcui_hip_png_workspace_bytes(const int* infos, int count);
/* raw [dev] + raw_offsets [host]: scan lines of file i at raw + raw_offsets[i]; infos [host, count x 8]; palettes [dev, count x 768] or NULL;
 * out [dev] + out_offsets [host]: the decoded image of file i. */
int imcui_hip_png_reconstruct_batch(imcui_hip_t* h, const unsigned char* raw, const size_t* raw_offsets, const int* infos, const unsigned char* palettes, int count,
                                    unsigned char* out, const size_t* out_offsets, void* ws, size_t ws_bytes, void* stream);

/* ---- test hook: ONE launch of the similarity-and-reduce kernel (csrc/simred.hip) on raw matrices (tests/test_gpu_simred.py) ----
 * sim[b] = alpha * A[b] . Bm[b]^T is reduced, never stored.  A [dev, batch,M,K], Bm [dev, batch,N,K] f32, K in {64, 128, 256}; mcnt / ncnt
 * [dev, batch] live rows / columns per batch or NULL.  mode 0: nearest neighbours (best, first index, second best); 1: soft-max statistics
 * (max, sum exp); 2: dual-softmax confidence, row best + first column, column best (needs rmax / rsum / cmax / csum, optional tile flags
 * [batch][ceil(M/128)][ceil(N/128)]); 3: LightGlue's log assignment, row best + first column, column best + first row (rsum / csum = LOG
 * sums, l0 [batch,M], l1 [batch,N]); 4: mode 0 without the second best (r1 / c1 untouched: find_nn without a ratio test).  alpha > 0, and 1
 * for the nearest-neighbour modes.  Row outputs r0 / r1 / ri [batch][nchunk][M] (nchunk 0: imcui_hip_simred_chunks), column outputs
 * c0 / c1 / ci [batch][ceil(M/128)][N]. */
int imcui_hip_simred_chunks(int batch, int M, int N);
size_t imcui_hip_simred_debug_workspace_bytes(int batch, int M, int N, int K);
int imcui_hip_simred_debug(imcui_hip_t* h, int mode, const float* A, const float* Bm, int batch, int M, int N, int K, const int* mcnt, const int* ncnt, float alpha,
                           int nchunk, float* r0, float* r1, int* ri, float* c0, float* c1, int* ci, const float* rmax, const float* rsum, const float* cmax,
                           const float* csum, const float* l0, const float* l1, const unsigned char* flags, void* ws, size_t ws_bytes, void* stream);

/* ---- LISRD's matcher (zoo entries LISRD+SuperPoint / +ALIKED / +SIFT; imcui/hloc/matchers/lisrd.py) -- csrc/lisrd.hip ----
 * imcui_hip_lisrd_match replaces `_lisrd_matcher` (lisrd.py:122-134) and `_compute_confidence` (lisrd.py:137-149) as `_forward` calls
 * them (lisrd.py:279-290) on the sampled sets of `_extract_descriptors` (lisrd.py:90-119): desc0 [dev, B,N,4,128], meta0 [dev, B,N,4,Dm],
 * desc1 [dev, B,M,4,128], meta1 [dev, B,M,4,Dm], one row per key-point and variance, Dm a multiple of 128 up to 1024; cnt0 / cnt1
 * [dev, B] int32 live key-points per image or NULL (all N / M).  The similarity sum_v softmax_v(<meta0, meta1>) * <desc0, desc1> is
 * reduced tile by tile on the matrix cores; neither [N,4,M] tensor nor the N x M matrix exists.  Among equal similarities the FIRST
 * index wins (`torch.max` leaves it open).  Outputs: matches0 [dev, B,N] int32 = nn12[i] where nn21[nn12[i]] == i, else -1 (rows past
 * cnt0: -1); best0 [dev, B,N] or NULL = the row-best similarity (0 for rows without a partner); mconf [dev, B,N] or NULL = the
 * confidence of the matched pair (0 where unmatched); nn12 [dev, B,N] / nn21 [dev, B,M] or NULL = the row / column arg-maxima (-1
 * past the counts) and best1 [dev, B,M] or NULL = the column-best similarity, for tests.  No host synchronisation; capturable. */
size_t imcui_hip_lisrd_match_workspace_bytes(int B, int N, int M, int Dm);
int imcui_hip_lisrd_match(imcui_hip_t* h, const float* desc0, const float* meta0, const int* cnt0, const float* desc1, const float* meta1, const int* cnt1, int B,
                          int N, int M, int Dm, int* matches0, float* best0, float* mconf, int* nn12, int* nn21, float* best1, void* ws, size_t ws_bytes, void* stream);
/* The network.  `lisrd.models` (lisrd.py:25-29) is not part of the reference checkout (third_party is empty): it is restated from its
 * description (tests/lisrd_reference.py) and parity with upstream's code is NOT pinned ("LISRD: what is pinned").  One
 * configuration is built: LISRD_CONFIG of lisrd.py:33-42 (desc_size 128, tile 3, n_clusters 8, meta_desc_dim 128, compute_meta_desc).
 * Host-side packing (replaces `self.net.load(weight_file, Mode.EXPORT)`, lisrd.py:187-189): tensor i is the state-dict entry named
 * imcui_hip_lisrd_tensor_name(i); imcui_hip_lisrd_tensor_shape(i, out4) returns its number of dimensions and writes them.  imcui_hip_lisrd_variance(v):
 * the name of variance v < 4, in the order the wrapper's dictionaries iterate in.  imcui_hip_lisrd_layer: entry i of the ONE launch table
 * (csrc/lisrd.hip, LISRD_LAYERS): its name, out5 = kind (0 first layer on the VALU, 1 3x3 on the implicit GEMM, 2 the eight hidden head
 * layers as one launch, 3 a head's 1x1 layer), cin, cout, pool (AvgPool2d(2, 2) behind the block), first channel it reads of its input. */
int imcui_hip_lisrd_num_layers(void);
const char* imcui_hip_lisrd_layer(int i, int* out5);
int imcui_hip_lisrd_num_tensors(void);
const char* imcui_hip_lisrd_tensor_name(int i);
int imcui_hip_lisrd_tensor_shape(int i, int* out4);
const char* imcui_hip_lisrd_variance(int v);
size_t imcui_hip_lisrd_packed_floats(void);
int imcui_hip_lisrd_pack_weights(const float* const* tensors, float* packed);
/* imcui_hip_lisrd_describe replaces, per image batch, `img * 255.0` (lisrd.py:209-210), `self.net._forward(...)` (lisrd.py:260-268), the
 * (x, y) -> (row, col) flip (lisrd.py:256-257) and `_extract_descriptors` with `_keypoints_to_grid` (lisrd.py:77-119, called at
 * lisrd.py:271-276): image [dev, B,3,H,W] in [0, 1] (H, W >= 24; all images of a call have one size), keypoints [dev, B,K,2] (x, y) in
 * pixels, counts [dev, B] int32 -> desc [dev, B,K,4,128], meta [dev, B,K,4,1024], every vector v / max(|v|, 1e-12), rows past the count
 * zero; status [dev, 1] int32 or NULL (always 0).  The dense maps stay in the workspace. */
size_t imcui_hip_lisrd_describe_workspace_bytes(int B, int H, int W);
int imcui_hip_lisrd_describe(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, const float* keypoints, const int* counts, int K,
                             float* desc, float* meta, int* status, void* ws, size_t ws_bytes, void* stream);
/* Test entries (device pointers).  dense: the eight dense maps [8][B,H/8,W/8,128] (descriptor maps of the four variances, then the raw
 * meta maps) and the meta maps [B,4,3,3,1024] (either may be NULL); ws of imcui_hip_lisrd_describe_workspace_bytes.  layers_probe: entries
 * [first, last] of the launch table through the forward's own launch list (entries 8 .. 16 one at a time; entries >= 9 read the
 * 2048-channel hidden map).  affine_probe: the BatchNorm pass behind the ReLU alone, y = x a + b on x [B,H,W,C] (pool = 1: through the 2x2
 * average pool, out [B,H/2,W/2,C]).  vlad_probe: regional NetVLAD with the weights of variance v on map [B,hc,wc,128] -> [B,3,3,1024].
 * sample_probe: the sparse sampling on given maps dmaps [4][B,hc,wc,128] and vlad [B,4,3,3,1024]. */
int imcui_hip_lisrd_dense(imcui_hip_t* h, const float* packed, const float* image, int B, int C, int H, int W, float* dense, float* vlad, void* ws, size_t ws_bytes,
                          void* stream);
size_t imcui_hip_lisrd_layers_workspace_bytes(int first, int last, int B, int H, int W);
int imcui_hip_lisrd_layers_probe(imcui_hip_t* h, const float* packed, const float* in, int first, int last, int B, int H, int W, float* out, void* ws,
                                 size_t ws_bytes, void* stream);
int imcui_hip_lisrd_affine_probe(imcui_hip_t* h, const float* x, const float* a, const float* b, int B, int H, int W, int C, int pool, float* out, void* stream);
size_t imcui_hip_lisrd_vlad_workspace_bytes(int B, int hc, int wc);
int imcui_hip_lisrd_vlad_probe(imcui_hip_t* h, const float* packed, int v, const float* map, int B, int hc, int wc, float* out, void* ws, size_t ws_bytes,
                               void* stream);
int imcui_hip_lisrd_sample_probe(imcui_hip_t* h, const float* dmaps, const float* vlad, int B, int hc, int wc, int H, int W, const float* keypoints,
                                 const int* counts, int K, float* desc, float* meta, void* stream);

/* ---- dual-softmax matcher (imcui/hloc/matchers/dual_softmax.py; zoo entries disk+dualsoftmax, superpoint+dualsoftmax) */
size_t imcui_hip_dual_softmax_workspace_bytes(int B, int C, int N, int M);
/* desc0 [dev, B,C,N], desc1 [dev, B,C,M] channels-first as the plugin receives them (any C >= 1); the matcher
 * L2-normalises over C when `normalize` (dual_softmax.py:20-22), sim = D0^T D1 * inv_temperature,
 * P = softmax(sim, rows) * softmax(sim, columns); matches0 [dev, B,N] int32 = the last column that is the row
 * maximum, the column maximum and > threshold (-1 = none), scores0 [dev, B,N] = P there (0 otherwise).
 * Per batch item (the reference is only ever driven with B = 1). */
int imcui_hip_dual_softmax(imcui_hip_t* h, const float* desc0, const float* desc1, int B, int C, int N, int M, double threshold,
                           double inv_temperature, int normalize, int* matches0, float* scores0, void* ws, size_t ws_bytes,
                           void* stream);

/* ---- building blocks (exported for tests and for the LoFTR path to come) --------------------- */
/* C[M,N] = A[M,K] * W[N,K]^T + bias ; relu optional ; K % 32 == 0 */
int imcui_hip_linear_f32(imcui_hip_t* h, const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                         int relu, void* stream);
/* NHWC 3x3 conv (pad 1) + bias (+ReLU) (+2x2 max-pool); weights OIHW on the HOST are packed with
 * imcui_hip_conv3x3_pack (Cin % 32 == 0, Cout % 64 == 0) into Cout*Cin*9 floats. */
int imcui_hip_conv3x3_pack(const float* w_oihw, int Cout, int Cin, float* packed);
int imcui_hip_conv3x3_f32(imcui_hip_t* h, const float* in_nhwc, const float* packed_w, const float* bias, float* out_nhwc,
                          int B, int H, int W, int Cin, int Cout, int relu, int pool, void* stream);
/* split-precision variants of the conv building block (mode 1 packing / launch) */
float imcui_hip_conv3x3_pack_split(const float* w_oihw, int Cout, int Cin, unsigned short* hi, unsigned short* lo);
/* Step before the path: the host preprocessing of imcui/hloc/extract_features.py:120-160 for
 * images that need no resize -- cv2.cvtColor(RGB2GRAY) on 8-bit pixels (OpenCV 4.x fixed point:
 * (9798 R + 19235 G + 3735 B + 16384) >> 15), astype(float32), / 255.0 -- on the device.
 * rgb: uint8 [B,H,W,3] (interleaved, as decoded), out: float32 [B,1,H,W].  H*W % 4 == 0. */
int imcui_hip_rgb_to_gray_f32(imcui_hip_t* h, const unsigned char* rgb_hwc, float* out, int B, int H, int W, void* stream);

/* The same step WITH a resize (imcui/hloc/extract_features.py:26-40 `resize_image(.., "cv2_area")`, :80-99, :120-148):
 *   uint8 [B,H,W,C] (C = 1 gray, C = 3 RGB interleaved) -> [cv2 RGB2GRAY fixed point] -> float32 -> cv2.resize(INTER_AREA)
 *   to oh x ow -> / 255.0 -> out float32 [B,1,oh,ow].  Shrinking only (the reference switches to INTER_LINEAR when a side
 * grows: IMCUI_HIP_ERR_UNSUPPORTED).  Non-integer factors use OpenCV's decimation tables, built on the HOST by
 * imcui_hip_area_table(ssize, dsize, start[dsize+1], index, weight) (returns the entry count; call it with
 * index = weight = NULL first to size the arrays) and uploaded by the caller: x tables for W -> ow, y tables for H -> oh
 * (NULL for integer factors).  float32 arithmetic in OpenCV's order; equals oracle/preprocess.py bit for bit. */
int imcui_hip_area_table(int ssize, int dsize, int* start, int* index, float* weight);
int imcui_hip_preprocess_area_f32(imcui_hip_t* h, const unsigned char* src, int B, int H, int W, int C, const int* xstart,
                                  const int* xindex, const float* xweight, const int* ystart, const int* yindex,
                                  const float* yweight, float* out, int oh, int ow, void* stream);
/* RGB mode of the same resize for extractors that take colour (DISK, `grayscale: False`): src uint8 [dev, B,H,W,3] -> float32 ->
 * INTER_AREA per channel -> / 255 -> out float32 planar [dev, B,3,oh,ow] (imcui/hloc/extract_features.py:80-99).  Tables as above;
 * oh = H, ow = W converts without resizing.  Shrinking only. */
int imcui_hip_preprocess_area_rgb_f32(imcui_hip_t* h, const unsigned char* src, int B, int H, int W, const int* xstart, const int* xindex,
                                      const float* xweight, const int* ystart, const int* yindex, const float* yweight, float* out, int oh,
                                      int ow, void* stream);

/* Growing resize of the same preprocessing step: `resize_image(image, size, "cv2_area")` runs cv2.INTER_LINEAR as soon as a
 * side grows (imcui/hloc/extract_features.py:29-31; `superpoint_max` force-resizes every image to 640 x 480).  Host table of
 * OpenCV's float-image set-up (half-pixel centres, float weights): per destination index the two source indices and the weight
 * of the second; horizontal = 1 pins out-of-range taps to the border with weight 0, horizontal = 0 (rows) clips the indices. */
int imcui_hip_linear_table(int ssize, int dsize, int horizontal, int* i0, int* i1, float* w1);
/* uint8 [B][H][W][C] (C = 1 gray, 3 RGB -> cv2's fixed-point gray) -> float32 [B][1][oh][ow] = INTER_LINEAR(float image) / 255:
 * horizontal pass of the two rows, then the vertical weights; multiply, multiply, add in float32 (no fused multiply-add).
 * Tables on the device.  Bit-exact against oracle/preprocess.py: linear_resize_f32 (parity unpinned: cv2 is absent). */
int imcui_hip_preprocess_linear_f32(imcui_hip_t* h, const unsigned char* src, int B, int H, int W, int C, const int* x0, const int* x1,
                                    const float* a1, const int* y0, const int* y1, const float* b1, float* out, int oh, int ow,
                                    void* stream);

/* The dfactor resize of the float image: `F.resize(image, size=size_new, antialias=True)` (extract_features.py:142-148,
 * match_dense.py:182) = ATen's anti-aliased bilinear kernel.  Host table of `_compute_indices_weights_aa` (float32): first
 * source index, tap count and normalised weights [out_size][kmax] per output index; returns the largest tap count (call with
 * w == NULL to size kmax). */
int imcui_hip_aa_table(int in_size, int out_size, int* first, int* count, float* w, int kmax);
/* float32 [planes][H][W] -> [planes][oh][ow]: the width pass of every needed source row (src[0] * w[0], then fused
 * multiply-adds in tap order), then the same along the height -- the arithmetic of ATen's CPU kernel, bit for bit
 * (tests/test_oracle_preprocess.py pins the restatement to torch; tests/test_gpu_preprocess.py the kernel). */
int imcui_hip_resize_aa_f32(imcui_hip_t* h, const float* src, int planes, int H, int W, const int* xfirst, const int* xcount,
                            const float* xweight, int kx, const int* yfirst, const int* ycount, const float* yweight, int ky, float* out,
                            int oh, int ow, void* stream);

/* nn.Linear weight [N][K] (K % 16 == 0) -> f16 hi / lo planes of w * 2^e in the FRAGMENT-MAJOR order the split GEMM
 * streams ([ceil(N/32)][K/16][2][32][8] halves per plane, rows >= N zero: each 1 KiB block is one MFMA operand
 * fragment of a wave); returns 2^-e (0 on bad arguments).  Planes hold roundup(N,32) * K halves each. */
float imcui_hip_linear_pack_split(const float* w, int N, int K, unsigned short* hi, unsigned short* lo);
/* C = act(A[M,K] * W^T + bias) with pre-split weights (device planes from imcui_hip_linear_pack_split, wscale = device
 * float holding the returned 2^-e).  Building block of every network projection in the split mode
 * (imcui/hloc/matchers/lightglue.py:75 -> upstream nn.Linear); precision 1 only, K % 32 == 0. */
int imcui_hip_linear_split_f32(imcui_hip_t* h, const float* A, const unsigned short* wh, const unsigned short* wl,
                               const float* wscale, const float* bias, float* C, int M, int N, int K, int relu, void* stream);

/* Opt-in range check of the split arithmetic (debugging aid; also switched on by the environment variable
 * IMCUI_HIP_CHECK_RANGE=1 at imcui_hip_create).  The 3 x f16 split of an f32 activation saturates its hi part at 65504 and is
 * no longer fp32-grade above that; weights are rescaled at pack time, activations are not.  With the check enabled every
 * split-mode GEMM / 3x3 convolution / fused-FFN launch first scans its f32 activation operand.  imcui_hip_get_range_status
 * synchronises the device, returns the accumulated word (bit 0: a value beyond the f16 range, bit 1: NaN / Inf) and clears it. */
int imcui_hip_set_range_check(imcui_hip_t* h, int enable);
int imcui_hip_get_range_status(imcui_hip_t* h, int* status);

/* Projection of a transformer block into the attention kernels' operand layout (upstream LightGlue SelfBlock `Wqkv` + rotary
 * encoding, CrossBlock `to_qk` / `to_v`; reached from imcui/hloc/matchers/lightglue.py:75): x [nseq * rows_per_seq][256] ->
 * f16 hi / lo planes (hi plane first, lo plane nseq*rows_per_seq*256 halves behind it) of Q, K [seq][head][row][64] and of
 * V^T [seq][head][64][row], 4 heads.  cross == 0: W [768][256] packed rows (q | k | v), rotary encoding (cos / sin
 * [rows][32]) on q and k, q *= alpha.  cross == 1: W [512][256] rows (qk | v), no rotation, qk *= alpha, `k` unused.
 * Weights as planes from imcui_hip_linear_pack_split; precision 1 only; rows_per_seq % 128 == 0; row tiles whose first row is
 * >= cnt[seq] are skipped.  Building block of the parity tests (both GEMM kernels that implement it are compared). */
int imcui_hip_qkv_split_f32(imcui_hip_t* h, const float* x, const unsigned short* wh, const unsigned short* wl, const float* wscale,
                            const float* bias, const float* rope_cos, const float* rope_sin, const int* cnt, int nseq,
                            int rows_per_seq, float alpha, int cross, float* q, float* k, float* v, void* stream);

/* Fused transformer FFN of a LightGlue block (upstream TransformerLayer.ffn on cat([x, message]) with the attention
 * out-projection folded into W1; reached from imcui/hloc/matchers/lightglue.py:75):
 *   out = x + W2 * GELU(LayerNorm_512(W1 * [x | ctx] + b1)) + b2,   x, ctx, out [M][256] (out may alias x).
 * W1 [512][512] as planes from imcui_hip_linear_pack_split; W2 [256][512] as planes from imcui_hip_ffn_pack_w2 (the
 * same fragment-major planes with the K axis in the order the kernel's first GEMM hands its accumulators over);
 * s1 / s2 = device floats holding the returned 2^-e.  precision 1 only.  One kernel: the 512-wide hidden row stays
 * on the CU (registers -> LDS), no LayerNorm / GELU pass over HBM.  act = 1 replaces LayerNorm + GELU by ReLU (gamma, beta
 * may be NULL): SuperGlue's MLP([512, 512, 256]) with its BatchNorm folded into W1 / b1 (imcui/hloc/matchers/superglue.py:26).
 * act = 2 / 3: out = x + LayerNorm_256(W2 * act(W1 * [x | ctx] + b1) + b2) with LeakyReLU(0.01) / ReLU and gamma, beta [256]
 * (b1, b2 may be NULL): the coarse MLPs of EfficientLoFTR (eloftr.py:79) / LoFTR (loftr.py:54). */
float imcui_hip_ffn_pack_w2(const float* w2, unsigned short* hi, unsigned short* lo);
int imcui_hip_ffn_split_f32(imcui_hip_t* h, const float* x, const float* ctx, const unsigned short* w1h, const unsigned short* w1l,
                            const float* s1, const float* b1, const float* gamma, const float* beta, const unsigned short* w2h,
                            const unsigned short* w2l, const float* s2, const float* b2, float* out, int M, int act, void* stream);

/* Lab hook (tools/ffn_bench.py): when `stamps` is non-NULL every workgroup of the next imcui_hip_ffn_split_f32 calls
 * writes 8 wall-clock (100 MHz) values at its phase boundaries to stamps[8 * workgroup ..]; NULL switches it off. */
int imcui_hip_ffn_set_debug(imcui_hip_t* h, long long* stamps);

int imcui_hip_conv3x3_split_f32(imcui_hip_t* h, const float* in_nhwc, const unsigned short* wh, const unsigned short* wl,
                                const float* wscale, const float* bias, float* out_nhwc, int B, int H, int W, int Cin,
                                int Cout, int relu, int pool, void* stream);
/* NHWC convolution as an implicit-im2col GEMM: weights [Cout][k*k*Cin] (tap-major), Cin % 32 == 0,
 * optional residual [B,Hout,Wout,Cout] added before the activation (0 none, 1 ReLU, 2 LeakyReLU 0.01) */
int imcui_hip_conv_gemm_f32(imcui_hip_t* h, const float* in_nhwc, const float* w_gemm, const float* bias, const float* resid,
                            float* out_nhwc, int B, int Hin, int Win, int Cin, int Cout, int ksize, int stride, int act,
                            void* stream);
/* softmax(Q K^T) V, head_dim 64, operands head-major [S][heads][rows][64] (Q pre-scaled),
 * output token-major [S*rows][heads*64]; cnt [dev, S] valid rows; cross: keys of sequence s^1.
 * log2_domain = 1: Q additionally carries a factor log2(e) and the soft-max is evaluated in base 2 (what the LightGlue /
 * SuperGlue layers do: one v_exp_f32 per probability, no multiply); 0: natural-log operands. */
int imcui_hip_attention_f32(imcui_hip_t* h, const float* Q, const float* K, const float* V, float* O, const int* cnt, int S,
                            int heads, int rows, int cross, int log2_domain, void* stream);
/* The same block in attention variant 9 (round 6; split mode, log2 domain only: what LightGlue's layers run when option "attn_variant" = 9):
 * K.Q^T in three f16 products, P.V as one f16 product + two block-scaled fp6 correction products (csrc/attention_mx.hip).  Operands as
 * for imcui_hip_attention_f32 in mode 1 (pre-split planes; the lo plane of V^T is read once, to build the fp6 planes); `scratch` [dev,
 * imcui_hip_attention_mx_scratch_bytes(S, heads, rows)] receives the fp6 planes of V^T. */
size_t imcui_hip_attention_mx_scratch_bytes(int S, int heads, int rows);
int imcui_hip_attention_mx_f32(imcui_hip_t* h, const float* Q, const float* K, const float* V, float* O, const int* cnt, int S,
                               int heads, int rows, int cross, void* scratch, size_t scratch_bytes, void* stream);

/* ---- test entry into the shared GEMM (tests/test_gpu_gemm_variants.py) ------------------------------------------------------
 * The fields the networks set on the one matrix engine under every network (csrc/gemm.h, GemmP; meanings there).  Device pointers;
 * unset fields zero except M / N / K, batch = cnt_stride = 1, conv_stride = 1, rup_align = 1, heads = 4, alpha = 1. */
typedef struct imcui_hip_gemm_desc {
    int epi;
    const float* A;
    long lda;
    const float* A2;
    long lda2;
    int K1;
    const float* W;
    long ldw;
    const unsigned short* Wh;
    const unsigned short* Wl;
    const float* wscale;
    const float* bias;
    float* C;
    long ldc;
    int M, N, K;
    float alpha;
    const int* cnt;
    const int* active;
    int rows_per_seq;
    const int* wsel;
    int wsel_off;
    long w_stride, b_stride;
    int batch;
    long a_bs, a2_bs, w_bs, c_bs;
    const int* mcnt;
    const int* ncnt;
    int cnt_stride;
    float* Q;
    float* Kt;
    float* V;
    int v_transposed, split_out;
    size_t plane_halves;
    int conv_k, conv_stride, conv_pad, conv_hin, conv_win, conv_hout, conv_wout, conv_cin;
    const float* resid;
    long ldr;
    int rup_h, rup_w, rup_align, act, single;
    const float* rope_cos;
    const float* rope_sin;
    int heads, role0;
    const int* rope_seq_row0;
    const float* ln_stats;
    const float* ln_rowsum;
    long ln_stride;
    int conv_dil; /* implicit im2col: taps conv_dil pixels apart (torch's dilation); 0 / 1 = none */
} imcui_hip_gemm_desc;
/* Copies *d into the kernel parameters and calls the GEMM launcher unchanged (its own refusals are the only checks); a null
 * handle or descriptor is IMCUI_HIP_ERR_ARG.  sizeof(imcui_hip_gemm_desc) for the bindings' mirror: imcui_hip_gemm_desc_bytes. */
int imcui_hip_gemm_probe_f32(imcui_hip_t* h, const imcui_hip_gemm_desc* d, void* stream);
size_t imcui_hip_gemm_desc_bytes(void);
/* Route of the last GEMM launch on this handle = 16 kind + epilogue (csrc/gemm.h GemmRouteKind, GemmEpi; 0 = nothing launched,
 * e.g. a refused call), and launches per route since imcui_hip_gemm_route_reset: route_counts copies min(n, slots) counters to
 * out and returns the slot count.  Every GEMM launch of every network records its route (one host-side store) and ORs the features
 * it ran with (csrc/gemm.h GemmFeature: tap size, stride, padding, dilation, residual kind, activation, output stride, partial
 * tiles, second K slab, batch and device-side counts, ...; derived from the launch parameters on the host) into its route's mask:
 * route_features copies the masks the same way.  route_reset clears both tables. */
int imcui_hip_gemm_last_route(const imcui_hip_t* h);
int imcui_hip_gemm_route_counts(const imcui_hip_t* h, int* out, int n);
int imcui_hip_gemm_route_features(const imcui_hip_t* h, int* out, int n);
int imcui_hip_gemm_route_reset(imcui_hip_t* h);

/* ---- test entry into the attention launcher (tests/test_gpu_attention_variants.py) -------------------------------------------
 * Every field of the launcher's parameters (csrc/attention.h, AttnP; meanings there).  Device pointers; unset fields zero except
 * heads = 4 and variant = -1 (the handle's "attn_variant").  V6_bytes / part_bytes: sizes of the two scratch buffers. */
typedef struct imcui_hip_attn_desc {
    const float* Q;
    const float* K;
    const float* V;
    float* O;
    const int* cnt;
    const int* active;
    int nseq, heads, rows_per_seq;
    int cross, log2_domain, single, variant;
    unsigned char* V6;
    size_t V6_bytes;
    int v6_ready;
    float* part;
    size_t part_bytes;
} imcui_hip_attn_desc;
/* Copies *d into the kernel parameters and calls the attention launcher unchanged.  Checks of its own: a null handle, descriptor, Q, K,
 * V, O or cnt is IMCUI_HIP_ERR_ARG; a V6 or part scratch shorter than the launch would use (imcui_hip_attention_mx_scratch_bytes,
 * 4 * imcui_hip_attention_part_floats) is IMCUI_HIP_ERR_WS.  Nothing is launched by a refused call. */
int imcui_hip_attention_probe_f32(imcui_hip_t* h, const imcui_hip_attn_desc* d, void* stream);
size_t imcui_hip_attn_desc_bytes(void);
/* floats of the key-split scratch (AttnP.part) for S sequences of `rows` rows; 0 for arguments that are not positive */
size_t imcui_hip_attention_part_floats(int S, int heads, int rows);
/* Route of the last attention launch on this handle = 2 kind + split (csrc/attention.h AttnRouteKind; 0 = nothing launched), and
 * launches per route since imcui_hip_attn_route_reset, as for the GEMM above. */
int imcui_hip_attn_last_route(const imcui_hip_t* h);
int imcui_hip_attn_route_counts(const imcui_hip_t* h, int* out, int n);
int imcui_hip_attn_route_reset(imcui_hip_t* h);

/* ---- test entry into the 3x3 convolution launchers (tests/test_gpu_conv_variants.py) ------------------------------------------
 * Every argument of the four launchers of csrc/conv.h (meanings there).  Device pointers; unset fields zero.
 * entry 0: conv3x3_launch (exact f32; in, wp, bias, out, B, H, W, Cin, Cout, relu, pool)
 * entry 1: conv3x3_split_launch (in, wh, wl, wscale, bias, out, B, H, W, Cin, Cout, relu, pool, resid, cin_stride, cout_live, single,
 *          resid2; the point-map head {head_w, head_b, head_pts, head_conf, head_raw} is passed when `head` is not 0)
 * entry 2: conv1ab_fused_split_launch (in = image [B,H,W], w1a [9][64], b1a, wh, wl, wscale, bias, out, B, H, W, pool)
 * entry 3: conv1a_launch (in = image [B,H,W], w1a [9][64], b1a, out, B, H, W) */
typedef struct imcui_hip_conv_desc {
    int entry;
    const float* in;
    const float* wp;
    const unsigned short* wh;
    const unsigned short* wl;
    const float* wscale;
    const float* bias;
    float* out;
    int B, H, W, Cin, Cout;
    int relu, pool;
    const float* resid;
    const float* resid2;
    int cin_stride, cout_live, single;
    int head;
    const float* head_w;
    const float* head_b;
    float* head_pts;
    float* head_conf;
    float* head_raw;
    const float* w1a;
    const float* b1a;
} imcui_hip_conv_desc;
/* Calls the launcher named by `entry` with the fields unchanged.  Checks of its own: a null handle, descriptor or a null pointer the
 * launcher would dereference without a check of its own (in, the weights and bias of the entry, `out` of entries 0, 2 and 3) is
 * IMCUI_HIP_ERR_ARG; `out` and the head's pointers of entry 1 are left to the launcher's refusals.  Nothing is launched by a refused call. */
int imcui_hip_conv_probe_f32(imcui_hip_t* h, const imcui_hip_conv_desc* d, void* stream);
size_t imcui_hip_conv_desc_bytes(void);
/* Route of the last convolution launch on this handle (csrc/conv.h ConvRouteKind; 0 = nothing launched: a refused call, an empty map),
 * launches per route since imcui_hip_conv_route_reset, and per route the OR of the fused features its launches ran with (ConvFeature
 * bits); both copy min(n, slots) values to out and return the slot count. */
int imcui_hip_conv_last_route(const imcui_hip_t* h);
int imcui_hip_conv_route_counts(const imcui_hip_t* h, int* out, int n);
int imcui_hip_conv_route_features(const imcui_hip_t* h, int* out, int n);
int imcui_hip_conv_route_reset(imcui_hip_t* h);

/* ---- test entry into the fused-FFN launcher (tests/test_gpu_ffn_variants.py) --------------------------------------------------
 * Every field of the launcher's parameters (csrc/ffn.h, FfnP; meanings there) except the lab's stamp buffer.  Device pointers; unset
 * fields zero.  What imcui_hip_ffn_split_f32 cannot express: the ragged form LightGlue and SuperGlue launch (cnt [S], active [S / 2],
 * rows_per_seq % 128 == 0, M = S * rows_per_seq) and the null arrays the networks pass (b1 = b2 = NULL: LoFTR, EfficientLoFTR;
 * gamma = beta = NULL with act 1: SuperGlue). */
typedef struct imcui_hip_ffn_desc {
    const float* x;
    const float* ctx;
    float* out;
    const unsigned short* w1h;
    const unsigned short* w1l;
    const unsigned short* w2h;
    const unsigned short* w2l;
    const float* s1;
    const float* s2;
    const float* b1;
    const float* gamma;
    const float* beta;
    const float* b2;
    int act;
    int M;
    const int* cnt;
    const int* active;
    int rows_per_seq;
} imcui_hip_ffn_desc;
/* Copies *d into the kernel parameters and calls the FFN launcher unchanged (its own refusals are the only checks: precision 0 is
 * IMCUI_HIP_ERR_UNSUPPORTED; a null mandatory pointer, an act outside 0 .. 3, rows_per_seq % 128 != 0 are IMCUI_HIP_ERR_ARG); a null
 * handle or descriptor is IMCUI_HIP_ERR_ARG.  Nothing is launched by a refused call or by M <= 0 (which is IMCUI_HIP_OK). */
int imcui_hip_ffn_probe_f32(imcui_hip_t* h, const imcui_hip_ffn_desc* d, void* stream);
size_t imcui_hip_ffn_desc_bytes(void);
/* Route of the last fused-FFN launch on this handle = 1 + 4 kind + act (csrc/ffn.h FfnRouteKind: the token tile; 0 = nothing launched:
 * a refused or empty call), and launches per route since imcui_hip_ffn_route_reset, as for the GEMM above.  Every launch of every
 * network records its route (one host-side store), imcui_hip_ffn_split_f32 included. */
int imcui_hip_ffn_last_route(const imcui_hip_t* h);
int imcui_hip_ffn_route_counts(const imcui_hip_t* h, int* out, int n);
int imcui_hip_ffn_route_reset(imcui_hip_t* h);

/* ---- test entry into the list-building blocks of csrc/select.h (tests/test_gpu_select.py) --------------------------------------
 * One op = one block (or the chain of blocks its callers launch together) with the template arguments the tree uses, on arrays GIVEN
 * by the caller.  The blocks are templates in an anonymous namespace: this entry runs the copy compiled into csrc/select_probe.hip, i.e.
 * it tests the SOURCE of select.h, not the copies compiled into each owner (those are reached by the stage probes below and by the
 * network tests).  Device pointers unless said otherwise; unset fields zero.  B images / rows (1 .. IMCUI_SELECT_MAXB); `capacity` =
 * elements per row of every per-row array (the row stride).
 *  op 0 COMPACT   cand_count_kernel -> exclusive_scan_kernel<int> -> cand_compact_kernel<., EmitScoreIndex>, predicate
 *                 score[b][i] > thr[b] with bind(b) fetching thr[b].  n = pixels per image (>= 1), score [B][n], thr [B],
 *                 cap <= capacity = the list's cap.  out_score / out_idx [B][capacity] (written below min(count, cap)), out_count [B]
 *                 (the true count), out_aux / out_i32 [B][cdiv(n, 4096)] chunk counts / offsets.
 *  op 1 SCAN      exclusive_scan_kernel<int> of in_i32 [B][capacity] -> out_i32 (may be in_i32: in place), out_count [B] totals;
 *                 n = n_cap <= capacity, n_dev [B] optional.
 *  op 2 ORDER_KEY out_key32[i] = order_key(score[i]), i < n <= capacity.
 *  op 3 KTH32     radix_select_kth<1024, unsigned> over order_key(score[b][i]), one workgroup per row, i < n_row[b], k_row[b]-th
 *                 largest -> out_key32 [B], out_count [B] = n_equal.
 *  op 4 KTH64     radix_select_kth<1024, unsigned long long> over key64 [B][capacity] -> out_key64 [B], out_count [B].
 *  op 5 RANK4, 6 RANK16   block_ordered_rank<4> (256 threads) / <16> (1024 threads) over the flags in_i32 [b][0 .. n_row[b]) walked in
 *                 batches with the running base in a register -> out_idx [b][i] = position of flagged entry i, out_count [B] totals.
 *  op 7 KEEP      keep_kth_in_order over key64 [b][0 .. n_row[b]) with `filter`, `kth`, `limit` -> out_idx [b][0 .. limit),
 *                 out_count [B] = the returned count (not clamped).
 *  op 8 CUT       zero_i32_kernel (base, status), advance_base_kernel once per level with the counts in_i32 [nlev][B] (nlev >= 2),
 *                 cand_cut_kernel on score [B][capacity] (capacity = kcap) with limit_ = `limit`, then kept_rank_ascending from a
 *                 256-thread kernel -> out_idx = kslot [B][capacity], out_count = nkept [B], out_aux = base [B] (the summed counts),
 *                 out_i32 = rank [B][capacity] (written below nkept), status [1]. */
#define IMCUI_SELECT_MAXB 8
typedef struct imcui_hip_select_desc {
    int op;
    int B;
    int n;
    int capacity;
    int cap;
    int limit;
    int filter;
    int nlev;
    int n_row[IMCUI_SELECT_MAXB]; /* host values */
    int k_row[IMCUI_SELECT_MAXB]; /* host values */
    unsigned long long kth;
    const float* score;
    const float* thr;
    const unsigned long long* key64;
    const int* in_i32;
    const int* n_dev;
    float* out_score;
    int* out_idx;
    int* out_count;
    int* out_i32;
    int* out_aux;
    unsigned* out_key32;
    unsigned long long* out_key64;
    int* status;
} imcui_hip_select_desc;
/* Host-only check of a descriptor, the one the probe makes before it launches anything: 0 = fine, else the first violated rule:
 * 1 op outside 0 .. 8; 2 B outside 1 .. IMCUI_SELECT_MAXB; 3 capacity outside 1 .. 2^24, n outside 0 .. capacity (COMPACT: n outside
 * 1 .. 2^24), an n_row[b] outside 0 .. capacity; 4 a k_row[b] outside 1 .. n_row[b] (KTH32, KTH64); 5 cap < 0 or cap > capacity
 * (COMPACT), limit < 0 (KEEP, CUT); 6 a null pointer among those the op reads or writes; 7 nlev outside 2 .. 16 (CUT).  A null
 * descriptor is rule 6. */
int imcui_hip_select_desc_check(const imcui_hip_select_desc* d);
/* A null handle or a descriptor that fails the check is IMCUI_HIP_ERR_ARG; nothing is launched by a refused call. */
int imcui_hip_select_probe(imcui_hip_t* h, const imcui_hip_select_desc* d, void* stream);
size_t imcui_hip_select_desc_bytes(void);

/* ---- test entries into two rule stages, entered through the launcher their `forward` calls ---------------------------------------
 * SuperPoint's "a5: select": status memset, candidate count / scan / compact (nms > threshold inside the border band, 64-bit keys) and
 * sp_topk_kernel, on a post-NMS map nms [dev, B,H,W] GIVEN by the caller.  cand_cap = room of the candidate list per image (`forward`
 * uses H * W).  Outputs as imcui_hip_superpoint_forward: keypoints [dev, B,kcap,2], scores [dev, B,kcap], num_keypoints [dev, B],
 * status [dev, 1] (1 = more candidates than cand_cap, 2 = more key-points than kcap, 4 = a top-k above 16384; a count under status 4 is
 * zero).  Slots past the count are not written.  Unlike `forward` the probe does not refuse max_keypoints > 16384 on the host, so that
 * the device's status-4 branch can be reached (it returns before any on-chip memory is touched).  H, W >= 1 with H * W <= 2^24,
 * 1 <= B <= 1024, kcap >= 1, cand_cap >= 1, null pointers and a short workspace are refused before anything is launched. */
size_t imcui_hip_superpoint_select_workspace_bytes(int B, int H, int W, int cand_cap);
int imcui_hip_superpoint_select_probe(imcui_hip_t* h, const float* nms, int B, int H, int W, float keypoint_threshold, int remove_borders,
                                      int max_keypoints, int kcap, int cand_cap, float* keypoints, float* scores, int* num_keypoints,
                                      int* status, void* ws, size_t ws_bytes, void* stream);
/* DISK's detection stage: status memset, candidate count / scan / compact (the window NMS and the strict threshold of `forward`) and
 * dk_select_kernel, on a heat map heat [dev, B,H,W] GIVEN by the caller.  ccap = room of the candidate list per image (`forward` uses
 * H * W).  Outputs as imcui_hip_disk_forward without the descriptors (zero past the count; status 2 = more key-points than kcap).
 * window odd >= 1, otherwise the refusals of the SuperPoint entry. */
size_t imcui_hip_disk_select_workspace_bytes(int B, int H, int W, int ccap);
int imcui_hip_disk_select_probe(imcui_hip_t* h, const float* heat, int B, int H, int W, int window, float threshold, int max_keypoints, int kcap,
                                int ccap, float* keypoints, float* scores, int* num_keypoints, int* status, void* ws, size_t ws_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMCUI_HIP_H */
