"""Seeded synthetic weights in the upstream state-dict layouts.

No checkpoint exists offline (weights come from the HF hub at `_init` time,
imcui/hloc/extractors/superpoint.py:48-53, imcui/hloc/matchers/lightglue.py:39-51), so benches, the smoke test and
the parity tests load the SAME seeded tensors into the HIP backend and -- in the tests -- into the oracle.  Key names /
shapes follow SURVEY.md Appendix A.1 / A.2, so a real `superpoint_v1.pth` / `superpoint_lightglue.pth` /
`superglue_outdoor.pth` state dict drops in unchanged.  This module is data generation only (like synth.py): it holds
no model arithmetic and imports nothing from `oracle/`.
"""
from __future__ import annotations

import math

import torch

SP_LAYERS = [
    # name, cout, cin, k
    ("conv1a", 64, 1, 3),
    ("conv1b", 64, 64, 3),
    ("conv2a", 64, 64, 3),
    ("conv2b", 64, 64, 3),
    ("conv3a", 128, 64, 3),
    ("conv3b", 128, 128, 3),
    ("conv4a", 128, 128, 3),
    ("conv4b", 128, 128, 3),
    ("convPa", 256, 128, 3),
    ("convPb", 65, 256, 1),
    ("convDa", 256, 128, 3),
    ("convDb", 256, 256, 1),
]


def superpoint_state_dict(seed: int = 0, peaky: bool = True) -> dict:
    """Kaiming-scaled random SuperPoint weights (1 300 865 params).

    `peaky=True` scales the detector logits (convPb) up and biases the dustbin
    channel so the soft-max heat-map has many well separated peaks above the
    0.005 threshold -- random heads otherwise give a near-uniform 1/65 map and
    NMS / top-k are exercised degenerately (golden data (i)).
    """
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cout, cin, k in SP_LAYERS:
        fan_in = cin * k * k
        w = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / fan_in)
        b = torch.randn(cout, generator=g) * 0.05
        sd[f"{name}.weight"] = w
        sd[f"{name}.bias"] = b
    if peaky:
        sd["convPb.weight"] = sd["convPb.weight"] * 6.0
        sd["convPb.bias"][-1] += 2.0
        # ReLU features have a large positive mean; centre the descriptor projection over
        # its inputs so descriptors are not dominated by one common direction.
        w = sd["convDb.weight"]
        sd["convDb.weight"] = (w - w.mean(dim=1, keepdim=True)) * 3.0
        sd["convDb.bias"] = -_mean_descriptor_logits(sd, g)
    return sd


def _mean_descriptor_logits(sd: dict, g: torch.Generator) -> torch.Tensor:
    """Mean convDb pre-activation over a small noise image (used to centre descriptors)."""
    import torch.nn.functional as F

    x = torch.rand(1, 1, 96, 128, generator=g)
    with torch.no_grad():
        for name in ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convDa"):
            x = F.relu(F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=1))
            if name in ("conv1b", "conv2b", "conv3b"):
                x = F.max_pool2d(x, 2, 2)
        y = F.conv2d(x, sd["convDb.weight"], None)
    return y.mean(dim=(0, 2, 3))


def lightglue_state_dict(seed: int = 0, n_layers: int = 9, dim: int = 256, heads: int = 4, structured: bool = True,
                         damp: float | None = None, ln_noise: float | None = None, final_gain: float | None = None,
                         input_dim: int = 256, add_scale_ori: bool = False) -> dict:
    """Random LightGlue weights in the upstream (new-style) key layout.

    transformers.{i}.self_attn.{Wqkv,out_proj,ffn.0,ffn.1,ffn.3}
    transformers.{i}.cross_attn.{to_qk,to_v,to_out,ffn.0,ffn.1,ffn.3}
    log_assignment.{i}.{matchability,final_proj}, token_confidence.{i}.token.0,
    posenc.Wr.weight

    `structured=True` shapes the heads so the data-dependent control flow is
    exercised non-degenerately with random transformer weights: residual updates are
    damped, `final_proj` is a scaled identity + noise (true correspondences of
    SuperPoint descriptors then win the dual soft-max), matchability logits spread
    around +1 (a few points fall below the 1 - width_confidence prune threshold) and
    the token-confidence bias rises with depth (pairs early-stop at varying layers).

    `damp` / `ln_noise` override the residual damping (default 0.03 structured, 1.0 otherwise) and the spread of
    the LayerNorm gamma / beta (default 0 structured, 0.1 otherwise): `structured=True, damp=1.0, ln_noise=0.1`
    keeps the shaped heads but makes every layer a full-strength update, so an error in the attention / FFN
    arithmetic reaches the outputs undiminished (the "undamped" parity tests); `final_gain` rescales the identity part
    of `final_proj` (the residual stream grows with strong updates, and similarities far above ~100 turn fp32 round-off
    into score differences no two fp32 implementations can agree on to 1e-4).
    """
    g = torch.Generator().manual_seed(seed)

    def lin(out_f, in_f, scale=1.0, bias=True, prefix=""):
        bound = scale / math.sqrt(in_f)
        d = {prefix + ".weight": (torch.rand(out_f, in_f, generator=g) * 2 - 1) * bound * math.sqrt(3.0)}
        if bias:
            d[prefix + ".bias"] = (torch.rand(out_f, generator=g) * 2 - 1) * 0.1
        return d

    sd = {}
    head_dim = dim // heads
    # gamma = 1 -> std 1 upstream (nn.init.normal_(std=gamma**-2))
    sd["posenc.Wr.weight"] = torch.randn(head_dim // 2, 2, generator=g)
    damp = (0.03 if structured else 1.0) if damp is None else damp
    ln_noise = (0.0 if structured else 0.1) if ln_noise is None else ln_noise
    for i in range(n_layers):
        p = f"transformers.{i}."
        sd.update(lin(3 * dim, dim, scale=10.0 if structured else 1.0, prefix=p + "self_attn.Wqkv"))
        sd.update(lin(dim, dim, prefix=p + "self_attn.out_proj"))
        sd.update(lin(2 * dim, 2 * dim, prefix=p + "self_attn.ffn.0"))
        sd[p + "self_attn.ffn.1.weight"] = 1.0 + ln_noise * torch.randn(2 * dim, generator=g)
        sd[p + "self_attn.ffn.1.bias"] = ln_noise * torch.randn(2 * dim, generator=g)
        sd.update(lin(dim, 2 * dim, scale=damp, prefix=p + "self_attn.ffn.3"))
        if structured:  # zero-mean rows: no common-mode drift of the residual stream
            w = sd[p + "self_attn.ffn.3.weight"]
            sd[p + "self_attn.ffn.3.weight"] = w - w.mean(dim=1, keepdim=True)
            sd[p + "self_attn.ffn.3.bias"] = sd[p + "self_attn.ffn.3.bias"] * 0.05
        sd.update(lin(dim, dim, scale=10.0 if structured else 1.0, prefix=p + "cross_attn.to_qk"))
        sd.update(lin(dim, dim, prefix=p + "cross_attn.to_v"))
        sd.update(lin(dim, dim, prefix=p + "cross_attn.to_out"))
        sd.update(lin(2 * dim, 2 * dim, prefix=p + "cross_attn.ffn.0"))
        sd[p + "cross_attn.ffn.1.weight"] = 1.0 + ln_noise * torch.randn(2 * dim, generator=g)
        sd[p + "cross_attn.ffn.1.bias"] = ln_noise * torch.randn(2 * dim, generator=g)
        sd.update(lin(dim, 2 * dim, scale=damp, prefix=p + "cross_attn.ffn.3"))
        if structured:
            w = sd[p + "cross_attn.ffn.3.weight"]
            sd[p + "cross_attn.ffn.3.weight"] = w - w.mean(dim=1, keepdim=True)
            sd[p + "cross_attn.ffn.3.bias"] = sd[p + "cross_attn.ffn.3.bias"] * 0.05
        q = f"log_assignment.{i}."
        if structured:
            sd.update(lin(1, dim, scale=48.0, prefix=q + "matchability"))  # logit std ~2.5 per unit |x|
            sd[q + "matchability.bias"] = sd[q + "matchability.bias"] + 2.0
            sd.update(lin(dim, dim, scale=2.0, prefix=q + "final_proj"))
            sd[q + "final_proj.weight"] = sd[q + "final_proj.weight"] + (4.0 * math.sqrt(60.0) if final_gain is None else final_gain) * torch.eye(dim)
        else:
            sd.update(lin(1, dim, prefix=q + "matchability"))
            sd.update(lin(dim, dim, scale=4.0, prefix=q + "final_proj"))
        if i < n_layers - 1:
            t = f"token_confidence.{i}.token.0"
            if structured:
                sd.update(lin(1, dim, scale=12.0, prefix=t))  # logit std ~1 per unit |x|
                sd[t + ".bias"] = sd[t + ".bias"] + 1.2 + 0.4 * i
            else:
                sd.update(lin(1, dim, scale=2.0, prefix=t))
    # variants of upstream's `features` table, drawn last so that the 256-d superpoint tensors above do not change
    if add_scale_ori:
        sd["posenc.Wr.weight"] = torch.cat([sd["posenc.Wr.weight"], 0.3 * torch.randn(head_dim // 2, 2, generator=g)], 1)
    if input_dim != dim:
        # disk / aliked / sift: Linear(input_dim, 256); a scaled partial isometry + noise keeps distinctive descriptors distinctive
        q, _ = torch.linalg.qr(torch.randn(dim, input_dim, generator=g))
        sd["input_proj.weight"] = q + 0.02 * torch.randn(dim, input_dim, generator=g)
        sd["input_proj.bias"] = 0.01 * torch.randn(dim, generator=g)
    return sd


def loftr_state_dict(seed: int = 0, structured: bool = True) -> dict:
    """Random LoFTR weights in kornia's state-dict layout (ResNetFPN_8_2 + coarse/fine transformers).

    backbone.{conv1,bn1,layer{1,2,3}.{0,1}.{conv1,bn1,conv2,bn2[,downsample.{0,1}]},layer3_outconv,
    layer2_outconv,layer2_outconv2.{0,1,3},layer1_outconv,layer1_outconv2.{0,1,3}},
    loftr_coarse.layers.{0..7}.{q_proj,k_proj,v_proj,merge,mlp.0,mlp.2,norm1,norm2},
    fine_preprocess.{down_proj,merge_feat}, loftr_fine.layers.{0,1}.*
    `structured` damps the transformer updates so coarse features stay image-dependent and the
    dual soft-max produces confident mutual matches with random weights.
    """
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cout, cin, k, gain=1.0):
        sd[name + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k)) * gain

    def bn(name, c):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_var"] = 1.0 + 0.2 * torch.rand(c, generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(0)

    b = "backbone."
    conv(b + "conv1", 128, 1, 7)
    bn(b + "bn1", 128)
    dims = [128, 128, 196, 256]
    for li in range(1, 4):
        cin, cout = dims[li - 1], dims[li]
        for bi in range(2):
            p = f"{b}layer{li}.{bi}"
            c_in = cin if bi == 0 else cout
            conv(p + ".conv1", cout, c_in, 3)
            bn(p + ".bn1", cout)
            conv(p + ".conv2", cout, cout, 3, gain=0.5)
            bn(p + ".bn2", cout)
            if bi == 0 and li > 1:
                conv(p + ".downsample.0", cout, c_in, 1)
                bn(p + ".downsample.1", cout)
    conv(b + "layer3_outconv", 256, 256, 1)
    if structured:
        # x3 is post-ReLU and dominated by one common direction: project the mean feature of a small
        # calibration image out of every row, then apply a gain, so that the coarse dual soft-max is
        # driven by image content and produces confident mutual matches with random weights
        m = _loftr_mean_stage3_feature(sd, torch.rand(1, 1, 96, 128, generator=g))
        m = m / m.norm()
        wc = sd[b + "layer3_outconv.weight"][:, :, 0, 0]
        wc = wc - (wc @ m)[:, None] * m[None, :]
        sd[b + "layer3_outconv.weight"] = (wc * 4.0)[:, :, None, None].contiguous()
    conv(b + "layer2_outconv", 256, 196, 1)
    conv(b + "layer2_outconv2.0", 256, 256, 3)
    bn(b + "layer2_outconv2.1", 256)
    conv(b + "layer2_outconv2.3", 196, 256, 3)
    conv(b + "layer1_outconv", 196, 128, 1)
    conv(b + "layer1_outconv2.0", 196, 196, 3)
    bn(b + "layer1_outconv2.1", 196)
    conv(b + "layer1_outconv2.3", 128, 196, 3)

    def lin(name, out_f, in_f, gain=1.0, bias=False):
        sd[name + ".weight"] = (torch.rand(out_f, in_f, generator=g) * 2 - 1) * math.sqrt(3.0 / in_f) * gain
        if bias:
            sd[name + ".bias"] = (torch.rand(out_f, generator=g) * 2 - 1) * 0.1

    def encoder(prefix, n_layers, d):
        for i in range(n_layers):
            p = f"{prefix}.layers.{i}"
            for nm in ("q_proj", "k_proj", "v_proj", "merge"):
                lin(f"{p}.{nm}", d, d)
            lin(f"{p}.mlp.0", 2 * d, 2 * d)
            lin(f"{p}.mlp.2", d, 2 * d)
            for nm in ("norm1", "norm2"):
                sd[f"{p}.{nm}.weight"] = (0.25 if (structured and nm == "norm2") else 1.0) + 0.05 * torch.randn(d, generator=g)
                sd[f"{p}.{nm}.bias"] = 0.02 * torch.randn(d, generator=g)

    encoder("loftr_coarse", 8, 256)
    lin("fine_preprocess.down_proj", 128, 256, bias=True)
    lin("fine_preprocess.merge_feat", 128, 256, bias=True)
    encoder("loftr_fine", 2, 128)
    return sd


def _loftr_mean_stage3_feature(sd: dict, x: torch.Tensor) -> torch.Tensor:
    """Mean 1/8-resolution ResNet feature of a small calibration image (plain torch; weight shaping only, like
    `_mean_descriptor_logits` for SuperPoint).  Stages = conv7x7/2 + BN + ReLU, then three pairs of BasicBlocks."""
    import torch.nn.functional as F

    def bn(t, p):
        return F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)

    def block(t, p, stride):
        y = F.relu(bn(F.conv2d(t, sd[p + ".conv1.weight"], None, stride, 1), p + ".bn1"))
        y = bn(F.conv2d(y, sd[p + ".conv2.weight"], None, 1, 1), p + ".bn2")
        if p + ".downsample.0.weight" in sd:
            t = bn(F.conv2d(t, sd[p + ".downsample.0.weight"], None, stride, 0), p + ".downsample.1")
        return F.relu(t + y)

    b = "backbone."
    with torch.no_grad():
        t = F.relu(bn(F.conv2d(x, sd[b + "conv1.weight"], None, 2, 3), b + "bn1"))
        for li, stride in ((1, 1), (2, 2), (3, 2)):
            t = block(block(t, f"{b}layer{li}.0", stride), f"{b}layer{li}.1", 1)
    return t.mean(dim=(0, 2, 3))


def superglue_state_dict(seed: int = 0, structured: bool = True) -> dict:
    """Random SuperGlue weights in the upstream (magicleap / Vincentqyw fork) state-dict layout:

    kenc.encoder.{0,3,6,9,12}.{weight[out,in,1],bias}, kenc.encoder.{1,4,7,10}.{weight,bias,running_mean,
    running_var,num_batches_tracked}, gnn.layers.{i}.attn.{merge,proj.0,proj.1,proj.2}.{weight,bias},
    gnn.layers.{i}.mlp.{0,3}.{weight,bias}, gnn.layers.{i}.mlp.1.<BatchNorm>, final_proj.{weight,bias}, bin_score.

    `structured` damps the residual updates and makes `final_proj` a scaled identity + noise, so the optimal
    transport of random-weight features still resolves the true correspondences of distinctive descriptors
    (mutual matches above `match_threshold`, the rest in the dust-bins).
    """
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cout, cin, scale=1.0, bias_scale=0.1):
        bound = scale * math.sqrt(3.0 / cin)
        sd[name + ".weight"] = (torch.rand(cout, cin, 1, generator=g) * 2 - 1) * bound
        sd[name + ".bias"] = (torch.rand(cout, generator=g) * 2 - 1) * bias_scale

    def bn(name, c):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_var"] = 1.0 + 0.2 * torch.rand(c, generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(0)

    chans = [3, 32, 64, 128, 256, 256]
    for i in range(1, len(chans)):
        last = i == len(chans) - 1
        conv(f"kenc.encoder.{3 * (i - 1)}", chans[i], chans[i - 1], scale=(0.05 if structured else 1.0) if last else 1.4)
        if last:
            sd[f"kenc.encoder.{3 * (i - 1)}.bias"].zero_()  # nn.init.constant_(encoder[-1].bias, 0)
            if structured:  # ReLU features have a positive mean: zero-mean rows avoid a common-mode offset
                w = sd[f"kenc.encoder.{3 * (i - 1)}.weight"]
                sd[f"kenc.encoder.{3 * (i - 1)}.weight"] = w - w.mean(dim=1, keepdim=True)
        else:
            bn(f"kenc.encoder.{3 * (i - 1) + 1}", chans[i])
    for i in range(18):
        p = f"gnn.layers.{i}."
        conv(p + "attn.merge", 256, 256)
        for j in range(3):
            conv(p + f"attn.proj.{j}", 256, 256, scale=6.0 if (structured and j < 2) else 1.0)
        conv(p + "mlp.0", 512, 512, scale=1.4)
        bn(p + "mlp.1", 512)
        conv(p + "mlp.3", 256, 512, scale=0.08 if structured else 1.0)
        if structured:
            w = sd[p + "mlp.3.weight"]
            sd[p + "mlp.3.weight"] = w - w.mean(dim=1, keepdim=True)
        sd[p + "mlp.3.bias"].zero_()  # nn.init.constant_(mlp[-1].bias, 0)
    conv("final_proj", 256, 256, scale=2.0 if structured else 4.0)
    if structured:
        sd["final_proj.weight"] = sd["final_proj.weight"] + 4.0 * math.sqrt(60.0) * torch.eye(256)[:, :, None]
    sd["bin_score"] = torch.tensor(35.0 if structured else 1.0)  # above the best random-column score of an outlier
    return sd


def imp_synth_state(seed: int = 0) -> dict:
    """Random IMP weights in the state-dict layout of pram.nets.gml.GML (`imp_gml.920.pth` under its "model" key; names and shapes
    are the table of csrc/imp.hip): SuperGlue's key-point encoder and 18 attentional layers, plus

    input_proj.{weight[256,128,1],bias}       128-d descriptors -> the 256-d token states
    final_proj.{0..8}.{weight[256,256,1],bias} one per layer pair (training supervises every pair; inference reads .8)
    bin_score                                 scalar

    Structured like `superglue_state_dict`: damped residual updates and `final_proj.8` near a scaled identity.  `input_proj` is an
    isometry (orthonormal columns) plus small noise, so distinctive unit descriptors stay distinctive: their inner products, and with
    them the score of a true correspondence (about 60 cos), survive the projection, and 20 probability-domain Sinkhorn rounds resolve
    the true correspondences above the dust-bin score (tests/test_imp_cpu.py asserts the share).
    """
    sd = superglue_state_dict(seed, structured=True)
    g = torch.Generator().manual_seed(seed + 7919)
    fw, fb = sd.pop("final_proj.weight"), sd.pop("final_proj.bias")
    for k in range(9):
        if k == 8:
            sd["final_proj.8.weight"], sd["final_proj.8.bias"] = fw, fb
        else:  # read by no inference path; present because the checkpoint is loaded strictly
            sd[f"final_proj.{k}.weight"] = (torch.rand(256, 256, 1, generator=g) * 2 - 1) * math.sqrt(3.0 / 256)
            sd[f"final_proj.{k}.bias"] = (torch.rand(256, generator=g) * 2 - 1) * 0.1
    q, _ = torch.linalg.qr(torch.randn(256, 128, generator=g, dtype=torch.float64))
    sd["input_proj.weight"] = (q.float() + 0.01 * torch.randn(256, 128, generator=g))[:, :, None].contiguous()
    sd["input_proj.bias"] = 0.01 * torch.randn(256, generator=g)
    # true correspondences score about 80 after the 18 layers, the best outlier up to about 42 (512 .. 2100 points per image): between them,
    # far enough above the outliers that an unmatched row keeps less than 1e-6 outside its dust-bin
    sd["bin_score"] = torch.tensor(58.0)
    return sd


def eloftr_state_dict(seed: int = 0, gain: float = 1.0, shaped: bool = True) -> dict:
    """Random EfficientLoFTR weights in the layout of `transformers.EfficientLoFTRForKeypointMatching.state_dict()`
    (the maintained port of the upstream network the reference wrapper imports, imcui/hloc/matchers/eloftr.py:13-18):

    efficientloftr.backbone.stages.{s}.blocks.{b}.{conv1,conv2}.{conv.weight,norm.*}[, identity.*]   RepVGG 1-64-64-128-256
    efficientloftr.local_feature_transformer.layers.{0..3}.{self,cross}_attention.
        {aggregation.{q_aggregation.weight,norm.*}, attention.{q,k,v,o}_proj.weight, mlp.{fc1,fc2}.weight, mlp.layer_norm.*}
    refinement_layer.{out_conv.weight, out_conv_layers.{0,1}.{out_conv1,out_conv2,out_conv3}.weight, batch_norm.*}

    `gain` scales the transformer's residual updates (the LayerNorm that closes each block); `shaped` re-weights the last
    block so that with random weights the coarse features are content codes and the dual soft-max at temperature 0.1
    produces confident mutual matches on overlapping images.
    """
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cout, cin, k, s=1.0, groups=1):
        sd[name] = torch.randn(cout, cin // groups, k, k, generator=g) * math.sqrt(2.0 / (cin // groups * k * k)) * s

    def bn(name, c, wmean=1.0):
        sd[name + ".weight"] = wmean * (1.0 + 0.1 * torch.randn(c, generator=g))
        sd[name + ".bias"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".running_var"] = 1.0 + 0.2 * torch.rand(c, generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(0)

    def lin(name, out_f, in_f, s=1.0):
        sd[name] = (torch.rand(out_f, in_f, generator=g) * 2 - 1) * math.sqrt(3.0 / in_f) * s

    def ln(name, c, wmean=1.0):
        sd[name + ".weight"] = wmean * (1.0 + 0.05 * torch.randn(c, generator=g))
        sd[name + ".bias"] = 0.02 * torch.randn(c, generator=g)

    blocks, strides, dims = [1, 2, 4, 14], [2, 1, 2, 2], [64, 64, 128, 256]
    cin = 1
    for s in range(4):
        for b in range(blocks[s]):
            p = f"efficientloftr.backbone.stages.{s}.blocks.{b}"
            cout = dims[s]
            stride = strides[s] if b == 0 else 1
            has_id = cin == cout and stride == 1
            # three branches are summed before the ReLU: keep the sum at unit variance
            local = shaped and s == 3 and b > 0  # keep the receptive field of the 14-block stage small
            conv(p + ".conv1.conv.weight", cout, cin, 3, 0.3 if local else 0.8)
            bn(p + ".conv1.norm", cout)
            conv(p + ".conv2.conv.weight", cout, cin, 1, 0.7 if local else 0.5)
            bn(p + ".conv2.norm", cout)
            if has_id:
                bn(p + ".identity", cin, 0.6 if local else 0.5)
            cin = cout
    for i in range(4):
        for kind in ("self_attention", "cross_attention"):
            p = f"efficientloftr.local_feature_transformer.layers.{i}.{kind}"
            sd[p + ".aggregation.q_aggregation.weight"] = torch.randn(256, 1, 4, 4, generator=g) * 0.25 + 1.0 / 16
            ln(p + ".aggregation.norm", 256)
            for nm in ("q_proj", "k_proj", "v_proj", "o_proj"):
                lin(f"{p}.attention.{nm}.weight", 256, 256, 2.0 if nm in ("q_proj", "k_proj") else 1.0)
            lin(p + ".mlp.fc1.weight", 512, 512)
            lin(p + ".mlp.fc2.weight", 256, 512)
            ln(p + ".mlp.layer_norm", 256, 0.05 if shaped else gain * 0.25)  # shaped: the last block carries the code (below)
    if shaped:
        # The 1/8 features are post-ReLU, share one large common direction and vary smoothly, which makes a few cells
        # the nearest neighbour of everything.  Let the block every token passes through last (layer 3, cross
        # attention) add a large content code: its first linear layer reads the WHITENED deviation of the token from
        # the mean feature (principal components of a calibration image, each scaled to unit variance, then a random
        # mix) and mostly ignores the attention half; the LayerNorm that closes the block applies a big gamma.
        from .synth import _add_blobs, _band_limited_noise

        p = "efficientloftr.local_feature_transformer.layers.3.cross_attention"
        cal = _eloftr_stage3_cells(sd, _add_blobs(g, _band_limited_noise(g, 160, 192), 600))  # [480, 256]
        mean = cal.mean(0)
        _, sv, vt = torch.linalg.svd(cal - mean, full_matrices=False)
        k = 64
        white = vt[:k] / (sv[:k, None] / math.sqrt(cal.shape[0] - 1))  # [k, 256]: z = white @ (x - mean), unit variance
        mix = torch.randn(512, k, generator=g) / math.sqrt(k)
        wx = mix @ white
        w1 = sd[p + ".mlp.fc1.weight"]
        sd[p + ".mlp.fc1.weight"] = torch.cat([wx, w1[:, 256:] * 0.1], 1).contiguous()
        # fc1 has no bias: the mean feature is removed by making every row orthogonal to it
        wx = sd[p + ".mlp.fc1.weight"][:, :256]
        mh = mean / mean.norm()
        sd[p + ".mlp.fc1.weight"][:, :256] = wx - (wx @ mh)[:, None] * mh[None, :]
        sd[p + ".mlp.layer_norm.weight"] = sd[p + ".mlp.layer_norm.weight"] / 0.05 * 3.0
    conv("refinement_layer.out_conv.weight", 256, 256, 1)
    for i, (hid, mid) in enumerate([(128, 256), (64, 128)]):
        p = f"refinement_layer.out_conv_layers.{i}"
        conv(p + ".out_conv1.weight", mid, hid, 1)
        conv(p + ".out_conv2.weight", mid, mid, 3)
        bn(p + ".batch_norm", mid)
        conv(p + ".out_conv3.weight", hid, mid, 3)
    return sd


def _eloftr_stage3_cells(sd: dict, x: torch.Tensor) -> torch.Tensor:
    """1/8-resolution RepVGG features of a small calibration image as [cells, 256] (plain torch; weight shaping only)."""
    import torch.nn.functional as F

    def bn(t, p):
        return F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)

    for s, (nb, stride) in enumerate(zip([1, 2, 4, 14], [2, 1, 2, 2])):
        for b in range(nb):
            p = f"efficientloftr.backbone.stages.{s}.blocks.{b}"
            st = stride if b == 0 else 1
            y = bn(F.conv2d(x, sd[p + ".conv1.conv.weight"], None, st, 1), p + ".conv1.norm")
            y = y + bn(F.conv2d(x, sd[p + ".conv2.conv.weight"], None, st, 0), p + ".conv2.norm")
            if p + ".identity.weight" in sd:
                y = y + bn(x, p + ".identity")
            x = F.relu(y)
    return x[0].permute(1, 2, 0).reshape(-1, x.shape[1])


# ---------------------------------------------------------------------------------------------------------------- DUSt3R
DUST3R_CFG = {"enc_dim": 1024, "enc_depth": 24, "dec_dim": 768, "dec_depth": 12}  # DUSt3R_ViTLarge_BaseDecoder_512_dpt
DUST3R_LAYER_DIMS = (96, 192, 384, 768)


def dust3r_state_dict(seed: int = 0, cfg: dict | None = None, gain: float = 1.0) -> dict:
    """Random weights in the state-dict layout of `AsymmetricCroCo3DStereo` (head_type 'dpt', output_mode 'pts3d';
    imcui/hloc/matchers/duster.py:37 loads `duster_vit_large.pth` into it).  Linear layers are drawn at
    gain / sqrt(fan_in), so every sub-layer moves the residual stream by O(1) (attention logits have unit spread, the
    MLPs are not negligible next to the stream): the parity tests then see each block's arithmetic, which the usual
    std = 0.02 initialisation would hide.  The last 1x1 convolution is small enough that expm1(|xyz|) stays O(1).
    `cfg` overrides enc_dim / enc_depth / dec_dim / dec_depth (dims multiples of 64, dec_depth a multiple of 4); cfg["desc_dim"] > 0
    adds MASt3R's `head_local_features` (`AsymmetricMASt3R`, imcui/hloc/matchers/mast3r.py:41: 24 for the shipped checkpoint)."""
    c = {**DUST3R_CFG, **(cfg or {})}
    E, D = c["enc_dim"], c["dec_dim"]
    g = torch.Generator().manual_seed(seed)
    sd: dict = {}

    def lin(name, n, k, s=1.0, bias=True):
        sd[name + ".weight"] = torch.randn(n, k, generator=g) * (gain * s / math.sqrt(k))
        if bias:
            sd[name + ".bias"] = torch.randn(n, generator=g) * 0.1

    def norm(name, n):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(n, generator=g)
        sd[name + ".bias"] = 0.05 * torch.randn(n, generator=g)

    def conv(name, co, ci, k, s=1.0, bias=True, transposed=False):
        shape = (ci, co, k, k) if transposed else (co, ci, k, k)
        fan = ci if transposed else ci * k * k  # a transposed convolution with kernel = stride sums over Cin only
        sd[name + ".weight"] = torch.randn(*shape, generator=g) * (gain * s / math.sqrt(fan))
        if bias:
            sd[name + ".bias"] = torch.randn(co, generator=g) * 0.1

    conv("patch_embed.proj", E, 3, 16, s=2.0)
    for i in range(c["enc_depth"]):
        p = f"enc_blocks.{i}."
        norm(p + "norm1", E)
        lin(p + "attn.qkv", 3 * E, E)
        lin(p + "attn.proj", E, E, 0.5)
        norm(p + "norm2", E)
        lin(p + "mlp.fc1", 4 * E, E)
        lin(p + "mlp.fc2", E, 4 * E, 0.7)
    norm("enc_norm", E)
    lin("decoder_embed", D, E)
    for blocks in ("dec_blocks", "dec_blocks2"):
        for i in range(c["dec_depth"]):
            p = f"{blocks}.{i}."
            norm(p + "norm1", D)
            lin(p + "attn.qkv", 3 * D, D)
            lin(p + "attn.proj", D, D, 0.5)
            norm(p + "norm2", D)
            norm(p + "norm_y", D)
            for n in ("projq", "projk", "projv"):
                lin(p + "cross_attn." + n, D, D)
            lin(p + "cross_attn.proj", D, D, 0.5)
            norm(p + "norm3", D)
            lin(p + "mlp.fc1", 4 * D, D)
            lin(p + "mlp.fc2", D, 4 * D, 0.7)
    norm("dec_norm", D)
    for hd in (1, 2):
        p = f"downstream_head{hd}.dpt."
        dims_in = (E, D, D, D)
        for k, ld in enumerate(DUST3R_LAYER_DIMS):
            conv(f"{p}act_postprocess.{k}.0", ld, dims_in[k], 1)
            if k == 0:
                conv(f"{p}act_postprocess.0.1", ld, ld, 4, transposed=True)
            elif k == 1:
                conv(f"{p}act_postprocess.1.1", ld, ld, 2, transposed=True)
            elif k == 3:
                conv(f"{p}act_postprocess.3.1", ld, ld, 3)
            conv(f"{p}scratch.layer_rn.{k}", 256, ld, 3, bias=False)
            sd[f"{p}scratch.layer{k + 1}_rn.weight"] = sd[f"{p}scratch.layer_rn.{k}.weight"]  # upstream registers the module twice
        for r in (1, 2, 3, 4):
            for u in (1, 2):
                conv(f"{p}scratch.refinenet{r}.resConfUnit{u}.conv1", 256, 256, 3, 1.2)
                conv(f"{p}scratch.refinenet{r}.resConfUnit{u}.conv2", 256, 256, 3, 0.6)
            conv(f"{p}scratch.refinenet{r}.out_conv", 256, 256, 1, 0.8)
        conv(p + "head.0", 128, 256, 3)
        conv(p + "head.2", 128, 128, 3, 1.4)
        conv(p + "head.4", 4, 128, 1, 0.5)
        dd = c.get("desc_dim", 0)
        if dd:
            q = f"downstream_head{hd}.head_local_features."
            lin(q + "fc1", 4 * (E + D), E + D)
            lin(q + "fc2", (dd + 1) * 256, 4 * (E + D), 1.5)
    return sd


# DISK (kornia.feature.DISK, U-Net of 5x5 convolutions): (state-dict block, input channels, output channels, has norm / gate)
DISK_LAYERS = [
    ("unet.path_down.0.1", 3, 16, False),
    ("unet.path_down.1.1", 16, 32, True),
    ("unet.path_down.2.1", 32, 64, True),
    ("unet.path_down.3.1", 64, 64, True),
    ("unet.path_down.4.1", 64, 64, True),
    ("unet.path_up.0.conv", 128, 64, True),
    ("unet.path_up.1.conv", 128, 64, True),
    ("unet.path_up.2.conv", 96, 64, True),
    ("unet.path_up.3.conv", 80, 129, True),
]


def disk_state_dict(seed: int = 0, heat_gain: float = 4.0) -> dict:
    """Kaiming-scaled random DISK weights (26 tensors, 1 092 369 params, kornia's key names).  PReLU slopes scatter around
    PyTorch's 0.25 initial value.  The heatmap row (output channel 128 of the last convolution) is scaled by `heat_gain` so the
    logits spread over several units: many well separated NMS maxima above a 0.0 threshold, and a selection cut-off that
    falls inside a dense range of values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout, gated in DISK_LAYERS:
        if gated:
            sd[f"{name}.1.weight"] = 0.25 + 0.1 * torch.randn(cin, generator=g)
        w = torch.randn(cout, cin, 5, 5, generator=g) * math.sqrt(2.0 / (cin * 25))
        b = 0.05 * torch.randn(cout, generator=g)
        if cout == 129:
            w[128] *= heat_gain
            b[128] = 0.0
        sd[f"{name}.3.weight"] = w
        sd[f"{name}.3.bias"] = b
    return sd


def aliked_state_dict(seed: int = 0, score_gain: float = 4.0, score_shift: float = -3.6) -> dict:
    """Seeded ALIKED weights (aliked-n16 layout, upstream's key names, 65 tensors without the `num_batches_tracked` counters).
    Convolutions are LeCun-scaled (SELU keeps unit variance); BatchNorm running statistics are NOT the identity.  The offset
    convolutions of the deformable layers give offsets of a few pixels (some beyond the +-max(h, w) / 4 clamp of the 1/32 map, some
    samples outside the map), the descriptor head's offsets likewise.
    The score head has no bias anywhere, so the logits are centred through the weights: one channel is a constant all the way --
    x1[15] = SELU(block1.bn2.bias[15]) behind an all-zero filter, passed on by one-hot 1x1 / centre-tap weights (conv1 row 31,
    score_head.0 row 7, score_head.2 / .4 row 3), each SELU multiplying the positive constant by 1.0507 -- and score_head.6 weighs it
    so that every logit is shifted by exactly `score_shift`.  The other channels of score_head.6 carry `score_gain`.  With the
    defaults the 0.2 threshold falls inside the distribution of the NMS survivors (tests/test_aliked_cpu.py asserts it)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def conv(name, cout, cin, k, gain=1.0):
        sd[name] = rn(cout, cin, k, k, scale=gain / math.sqrt(cin * k * k))

    def bn(name, c):
        sd[f"{name}.weight"] = 1.0 + 0.2 * rn(c)
        sd[f"{name}.bias"] = 0.1 * rn(c)
        sd[f"{name}.running_mean"] = 0.2 * rn(c)
        sd[f"{name}.running_var"] = 0.5 + torch.rand(c, generator=g)

    ch = [3, 16, 32, 64, 128]
    for b in range(1, 5):
        cin, cout = ch[b - 1], ch[b]
        for j in (1, 2):
            ci = cin if j == 1 else cout
            if b >= 3:
                conv(f"block{b}.conv{j}.offset_conv.weight", 18, ci, 3, gain=3.0)
                sd[f"block{b}.conv{j}.offset_conv.bias"] = rn(18)
                conv(f"block{b}.conv{j}.regular_conv.weight", cout, ci, 3)
            else:
                conv(f"block{b}.conv{j}.weight", cout, ci, 3, gain=2.0 if b == 1 and j == 1 else 1.0)
            bn(f"block{b}.bn{j}", cout)
        if b >= 2:
            conv(f"block{b}.downsample.weight", cout, cin, 1)
    for i in range(1, 5):
        conv(f"conv{i}.weight", 32, ch[i], 1)
    conv("score_head.0.weight", 8, 128, 1)
    conv("score_head.2.weight", 4, 8, 3)
    conv("score_head.4.weight", 4, 4, 3)
    conv("score_head.6.weight", 1, 4, 3, gain=score_gain)
    # the constant channel (see above)
    sd["block1.conv2.weight"][15] = 0.0
    for k, v in (("weight", 1.0), ("bias", 1.0), ("running_mean", 0.0), ("running_var", 1.0)):
        sd[f"block1.bn2.{k}"][15] = v
    for name, row, col in (("conv1.weight", 31, 15), ("score_head.0.weight", 7, 31), ("score_head.2.weight", 3, 7), ("score_head.4.weight", 3, 3)):
        sd[name][row] = 0.0
        sd[name][row, col, sd[name].shape[2] // 2, sd[name].shape[3] // 2] = 1.0
    selu_scale = 1.0507009873554805
    sd["score_head.6.weight"][0, 3] = 0.0
    sd["score_head.6.weight"][0, 3, 1, 1] = score_shift / selu_scale**5
    sd["desc_head.agg_weights"] = rn(16, 128, 128, scale=1.0 / math.sqrt(16 * 128))
    sd["desc_head.offset_conv.0.weight"] = rn(32, 128, 3, 3, scale=1.0 / 3.0)  # (the patch is 9 unit vectors)
    sd["desc_head.offset_conv.0.bias"] = 0.3 * rn(32)
    sd["desc_head.offset_conv.2.weight"] = rn(32, 32, 1, 1, scale=3.0 / math.sqrt(32))
    sd["desc_head.offset_conv.2.bias"] = rn(32)
    sd["desc_head.sf_conv.weight"] = rn(128, 128, 1, 1)  # (a sample is a unit vector, or an interpolation of four)
    return sd


ALIKE_CFG = {"alike-t": (8, 16, 32, 64, 64), "alike-s": (8, 16, 48, 96, 96), "alike-n": (16, 32, 64, 128, 128)}  # (c1, c2, c3, c4, dim)


# logit shift that centres the NMS survivors of the seed-0 networks on the 0.5 threshold at score_gain 3 (measured with the restatement
# on the seeded test images: the survivors' median logit at gain 1 is about -0.85 / -1.3 / +1.0)
ALIKE_SCORE_SHIFT = {"alike-t": 2.5, "alike-s": 3.9, "alike-n": -3.0}


def alike_state_dict(variant: str = "alike-t", seed: int = 0, score_gain: float = 3.0, score_shift: float | None = None, fallback: bool = False) -> dict:
    """Seeded ALIKE weights (upstream's key names; the `num_batches_tracked` counters of the BatchNorms included, a loader has to skip
    them).  Convolutions are Kaiming-scaled (ReLU), BatchNorm running statistics are NOT the identity, the shortcuts carry a bias.
    convhead2 has no bias and sees ReLU outputs, all positive, so a plain draw leaves the score logits far from zero (alike-t below,
    alike-n above): the score row is centred over the channels of each branch and carries `score_gain`, and one channel is a constant
    all the way -- x1[c1 - 1] = ReLU(block1.bn2.bias) = 1 behind an all-zero filter, passed on by a one-hot row of conv1 -- which the
    score row weighs with `score_shift` (the descriptor rows with zero), so that every logit is shifted by exactly that.  With the
    defaults (`score_shift=None`: ALIKE_SCORE_SHIFT) the 0.5 threshold falls inside the distribution of the NMS survivors;
    `fallback=True` lowers the shift by 8, which keeps every score below it (the mean fallback).  tests/test_alike_cpu.py asserts both."""
    c1, c2, c3, c4, dim = ALIKE_CFG[variant]
    if score_shift is None:
        score_shift = ALIKE_SCORE_SHIFT[variant]
    if fallback:
        score_shift -= 8.0
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def conv(name, cout, cin, k, gain=math.sqrt(2.0)):
        sd[name] = rn(cout, cin, k, k, scale=gain / math.sqrt(cin * k * k))

    def bn(name, c):
        sd[f"{name}.weight"] = 1.0 + 0.2 * rn(c)
        sd[f"{name}.bias"] = 0.1 * rn(c)
        sd[f"{name}.running_mean"] = 0.2 * rn(c)
        sd[f"{name}.running_var"] = 0.5 + torch.rand(c, generator=g)
        sd[f"{name}.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    ch = [3, c1, c2, c3, c4]
    for b in range(1, 5):
        cin, cout = ch[b - 1], ch[b]
        for j in (1, 2):
            conv(f"block{b}.conv{j}.weight", cout, cin if j == 1 else cout, 3, gain=2.0 * math.sqrt(2.0) if b == 1 and j == 1 else math.sqrt(2.0))
            bn(f"block{b}.bn{j}", cout)
        if b >= 2:
            conv(f"block{b}.downsample.weight", cout, cin, 1, gain=1.0)
            sd[f"block{b}.downsample.bias"] = 0.1 * rn(cout)
    dq = dim // 4
    for i in range(1, 5):
        conv(f"conv{i}.weight", dq, ch[i], 1)
    head = rn(dim + 1, dim, 1, 1, scale=1.0 / math.sqrt(dim))
    row = head[dim, :, 0, 0].reshape(4, dq)
    row = (row - row.mean(dim=1, keepdim=True)) * score_gain
    head[dim, :, 0, 0] = row.reshape(-1)
    # the constant channel (see above)
    sd["block1.conv2.weight"][c1 - 1] = 0.0
    for k, v in (("weight", 1.0), ("bias", 1.0), ("running_mean", 0.0), ("running_var", 1.0)):
        sd[f"block1.bn2.{k}"][c1 - 1] = v
    sd["conv1.weight"][dq - 1] = 0.0
    sd["conv1.weight"][dq - 1, c1 - 1, 0, 0] = 1.0
    head[:dim, dq - 1] = 0.0
    head[dim, dq - 1, 0, 0] = score_shift
    sd["convhead2.weight"] = head
    return sd


# XFeat (verlab/accelerated_features XFeatModel): (state-dict block, [(cin, cout, kernel)] of its BasicLayers, final plain convolution)
XFEAT_BLOCKS = [
    ("block1", [(1, 4, 3), (4, 8, 3), (8, 8, 3), (8, 24, 3)], None),
    ("block2", [(24, 24, 3), (24, 24, 3)], None),
    ("block3", [(24, 64, 3), (64, 64, 3), (64, 64, 1)], None),
    ("block4", [(64, 64, 3), (64, 64, 3), (64, 64, 3)], None),
    ("block5", [(64, 128, 3), (128, 128, 3), (128, 128, 3), (128, 64, 1)], None),
    ("block_fusion", [(64, 64, 3), (64, 64, 3)], (64, 64)),
    ("heatmap_head", [(64, 64, 1), (64, 64, 1)], (64, 1)),
    ("keypoint_head", [(64, 64, 1), (64, 64, 1), (64, 64, 1)], (64, 65)),
]


def xfeat_state_dict(seed: int = 0, logit_gain: float = 0.5, dustbin_bias: float = 0.5, reliability_gain: float = 1.5) -> dict:
    """Seeded XFeat weights with upstream's key names, the `num_batches_tracked` counters and two `fine_matcher.*` tensors included
    (a loader has to skip both).  Convolutions are Kaiming-scaled, BatchNorm running statistics are NOT the identity.  The last
    key-point convolution carries `logit_gain` and the dustbin `dustbin_bias`, so that the 65-way soft-max has peaks on both sides of
    the 0.05 detection threshold (uniform would be 1/65).  The reliability convolution sees ReLU outputs, all positive: its weights are
    centred over the channels and its bias is -1, and `reliability_gain` then spreads the logits over about a unit either side of zero, so
    the sigmoid is not saturated (tests/test_xfeat_cpu.py asserts the key-point count on the seeded image and the reliability range)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    sd["skip1.1.weight"] = rn(24, 1, 1, 1, scale=0.5)
    sd["skip1.1.bias"] = rn(24, scale=0.1)
    for name, layers, last in XFEAT_BLOCKS:
        for i, (cin, cout, k) in enumerate(layers):
            sd[f"{name}.{i}.layer.0.weight"] = rn(cout, cin, k, k, scale=math.sqrt(2.0 / (cin * k * k)))
            sd[f"{name}.{i}.layer.1.running_mean"] = rn(cout, scale=0.2)
            sd[f"{name}.{i}.layer.1.running_var"] = 0.5 + torch.rand(cout, generator=g)
            sd[f"{name}.{i}.layer.1.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)
        if last is not None:
            cin, cout = last
            gain = {"keypoint_head": logit_gain, "heatmap_head": reliability_gain}.get(name, 1.0)
            sd[f"{name}.{len(layers)}.weight"] = rn(cout, cin, 1, 1, scale=gain / math.sqrt(cin))
            sd[f"{name}.{len(layers)}.bias"] = rn(cout, scale=0.05)
    sd["keypoint_head.3.bias"][64] = dustbin_bias
    sd["heatmap_head.2.weight"] -= sd["heatmap_head.2.weight"].mean()
    sd["heatmap_head.2.bias"][0] = -1.0
    sd["fine_matcher.0.weight"] = rn(512, 128, scale=1.0 / math.sqrt(128))
    sd["fine_matcher.0.bias"] = rn(512, scale=0.05)
    return sd


# (cin, cout, kernel, conv index in upstream's flat `ops` list, BatchNorm behind it): naver/r2d2 Quad_L2Net_ConfCFS
R2D2_LAYERS = ((3, 32, 3, 0, True), (32, 32, 3, 3, True), (32, 64, 3, 6, True), (64, 64, 3, 9, True), (64, 128, 3, 12, True),
               (128, 128, 3, 15, True), (128, 128, 2, 18, True), (128, 128, 2, 20, True), (128, 128, 2, 22, False))  # fmt: skip


def r2d2_state_dict(seed: int = 0, clf_gain: float = 0.15, sal_gain: float = 0.1, sal_shift: float = 2.2, checkpoint: bool = False) -> dict:
    """Seeded R2D2 weights (Quad_L2Net_ConfCFS, upstream's key names: `ops.N` of the flat ModuleList, `clf`, `sal`; the
    `num_batches_tracked` counters of the affine-free BatchNorms included, a loader has to skip them).  Convolutions are Kaiming-scaled
    and carry a bias, BatchNorm running statistics are NOT the identity.  Both heads see x^2, all positive: their rows are centred over
    the channels and scaled by the gains over sqrt(128) (the final map has a standard deviation near 3 on the seeded images), so the two logits differ by about a
    unit either side of zero and the saliency logit spreads around `sal_shift` = softplus^-1(0.7 / 0.3): the default thresholds 0.7 /
    0.7 cut through both maps instead of saturating (tests/test_r2d2_cpu.py asserts it).  checkpoint=True wraps the dict as upstream's
    files do: {'net': 'Quad_L2Net_ConfCFS()', 'state_dict': {'module.' + key: ...}}."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for cin, cout, k, op, bn in R2D2_LAYERS:
        sd[f"ops.{op}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
        sd[f"ops.{op}.bias"] = torch.randn(cout, generator=g) * 0.1
        if bn:
            sd[f"ops.{op + 1}.running_mean"] = torch.randn(cout, generator=g) * 0.2
            sd[f"ops.{op + 1}.running_var"] = 0.5 + torch.rand(cout, generator=g)
            sd[f"ops.{op + 1}.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)
    clf = torch.randn(2, 128, 1, 1, generator=g)
    sal = torch.randn(1, 128, 1, 1, generator=g)
    sd["clf.weight"] = (clf - clf.mean(dim=1, keepdim=True)) * (clf_gain / math.sqrt(128))
    sd["clf.bias"] = torch.tensor([0.0, 0.5])
    sd["sal.weight"] = (sal - sal.mean(dim=1, keepdim=True)) * (sal_gain / math.sqrt(128))
    sd["sal.bias"] = torch.tensor([sal_shift])
    if checkpoint:
        return {"net": "Quad_L2Net_ConfCFS()", "state_dict": {"module." + k: v for k, v in sd.items()}}
    return sd


# (cin, cout, index in DenseFeatureExtractionModule.model): mihaidusmanu/d2-net lib/model_test.py, VGG-16 cut at conv4_3
D2NET_LAYERS = ((3, 64, 0), (64, 64, 2), (64, 128, 5), (128, 128, 7), (128, 256, 10), (256, 256, 12), (256, 256, 14), (256, 512, 17), (512, 512, 19),
                (512, 512, 21))  # fmt: skip


def d2net_state_dict(seed: int = 0, checkpoint: bool = False) -> dict:
    """Seeded D2-Net / RoRD weights under upstream's key names (`dense_feature_extraction.model.N.{weight,bias}`): Kaiming-scaled 3x3
    convolutions, biases near 0.1 in size.  The first layer sees `x * 255 - mean` (hundreds), so the maps grow to the thousands; the
    detector is scale-free.  checkpoint=True wraps the dict as upstream's files do: {'model': state dict}."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for cin, cout, op in D2NET_LAYERS:
        sd[f"dense_feature_extraction.model.{op}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
        sd[f"dense_feature_extraction.model.{op}.bias"] = torch.randn(cout, generator=g) * 0.1
    return {"model": sd} if checkpoint else sd


# torchvision cfg "E" / "A" up to the fourth pool: Parskatt/DeDoDe encoders VGG19 (vgg19_bn().features[:40]) and VGG (size "11",
# vgg11_bn().features[:22]); "M" = MaxPool2d(2, 2)
DEDODE_ENCODERS = {"detector": (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M"),
                   "descriptor": (64, "M", 128, "M", 256, 256, "M", 512, 512, "M")}  # fmt: skip
# ConvRefiner(in, hidden, out) per scale 8, 4, 2, 1 and the number of hidden blocks: dedode_detector_L / dedode_descriptor_B as recalled
# from upstream's factory functions (out = context for the next scale + 1 key-point logit / 256 description channels)
DEDODE_REFINERS = {"detector": (8, ((512, 512, 256 + 1), (512, 256, 128 + 1), (256, 128, 64 + 1), (128, 64, 1 + 1))),
                   "descriptor": (5, ((512, 512, 256 + 256), (512, 256, 128 + 256), (256, 64, 32 + 256), (96, 32, 1 + 256)))}  # fmt: skip


def dedode_state_dicts(seed: int = 0, logit_gain: float = 0.3, refiners: dict | None = None) -> tuple:
    """Seeded DeDoDe weights -> (detector state dict, descriptor state dict) under upstream's key names (`encoder.layers.N.*` of the
    truncated torchvision VGG-BN, `decoder.layers.S.{block1,hidden_blocks.I}.{0,1,3}.*`, `.out_conv.*`), the BatchNorm
    `num_batches_tracked` counters included (a loader has to skip them).  BatchNorm statistics are NOT the identity.  Convolutions in
    front of a ReLU'd input carry sqrt(2 / fan_in), the depth-wise 5x5 (which sees a linear layer's output) sqrt(1 / 25), so a
    refiner's eight residual-free blocks neither grow nor fade and nothing comes near the 65504 of the split mode's f16 planes; the
    logit rows of every out_conv carry `logit_gain` / sqrt(hidden): four scales add up to key-point logits a few units wide, which the
    soft-max over the image turns into scores spread over decades instead of one saturated peak.  `refiners` replaces the table of
    widths (tests: a checkpoint with other widths must load)."""
    g = torch.Generator().manual_seed(seed)
    refiners = refiners or DEDODE_REFINERS

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def bn(sd, p, c):
        sd[p + ".weight"] = 1.0 + rn(c, scale=0.1)
        sd[p + ".bias"] = rn(c, scale=0.1)
        sd[p + ".running_mean"] = rn(c, scale=0.2)
        sd[p + ".running_var"] = 0.5 + torch.rand(c, generator=g)
        sd[p + ".num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    def block(sd, p, cin, c, depthwise):
        sd[p + ".0.weight"] = rn(c, 1, 5, 5, scale=0.2) if depthwise else rn(c, cin, 1, 1, scale=math.sqrt(2.0 / cin))
        sd[p + ".0.bias"] = rn(c, scale=0.1)
        bn(sd, p + ".1", c)
        sd[p + ".3.weight"] = rn(c, c, 1, 1, scale=math.sqrt(2.0 / c))
        sd[p + ".3.bias"] = rn(c, scale=0.1)

    out = []
    for model in ("detector", "descriptor"):
        sd, op, cin = {}, 0, 3
        for v in DEDODE_ENCODERS[model]:
            if v == "M":
                op += 1
                continue
            sd[f"encoder.layers.{op}.weight"] = rn(v, cin, 3, 3, scale=math.sqrt(2.0 / (cin * 9)))
            sd[f"encoder.layers.{op}.bias"] = rn(v, scale=0.1)
            bn(sd, f"encoder.layers.{op + 1}", v)
            cin, op = v, op + 3
        nblk, table = refiners[model]
        P = 1 if model == "detector" else 256
        for s, (rin, hidden, rout) in zip((8, 4, 2, 1), table):
            p = f"decoder.layers.{s}"
            block(sd, p + ".block1", rin, hidden, False)
            for i in range(nblk):
                block(sd, f"{p}.hidden_blocks.{i}", hidden, hidden, True)
            w = rn(rout, hidden, 1, 1, scale=1.0 / math.sqrt(hidden))
            w[:P] *= logit_gain
            sd[p + ".out_conv.weight"] = w
            sd[p + ".out_conv.bias"] = rn(rout, scale=0.1)
        out.append(sd)
    return tuple(out)


# (cin, cout, index in torchvision's vgg16().features): VGG-16 to conv5_3, imcui/hloc/extractors/netvlad.py:64-68
NETVLAD_LAYERS = ((3, 64, 0), (64, 64, 2), (64, 128, 5), (128, 128, 7), (128, 256, 10), (256, 256, 12), (256, 256, 14), (256, 512, 17), (512, 512, 19),
                  (512, 512, 21), (512, 512, 24), (512, 512, 26), (512, 512, 28))  # fmt: skip
NETVLAD_MODEL_NAMES = ("VGG16-NetVLAD-Pitts30K", "VGG16-NetVLAD-TokyoTM")


def netvlad_synth_state(seed: int = 0, whiten: bool = True, score_gain: float = 6.0) -> dict:
    """Seeded NetVLAD weights under the names of the reference module's state dict (`backbone.N.{weight,bias}`, `netvlad.score_proj.weight`
    [64,512,1], `netvlad.centers` [512,64], `whiten.{weight,bias}`) plus `preprocess.mean` [3] (the checkpoint's averageImage), float32 torch
    tensors.  numpy's default_rng, one stream in a fixed order with the whitening LAST: the 134 M whitening weights (512 MB) are regenerated
    wherever they are needed and never stored, and `whiten=False` gives the same other tensors.  Kaiming-scaled 3x3 convolutions; the score
    rows have norm `score_gain`, so that a unit-norm pixel gets scores of that spread and the soft-max is sharp but not one-hot; centers of
    the size of a unit vector's entries."""
    import numpy as np

    rng = np.random.default_rng(seed)
    sd = {}
    for cin, cout, op in NETVLAD_LAYERS:
        sd[f"backbone.{op}.weight"] = rng.standard_normal((cout, cin, 3, 3), dtype=np.float32) * np.float32(math.sqrt(2.0 / (cin * 9)))
        sd[f"backbone.{op}.bias"] = rng.standard_normal(cout, dtype=np.float32) * np.float32(0.1)
    sd["netvlad.score_proj.weight"] = rng.standard_normal((64, 512, 1), dtype=np.float32) * np.float32(score_gain)
    sd["netvlad.centers"] = rng.standard_normal((512, 64), dtype=np.float32) * np.float32(1.0 / math.sqrt(512.0))
    sd["preprocess.mean"] = np.array([122.68, 116.67, 104.01], dtype=np.float32)
    if whiten:
        sd["whiten.weight"] = rng.standard_normal((4096, 32768), dtype=np.float32) * np.float32(1.0 / math.sqrt(32768.0))
        sd["whiten.bias"] = rng.standard_normal(4096, dtype=np.float32) * np.float32(0.01)
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def netvlad_write_mat(path, state: dict) -> None:
    """`state` (netvlad_synth_state) as the MATLAB checkpoint that imcui/hloc/extractors/netvlad.py:76-120 parses: `net.layers` a 1-D cell of
    structs with a `weights` cell -- layers 0..28 line up with the truncated VGG `features` (convolutions [S,S,IN,OUT] + bias), layer 30 the
    score [D,K] / NEGATED centre [D,K] pair, layer 33 the whitening pair ([1,1,IN,OUT], [OUT]; empty without whitening) -- and
    `net.meta.normalization.averageImage` [2,2,3] (an image of the mean colour, read at [0, 0]).  Data only; needs scipy."""
    import numpy as np
    from scipy.io import savemat

    def cell(*arrs):
        c = np.empty(len(arrs), dtype=object)  # filled element by element: np.array([a, b], dtype=object) of equal shapes collapses
        for i, a in enumerate(arrs):
            c[i] = a
        return c

    convs = {op: (state[f"backbone.{op}.weight"].numpy(), state[f"backbone.{op}.bias"].numpy()) for _, _, op in NETVLAD_LAYERS}
    layers = np.empty(34, dtype=object)
    for i in range(34):
        layers[i] = {"weights": cell()}
    for op, (w, b) in convs.items():
        layers[op] = {"weights": cell(np.ascontiguousarray(w.transpose(2, 3, 1, 0)), b)}
    layers[30] = {"weights": cell(np.ascontiguousarray(state["netvlad.score_proj.weight"].numpy()[:, :, 0].T), -state["netvlad.centers"].numpy())}
    if "whiten.weight" in state:
        layers[33] = {"weights": cell(state["whiten.weight"].numpy().T[None, None], state["whiten.bias"].numpy())}
    mean = np.ascontiguousarray(np.broadcast_to(state["preprocess.mean"].numpy().reshape(1, 1, 3), (2, 2, 3)))  # (loadmat squeezes a [1,1,3] to [3])
    savemat(str(path), {"net": {"layers": layers, "meta": {"normalization": {"averageImage": mean}}}})


PLACES_DEPTHS = {18: (2, 2, 2, 2), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}  # torchvision's resnetNN `layers`


def places_synth_state(backbone: int = 50, fc_output_dim: int = 2048, seed: int = 0) -> dict:
    """Seeded CosPlace / EigenPlaces weights under the state-dict names of upstream's GeoLocalizationNet on a torchvision ResNet
    (`backbone.0.weight`, `backbone.1.*`, `backbone.{4..7}.<block>.conv{1,2,3}.weight` / `.bn{1,2,3}.*` / `.downsample.{0,1}.*`,
    `aggregation.1.p`, `aggregation.3.{weight,bias}`), in the module's own order, `num_batches_tracked` included.  backbone 18 / 50 / 101 /
    152.  numpy's default_rng, one stream in that order.  He-initialised convolutions; BatchNorm weights in [0.8, 1.2), biases and running
    means of spread 0.1 and running variances in [0.5, 1.5), so a fold that is skipped or mis-ordered shows; the last BatchNorm of every
    block has a tenth of that weight, so the residual sum stays O(1) through 50 blocks; p = 2.7, a non-integer exponent."""
    import numpy as np

    rng = np.random.default_rng(seed)
    sd = {}

    def conv(name, cout, cin, k):
        sd[name + ".weight"] = rng.standard_normal((cout, cin, k, k), dtype=np.float32) * np.float32(math.sqrt(2.0 / (cin * k * k)))

    def bn(name, c, gain=1.0):
        sd[name + ".weight"] = (np.float32(0.8) + np.float32(0.4) * rng.random(c, dtype=np.float32)) * np.float32(gain)
        sd[name + ".bias"] = rng.standard_normal(c, dtype=np.float32) * np.float32(0.1)
        sd[name + ".running_mean"] = rng.standard_normal(c, dtype=np.float32) * np.float32(0.1)
        sd[name + ".running_var"] = np.float32(0.5) + rng.random(c, dtype=np.float32)
        sd[name + ".num_batches_tracked"] = np.array(1000, dtype=np.int64)

    bott = backbone != 18
    conv("backbone.0", 64, 3, 7)
    bn("backbone.1", 64)
    cin = 64
    for L, depth in enumerate(PLACES_DEPTHS[backbone]):
        width = 64 << L
        cout = 4 * width if bott else width
        for i in range(depth):
            p, stride = f"backbone.{4 + L}.{i}", 2 if (i == 0 and L > 0) else 1
            convs = ((cin, width, 1), (width, width, 3), (width, cout, 1)) if bott else ((cin, width, 3), (width, width, 3))
            for j, (ci, co, k) in enumerate(convs, 1):
                conv(f"{p}.conv{j}", co, ci, k)
                bn(f"{p}.bn{j}", co, 0.1 if j == len(convs) else 1.0)
            if stride != 1 or cin != cout:
                conv(f"{p}.downsample.0", cout, cin, 1)
                bn(f"{p}.downsample.1", cout)
            cin = cout
    sd["aggregation.1.p"] = np.array([2.7], dtype=np.float32)
    sd["aggregation.3.weight"] = rng.standard_normal((fc_output_dim, cin), dtype=np.float32) * np.float32(1.0 / math.sqrt(cin))
    sd["aggregation.3.bias"] = rng.standard_normal(fc_output_dim, dtype=np.float32) * np.float32(0.01)
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


# (cin, cout, kernel) of kornia.feature.HardNet / SOSNet and the index of each convolution in their nn.Sequential (BatchNorm at + 1)
PATCHDESC_LAYERS = ((1, 32, 3), (32, 32, 3), (32, 64, 3), (64, 64, 3), (64, 128, 3), (128, 128, 3), (128, 128, 8))
HARDNET_CONV_OPS = (0, 3, 6, 9, 12, 15, 19)
SOSNET_CONV_OPS = (1, 4, 7, 10, 13, 16, 20)


def _patchdesc_synth_state(seed: int, root: str, ops) -> dict:
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for (cin, cout, k), op in zip(PATCHDESC_LAYERS, ops):
        sd[f"{root}.{op}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
        sd[f"{root}.{op + 1}.running_mean"] = torch.randn(cout, generator=g) * 0.2
        sd[f"{root}.{op + 1}.running_var"] = 0.5 + torch.rand(cout, generator=g)
        sd[f"{root}.{op + 1}.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)
    return sd


def hardnet_synth_state(seed: int = 0) -> dict:
    """Seeded HardNet weights under kornia.feature.HardNet's key names (`features.N.weight`, bias-free convolutions; `features.N+1.
    running_mean / running_var / num_batches_tracked` of the BatchNorm2d(affine=False) behind each).  Kaiming-scaled convolutions; the
    running variances lie in [0.5, 1.5) and the running means are not zero, so a BatchNorm fold that is skipped or mis-ordered shows."""
    return _patchdesc_synth_state(seed, "features", HARDNET_CONV_OPS)


def sosnet_synth_state(seed: int = 0) -> dict:
    """The same for kornia.feature.SOSNet (`layers.N.*`; `layers.0` is the parameter-free InstanceNorm2d)."""
    return _patchdesc_synth_state(seed, "layers", SOSNET_CONV_OPS)


LANET_WIDTHS = (32, 64, 128, 256)
LANET_PREFIX = "interestpoint_module."


def lanet_synth_state(seed: int = 0, k: int = 3, bias: bool = True, bn: bool = False, widths=LANET_WIDTHS, conv_bias: bool = False,
                      score_gain: float = 2.0, loc_gain: float = 0.6, aware_gain: float = 0.5) -> dict:
    """Seeded LANet (network_v0 PointModel) weights under the key names tests/lanet_reference.py restates (`interestpoint_module.*`,
    the `num_batches_tracked` counters included, a loader has to skip them).  Convolutions are He-initialised, BatchNorm statistics are
    away from (0, 1).  The two tails see ReLU outputs, all positive and growing with depth, so a plain draw leaves their outputs far
    from zero: every tail row is calibrated on a seeded 64 x 64 uniform image (drawn from the same generator, evaluated here with
    torch's own convolutions) to zero mean and a chosen standard deviation -- `score_gain` spreads the sigmoid over (0, 1), `loc_gain`
    keeps the tanh out of saturation on most cells, `aware_gain` keeps the three level weights well away from one-hot
    (tests/test_lanet_cpu.py asserts the three).  `k`, `bias`, `bn`: the kernel size of des_conv2 / des_conv3, whether they carry a bias, whether a BatchNorm follows."""
    c1, c2, c3, c4 = widths
    g = torch.Generator().manual_seed(seed)
    sd = {}
    p = LANET_PREFIX

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def conv(name, cout, cin, kk, gain=math.sqrt(2.0), with_bias=False):
        sd[f"{p}{name}.weight"] = rn(cout, cin, kk, kk, scale=gain / math.sqrt(cin * kk * kk))
        if with_bias:
            sd[f"{p}{name}.bias"] = 0.1 * rn(cout)

    def norm(name, c):
        sd[f"{p}{name}.weight"] = 1.0 + 0.2 * rn(c)
        sd[f"{p}{name}.bias"] = 0.1 * rn(c)
        sd[f"{p}{name}.running_mean"] = 0.2 * rn(c)
        sd[f"{p}{name}.running_var"] = 0.5 + torch.rand(c, generator=g)
        sd[f"{p}{name}.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    for name, cin, cout in (("1a", 3, c1), ("1b", c1, c1), ("2a", c1, c2), ("2b", c2, c2), ("3a", c2, c3), ("3b", c3, c3), ("4a", c3, c4), ("4b", c4, c4),
                            ("Da", c4, 256), ("Pa", c4, 256)):  # fmt: skip
        conv("conv" + name, cout, cin, 3, gain=2.0 * math.sqrt(2.0) if name == "1a" else math.sqrt(2.0), with_bias=conv_bias)
        norm("bn" + name, cout)

    # the hidden maps of the two heads on a seeded 64 x 64 uniform image, with the weights drawn so far (eval BatchNorm, ReLU)
    import torch.nn.functional as F

    def layer(name, x):
        x = F.conv2d(x, sd[f"{p}conv{name}.weight"], sd.get(f"{p}conv{name}.bias"), padding=1)
        x = F.batch_norm(x, sd[f"{p}bn{name}.running_mean"], sd[f"{p}bn{name}.running_var"], sd[f"{p}bn{name}.weight"], sd[f"{p}bn{name}.bias"], False, 0.0, 1e-5)
        return F.relu(x)

    x = (torch.rand(1, 3, 64, 64, generator=g) - 0.5) / 0.225
    for name in ("1a", "1b", "2a", "2b", "3a", "3b", "4a", "4b"):
        x = layer(name, x)
        if name in ("1b", "2b", "3b"):
            x = F.max_pool2d(x, 2, 2)

    def tail(name, hidden, stds):
        w = rn(len(stds), 256, 3, 3, scale=1.0 / math.sqrt(256 * 9))
        raw = F.conv2d(hidden, w, None, padding=1)[0]
        mean, std = raw.mean(dim=(1, 2)), raw.std(dim=(1, 2))
        scale = torch.tensor(stds) / std
        sd[f"{p}{name}.weight"] = w * scale.view(-1, 1, 1, 1)
        sd[f"{p}{name}.bias"] = -mean * scale + 0.05 * rn(len(stds))

    tail("convDb", layer("Da", x), [aware_gain] * 3 + [score_gain])
    tail("convPb", layer("Pa", x), [loc_gain] * 2)
    for lvl, cin in ((2, c2), (3, c3)):
        conv(f"des_conv{lvl}", 256, cin, k, gain=1.0, with_bias=bias)
        if bn:
            norm(f"des_bn{lvl}", 256)
    return sd


# name, cin, cout, stride, InstanceNorm + ReLU behind it, score level of the raw output: the backbone tests/darkfeat_reference.py restates
DARKFEAT_LAYERS = (("conv0", 3, 32, 1, True, -1), ("conv1", 32, 32, 1, True, 0), ("conv2", 32, 64, 2, True, -1), ("conv3", 64, 64, 1, True, 1),
                   ("conv4", 64, 128, 2, True, -1), ("conv5", 128, 128, 1, True, -1), ("conv6_0", 128, 128, 1, True, -1),
                   ("conv6_1", 128, 128, 1, True, -1), ("conv6_2", 128, 128, 1, False, 2))  # fmt: skip


def darkfeat_synth_state(seed: int = 0, bias: bool = False, peak_gain: float = 1.0, share: float = 0.5) -> dict:
    """Seeded DarkFeat weights under upstream's key names (`convN.0.weight`, with `bias` also `convN.0.bias`; `clf.*`; the 0-d
    `moving_avg_params.{0,1,2}`), plus the BatchNorm-statistics keys of a `conv0.1` that upstream drops before loading (a loader has to
    skip them).  Convolutions are He-initialised.  A plain draw leaves every score near softplus(0)^2 = 0.48 times the classifier's
    probability, far below the 0.5 threshold, and such a network tests nothing.  So the rest is calibrated on a seeded 64 x 64 uniform
    image (drawn from the same generator, evaluated here with torch's own operations): `moving_avg_params[i]` = the standard deviation
    of raw map i / `peak_gain` (the peakiness sees unit-variance input), the classifier's logit difference gets unit standard deviation,
    and its bias is bisected so that `share` of the 3x3 maxima of the score map inside the 5-pixel border band lie above 0.5 on that
    image.  At the sizes the tests use (32x48, 50x70, 96x128 and 40x56, seed 0) 70 %, 53 %, 47 % and 62 % of those maxima (10, 36, 207
    and 21 of them) lie above 0.5; tests/test_darkfeat_cpu.py asserts 40 % .. 75 %."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(seed)
    sd = {}

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    for name, cin, cout, _, _, _ in DARKFEAT_LAYERS:
        sd[f"{name}.0.weight"] = rn(cout, cin, 3, 3, scale=math.sqrt(2.0) / math.sqrt(cin * 9))
        if bias:
            sd[f"{name}.0.bias"] = 0.1 * rn(cout)
    sd["conv0.1.running_mean"], sd["conv0.1.running_var"] = 0.2 * rn(32), 0.5 + torch.rand(32, generator=g)
    sd["conv0.1.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    # ---- the calibration image through the backbone
    img = torch.rand(1, 3, 64, 64, generator=g)
    H, W = img.shape[-2:]
    x = (img - img.mean()) / img.std()
    peaks = [None] * 3

    def peak(x, d):
        h, w = x.shape[-2:]
        xp = F.pad(x, (d, d, d, d), mode="reflect")
        box = sum(xp[..., i * d : i * d + h, j * d : j * d + w] for i in range(3) for j in range(3)) / 9.0
        return (F.softplus(x - box) * F.softplus(x - x.mean(dim=1, keepdim=True))).max(dim=1, keepdim=True).values

    for name, _, _, stride, norm, tap in DARKFEAT_LAYERS:
        x = F.conv2d(x, sd[f"{name}.0.weight"], sd.get(f"{name}.0.bias"), stride=stride, padding=1)
        if tap >= 0:
            m = x.std() / peak_gain
            sd[f"moving_avg_params.{tap}"] = m.clone()
            peaks[tap] = F.interpolate(peak(x / m, (3, 2, 1)[tap]), size=(H, W), mode="bilinear", align_corners=True)
        if norm:
            x = F.relu(F.instance_norm(x, eps=1e-5))
    level_sum = (peaks[0] / 6.0 + peaks[1] * (2.0 / 6.0)) + peaks[2] * (3.0 / 6.0)
    w = rn(2, 128, 1, 1, scale=1.0 / math.sqrt(128))
    logit = F.conv2d(x * x, w)
    diff = logit[:, 1] - logit[:, 0]
    w = w / diff.std()
    logit = F.conv2d(x * x, w)

    def share_above(b1):
        prob = torch.softmax(logit + torch.tensor([0.0, b1]).view(1, 2, 1, 1), dim=1)[:, 1:2]
        score = (level_sum * F.interpolate(prob, size=(H, W), mode="bilinear", align_corners=True))[0, 0]
        peaks_ = (score == F.max_pool2d(score[None, None], 3, 1, 1)[0, 0])[5:-5, 5:-5]
        return (score[5:-5, 5:-5][peaks_] > 0.5).float().mean().item()

    lo, hi = -30.0, 30.0
    for _ in range(40):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if share_above(mid) < share else (lo, mid)
    sd["clf.weight"] = w
    sd["clf.bias"] = torch.tensor([0.0, (lo + hi) / 2])
    return sd


# ------------------------------------------------------------------ SFD2
def _sfd2_simple_nms(s: torch.Tensor, r: int) -> torch.Tensor:
    """SuperPoint's simple_nms on [B,H,W]."""
    import torch.nn.functional as F

    def mp(x):
        return F.max_pool2d(x, 2 * r + 1, 1, r)

    zeros = torch.zeros_like(s)
    mask = s == mp(s)
    for _ in range(2):
        supp = mp(mask.float()) > 0
        ss = torch.where(supp, zeros, s)
        mask = mask | ((ss == mp(ss)) & ~supp)
    return torch.where(mask, s, zeros)


def sfd2_synth_state(seed: int = 0, widths=(64, 128, 256), blocks: int = 3, groups: int = 32, hidden: int = 256, k_pb: int = 3, k_db: int = 1,
                     bn: bool = True, bias: bool = True, share: float = 0.5) -> dict:
    """Seeded SFD2 (ResNet4x) weights under the recalled key names: `conv1a.0.weight` / `.0.bias` / `.1.{weight, bias, running_mean,
    running_var, num_batches_tracked}` .. `conv3b`, `conv4.{i}.conv{1,2,3}.weight` + `bn{1,2,3}.*` (conv2 grouped: [C, C / groups, 3, 3]),
    `convPa` / `convDa` like the trunk, `convPb.*` (16 outputs), `convDb.*` (128).  Convolutions are He-initialised, BatchNorm statistics
    are drawn near the identity.  A plain draw leaves every score near sigmoid(0) with a spread nobody chose, so convPb is calibrated on a
    seeded 64 x 64 uniform image (drawn from the same generator, evaluated here with torch's own operations): its logits get a standard
    deviation of 2 and its bias is bisected so that `share` of the radius-4 NMS maxima inside the 4-pixel border band lie above 0.5 on
    that image.  At the sizes the tests use (32x48, 50x70, 96x128 and 40x56, seed 0) 32 %, 38 %, 53 % and 42 % of those maxima (19, 53,
    198 and 31 of them) lie above 0.5; tests/test_sfd2_cpu.py asserts 30 % .. 70 %.  Every maximum is far above the default conf_th of
    0.001."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(seed)
    sd = {}
    c1, c2, c3 = widths

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def conv(stem, bnstem, cout, cin, k, with_bias, gain=1.0):
        sd[f"{stem}.weight"] = rn(cout, cin, k, k, scale=math.sqrt(2.0) / math.sqrt(cin * k * k))
        if with_bias:
            sd[f"{stem}.bias"] = 0.1 * rn(cout)
        if bn:
            sd[f"{bnstem}.weight"] = gain * (1.0 + 0.1 * rn(cout))
            sd[f"{bnstem}.bias"] = 0.1 * rn(cout)
            sd[f"{bnstem}.running_mean"] = 0.1 * rn(cout)
            sd[f"{bnstem}.running_var"] = 0.75 + 0.5 * torch.rand(cout, generator=g)
            sd[f"{bnstem}.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    chain = (("conv1a", 3, c1), ("conv1b", c1, c1), ("conv2a", c1, c2), ("conv2b", c2, c2), ("conv3a", c2, c3), ("conv3b", c3, c3))
    for name, cin, cout in chain:
        conv(f"{name}.0", f"{name}.1", cout, cin, 3, bias)
    for i in range(blocks):
        conv(f"conv4.{i}.conv1", f"conv4.{i}.bn1", c3, c3, 1, False)
        conv(f"conv4.{i}.conv2", f"conv4.{i}.bn2", c3, c3 // groups, 3, False)
        conv(f"conv4.{i}.conv3", f"conv4.{i}.bn3", c3, c3, 1, False, gain=0.5)
    conv("convPa.0", "convPa.1", hidden, c3, 3, bias)
    conv("convDa.0", "convDa.1", hidden, c3, 3, bias)
    sd["convDb.weight"] = rn(128, hidden, k_db, k_db, scale=1.0 / math.sqrt(hidden * k_db * k_db))
    sd["convDb.bias"] = 0.1 * rn(128)
    wpb = rn(16, hidden, k_pb, k_pb, scale=1.0 / math.sqrt(hidden * k_pb * k_pb))

    # ---- the calibration image through the network
    def layer(x, stem, bnstem, stride=1, ngroups=1, pad=1):
        x = F.conv2d(x, sd[f"{stem}.weight"], sd.get(f"{stem}.bias"), stride=stride, padding=pad, groups=ngroups)
        if bn:
            x = F.batch_norm(x, sd[f"{bnstem}.running_mean"], sd[f"{bnstem}.running_var"], sd[f"{bnstem}.weight"], sd[f"{bnstem}.bias"], False, 0.0, 1e-5)
        return x

    img = torch.rand(1, 3, 64, 64, generator=g)
    x = (img - torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    for name, _, _ in chain:
        x = F.relu(layer(x, f"{name}.0", f"{name}.1", stride=2 if name in ("conv1b", "conv2b") else 1))
    for i in range(blocks):
        y = F.relu(layer(x, f"conv4.{i}.conv1", f"conv4.{i}.bn1", pad=0))
        y = F.relu(layer(y, f"conv4.{i}.conv2", f"conv4.{i}.bn2", ngroups=groups))
        x = F.relu(layer(y, f"conv4.{i}.conv3", f"conv4.{i}.bn3", pad=0) + x)
    hid = F.relu(layer(x, "convPa.0", "convPa.1"))
    logit = F.conv2d(hid, wpb, padding=k_pb // 2)
    wpb = wpb * (2.0 / logit.std())
    logit = F.conv2d(hid, wpb, padding=k_pb // 2)

    def share_above(b0):
        s = F.pixel_shuffle(torch.sigmoid(logit + b0), 4)[:, 0]
        nms = _sfd2_simple_nms(s, 4)[0, 4:-4, 4:-4]
        return (nms[nms > 0] > 0.5).float().mean().item()

    lo, hi = -30.0, 30.0
    for _ in range(40):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if share_above(mid) < share else (lo, mid)
    sd["convPb.weight"] = wpb
    sd["convPb.bias"] = torch.full((16,), (lo + hi) / 2)
    return sd


def liftfeat_synth_state(seed: int = 0, kenc: bool = True, ffn: int = 128, n_layers: int = 3, logit_gain: float = 0.7, dustbin_bias: float = 0.5,
                         key_gain: float = 0.5) -> dict:
    """Seeded LiftFeat weights under the key names of tests/liftfeat_reference.py's table: XFeat's trunk (`xfeat_state_dict` without
    `heatmap_head.*` and `fine_matcher.*`, counters included), `normal_head.{0,1,2}.{conv,bn}.*` + `normal_head.3.*`, and
    `feature_boost.{denc,nenc,kenc}.{0,2,4}.*`, `.layers.{i}.{attn.{q,k,v,proj},norm1,ffn.{0,2},norm2}.*`, `.final_proj.*`.  Linears are
    drawn at 1 / sqrt(fan-in), BatchNorm and LayerNorm near the identity.  The key-point head takes XFeat's `logit_gain` / `dustbin_bias`
    (0.7: peaks on both sides of the 0.05 threshold, 24 key-points on the 32x48 image of the tests); the AFT key projections carry `key_gain`, so that the soft-max over the tokens is spread
    (tests/test_liftfeat_cpu.py asserts the key-point counts at 96x128 and 32x48 and that no soft-max column puts more than 0.9 of its
    weight on one token)."""
    sd = {k: v for k, v in xfeat_state_dict(seed, logit_gain=logit_gain, dustbin_bias=dustbin_bias).items()
          if not k.startswith(("heatmap_head.", "fine_matcher."))}  # fmt: skip
    g = torch.Generator().manual_seed(seed + 7919)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def linear(stem, cin, cout, gain=1.0):
        sd[f"{stem}.weight"] = rn(cout, cin, scale=gain / math.sqrt(cin))
        sd[f"{stem}.bias"] = rn(cout, scale=0.05)

    for s, c in enumerate((64, 32, 16)):
        sd[f"normal_head.{s}.conv.weight"] = rn(c // 2, c, 3, 3, scale=math.sqrt(2.0 / (c * 9)))
        sd[f"normal_head.{s}.conv.bias"] = rn(c // 2, scale=0.1)
        sd[f"normal_head.{s}.bn.weight"] = 1.0 + 0.1 * rn(c // 2)
        sd[f"normal_head.{s}.bn.bias"] = 0.1 * rn(c // 2)
        sd[f"normal_head.{s}.bn.running_mean"] = 0.1 * rn(c // 2)
        sd[f"normal_head.{s}.bn.running_var"] = 0.75 + 0.5 * torch.rand(c // 2, generator=g)
        sd[f"normal_head.{s}.bn.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)
    sd["normal_head.3.weight"] = rn(3, 8, 1, 1, scale=1.0 / math.sqrt(8))
    sd["normal_head.3.bias"] = rn(3, scale=0.1)
    fb = "feature_boost"
    encoders = {"denc": (64, 64, 64), "nenc": (192, 128, 64, 64)}
    if kenc:
        encoders["kenc"] = (65, 128, 64, 64)
    for name, widths in encoders.items():
        for i in range(len(widths) - 1):
            linear(f"{fb}.{name}.{2 * i}", widths[i], widths[i + 1])
    for i in range(n_layers):
        p = f"{fb}.layers.{i}"
        linear(f"{p}.attn.q", 64, 64)
        linear(f"{p}.attn.k", 64, 64, gain=key_gain)
        linear(f"{p}.attn.v", 64, 64)
        linear(f"{p}.attn.proj", 64, 64)
        linear(f"{p}.ffn.0", 64, ffn)
        linear(f"{p}.ffn.2", ffn, 64)
        for n in ("norm1", "norm2"):
            sd[f"{p}.{n}.weight"] = 1.0 + 0.1 * rn(64)
            sd[f"{p}.{n}.bias"] = 0.1 * rn(64)
    linear(f"{fb}.final_proj", 64, 64)
    return sd


LISRD_BACKBONE = (("1_1", 3, 64, False), ("1_2", 64, 64, True), ("2_1", 64, 64, False), ("2_2", 64, 64, True), ("3_1", 64, 128, False), ("3_2", 128, 128, True),
                  ("4_1", 128, 256, False), ("4_2", 256, 256, False))  # fmt: skip


def lisrd_synth_state(seed: int = 0) -> dict:
    """Seeded LISRD weights (LISRD_CONFIG of the wrapper: desc_size 128, tile 3, n_clusters 8, meta_desc_dim 128) under the recalled key
    names: `_backbone._conv{a}_{b}.*` / `_backbone._bn{a}_{b}.*`, per variance `conv_{v}_1` / `bn_{v}_1` / `conv_{v}_2` (descriptor head),
    `conv_meta_{v}_1` / `bn_meta_{v}_1` / `conv_meta_{v}_2` (meta head), `vlad_{v}.conv.weight` [8,128,1,1] and `vlad_{v}.centroids` [8,128].
    Convolutions are He-initialised.  Every block is conv -> ReLU -> BatchNorm, so a plain draw of the statistics would let the scale of
    the activations drift from layer to layer: each BatchNorm is calibrated on a seeded 64 x 64 uniform image (drawn from the same
    generator, evaluated here with torch's own operations) -- running_mean / running_var are the measured per-channel statistics of the
    ReLU output times a factor drawn in 0.8 .. 1.25, weight 1 +- 0.1, bias 0.1 N(0, 1) -- so every layer's output has about zero mean and
    unit variance and no channel dies.  NetVLAD's assignment layer is drawn N(0, 1) / sqrt(128) and scaled so that its logits have a
    standard deviation of 2 on the calibration image's unit vectors: the median top assignment lies near 0.6, well away from 1 / 8
    (tests/test_lisrd_cpu.py asserts 0.3 .. 0.9)."""
    import torch.nn.functional as F

    from .backend import lisrd_variances  # (the library's own statement of the four names and their order)

    g = torch.Generator().manual_seed(seed)
    sd = {}

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def block(x, conv, bn, cin, cout):
        sd[f"{conv}.weight"] = rn(cout, cin, 3, 3, scale=math.sqrt(2.0) / math.sqrt(cin * 9))
        sd[f"{conv}.bias"] = 0.1 * rn(cout)
        y = F.relu(F.conv2d(x, sd[f"{conv}.weight"], sd[f"{conv}.bias"], padding=1))
        sd[f"{bn}.weight"] = 1.0 + 0.1 * rn(cout)
        sd[f"{bn}.bias"] = 0.1 * rn(cout)
        sd[f"{bn}.running_mean"] = y.mean((0, 2, 3)) + 0.05 * rn(cout)
        sd[f"{bn}.running_var"] = (y.var((0, 2, 3)) + 1e-3) * (0.8 + 0.45 * torch.rand(cout, generator=g))
        sd[f"{bn}.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)
        return F.batch_norm(y, sd[f"{bn}.running_mean"], sd[f"{bn}.running_var"], sd[f"{bn}.weight"], sd[f"{bn}.bias"], False, 0.0, 1e-5)

    x = torch.rand(1, 3, 64, 64, generator=g)
    for tag, cin, cout, pool in LISRD_BACKBONE:
        x = block(x, f"_backbone._conv{tag}", f"_backbone._bn{tag}", cin, cout)
        if pool:
            x = F.avg_pool2d(x, 2, 2)
    for v in lisrd_variances():
        for pre in ("", "_meta"):
            hid = block(x, f"conv{pre}_{v}_1", f"bn{pre}_{v}_1", 256, 256)
            sd[f"conv{pre}_{v}_2.weight"] = rn(128, 256, 1, 1, scale=1.0 / math.sqrt(256))
            sd[f"conv{pre}_{v}_2.bias"] = 0.1 * rn(128)
        meta = F.normalize(F.conv2d(hid, sd[f"conv_meta_{v}_2.weight"], sd[f"conv_meta_{v}_2.bias"]), dim=1)
        w = rn(8, 128, 1, 1, scale=1.0 / math.sqrt(128))
        sd[f"vlad_{v}.conv.weight"] = w * (2.0 / F.conv2d(meta, w).std())
        sd[f"vlad_{v}.centroids"] = rn(8, 128, scale=1.0 / math.sqrt(128))
    return sd
