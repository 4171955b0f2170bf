"""LiftFeat (`models.liftfeat_wrapper.LiftFeat`, the class imcui/hloc/extractors/liftfeat.py:9 imports from the reference's empty
third_party directory) restated in plain torch from its description: the checker of the HIP path (csrc/liftfeat.hip).  Upstream's network
is not vendored and no checkpoint was at hand, so parity with upstream's code is NOT pinned: this file is the project's definition of the
network.  Everything recalled rather than read -- layer names, widths, `align_corners`, slopes, state-dict keys -- stands in ONE table
(`TABLE`) below, so that a later correction is an edit of the table; INTEGRATION.md ("LiftFeat: what is pinned") lists each item.

    LiftFeat(weight, top_k, detect_threshold).extract(image HWC float 0..255) -> {"keypoints" [N,2], "scores" [N], "descriptors" [N,64]}

The trunk is XFeat's (tests/xfeat_reference.py: the same modules, the same key names).  Widths of the booster's MLPs and of the FFN, the
number of AFT layers and the presence of `kenc` are read from the checkpoint's shapes and keys.  Every step that has an ATen kernel uses
it.  `torch.argsort` leaves the order of equal scores open; `wrapper_cut` sorts stably (row-major index among equals)."""
from __future__ import annotations

import re

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import xfeat_reference as X

# ---------------------------------------------------------------- the ONE table of what is recalled (INTEGRATION.md lists each line)
TABLE = {
    "trunk_blocks": ("skip1", "block1", "block2", "block3", "block4", "block5", "block_fusion", "keypoint_head"),  # XFeat's names; no heatmap_head
    "trunk_widths": {"block1.3.layer.0.weight": (24, 8, 3, 3), "block3.0.layer.0.weight": (64, 24, 3, 3), "block5.3.layer.0.weight": (64, 128, 1, 1),
                     "block_fusion.2.weight": (64, 64, 1, 1), "keypoint_head.3.weight": (65, 64, 1, 1)},
    "pad_multiple": 32,  # zero padding at the bottom and right, then / 255
    "normal_head": "normal_head",  # .{0,1,2}.conv.{weight,bias}, .{0,1,2}.bn.{weight,bias,running_mean,running_var}, .3.{weight,bias}
    "normal_channels": (64, 32, 16, 8, 3),
    "upsample_align_corners": True,
    "upsample_slope": 0.1,  # LeakyReLU
    "normalize_eps": 1e-12,
    "booster": "feature_boost",  # .denc / .nenc / .kenc (Sequential: Linear at 0, 2, 4), .layers.{i}, .final_proj
    "booster_inputs": {"denc": 64, "nenc": 192, "kenc": 65},
    "use_normal": True,
    "aft_keys": ("attn.q", "attn.k", "attn.v", "attn.proj", "norm1", "ffn.0", "ffn.2", "norm2"),
    "layernorm_eps": 1e-6,
    "gelu": "erf",
    "nms_kernel": 5,
    "score_mode": "nearest",
    "descriptor_mode": "bicubic",
    "top_k_applied_by_extract": False,  # stored, not applied: the wrapper's own cut (liftfeat.py:42-46) is the only one
    "ignored_suffixes": ("num_batches_tracked",),
}
KNOWN_GROUPS = TABLE["trunk_blocks"] + (TABLE["normal_head"], TABLE["booster"])


def check_keys(sd: dict) -> None:
    """Refuse, naming the tensor, a key group the table does not know and a trunk width that differs from XFeat's."""
    for k, v in sd.items():
        if k.split(".")[0] not in KNOWN_GROUPS:
            raise ValueError(f"LiftFeat state dict: '{k}' belongs to no group the table knows ({', '.join(KNOWN_GROUPS)})")
    for k, shape in TABLE["trunk_widths"].items():
        if k not in sd:
            raise ValueError(f"LiftFeat state dict: '{k}' is missing")
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"LiftFeat state dict: '{k}' has shape {tuple(sd[k].shape)}, XFeat's trunk has {shape}")


def booster_config(sd: dict) -> dict:
    """Widths, depth and optional parts from the checkpoint's shapes and keys."""
    fb = TABLE["booster"]
    n_layers = 1 + max(int(m.group(1)) for k in sd for m in [re.match(rf"{fb}\.layers\.(\d+)\.", k)] if m)
    mlp = lambda name: [sd[f"{fb}.{name}.0.weight"].shape[1]] + [sd[f"{fb}.{name}.{i}.weight"].shape[0] for i in (0, 2, 4) if f"{fb}.{name}.{i}.weight" in sd]
    cfg = {"n_layers": n_layers, "ffn": sd[f"{fb}.layers.0.ffn.0.weight"].shape[0], "denc": mlp("denc"), "nenc": mlp("nenc"),
           "kenc": mlp("kenc") if f"{fb}.kenc.0.weight" in sd else None}  # fmt: skip
    for name, cin in TABLE["booster_inputs"].items():
        if cfg[name] is not None and (cfg[name][0] != cin or cfg[name][-1] != 64):
            raise ValueError(f"LiftFeat state dict: '{fb}.{name}' maps {cfg[name][0]} -> {cfg[name][-1]}, expected {cin} -> 64")
    return cfg


def mlp(widths) -> nn.Sequential:
    mods = []
    for i in range(len(widths) - 1):
        mods.append(nn.Linear(widths[i], widths[i + 1]))
        if i < len(widths) - 2:
            mods.append(nn.ReLU())
    return nn.Sequential(*mods)


class UpsampleLayer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c // 2, 3, padding=1, bias=True)
        self.bn = nn.BatchNorm2d(c // 2)

    def forward(self, x, align_corners=TABLE["upsample_align_corners"]):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=align_corners)
        return F.leaky_relu(self.bn(self.conv(x)), TABLE["upsample_slope"])


class AFTAttention(nn.Module):
    def __init__(self):
        super().__init__()
        self.q, self.k, self.v, self.proj = (nn.Linear(64, 64) for _ in range(4))

    def kv(self, x):  # x [N, 64] -> [64]
        return (F.softmax(self.k(x), dim=0) * self.v(x)).sum(0)

    def forward(self, x):
        return self.proj(torch.sigmoid(self.q(x)) * self.kv(x)[None])


class AttentionalLayer(nn.Module):
    def __init__(self, ffn):
        super().__init__()
        self.attn = AFTAttention()
        self.norm1 = nn.LayerNorm(64, eps=TABLE["layernorm_eps"])
        self.ffn = nn.Sequential(nn.Linear(64, ffn), nn.GELU(), nn.Linear(ffn, 64))
        self.norm2 = nn.LayerNorm(64, eps=TABLE["layernorm_eps"])

    def forward(self, x):
        x = self.norm1(x + self.attn(x))
        return self.norm2(x + self.ffn(x))


class FeatureBooster(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.denc, self.nenc = mlp(cfg["denc"]), mlp(cfg["nenc"])
        if cfg["kenc"] is not None:
            self.kenc = mlp(cfg["kenc"])
        self.layers = nn.ModuleList(AttentionalLayer(cfg["ffn"]) for _ in range(cfg["n_layers"]))
        self.final_proj = nn.Linear(64, 64)

    def encode(self, d, k, n):
        x = d + self.denc(d)
        if TABLE["use_normal"]:
            x = x + self.nenc(n)
        if hasattr(self, "kenc"):
            x = x + self.kenc(k)
        return x

    def forward(self, d, k, n):  # [N, 64], [N, 65], [N, 192] of ONE image -> [N, 64]
        x = self.encode(d, k, n)
        for layer in self.layers:
            x = layer(x)
        return self.final_proj(x)


class LiftFeatModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        t = X.XFeatModel()
        self.norm = t.norm
        for name in TABLE["trunk_blocks"]:
            setattr(self, name, getattr(t, name))
        c = TABLE["normal_channels"]
        self.normal_head = nn.Sequential(UpsampleLayer(c[0]), UpsampleLayer(c[1]), UpsampleLayer(c[2]), nn.Conv2d(c[3], c[4], 1))
        self.feature_boost = FeatureBooster(cfg)

    def forward1(self, x):
        """x [B,C,Hp,Wp] -> M1 [B,64,h,w], K1 [B,65,h,w], D1 [B,3,Hp,Wp]."""
        x = self.norm(x.mean(dim=1, keepdim=True))
        x1 = self.block1(x)
        x2 = self.block2(x1 + self.skip1(x))
        x3 = self.block3(x2)
        x4 = self.block4(x3)
        x5 = self.block5(x4)
        x4 = F.interpolate(x4, (x3.shape[-2], x3.shape[-1]), mode="bilinear")
        x5 = F.interpolate(x5, (x3.shape[-2], x3.shape[-1]), mode="bilinear")
        feats = self.block_fusion(x3 + x4 + x5)
        K1 = self.keypoint_head(X.unfold8(x))
        D1 = F.normalize(self.normal_head(feats), dim=1, eps=TABLE["normalize_eps"])
        return feats, K1, D1

    def forward2(self, M1, K1, D1):
        """Per image over all (Hp/8)(Wp/8) cells -> the boosted map [B,64,h,w], unit channels."""
        B, _, h, w = M1.shape
        n = X.unfold8(D1)  # channel c * 64 + dy * 8 + dx
        out = []
        for b in range(B):
            tok = lambda m: m[b].reshape(m.shape[1], -1).t()
            out.append(self.feature_boost(tok(M1), tok(K1), tok(n)).t().reshape(64, h, w))
        return F.normalize(torch.stack(out), dim=1, eps=TABLE["normalize_eps"])


def load_model(state_dict: dict) -> LiftFeatModel:
    sd = {k: v for k, v in state_dict.items() if not k.endswith(TABLE["ignored_suffixes"])}
    check_keys(sd)
    net = LiftFeatModel(booster_config(sd)).eval()
    missing, unexpected = net.load_state_dict(sd, strict=False)
    missing = [k for k in missing if not k.endswith(TABLE["ignored_suffixes"])]
    if missing or unexpected:
        raise ValueError(f"LiftFeat state dict: missing {missing[:4]}, unexpected {list(unexpected)[:4]}")
    return net


def pad_image(image: np.ndarray, dtype=torch.float32) -> torch.Tensor:
    """HWC float 0..255 -> [1,C,Hp,Wp]: zero padding at the bottom and right to multiples of 32, then / 255 (in float32, as numpy does)."""
    m = TABLE["pad_multiple"]
    H, W = image.shape[:2]
    x = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).permute(2, 0, 1)[None]
    x = F.pad(x, (0, (-W) % m, 0, (-H) % m)) / 255
    return x.to(dtype)


def dense_maps(net: LiftFeatModel, image: np.ndarray, dtype=torch.float32) -> dict:
    """heat [1,1,Hp,Wp], D1 [1,3,Hp,Wp], boosted [1,64,h,w] of one HWC image, in `dtype` (the net must be in it)."""
    with torch.no_grad():
        M1, K1, D1 = net.forward1(pad_image(image, dtype))
        boosted = net.forward2(M1, K1, D1)
        heat = X.unshuffle_heatmap(F.softmax(K1, 1)[:, :64])
    return {"M1": M1, "K1": K1, "D1": D1, "boosted": boosted, "heat": heat}


def select(heat: torch.Tensor, boosted: torch.Tensor, H: int, W: int, threshold: float) -> dict:
    """The selection of `extract` on given maps of ONE image: NMS over the PADDED map, then x < W and y < H; row-major (`nonzero`)."""
    with torch.no_grad():
        Hp, Wp = heat.shape[-2:]
        mk = X.nms(heat, threshold=threshold, kernel_size=TABLE["nms_kernel"])[0]
        mk = mk[(mk[:, 0] < W) & (mk[:, 1] < H)][None]
        sc = X.sample(heat, mk, Hp, Wp, TABLE["score_mode"]).squeeze(-1)[0]
        de = F.normalize(X.sample(boosted, mk, Hp, Wp, TABLE["descriptor_mode"]), dim=-1)[0]
    return {"keypoints": mk[0].to(heat.dtype), "scores": sc, "descriptors": de}


class LiftFeat:
    """`models.liftfeat_wrapper.LiftFeat`: `weight` is a checkpoint path or a state dict."""

    def __init__(self, weight, top_k=5000, detect_threshold=0.05, dtype=torch.float32):
        sd = torch.load(weight, map_location="cpu") if isinstance(weight, (str, bytes)) or hasattr(weight, "__fspath__") else weight
        self.net = load_model(sd).to(dtype)
        self.top_k = top_k  # stored and NOT applied by extract (TABLE["top_k_applied_by_extract"])
        self.detect_threshold = detect_threshold
        self.dtype = dtype

    def extract(self, image: np.ndarray) -> dict:
        H, W = image.shape[:2]
        m = dense_maps(self.net, image, self.dtype)
        return select(m["heat"], m["boosted"], H, W, self.detect_threshold)


def wrapper_cut(pred: dict, max_keypoints: int) -> dict:
    """liftfeat.py:42-46 with the ONE intended divergence: the argsort is stable (equal scores in row-major order)."""
    kp, de, sc = pred["keypoints"], pred["descriptors"], pred["scores"]
    if max_keypoints < len(kp):
        idxs = torch.argsort(sc, stable=True)[-max_keypoints or None :]
        kp, de, sc = kp[idxs, :2], de[idxs], sc[idxs]
    return {"keypoints": kp, "descriptors": de, "scores": sc}
