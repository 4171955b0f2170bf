"""Torch restatement of XFeat (verlab/accelerated_features: modules/model.py `XFeatModel`, modules/xfeat.py `XFeat.detectAndCompute`,
modules/interpolator.py `InterpolateSparse2d`), the call behind imcui/hloc/extractors/xfeat.py:26-34, for the XFeat parity tests.
Upstream's source is not vendored, so this file is the written definition the HIP path is checked against; every step that has an ATen
kernel uses it (F.interpolate, F.grid_sample, F.max_pool2d, F.instance_norm through nn.InstanceNorm2d, softmax), so sampling and
rounding rules are torch's.  State-dict key names are upstream's: a real `xfeat.pt` loads (its `fine_matcher.*` entries are ignored).

One choice upstream leaves open is made canonical here: `argsort(-scores)` does not order equal scores; this file sorts stably, so
equal scores keep row-major (flat index ascending) order."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

DETECTION_THRESHOLD = 0.05  # XFeat.__init__'s default; imcui/hloc/extractors/xfeat.py never passes its own `keypoint_threshold`


class BasicLayer(nn.Module):
    def __init__(self, cin, cout, kernel_size=3, stride=1, padding=1):
        super().__init__()
        self.layer = nn.Sequential(nn.Conv2d(cin, cout, kernel_size, padding=padding, stride=stride, bias=False),
                                   nn.BatchNorm2d(cout, affine=False), nn.ReLU(inplace=True))  # fmt: skip

    def forward(self, x):
        return self.layer(x)


def unfold8(x: torch.Tensor) -> torch.Tensor:
    """[B,C,H,W] -> [B,C*64,H/8,W/8]: each 8x8 cell as 64 channels, channel = dy * 8 + dx (upstream's `_unfold2d(x, ws=8)`)."""
    B, C, H, W = x.shape
    x = x.unfold(2, 8, 8).unfold(3, 8, 8).reshape(B, C, H // 8, W // 8, 64)
    return x.permute(0, 1, 4, 2, 3).reshape(B, -1, H // 8, W // 8)


def unshuffle_heatmap(scores: torch.Tensor) -> torch.Tensor:
    """[B,64,h,w] -> [B,1,8h,8w]: channel dy * 8 + dx of cell (y, x) goes to pixel (8y + dy, 8x + dx)."""
    B, _, h, w = scores.shape
    return scores.permute(0, 2, 3, 1).reshape(B, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, 1, h * 8, w * 8)


class XFeatModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm = nn.InstanceNorm2d(1)
        self.skip1 = nn.Sequential(nn.AvgPool2d(4, stride=4), nn.Conv2d(1, 24, 1, stride=1, padding=0))
        self.block1 = nn.Sequential(BasicLayer(1, 4, stride=1), BasicLayer(4, 8, stride=2), BasicLayer(8, 8, stride=1), BasicLayer(8, 24, stride=2))
        self.block2 = nn.Sequential(BasicLayer(24, 24, stride=1), BasicLayer(24, 24, stride=1))
        self.block3 = nn.Sequential(BasicLayer(24, 64, stride=2), BasicLayer(64, 64, stride=1), BasicLayer(64, 64, 1, padding=0))
        self.block4 = nn.Sequential(BasicLayer(64, 64, stride=2), BasicLayer(64, 64, stride=1), BasicLayer(64, 64, stride=1))
        self.block5 = nn.Sequential(BasicLayer(64, 128, stride=2), BasicLayer(128, 128, stride=1), BasicLayer(128, 128, stride=1),
                                    BasicLayer(128, 64, 1, padding=0))  # fmt: skip
        self.block_fusion = nn.Sequential(BasicLayer(64, 64, stride=1), BasicLayer(64, 64, stride=1), nn.Conv2d(64, 64, 1, padding=0))
        self.heatmap_head = nn.Sequential(BasicLayer(64, 64, 1, padding=0), BasicLayer(64, 64, 1, padding=0), nn.Conv2d(64, 1, 1), nn.Sigmoid())
        self.keypoint_head = nn.Sequential(BasicLayer(64, 64, 1, padding=0), BasicLayer(64, 64, 1, padding=0), BasicLayer(64, 64, 1, padding=0),
                                           nn.Conv2d(64, 65, 1))  # fmt: skip

    def forward(self, x):
        with torch.no_grad():
            x = x.mean(dim=1, keepdim=True)
            x = self.norm(x)
        x1 = self.block1(x)
        x2 = self.block2(x1 + self.skip1(x))
        x3 = self.block3(x2)
        x4 = self.block4(x3)
        x5 = self.block5(x4)
        x4 = F.interpolate(x4, (x3.shape[-2], x3.shape[-1]), mode="bilinear")
        x5 = F.interpolate(x5, (x3.shape[-2], x3.shape[-1]), mode="bilinear")
        feats = self.block_fusion(x3 + x4 + x5)
        heatmap = self.heatmap_head(feats)
        keypoints = self.keypoint_head(unfold8(x))
        return feats, keypoints, heatmap


def load_model(state_dict: dict) -> XFeatModel:
    """Strict on the network's own keys; `fine_matcher.*` (the semi-dense refinement MLP) and BatchNorm counters are ignored."""
    net = XFeatModel().eval()
    own = {k: v for k, v in state_dict.items() if not k.startswith("fine_matcher.")}
    missing, unexpected = net.load_state_dict(own, strict=False)
    missing = [k for k in missing if not k.endswith("num_batches_tracked")]
    if missing or unexpected:
        raise ValueError(f"XFeat state dict: missing {missing[:4]}, unexpected {list(unexpected)[:4]}")
    return net


def preprocess(x: torch.Tensor):
    """`preprocess_tensor`: bilinear resize to multiples of 32 -> (image, rh, rw)."""
    H, W = x.shape[-2:]
    Hr, Wr = (H // 32) * 32, (W // 32) * 32
    rh, rw = H / Hr, W / Wr
    return F.interpolate(x, (Hr, Wr), mode="bilinear", align_corners=False), rh, rw


def nms(x: torch.Tensor, threshold: float = DETECTION_THRESHOLD, kernel_size: int = 5) -> list[torch.Tensor]:
    """`XFeat.NMS` for [B,1,H,W]: per image the (x, y) long pixels, row-major, that equal their window's maximum and exceed the threshold."""
    local_max = F.max_pool2d(x, kernel_size=kernel_size, stride=1, padding=kernel_size // 2)
    pos = (x == local_max) & (x > threshold)
    return [k.nonzero()[..., 1:].flip(-1) for k in pos]


def sample(x: torch.Tensor, pos: torch.Tensor, H: int, W: int, mode: str) -> torch.Tensor:
    """`InterpolateSparse2d(mode)(x, pos, H, W)`: x [B,C,h,w], pos [B,N,2] -> [B,N,C]; the grid is normalised by the IMAGE size (H, W)
    whatever the size of x, in pos's arithmetic (integer pixels / integer sizes -> float32)."""
    grid = 2.0 * (pos / torch.tensor([W - 1, H - 1], device=pos.device, dtype=pos.dtype)) - 1.0
    out = F.grid_sample(x, grid.unsqueeze(-2).to(x.dtype), mode=mode, align_corners=False)
    return out.permute(0, 2, 3, 1).squeeze(-2)


def dense_maps(net: XFeatModel, image: torch.Tensor) -> dict:
    """M1 [B,64,Hr/8,Wr/8] (L2-normalised feats), K1h [B,1,Hr,Wr], reliability [B,1,Hr/8,Wr/8], rh, rw."""
    with torch.no_grad():
        x, rh, rw = preprocess(image.float())
        M1, K1, H1 = net(x)
        M1 = F.normalize(M1, dim=1)
        scores = F.softmax(K1 * 1.0, 1)[:, :64]
        K1h = unshuffle_heatmap(scores)
    return {"M1": M1, "K1h": K1h, "reliability": H1, "rh": rh, "rw": rw}


def select(M1: torch.Tensor, K1h: torch.Tensor, H1: torch.Tensor, rh: float, rw: float, top_k: int, threshold: float = DETECTION_THRESHOLD) -> dict:
    """Steps 5-11 of detectAndCompute on given maps of ONE image ([1,...] tensors), as the wrapper's batch of one runs them ->
    keypoints [N,2], scores [N], descriptors [N,64], plus the unscaled integer pixels `xy` [N,2]."""
    with torch.no_grad():
        _, _, Hr, Wr = K1h.shape
        mk = nms(K1h, threshold=threshold, kernel_size=5)[0][None]  # [1,N,2] long (a batch of one has no padding rows)
        sc = (sample(K1h, mk, Hr, Wr, "nearest") * sample(H1, mk, Hr, Wr, "bilinear")).squeeze(-1)
        sc[torch.all(mk == 0, dim=-1)] = -1
        idxs = torch.argsort(-sc, dim=-1, stable=True)
        mk = torch.gather(mk, 1, idxs[..., None].expand(-1, -1, 2))[:, :top_k]
        sc = torch.gather(sc, -1, idxs)[:, :top_k]
        feats = F.normalize(sample(M1, mk, Hr, Wr, "bicubic"), dim=-1)
        kp = mk * torch.tensor([rw, rh], device=mk.device).view(1, 1, -1)
        valid = sc[0] > 0
    return {"keypoints": kp[0][valid], "scores": sc[0][valid], "descriptors": feats[0][valid], "xy": mk[0][valid]}


def detect_and_compute(net: XFeatModel, image: torch.Tensor, top_k: int = -1, threshold: float = DETECTION_THRESHOLD) -> list[dict]:
    """`XFeat.detectAndCompute(image, top_k)` evaluated per image (what the wrapper's batch of one returns for each)."""
    out = []
    for b in range(image.shape[0]):
        m = dense_maps(net, image[b : b + 1])
        out.append(select(m["M1"], m["K1h"], m["reliability"], m["rh"], m["rw"], top_k, threshold))
    return out
