"""ALIKE (alike-t / alike-s / alike-n) restated in plain torch from the published source (Shiaoming/ALIKE: alnet.py, soft_detect.py,
alike.py) and the wrapper imcui/hloc/extractors/alike.py: the checker of the HIP path.  Upstream's source is not vendored, so this
file is the written definition (parity-unpinned, like DISK, ALIKED and XFeat; INTEGRATION.md, "ALIKE: what is pinned").

Module and parameter names are upstream's, so an upstream checkpoint loads strictly.  Every function works in the dtype of its
input (float32 or float64).  The position arithmetic is written operation by operation, because upstream's float32 round trip
`idx / (w - 1) * 2 - 1` -> `(n + 1) / 2 * (w - 1)` does not always return the integer it started from, and the descriptor is read at the
TRUNCATED result; `bilinear_zero` is grid_sample(bilinear, align_corners=True, zeros) in the operation order of ATen's scalar kernel
(`((g + 1) / 2) * (size - 1)`, weights from the opposite corners), so that both sides round alike.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

# (c1, c2, c3, c4, dim); DKD radius 2 for all.  alike-l (32, 64, 128, 128, 128) has a second head layer and is not restated.
CFG = {"alike-t": (8, 16, 32, 64, 64), "alike-s": (8, 16, 48, 96, 96), "alike-n": (16, 32, 64, 128, 128)}
RADIUS = 2


def conv3x3(cin, cout):
    return nn.Conv2d(cin, cout, 3, padding=1, bias=False)


class ConvBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1, self.bn1 = conv3x3(cin, cout), nn.BatchNorm2d(cout)
        self.conv2, self.bn2 = conv3x3(cout, cout), nn.BatchNorm2d(cout)

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(x)))


class ResBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1, self.bn1 = conv3x3(cin, cout), nn.BatchNorm2d(cout)
        self.conv2, self.bn2 = conv3x3(cout, cout), nn.BatchNorm2d(cout)
        self.downsample = nn.Conv2d(cin, cout, 1, bias=True)

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return F.relu(out + self.downsample(x))


def simple_nms(scores: torch.Tensor, radius: int) -> torch.Tensor:
    """SuperPoint's simple_nms, [B,1,H,W]."""

    def mp(x):
        return F.max_pool2d(x, kernel_size=radius * 2 + 1, stride=1, padding=radius)

    zeros = torch.zeros_like(scores)
    mask = scores == mp(scores)
    for _ in range(2):
        supp = mp(mask.to(scores.dtype)) > 0
        ss = torch.where(supp, zeros, scores)
        new = ss == mp(ss)
        mask = mask | (new & ~supp)
    return torch.where(mask, scores, zeros)


def banded_nms(score: torch.Tensor, radius: int = RADIUS) -> torch.Tensor:
    """simple_nms of one score map [h,w] with rows / columns [0, r] and [h - r, h) / [w - r, w) zeroed."""
    nms = simple_nms(score[None, None], radius)[0, 0].clone()
    nms[: radius + 1] = 0
    nms[:, : radius + 1] = 0
    nms[-radius:] = 0
    nms[:, -radius:] = 0
    return nms


def select(score: torch.Tensor, conf: dict, radius: int = RADIUS):
    """ALIKE's selection on one score map [h,w] -> (flat indices in OUTPUT order, branch, cut) with branch one of "topk", "threshold",
    "mean" and cut = whether the n_limit / top_k cut dropped candidates.  Output order: row-major, or descending score (ties to the
    lower flat index) for the top_k route and after an n_limit cut.  conf: top_k, detection_threshold, max_keypoints (= n_limit; <= 0:
    no limit)."""
    top_k, thr, n_limit = int(conf["top_k"]), float(conf["detection_threshold"]), int(conf["max_keypoints"])
    flat = banded_nms(score, radius).reshape(-1)
    desc = False
    cut = False
    if top_k > 0:
        branch = "topk"
        idx = torch.nonzero(flat > 0)[:, 0]  # (only positive survivors: upstream's topk would pad with zero-score pixels)
        order = torch.argsort(flat[idx], descending=True, stable=True)  # idx ascending + stable: ties to the lower index
        cut = len(idx) > top_k
        idx = idx[order][:top_k]
        desc = True
    else:
        branch = "threshold"
        idx = torch.nonzero(flat > thr)[:, 0] if thr > 0 else flat.new_zeros(0, dtype=torch.long)
        if thr <= 0 or len(idx) == 0:
            branch = "mean"
            idx = torch.nonzero(flat > score.mean())[:, 0]
    if n_limit > 0 and len(idx) > n_limit:
        cut = True
        if not desc:
            order = torch.argsort(flat[idx], descending=True, stable=True)
            idx = idx[order]
        idx = idx[:n_limit]
    return idx, branch, cut


def norm_pos(v: torch.Tensor, size: int) -> torch.Tensor:
    return v / (size - 1) * 2 - 1


def pix_pos(n: torch.Tensor, size: int) -> torch.Tensor:
    return (n + 1) / 2 * (size - 1)


def bilinear_zero(x: torch.Tensor, fx: torch.Tensor, fy: torch.Tensor) -> torch.Tensor:
    """x [C,h,w] sampled at pixel positions (fx, fy) [N] -> [N,C]: grid_sample's bilinear rule, corners outside the map are zero; the
    sum runs nw, ne, sw, se with one rounding per operation."""
    C, h, w = x.shape
    x0, y0 = torch.floor(fx), torch.floor(fy)
    x1, y1 = x0 + 1, y0 + 1
    wx0, wx1, wy0, wy1 = x1 - fx, fx - x0, y1 - fy, fy - y0
    flat = x.reshape(C, -1)
    out = None
    for yy, xx, wgt in ((y0, x0, wx0 * wy0), (y0, x1, wx1 * wy0), (y1, x0, wx0 * wy1), (y1, x1, wx1 * wy1)):
        yi, xi = yy.long(), xx.long()
        ok = (yi >= 0) & (yi < h) & (xi >= 0) & (xi < w)
        v = flat[:, yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)] * ok.to(x.dtype)[None]
        term = v * wgt[None]
        out = term if out is None else out + term
    return out.t()


def soft_argmax(score: torch.Tensor, idx: torch.Tensor, radius: int = RADIUS, temperature: float = 0.1) -> torch.Tensor:
    """Sub-pixel positions (x, y) [N,2] in pixels of candidates idx (flat) on the raw score map [h,w] (DKD's soft-argmax)."""
    h, w = score.shape
    k = 2 * radius + 1
    xy = torch.stack([idx % w, idx // w], 1).to(score.dtype)
    if len(idx) == 0:
        return xy
    patches = F.unfold(score[None, None], k, padding=radius)[0].t()[idx]  # [N, k*k]
    lin = torch.linspace(-radius, radius, k, dtype=score.dtype, device=score.device)
    grid = torch.stack(torch.meshgrid(lin, lin, indexing="ij")[::-1], -1).reshape(-1, 2)  # (x, y) per patch cell, row-major
    mx = patches.max(dim=1).values[:, None]
    e = ((patches - mx) / temperature).exp()
    return xy + e @ grid / e.sum(dim=1)[:, None]


def keypoints_from(score: torch.Tensor, idx: torch.Tensor, sub_pixel: bool):
    """-> (normalised positions [N,2], key-points in pixels [N,2], scores [N], truncated descriptor pixel (x, y) [N,2] long)."""
    h, w = score.shape
    if sub_pixel:
        xy = soft_argmax(score, idx)
    else:
        xy = torch.stack([idx % w, idx // w], 1).to(score.dtype)
    kn = torch.stack([norm_pos(xy[:, 0], w), norm_pos(xy[:, 1], h)], 1)
    kp = torch.stack([pix_pos(kn[:, 0], w), pix_pos(kn[:, 1], h)], 1)
    ks = bilinear_zero(score[None], kp[:, 0], kp[:, 1])[:, 0] if len(idx) else score.new_zeros(0)
    return kn, kp, ks, kp.long()


def describe(descriptor_map: torch.Tensor, kp: torch.Tensor, sub_pixel: bool) -> torch.Tensor:
    """descriptor_map [dim,h,w] (normalised), kp [N,2] key-points in pixels -> descriptors [N,dim], normalised once more."""
    if len(kp) == 0:
        return descriptor_map.new_zeros(0, descriptor_map.shape[0])
    if sub_pixel:
        d = bilinear_zero(descriptor_map, kp[:, 0], kp[:, 1])
    else:
        pix = kp.long()
        d = descriptor_map[:, pix[:, 1], pix[:, 0]].t()
    return F.normalize(d, p=2.0, dim=1)


class ALIKEReference(nn.Module):
    def __init__(self, state_dict: dict | None = None, model_name: str = "alike-t"):
        super().__init__()
        c1, c2, c3, c4, dim = CFG[model_name]
        self.dim = dim
        self.block1 = ConvBlock(3, c1)
        self.block2, self.block3, self.block4 = ResBlock(c1, c2), ResBlock(c2, c3), ResBlock(c3, c4)
        self.conv1, self.conv2 = nn.Conv2d(c1, dim // 4, 1, bias=False), nn.Conv2d(c2, dim // 4, 1, bias=False)
        self.conv3, self.conv4 = nn.Conv2d(c3, dim // 4, 1, bias=False), nn.Conv2d(c4, dim // 4, 1, bias=False)
        self.convhead2 = nn.Conv2d(dim, dim + 1, 1, bias=False)
        if state_dict is not None:
            self.load_state_dict(state_dict, strict=True)
        self.eval().requires_grad_(False)

    @staticmethod
    def pad(image: torch.Tensor) -> torch.Tensor:
        h, w = image.shape[-2:]
        return F.pad(image, (0, (32 - w % 32) % 32, 0, (32 - h % 32) % 32))

    def branches(self, image: torch.Tensor):
        """padded image -> (x1, x2, x3, x4) and the four dim/4-channel branch maps before up-sampling."""
        x1 = self.block1(image)
        x2 = self.block2(F.max_pool2d(x1, 2))
        x3 = self.block3(F.max_pool2d(x2, 4))
        x4 = self.block4(F.max_pool2d(x3, 4))
        f = [F.relu(c(x)) for c, x in ((self.conv1, x1), (self.conv2, x2), (self.conv3, x3), (self.conv4, x4))]
        return (x1, x2, x3, x4), f

    def dense(self, image: torch.Tensor) -> dict:
        """image [B,3,h,w] in [0,1] -> score_map [B,1,h,w], descriptor_map [B,dim,h,w] (normalised, cropped), x4 and f2..f4 (padded
        size).  The wrapper multiplies by 255.0 and upstream divides by 255.0 again, in the image's dtype."""
        assert image.shape[1] == 3, "ALIKE asserts three channels"
        h, w = image.shape[-2:]
        img = self.pad((image * 255.0) / 255.0)
        xs, f = self.branches(img)
        up = [f[0]] + [F.interpolate(t, scale_factor=s, mode="bilinear", align_corners=True) for t, s in zip(f[1:], (2, 8, 32))]
        y = self.convhead2(torch.cat(up, 1))[:, :, :h, :w]
        return {"score_map": torch.sigmoid(y[:, self.dim :]), "descriptor_map": F.normalize(y[:, : self.dim], p=2.0, dim=1),
                "x4": xs[3], "f2": f[1], "f3": f[2], "f4": f[3]}  # fmt: skip

    def forward(self, image: torch.Tensor, conf: dict) -> dict:
        """The wrapper's outputs per image (lists): keypoints [N,2] pixels, scores [N], descriptors [N,dim]; + the dense maps."""
        d = self.dense(image)
        out = {"keypoints": [], "scores": [], "descriptors": [], "pixels": [], "score_map": d["score_map"], "descriptor_map": d["descriptor_map"]}
        sub = bool(conf.get("sub_pixel", False))
        for b in range(image.shape[0]):
            sm = d["score_map"][b, 0]
            idx, _, _ = select(sm, conf)
            _, kp, ks, pix = keypoints_from(sm, idx, sub)
            out["keypoints"].append(kp)
            out["scores"].append(ks)
            out["pixels"].append(pix)
            out["descriptors"].append(describe(d["descriptor_map"][b], kp, sub))
        return out
