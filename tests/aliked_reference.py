"""ALIKED (aliked-n16 / aliked-n16rot) restated in plain torch from the published source (LightGlue's `lightglue/aliked.py`, itself
a port of Shiaoming/ALIKED): the checker of the HIP path.  `torchvision.ops.deform_conv2d` is restated with explicit bilinear
gathers (zero outside the map, torchvision's offset channel order: channel 2k = dy, 2k + 1 = dx of tap k).

Module and parameter names are upstream's, so an upstream checkpoint loads strictly.  DKD is decided per image (upstream's
empty-set test sums over the batch; its wrapper only ever passes one image).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

CFG = {"aliked-n16": (16, 32, 64, 128, 128, 3, 16), "aliked-n16rot": (16, 32, 64, 128, 128, 3, 16)}
N_LIMIT_MAX = 20000


def conv3x3(cin, cout):
    return nn.Conv2d(cin, cout, 3, padding=1, bias=False)


def conv1x1(cin, cout):
    return nn.Conv2d(cin, cout, 1, bias=False)


def bilinear_zero(x: torch.Tensor, py: torch.Tensor, px: torch.Tensor) -> torch.Tensor:
    """x [C,H,W]; py, px float positions of any shape S -> [C, *S]; corners outside the map contribute zero."""
    C, H, W = x.shape
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    out = x.new_zeros((C,) + tuple(py.shape))
    flat = x.reshape(C, -1)
    for dy, wy in ((0, 1 - ly), (1, ly)):
        for dx, wx in ((0, 1 - lx), (1, lx)):
            yy, xx = (y0 + dy).long(), (x0 + dx).long()
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(-1)
            v = flat[:, idx].reshape((C,) + tuple(py.shape))
            out = out + v * (wy * wx * ok)[None]
    return out


def deform_conv2d_ref(x: torch.Tensor, offset: torch.Tensor, weight: torch.Tensor, padding: int = 1) -> torch.Tensor:
    """torchvision.ops.deform_conv2d(x, offset, weight, padding=padding), stride 1, no mask, no bias.
    x [B,Cin,H,W]; offset [B, 2 k k, H, W]; weight [Cout,Cin,k,k]."""
    B, C, H, W = x.shape
    cout, _, k, _ = weight.shape
    ys = torch.arange(H, dtype=x.dtype, device=x.device)[:, None].expand(H, W)
    xs = torch.arange(W, dtype=x.dtype, device=x.device)[None, :].expand(H, W)
    cols = []
    for b in range(B):
        taps = []
        for t in range(k * k):
            py = ys - padding + t // k + offset[b, 2 * t]
            px = xs - padding + t % k + offset[b, 2 * t + 1]
            taps.append(bilinear_zero(x[b], py, px))  # [C,H,W]
        cols.append(torch.stack(taps, 1))  # [C, k*k, H, W]
    col = torch.stack(cols).reshape(B, C * k * k, H * W)
    return (weight.reshape(cout, -1) @ col).reshape(B, cout, H, W)


class DeformableConv2d(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.offset_conv = nn.Conv2d(cin, 18, 3, padding=1, bias=True)
        self.regular_conv = nn.Conv2d(cin, cout, 3, padding=1, bias=False)

    def offsets(self, x):
        h, w = x.shape[2:]
        m = max(h, w) / 4.0
        return self.offset_conv(x).clamp(-m, m)

    def forward(self, x):
        return deform_conv2d_ref(x, self.offsets(x), self.regular_conv.weight, padding=1)


class ConvBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1, self.bn1 = conv3x3(cin, cout), nn.BatchNorm2d(cout)
        self.conv2, self.bn2 = conv3x3(cout, cout), nn.BatchNorm2d(cout)

    def forward(self, x):
        x = F.selu(self.bn1(self.conv1(x)))
        return F.selu(self.bn2(self.conv2(x)))


class ResBlock(nn.Module):
    def __init__(self, cin, cout, deform):
        super().__init__()
        mk = DeformableConv2d if deform else conv3x3
        self.conv1, self.bn1 = mk(cin, cout), nn.BatchNorm2d(cout)
        self.conv2, self.bn2 = mk(cout, cout), nn.BatchNorm2d(cout)
        self.downsample = conv1x1(cin, cout)

    def forward(self, x):
        out = F.selu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return F.selu(out + self.downsample(x))


class SDDH(nn.Module):
    def __init__(self, dim, K, M):
        super().__init__()
        self.K, self.M = K, M
        self.offset_conv = nn.Sequential(nn.Conv2d(dim, 2 * M, K, bias=True), nn.SELU(), nn.Conv2d(2 * M, 2 * M, 1, bias=True))
        self.sf_conv = nn.Conv2d(dim, dim, 1, bias=False)
        self.agg_weights = nn.Parameter(torch.rand(M, dim, dim))

    def forward(self, fmap: torch.Tensor, kn: torch.Tensor) -> torch.Tensor:
        """fmap [C,h,w] (normalised, cropped), kn [N,2] key-points in [-1,1] -> descriptors [N,C]."""
        C, h, w = fmap.shape
        wh = fmap.new_tensor([w - 1.0, h - 1.0])
        max_offset = max(h, w) / 4.0
        kwh = (kn / 2 + 0.5) * wh
        N = len(kn)
        if N == 0:
            return fmap.new_zeros(0, C)
        ki = kwh.long()
        r = self.K // 2
        pad = F.pad(fmap, (r, r, r, r))
        dd = torch.arange(self.K, device=fmap.device)
        yy = (ki[:, 1, None, None] + dd[None, :, None]).expand(N, self.K, self.K)
        xx = (ki[:, 0, None, None] + dd[None, None, :]).expand(N, self.K, self.K)
        patch = pad[:, yy, xx].permute(1, 0, 2, 3)  # [N,C,K,K]
        offset = self.offset_conv(patch).clamp(-max_offset, max_offset)[:, :, 0, 0].view(N, self.M, 2)
        pos = kwh[:, None] + offset
        pos = 2.0 * pos / wh[None] - 1
        feats = F.grid_sample(fmap[None], pos.reshape(1, N * self.M, 1, 2), mode="bilinear", align_corners=True)
        feats = feats.reshape(C, N, self.M, 1).permute(1, 0, 2, 3)  # [N,C,M,1]
        feats = F.selu(self.sf_conv(feats)).squeeze(-1)  # [N,C,M]
        descs = torch.einsum("ncp,pcd->nd", feats, self.agg_weights)
        return F.normalize(descs, p=2.0, dim=1)


def simple_nms(scores: torch.Tensor, radius: int) -> torch.Tensor:
    """SuperPoint's simple_nms, [B,1,H,W]."""

    def mp(x):
        return F.max_pool2d(x, kernel_size=radius * 2 + 1, stride=1, padding=radius)

    zeros = torch.zeros_like(scores)
    mask = scores == mp(scores)
    for _ in range(2):
        supp = mp(mask.float()) > 0
        ss = torch.where(supp, zeros, scores)
        new = ss == mp(ss)
        mask = mask | (new & ~supp)
    return torch.where(mask, scores, zeros)


def dkd_select(score: torch.Tensor, radius: int, threshold: float, max_num_keypoints: int):
    """Selection rule of DKD on one score map [h,w] -> (flat indices in row-major order, branch) with branch one of "threshold",
    "mean" (fallback or threshold <= 0 without a count), "topk"; the n_limit cut keeps the highest scores, ties to the lower index."""
    h, w = score.shape
    nms = simple_nms(score[None, None], radius)[0, 0].clone()
    nms[:radius] = 0
    nms[-radius:] = 0
    nms[:, :radius] = 0
    nms[:, -radius:] = 0
    flat = nms.reshape(-1)
    if threshold <= 0 and max_num_keypoints > 0:
        branch, limit = "topk", max_num_keypoints
        idx = torch.nonzero(flat > 0)[:, 0]
    else:
        limit = max_num_keypoints if max_num_keypoints > 0 else N_LIMIT_MAX
        branch = "threshold"
        idx = torch.nonzero(flat > threshold)[:, 0] if threshold > 0 else flat.new_zeros(0, dtype=torch.long)
        if threshold <= 0 or len(idx) == 0:
            branch = "mean"
            idx = torch.nonzero(flat > score.mean())[:, 0]
    if len(idx) > limit:
        sc = score.reshape(-1)[idx]
        order = torch.argsort(sc, descending=True, stable=True)[:limit]  # idx ascending + stable: ties to the lower index
        idx = torch.sort(idx[order]).values
    return idx, branch


def dkd_refine(score: torch.Tensor, idx: torch.Tensor, radius: int, temperature: float = 0.1):
    """Soft-argmax refinement of candidates `idx` (flat) on the raw score map [h,w] -> (normalised xy [N,2], key-point scores [N])."""
    h, w = score.shape
    k = 2 * radius + 1
    if len(idx) == 0:
        return score.new_zeros(0, 2), score.new_zeros(0)
    patches = F.unfold(score[None, None], k, padding=radius)[0].t()[idx]  # [N, k*k]
    lin = torch.linspace(-radius, radius, k, device=score.device)
    grid = torch.stack(torch.meshgrid(lin, lin, indexing="ij")[::-1], -1).reshape(-1, 2)  # (x, y) per patch cell, row-major
    mx = patches.max(dim=1).values[:, None]
    e = ((patches - mx) / temperature).exp()
    res = e @ grid / e.sum(dim=1)[:, None]
    xy = torch.stack([idx % w, idx // w], 1).float() + res
    xy = xy / xy.new_tensor([w - 1, h - 1]) * 2 - 1
    ks = F.grid_sample(score[None, None], xy.view(1, 1, -1, 2), mode="bilinear", align_corners=True)[0, 0, 0]
    return xy, ks


class ALIKEDReference(nn.Module):
    def __init__(self, state_dict: dict | None = None, model_name: str = "aliked-n16"):
        super().__init__()
        c1, c2, c3, c4, dim, K, M = CFG[model_name]
        self.dim = dim
        self.block1 = ConvBlock(3, c1)
        self.block2 = ResBlock(c1, c2, False)
        self.block3 = ResBlock(c2, c3, True)
        self.block4 = ResBlock(c3, c4, True)
        self.conv1, self.conv2 = conv1x1(c1, dim // 4), conv1x1(c2, dim // 4)
        self.conv3, self.conv4 = conv1x1(c3, dim // 4), conv1x1(dim, dim // 4)
        self.score_head = nn.Sequential(conv1x1(dim, 8), nn.SELU(), conv3x3(8, 4), nn.SELU(), conv3x3(4, 4), nn.SELU(), conv3x3(4, 1))
        self.desc_head = SDDH(dim, K, M)
        if state_dict is not None:
            self.load_state_dict(state_dict, strict=True)
        self.eval().requires_grad_(False)

    # ---- the dense part
    @staticmethod
    def pad(image: torch.Tensor):
        h, w = image.shape[-2:]
        ph, pw = (32 - h % 32) % 32, (32 - w % 32) % 32
        pads = [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]
        return F.pad(image, pads, mode="replicate"), pads

    def branches(self, image: torch.Tensor):
        """padded image -> (x1, x2, x3, x4) encoder maps and the four 32-channel branch maps before up-sampling."""
        x1 = self.block1(image)
        x2 = self.block2(F.avg_pool2d(x1, 2))
        x3 = self.block3(F.avg_pool2d(x2, 4))
        x4 = self.block4(F.avg_pool2d(x3, 4))
        f = [F.selu(c(x)) for c, x in ((self.conv1, x1), (self.conv2, x2), (self.conv3, x3), (self.conv4, x4))]
        return (x1, x2, x3, x4), f

    def dense(self, image: torch.Tensor) -> dict:
        """image [B,3,h,w] (or 1 channel) -> score_map [B,1,h,w], feature_map [B,128,h,w] (cropped), x3 / x4 (padded size)."""
        if image.shape[1] == 1:
            image = image.repeat(1, 3, 1, 1)
        h, w = image.shape[-2:]
        img, pads = self.pad(image)
        xs, f = self.branches(img)
        up = [f[0]] + [F.interpolate(t, scale_factor=s, mode="bilinear", align_corners=True) for t, s in zip(f[1:], (2, 8, 32))]
        x1234 = torch.cat(up, 1)
        score = torch.sigmoid(self.score_head(x1234))
        fmap = F.normalize(x1234, p=2, dim=1)
        crop = (slice(None), slice(None), slice(pads[2], pads[2] + h), slice(pads[0], pads[0] + w))
        return {"score_map": score[crop], "feature_map": fmap[crop], "x3": xs[2], "x4": xs[3]}

    def score_head0_branchwise(self, f) -> torch.Tensor:
        """score_head.0 over the concatenation, evaluated as the sum of its four 32-column slices at each branch's own resolution."""
        wgt = self.score_head[0].weight
        out = 0
        for i, (t, s) in enumerate(zip(f, (1, 2, 8, 32))):
            g = F.conv2d(t, wgt[:, 32 * i : 32 * i + 32])
            out = out + (g if s == 1 else F.interpolate(g, scale_factor=s, mode="bilinear", align_corners=True))
        return out

    # ---- the whole extractor, per image
    def forward(self, image: torch.Tensor, conf: dict) -> dict:
        d = self.dense(image)
        r = int(conf["nms_radius"])
        out = {"keypoints": [], "keypoints_norm": [], "scores": [], "descriptors": [], "score_map": d["score_map"]}
        for b in range(image.shape[0]):
            sm = d["score_map"][b, 0]
            h, w = sm.shape
            idx, _ = dkd_select(sm, r, float(conf["detection_threshold"]), int(conf["max_num_keypoints"]))
            kn, ks = dkd_refine(sm, idx, r)
            out["keypoints_norm"].append(kn)
            out["keypoints"].append(kn.new_tensor([w - 1, h - 1]) * (kn + 1) / 2.0)
            out["scores"].append(ks)
            out["descriptors"].append(self.desc_head(d["feature_map"][b], kn))
        return out
