"""SFD2 (`pram.nets.sfd2`: `load_sfd2`, `ResNet4x`, `extract_local_global`) restated in plain torch from its description: the checker of
the HIP path behind imcui/hloc/extractors/sfd2.py.  Upstream's network is not vendored (third_party is empty) and no checkpoint was at
hand, so this file is the written definition (parity-unpinned; INTEGRATION.md, "SFD2: what is pinned", lists what rests on memory).

Every function works in the dtype of its input (float32, or float64 after `.double()`).  Next to the torch forms stand the explicit-order
forms -- one product, one sum, one quotient at a time -- of the three stages whose order the HIP path promises: the sigmoid
(`sigmoid_explicit`), the selection rule (`select`) and the sampler (`sample_explicit`).

    load_sfd2(weight_path).extract_local_global(data={"image": [1,3,H,W] normalised}, config=conf)
        -> {"keypoints": [[N,2] (x, y)], "scores": [[N]], "descriptors": [[128,N]]}

which is what sfd2.py:39-43 indexes (`pred[...][0][None]`).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

DIM = 128
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # sfd2.py:24-26
NMS_RADIUS = 4
SELECT = {"conf_th": 0.001, "max_keypoints": 4096, "min_keypoints": 128, "remove_borders": 4}
TRUNK = (("conv1a", 1), ("conv1b", 2), ("conv2a", 1), ("conv2b", 2), ("conv3a", 1), ("conv3b", 1))  # name, stride


def normalise_image(x: torch.Tensor) -> torch.Tensor:
    """tvf.Normalize(mean, std) (sfd2.py:37): (x - mean_c) / std_c with the constants in the dtype of x."""
    return (x - torch.tensor(MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)


def down(n: int) -> int:
    """rows / columns behind a 3x3 stride-2 pad-1 layer."""
    return (n - 1) // 2 + 1


def sigmoid_explicit(v: torch.Tensor) -> torch.Tensor:
    """1 / (1 + exp(-v)): a negation, an exponential, a sum, a quotient."""
    return 1.0 / (1.0 + torch.exp(-v))


def depth_to_space(s16: torch.Tensor) -> torch.Tensor:
    """[B,16,Hc,Wc] -> [B,4Hc,4Wc], channel c = 4 dy + dx at pixel (4 cy + dy, 4 cx + dx)."""
    B, _, Hc, Wc = s16.shape
    return s16.view(B, 4, 4, Hc, Wc).permute(0, 3, 1, 4, 2).reshape(B, 4 * Hc, 4 * Wc)


def simple_nms(scores: torch.Tensor, r: int = NMS_RADIUS) -> torch.Tensor:
    """SuperPoint's simple_nms on [B,H,W]: maxima of (2r+1)^2 windows keep their score, everything else is 0."""

    def mp(x):
        return F.max_pool2d(x, 2 * r + 1, 1, r)

    zeros = torch.zeros_like(scores)
    mask = scores == mp(scores)
    for _ in range(2):
        supp = mp(mask.to(scores.dtype)) > 0
        ss = torch.where(supp, zeros, scores)
        mask = mask | ((ss == mp(ss)) & ~supp)
    return torch.where(mask, scores, zeros)


def select(score: torch.Tensor, image_size, conf: dict | None = None):
    """The selection on ONE score map [Hs,Ws] of an image of image_size = (H, W), H <= Hs, W <= Ws:
    simple_nms radius 4; candidates = nms > conf_th (strict) with b <= y < H - b, b <= x < W - b (the IMAGE's size, b = remove_borders);
    fewer than min_keypoints of them: candidates = nms > 0 inside the same band; sorted by descending score, equal scores by ascending
    pixel index (torch.topk leaves that open); the first max_keypoints (0: all).
    -> (pixel indices on the Ws-wide map, keypoints [N,2] (x, y), scores [N], the threshold that applied)."""
    c = dict(SELECT, **(conf or {}))
    if c["max_keypoints"] is None or c["max_keypoints"] < 0:
        raise ValueError("max_keypoints is negative")
    Hs, Ws = score.shape
    H, W = image_size
    b = c["remove_borders"]
    nms = simple_nms(score[None])[0]
    band = torch.zeros_like(nms, dtype=torch.bool)
    if H > 2 * b and W > 2 * b:
        band[b : H - b, b : W - b] = True
    th = torch.tensor(c["conf_th"], dtype=score.dtype)
    cand = (nms > th) & band
    if int(cand.sum()) < c["min_keypoints"]:
        th = torch.zeros((), dtype=score.dtype)
        cand = (nms > th) & band
    pix = torch.nonzero(cand.flatten()).flatten()
    s = nms.flatten()[pix]
    order = torch.sort(-s, stable=True).indices  # (pix ascends, so equal scores keep ascending pixel order)
    if c["max_keypoints"] > 0:
        order = order[: c["max_keypoints"]]
    pix = pix[order]
    kp = torch.stack([(pix % Ws).to(score.dtype), (pix // Ws).to(score.dtype)], dim=1)
    return pix, kp, nms.flatten()[pix], float(th)


def sample_descriptors(kpts: torch.Tensor, dmap: torch.Tensor, s: int = 4) -> torch.Tensor:
    """SuperPoint's sample_descriptors: kpts [N,2] (x, y), dmap [1,C,h,w] (normalised) -> [1,C,N]."""
    b, c, h, w = dmap.shape
    k = kpts - s / 2 + 0.5
    k = k / torch.tensor([(w * s - s / 2 - 0.5), (h * s - s / 2 - 0.5)], dtype=kpts.dtype, device=kpts.device)[None]
    k = k * 2 - 1
    d = F.grid_sample(dmap, k.view(b, 1, -1, 2), mode="bilinear", align_corners=True)
    return F.normalize(d.reshape(b, c, -1), p=2, dim=1)


def sample_explicit(kpts: torch.Tensor, dmap: torch.Tensor) -> torch.Tensor:
    """The same, operation by operation (the HIP order): kpts [N,2], dmap [C,h,w] (normalised) -> [N,C].
    g = ((k - 2) + 0.5) / ((size * 4 - 2) - 0.5) * 2 - 1;  i = ((g + 1) / 2) * (size - 1);  corners floor(i), floor(i) + 1 with the weights
    (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0), (ix - x0)(iy - y0), zero outside the map;
    ((nw w_nw + ne w_ne) + sw w_sw) + se w_se;  d / max(|d|, 1e-12)."""
    C, h, w = dmap.shape
    dt = dmap.dtype

    def unnorm(k, size):
        den = (torch.tensor(size * 4.0, dtype=dt) - 2.0) - 0.5
        g = (((k - 2.0) + 0.5) / den) * 2.0 - 1.0
        return ((g + 1.0) / 2.0) * float(size - 1)

    ix, iy = unnorm(kpts[:, 0], w), unnorm(kpts[:, 1], h)
    fx, fy = torch.floor(ix), torch.floor(iy)
    ax, bx, ay, by = (fx + 1.0) - ix, ix - fx, (fy + 1.0) - iy, iy - fy
    x0, y0 = fx.long(), fy.long()
    f = dmap.permute(1, 2, 0)

    def at(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = f[yy.clamp(0, h - 1), xx.clamp(0, w - 1)]
        return torch.where(ok[:, None], v, torch.zeros_like(v))

    d = ((at(y0, x0) * (ax * ay)[:, None] + at(y0, x0 + 1) * (bx * ay)[:, None]) + at(y0 + 1, x0) * (ax * by)[:, None]) + at(y0 + 1, x0 + 1) * (bx * by)[:, None]
    nrm = torch.sqrt((d * d).sum(dim=1, keepdim=True)).clamp_min(1e-12)
    return d / nrm


class ResBlock(nn.Module):
    """1x1 + BN + ReLU, grouped 3x3 + BN + ReLU, 1x1 + BN, + identity, ReLU."""

    def __init__(self, c: int, groups: int, bn: bool, bias: bool):
        super().__init__()
        self.conv1 = nn.Conv2d(c, c, 1, bias=bias)
        self.conv2 = nn.Conv2d(c, c, 3, 1, 1, groups=groups, bias=bias)
        self.conv3 = nn.Conv2d(c, c, 1, bias=bias)
        self.bn1, self.bn2, self.bn3 = (nn.BatchNorm2d(c) if bn else nn.Identity() for _ in range(3))

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = F.relu(self.bn2(self.conv2(y)))
        return F.relu(self.bn3(self.conv3(y)) + x)


def _cbr(cin: int, cout: int, stride: int, bn: bool, bias: bool) -> nn.Sequential:
    mods = [nn.Conv2d(cin, cout, 3, stride, 1, bias=bias)] + ([nn.BatchNorm2d(cout)] if bn else [])
    return nn.Sequential(*mods, nn.ReLU())


class ResNet4x(nn.Module):
    """Built from the SHAPES of a state dict (widths, bottleneck count, groups, head width, kernel size of convPb / convDb, BatchNorm,
    bias), then loaded strictly."""

    def __init__(self, sd: dict):
        super().__init__()
        sd = {k: v for k, v in sd.items()}
        bn, bias = "conv1a.1.weight" in sd, "conv1a.0.bias" in sd
        c = [3] + [sd[f"conv{i}b.0.weight"].shape[0] for i in (1, 2, 3)]
        widths = {"conv1a": (c[0], c[1]), "conv1b": (c[1], c[1]), "conv2a": (c[1], c[2]), "conv2b": (c[2], c[2]), "conv3a": (c[2], c[3]), "conv3b": (c[3], c[3])}
        for name, stride in TRUNK:
            setattr(self, name, _cbr(*widths[name], stride, bn, bias))
        nb = 0
        while f"conv4.{nb}.conv1.weight" in sd:
            nb += 1
        self.groups = c[3] // sd["conv4.0.conv2.weight"].shape[1] if nb else 1
        self.conv4 = nn.Sequential(*[ResBlock(c[3], self.groups, bn, "conv4.0.conv1.bias" in sd) for _ in range(nb)])
        ch = sd["convPa.0.weight"].shape[0]
        self.convPa, self.convDa = _cbr(c[3], ch, 1, bn, bias), _cbr(c[3], ch, 1, bn, bias)
        kp, kd = sd["convPb.weight"].shape[2], sd["convDb.weight"].shape[2]
        self.convPb = nn.Conv2d(ch, 16, kp, 1, kp // 2, bias="convPb.bias" in sd)
        self.convDb = nn.Conv2d(ch, DIM, kd, 1, kd // 2, bias="convDb.bias" in sd)
        self.load_state_dict(sd, strict=True)
        self.eval()

    def parts(self, x: torch.Tensor) -> dict:
        """x [B,3,H,W] NORMALISED -> every intermediate the tests compare: layers (name -> output, NCHW), logits [B,16,Hc,Wc], score
        [B,4Hc,4Wc], desc_map [B,128,Hc,Wc] (normalised)."""
        o = {"layers": {}}
        for name, _ in TRUNK:
            x = getattr(self, name)(x)
            o["layers"][name] = x
        for i, blk in enumerate(self.conv4):
            x = blk(x)
            o["layers"][f"conv4.{i}"] = x
        o["hidP"], o["hidD"] = self.convPa(x), self.convDa(x)
        o["logits"] = self.convPb(o["hidP"])
        o["score"] = depth_to_space(torch.sigmoid(o["logits"]))
        o["desc_map"] = F.normalize(self.convDb(o["hidD"]), p=2, dim=1)
        return o

    def det(self, x: torch.Tensor):
        """-> (score [B,4Hc,4Wc], desc_map [B,128,Hc,Wc])."""
        o = self.parts(x)
        return o["score"], o["desc_map"]

    def extract_local_global(self, data: dict, config: dict) -> dict:
        x = data["image"]
        H, W = x.shape[-2:]
        score, dmap = self.det(x)
        sel = {k: config[k] for k in SELECT if k in config}
        kps, scs, des = [], [], []
        for b in range(x.shape[0]):
            _, kp, sc, _ = select(score[b], (H, W), sel)
            kps.append(kp)
            scs.append(sc)
            des.append(sample_descriptors(kp, dmap[b : b + 1])[0])
        return {"keypoints": kps, "scores": scs, "descriptors": des}


def load_sfd2(weight_path=None, state_dict=None) -> ResNet4x:
    """`load_sfd2(weight_path=...)` as the reference's wrapper calls it (sfd2.py:31); `state_dict=` loads from memory instead.  A
    checkpoint may be the state dict itself or hold it under "model"."""
    sd = state_dict if state_dict is not None else torch.load(str(weight_path), map_location="cpu")
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    return ResNet4x(sd)


def between(values: torch.Tensor, q: float = 0.5) -> float:
    """A threshold at quantile q of `values` placed MIDWAY between two neighbouring values, so that none sits on it."""
    s = torch.sort(values.flatten().double()).values
    m = min(max(int(len(s) * q), 1), len(s) - 1)
    return float((s[m - 1] + s[m]) / 2) if len(s) > 1 else 0.5
