"""LANet (`lanet.network_v0.model.PointModel(is_test=True)`) restated in plain torch from its description, and the selection rule of the
wrapper imcui/hloc/extractors/lanet.py:39-63: the checker of the HIP path.  Upstream's network is not vendored and no checkpoint was at
hand, so this file is the written definition (parity-unpinned; INTEGRATION.md, "LANet: what is pinned", lists what rests on memory).

Every function works in the dtype of its input (float32, or float64 after `.double()`).  The position arithmetic is written operation
by operation -- one product, one sum -- because the HIP decode promises exactly that order.

    PointModel(image [B,3,H,W] RGB in [0,1]) -> score [B,1,Hc,Wc], coord [B,2,Hc,Wc] (x, y in pixels), desc [B,256,Hc,Wc]

which is the order lanet.py:41-45 relies on: it concatenates the first two outputs and reads column 0 as the score.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

CELL = 8
CROSS_RATIO = 2.0
MEAN, STD = 0.5, 0.225
WIDTHS = (32, 64, 128, 256)
DIM = 256
PREFIX = "interestpoint_module."


class InterestPointModule(nn.Module):
    def __init__(self, widths=WIDTHS, k=3, des_bias=True, des_bn=False, leaky=False, conv_bias=False):
        super().__init__()
        c1, c2, c3, c4 = widths
        self.leaky = leaky

        def conv(cin, cout):
            return nn.Conv2d(cin, cout, 3, padding=1, bias=conv_bias)

        for name, cin, cout in (("1a", 3, c1), ("1b", c1, c1), ("2a", c1, c2), ("2b", c2, c2), ("3a", c2, c3), ("3b", c3, c3), ("4a", c3, c4), ("4b", c4, c4),
                                ("Da", c4, DIM), ("Pa", c4, DIM)):  # fmt: skip
            setattr(self, "conv" + name, conv(cin, cout))
            setattr(self, "bn" + name, nn.BatchNorm2d(cout, eps=1e-5))
        self.convDb = nn.Conv2d(DIM, 4, 3, padding=1)  # score head: three level weights and the score
        self.convPb = nn.Conv2d(DIM, 2, 3, padding=1)  # location head
        self.des_conv2 = nn.Conv2d(c2, DIM, k, padding=k // 2, bias=des_bias)
        self.des_conv3 = nn.Conv2d(c3, DIM, k, padding=k // 2, bias=des_bias)
        if des_bn:
            self.des_bn2, self.des_bn3 = nn.BatchNorm2d(DIM, eps=1e-5), nn.BatchNorm2d(DIM, eps=1e-5)
        self.des_bn = des_bn

    def act(self, x):
        return F.leaky_relu(x, 0.01) if self.leaky else F.relu(x)

    def layer(self, name, x):
        return self.act(getattr(self, "bn" + name)(getattr(self, "conv" + name)(x)))

    def level_maps(self, x2, x3):
        """des_conv2(x2), des_conv3(x3): the dense 256-channel maps the HIP forward never writes."""
        d2, d3 = self.des_conv2(x2), self.des_conv3(x3)
        if self.des_bn:
            d2, d3 = self.des_bn2(d2), self.des_bn3(d3)
        return d2, d3


def decode(raw_s: torch.Tensor, raw_p: torch.Tensor, H: int, W: int):
    """Head outputs raw_s [B,4,Hc,Wc], raw_p [B,2,Hc,Wc] -> score [B,1,Hc,Wc], coord [B,2,Hc,Wc], aware [B,3,Hc,Wc], tanh [B,2,Hc,Wc]."""
    B, _, Hc, Wc = raw_s.shape
    aware = torch.softmax(raw_s[:, :3], dim=1)
    score = torch.sigmoid(raw_s[:, 3:4])
    mask = torch.zeros_like(score)
    if Hc > 2 and Wc > 2:
        mask[:, :, 1:-1, 1:-1] = 1.0
    score = score * mask
    t = torch.tanh(raw_p)
    return score, coord_from_tanh(t, H, W), aware, t


def coord_from_tanh(t: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """base = c * 8 + 3.5, coord = base + t * 7.0 (step (cell - 1) / 2 * cross_ratio), one product and one sum, clamped to the image."""
    _, _, Hc, Wc = t.shape
    step = (CELL - 1) / 2.0
    cx = torch.arange(Wc, dtype=t.dtype, device=t.device).view(1, 1, 1, Wc).expand(1, 1, Hc, Wc)
    cy = torch.arange(Hc, dtype=t.dtype, device=t.device).view(1, 1, Hc, 1).expand(1, 1, Hc, Wc)
    base = torch.cat([cx, cy], dim=1) * float(CELL) + step
    coord = base + t * (step * CROSS_RATIO)
    return torch.cat([coord[:, 0:1].clamp(0.0, float(W - 1)), coord[:, 1:2].clamp(0.0, float(H - 1))], dim=1)


def normalised_grid(coord: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """coord [..., 2] (x, y) pixels -> grid_sample's grid: c / float32((size - 1) / 2) - 1 (the divisor is exact in float32)."""
    div = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0], dtype=coord.dtype, device=coord.device)
    return coord / div - 1.0


def sample(m: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    return F.grid_sample(m, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def blend_levels(d2, d3, d4, grid, aware, normalise=True):
    """maps [B,256,h,w], grid [B,Ho,Wo,2], aware [B,3,Ho,Wo] -> [B,256,Ho,Wo]: the weighted sum of the three samples, / its norm (a
    plain quotient, no epsilon)."""
    d = aware[:, 0:1] * sample(d2, grid) + aware[:, 1:2] * sample(d3, grid) + aware[:, 2:3] * sample(d4, grid)
    return d / d.norm(dim=1, keepdim=True) if normalise else d


class PointModel(nn.Module):
    def __init__(self, is_test=True, **kw):
        super().__init__()
        self.is_test = is_test
        self.interestpoint_module = InterestPointModule(**kw)

    def parts(self, image: torch.Tensor) -> dict:
        """Every intermediate the tests compare: x1a (layer 0), x2, x3, x4, s1 / p1 (hidden head maps), raw_s / raw_p, score, coord,
        aware, tanh, d2 / d3 (dense level maps), desc."""
        m = self.interestpoint_module
        B, _, H, W = image.shape
        x = (image - MEAN) / STD
        o = {}
        o["x1a"] = x = m.layer("1a", x)
        x = F.max_pool2d(m.layer("1b", x), 2, 2)
        o["x2"] = x = m.layer("2b", m.layer("2a", x))
        x = F.max_pool2d(x, 2, 2)
        o["x3"] = x = m.layer("3b", m.layer("3a", x))
        x = F.max_pool2d(x, 2, 2)
        o["x4"] = x = m.layer("4b", m.layer("4a", x))
        o["s1"], o["p1"] = m.layer("Da", x), m.layer("Pa", x)
        o["raw_s"], o["raw_p"] = m.convDb(o["s1"]), m.convPb(o["p1"])
        o["score"], o["coord"], o["aware"], o["tanh"] = decode(o["raw_s"], o["raw_p"], H, W)
        o["d2"], o["d3"] = m.level_maps(o["x2"], o["x3"])
        grid = normalised_grid(o["coord"].permute(0, 2, 3, 1), H, W)
        o["desc"] = blend_levels(o["d2"], o["d3"], o["x4"], grid, o["aware"])
        return o

    def forward(self, image):
        o = self.parts(image)
        return o["score"], o["coord"], o["desc"]


def build(state_dict: dict, leaky: bool = False) -> PointModel:
    """The model a state dict describes (widths, k, bias / BatchNorm of the level convolutions read from its keys and shapes), loaded
    strictly, in eval mode."""
    sd = {k: v for k, v in state_dict.items()}
    p = PREFIX
    widths = tuple(int(sd[f"{p}conv{i}b.weight"].shape[0]) for i in (1, 2, 3, 4))
    net = PointModel(is_test=True, widths=widths, k=int(sd[f"{p}des_conv2.weight"].shape[-1]), des_bias=f"{p}des_conv2.bias" in sd,
                     des_bn=f"{p}des_bn2.weight" in sd, leaky=leaky, conv_bias=f"{p}conv1a.bias" in sd)  # fmt: skip
    net.load_state_dict(sd, strict=True)
    return net.eval()


def wrapper_rule(score: torch.Tensor, coord: torch.Tensor, desc: torch.Tensor | None, threshold: float, max_keypoints: int):
    """lanet.py:45-57 on the per-cell values of ONE image (score [np], coord [np,2], desc [np,256] or None), with the backend's stable
    order: kept cells sorted by ascending (score, cell index), the last max_keypoints of them (0 = all).  -> (cell indices, keypoints
    [N,2], scores [N], descriptors [N,256] or None)."""
    if max_keypoints < 0:
        raise ValueError("max_keypoints is negative")
    cells = torch.nonzero(score > threshold).flatten()
    order = torch.sort(score[cells], stable=True).indices
    if max_keypoints > 0:
        order = order[-max_keypoints:]
    cells = cells[order]
    return cells, coord[cells], score[cells], None if desc is None else desc[cells]


def median_threshold(score: torch.Tensor) -> float:
    """A threshold that splits the non-border cells in half: midway between the two scores around the middle of the sorted positive
    scores (the lower two of them for an odd count), so that no cell sits ON the threshold, where a last-bit difference would decide."""
    s = torch.sort(score[score > 0].flatten().double()).values
    m = max(len(s) // 2, 1)
    return float((s[m - 1] + s[m]) / 2) if len(s) > 1 else 0.5


def sparse_level(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, grid: torch.Tensor) -> torch.Tensor:
    """Sample-then-convolve, the form the HIP head evaluates: x [1,C,h,w], weight [256,C,k,k] (pad k // 2), grid [1,1,n,2] ->
    [n,256].  The k x k x C neighbourhoods of the four corners grid_sample touches (zero padding of the convolution inside, zero for a
    corner outside the map) are blended with the bilinear weights, the patch is multiplied by the weights, and the bias enters with
    the sum of the in-map corner weights."""
    _, C, h, w = x.shape
    k = weight.shape[-1]
    p = k // 2
    n = grid.shape[2]
    gx, gy = grid[0, 0, :, 0], grid[0, 0, :, 1]
    fx, fy = ((gx + 1) * w - 1) / 2, ((gy + 1) * h - 1) / 2
    x0, y0 = torch.floor(fx), torch.floor(fy)
    wx1, wy1 = fx - x0, fy - y0
    wx0, wy0 = (x0 + 1) - fx, (y0 + 1) - fy
    xp = F.pad(x[0], (p + 1, p + 1, p + 1, p + 1))  # one extra ring: corners at -1 / size index it safely
    patch = torch.zeros(n, C, k, k, dtype=x.dtype)
    wsum = torch.zeros(n, dtype=x.dtype)
    for j, (dx, dy, wj) in enumerate(((0, 0, wx0 * wy0), (1, 0, wx1 * wy0), (0, 1, wx0 * wy1), (1, 1, wx1 * wy1))):
        cx, cy = x0.long() + dx, y0.long() + dy
        inside = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        wj = torch.where(inside, wj, torch.zeros_like(wj))
        wsum = wsum + wj
        cxs, cys = cx.clamp(-1, w), cy.clamp(-1, h)
        for i in range(n):
            if wj[i] != 0:
                yy, xx = int(cys[i]) + 1, int(cxs[i]) + 1  # top-left of the k x k window in the padded map
                patch[i] += wj[i] * xp[:, yy : yy + k, xx : xx + k]
    out = patch.reshape(n, -1) @ weight.reshape(weight.shape[0], -1).t()
    if bias is not None:
        out = out + wsum[:, None] * bias[None]
    return out
