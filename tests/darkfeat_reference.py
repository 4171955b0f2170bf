"""DarkFeat (`darkfeat.DarkFeat(model_path)` of THU-LYJ-Lab/DarkFeat) restated in plain torch from its description, and the cut of the
wrapper imcui/hloc/extractors/darkfeat.py:31-44: the checker of the HIP path.  Upstream's network is not vendored (third_party/DarkFeat
is an empty submodule) and no checkpoint was at hand, so this file is the written definition (parity-unpinned; INTEGRATION.md,
"DarkFeat: what is pinned", lists what rests on memory).

Every function works in the dtype of its input (float32, or float64 after `.double()`).  The detector is written operation by operation
-- one product, one sum, one quotient -- because the HIP detector promises exactly that order.

    DarkFeat(model_path)({"image": [1,3,H,W]}) -> {"keypoints": [N,2] (x, y), "scores": [N], "descriptors": [128,N]}

which is what darkfeat.py:32-39 indexes (`keypoints[idxs, :2]`, `descriptors[:, idxs]`, `scores[idxs]`).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

# name, cin, cout, stride, norm (InstanceNorm + ReLU behind it; conv1 / conv3 are bare and followed by bn1 / bn3), score level of the RAW map
LAYERS = (("conv0", 3, 32, 1, True, -1), ("conv1", 32, 32, 1, True, 0), ("conv2", 32, 64, 2, True, -1), ("conv3", 64, 64, 1, True, 1),
          ("conv4", 64, 128, 2, True, -1), ("conv5", 128, 128, 1, True, -1), ("conv6_0", 128, 128, 1, True, -1), ("conv6_1", 128, 128, 1, True, -1),
          ("conv6_2", 128, 128, 1, False, 2))  # fmt: skip
DILATION = (3, 2, 1)
LEVEL_W = (1.0 / 6.0, 2.0 / 6.0, 3.0 / 6.0)
DIM = 128
DET = {"score_thld": 0.5, "nms_size": 3, "eof_mask": 5, "edge_thld": 10, "kpt_n": 5000}
DROPPED = ("running_mean", "running_var", "num_batches_tracked")
EPS = 1e-5


def normalise_image(x: torch.Tensor) -> torch.Tensor:
    """need_norm: per image (x - mean) / std over all 3 H W values, std unbiased."""
    mean = x.mean(dim=(1, 2, 3), keepdim=True)
    std = x.std(dim=(1, 2, 3), keepdim=True)
    return (x - mean) / std


def inorm_relu(x: torch.Tensor) -> torch.Tensor:
    """InstanceNorm2d(affine=False, eps 1e-5, biased variance) + ReLU, written out (F.instance_norm refuses a 1x1 map)."""
    mean = x.mean(dim=(2, 3), keepdim=True)
    var = x.var(dim=(2, 3), unbiased=False, keepdim=True)
    return F.relu((x - mean) / torch.sqrt(var + EPS))


def box3x3(x: torch.Tensor, d: int, pad_mode: str = "reflect") -> torch.Tensor:
    """Mean of the 3x3 taps at -d, 0, +d, padding of width d."""
    H, W = x.shape[-2:]
    xp = F.pad(x, (d, d, d, d), mode=pad_mode)
    acc = None
    for i in range(3):
        for j in range(3):
            t = xp[..., i * d : i * d + H, j * d : j * d + W]
            acc = t if acc is None else acc + t
    return acc / 9.0


def peakiness(x: torch.Tensor, d: int, mavg, pad_mode: str = "reflect") -> torch.Tensor:
    """x [B,C,h,w] raw -> [B,h,w]: max_c softplus(x - box(x)) * softplus(x - mean_c(x)) of x / mavg."""
    x = x / mavg
    alpha = F.softplus(x - box3x3(x, d, pad_mode))
    beta = F.softplus(x - x.mean(dim=1, keepdim=True))
    return (alpha * beta).max(dim=1).values


def up(m: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """[B,h,w] -> [B,H,W], bilinear, align_corners=True."""
    return F.interpolate(m[:, None], size=(H, W), mode="bilinear", align_corners=True)[:, 0]


def clf_prob(desc_map: torch.Tensor, clf_w: torch.Tensor, clf_b: torch.Tensor) -> torch.Tensor:
    """soft-max(clf(desc^2))[1]: [B,128,h,w] -> [B,h,w]."""
    return torch.softmax(F.conv2d(desc_map * desc_map, clf_w, clf_b), dim=1)[:, 1]


def assemble(peaks, desc_map, clf_w, clf_b, H: int, W: int) -> torch.Tensor:
    """score [B,H,W] = (sum_i w_i up(s_i)) * up(prob)."""
    s = (LEVEL_W[0] * up(peaks[0], H, W) + LEVEL_W[1] * up(peaks[1], H, W)) + LEVEL_W[2] * up(peaks[2], H, W)
    return s * up(clf_prob(desc_map, clf_w, clf_b), H, W)


def _shift(s: torch.Tensor, dy: int, dx: int) -> torch.Tensor:
    """s(y + dy, x + dx) with zeros outside the map."""
    H, W = s.shape
    p = max(abs(dy), abs(dx))
    return F.pad(s, (p, p, p, p))[p + dy : p + dy + H, p + dx : p + dx + W]


def detect_mask(score: torch.Tensor, det: dict = DET) -> torch.Tensor:
    """score [H,W] -> bool [H,W]: threshold (strict), 3x3 maximum, border band, dilation-3 Hessian edge test with zero padding."""
    H, W = score.shape
    s = score
    keep = s > det["score_thld"]
    if det["nms_size"]:
        k = det["nms_size"]
        keep &= s == F.max_pool2d(s[None, None], k, 1, k // 2)[0, 0]
    e = det["eof_mask"]
    band = torch.zeros_like(keep)
    if H > 2 * e and W > 2 * e:
        band[e : H - e, e : W - e] = True
    keep &= band
    s2 = 2.0 * s
    dii = (_shift(s, -3, 0) - s2) + _shift(s, 3, 0)
    djj = (_shift(s, 0, -3) - s2) + _shift(s, 0, 3)
    dij = 0.25 * (((_shift(s, -3, -3) - _shift(s, -3, 3)) - _shift(s, 3, -3)) + _shift(s, 3, 3))
    dt = dii * djj - dij * dij
    tr = dii + djj
    thr = torch.tensor((det["edge_thld"] + 1) ** 2 / det["edge_thld"], dtype=s.dtype)
    keep &= (dt > 0) & ((tr * tr) / dt <= thr)
    return keep


def select(score: torch.Tensor, det: dict = DET, max_keypoints: int = 0):
    """The detector, the kpt_n cut and the wrapper's cut (darkfeat.py:36) on ONE score map [H,W], with the backend's stable order:
    candidates in row-major order, sorted by ascending (score, pixel index), the last min(kpt_n, max_keypoints or all) of them.
    -> (pixel indices, keypoints [N,2] (x, y), scores [N])."""
    if max_keypoints < 0:
        raise ValueError("max_keypoints is negative")
    W = score.shape[1]
    pix = torch.nonzero(detect_mask(score, det).flatten()).flatten()
    flat = score.flatten()
    order = torch.sort(flat[pix], stable=True).indices
    limit = min(det["kpt_n"], max_keypoints) if max_keypoints > 0 else det["kpt_n"]
    pix = pix[order[-limit:]]
    kp = torch.stack([(pix % W).to(score.dtype), (pix // W).to(score.dtype)], dim=1)
    return pix, kp, flat[pix]


def describe(desc_map: torch.Tensor, kpts: torch.Tensor) -> torch.Tensor:
    """desc_map [128,h,w], kpts [N,2] (x, y) image pixels -> [N,128]: ASLFeat's bilinear rule at (y, x) / 4 -- floor / ceil corners
    clamped to the map, weights from the unclamped fractions -- then F.normalize."""
    _, h, w = desc_map.shape
    j, i = kpts[:, 0] / 4.0, kpts[:, 1] / 4.0
    it, jl = torch.floor(i), torch.floor(j)
    di, dj = i - it, j - jl
    ib, jr = torch.ceil(i), torch.ceil(j)
    it, ib = it.long().clamp(0, h - 1), ib.long().clamp(0, h - 1)
    jl, jr = jl.long().clamp(0, w - 1), jr.long().clamp(0, w - 1)
    wtl, wtr, wbl, wbr = (1 - di) * (1 - dj), (1 - di) * dj, di * (1 - dj), di * dj
    f = desc_map.permute(1, 2, 0)
    d = ((wtl[:, None] * f[it, jl] + wtr[:, None] * f[it, jr]) + wbl[:, None] * f[ib, jl]) + wbr[:, None] * f[ib, jr]
    return F.normalize(d, p=2, dim=1, eps=1e-12)


class DarkFeat(nn.Module):
    """`DarkFeat(model_path)` as the reference's wrapper builds it (darkfeat.py:28); `state_dict=` loads from memory instead."""

    def __init__(self, model_path=None, state_dict=None, det: dict | None = None):
        super().__init__()
        sd = state_dict if state_dict is not None else torch.load(str(model_path), map_location="cpu")
        sd = {k: v for k, v in sd.items() if not k.endswith(DROPPED)}
        self.det = dict(DET, **(det or {}))
        for name, cin, cout, stride, _, _ in LAYERS:
            setattr(self, name, nn.Sequential(nn.Conv2d(cin, cout, 3, stride, 1, bias=f"{name}.0.bias" in sd)))
        self.clf = nn.Conv2d(DIM, 2, 1)
        self.moving_avg_params = nn.ParameterList([nn.Parameter(torch.tensor(1.0), requires_grad=False) for _ in range(3)])
        sd = {k: (v.reshape(()) if k.startswith("moving_avg_params.") else v) for k, v in sd.items()}
        self.load_state_dict(sd, strict=True)
        self.eval()

    def parts(self, image: torch.Tensor) -> dict:
        """Every intermediate the tests compare: x0 (normalised image), raw / norm (per layer: the convolution's output and what the next
        layer reads), peaks (3 x [B,h,w]), prob, score [B,H,W], desc_map [B,128,h4,w4]."""
        H, W = image.shape[-2:]
        o = {"raw": [], "norm": [], "peaks": [None] * 3}
        o["x0"] = x = normalise_image(image)
        for name, _, _, _, norm, tap in LAYERS:
            x = getattr(self, name)(x)
            o["raw"].append(x)
            if tap >= 0:
                o["peaks"][tap] = peakiness(x, DILATION[tap], self.moving_avg_params[tap])
            if norm:
                x = inorm_relu(x)
            o["norm"].append(x)
        o["desc_map"] = x
        o["prob"] = clf_prob(x, self.clf.weight, self.clf.bias)
        o["score"] = assemble(o["peaks"], x, self.clf.weight, self.clf.bias, H, W)
        return o

    def forward(self, data: dict) -> dict:
        o = self.parts(data["image"])
        _, kp, sc = select(o["score"][0], self.det, 0)
        return {"keypoints": kp, "scores": sc, "descriptors": describe(o["desc_map"][0], kp).t()}


def wrapper_cut(pred: dict, max_keypoints: int) -> dict:
    """darkfeat.py:33-44 on the network's output, with a stable argsort."""
    idxs = torch.sort(pred["scores"], stable=True).indices[-max_keypoints or None :]
    return {"keypoints": pred["keypoints"][idxs, :2][None], "scores": pred["scores"][idxs][None], "descriptors": pred["descriptors"][:, idxs][None]}


def between(values: torch.Tensor, q: float = 0.5) -> float:
    """A threshold at quantile q of `values` placed MIDWAY between two neighbouring values, so that none sits on it."""
    s = torch.sort(values.flatten().double()).values
    m = min(max(int(len(s) * q), 1), len(s) - 1)
    return float((s[m - 1] + s[m]) / 2) if len(s) > 1 else 0.5
