"""Plain-torch restatement of the D2-Net / RoRD extractor as imcui/hloc/extractors/d2net.py:37-60 runs it (mihaidusmanu/d2-net:
lib/model_test.py DenseFeatureExtractionModule, HardDetectionModule, HandcraftedLocalizationModule; lib/pyramid.py process_multiscale;
lib/utils.py interpolate_dense_features, upscale_positions), CPU, float32 or float64.

Upstream's sources are not vendored: network, detector and pyramid are restated from their description and their parity with
upstream's code is not pinned ("D2-Net / RoRD: what is pinned"); RoRD's lib/model_test.py is taken to be D2-Net's.
The wrapper -- flip, normalisation, scales, column swap, the argsort cut -- is read from the reference and restated literally.

The detector exists in two forms: `hessian_conv` evaluates the second differences with F.conv2d as upstream does (its summation
order is the convolution's), `hessian_explicit` in ONE written-out float32 order, the one csrc/d2net.hip uses:
    dii = (up - 2c) + down, djj = (left - 2c) + right, dij = 0.25 (((ul - ur) - dl) + dr), det = dii djj - dij dij (both products
    rounded), (tr tr) / det <= 7.2, det > 0, step_i = -((djj / det) di + (-dij / det) dj), step_j = -((-dij / det) di + (dii / det) dj)
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

# (cin, cout, dilation, index in DenseFeatureExtractionModule.model); every convolution 3x3 with padding = dilation
LAYERS = ((3, 64, 1, 0), (64, 64, 1, 2), (64, 128, 1, 5), (128, 128, 1, 7), (128, 256, 1, 10), (256, 256, 1, 12), (256, 256, 1, 14),
          (256, 512, 2, 17), (512, 512, 2, 19), (512, 512, 2, 21))  # fmt: skip
MAXPOOL_AFTER, AVGPOOL_AFTER = (2, 7), 14  # MaxPool2d(2, 2) behind model.2 / model.7 (+ ReLU), AvgPool2d(2, stride=1) behind model.14
MEAN_BGR = (103.939, 116.779, 123.68)
EDGE_THRESHOLD = 5
DEFAULT_CONF = {"use_relu": True, "multiscale": False, "max_keypoints": 1024}
PREFIX = "dense_feature_extraction.model."


def strip(sd: dict) -> dict:
    return sd["model"] if "model" in sd else sd


def trunk(sd: dict, img: torch.Tensor, use_relu: bool = True) -> torch.Tensor:
    """img [B,3,h,w] (BGR, x * 255 - mean) -> dense features [B,512,h//4-1,w//4-1]."""
    x = img
    for cin, cout, d, op in LAYERS:
        x = F.conv2d(x, sd[f"{PREFIX}{op}.weight"].to(img), sd[f"{PREFIX}{op}.bias"].to(img), padding=d, dilation=d)
        if op != 21 or use_relu:
            x = F.relu(x)
        if op in MAXPOOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
        if op == AVGPOOL_AFTER:
            x = F.avg_pool2d(x, 2, 1)
    return x


def _shift(x: torch.Tensor, di: int, dj: int) -> torch.Tensor:
    """x[..., i + di, j + dj] with zero padding; x [C,h,w]."""
    p = F.pad(x, (1, 1, 1, 1))
    h, w = x.shape[-2:]
    return p[..., 1 + di : 1 + di + h, 1 + dj : 1 + dj + w]


def hessian_explicit(x: torch.Tensor):
    """x [C,h,w] -> dii, djj, dij, di, dj in the written-out order (every torch op rounds once)."""
    c2 = 2 * x
    up, dn, lf, rt = _shift(x, -1, 0), _shift(x, 1, 0), _shift(x, 0, -1), _shift(x, 0, 1)
    dii = (up - c2) + dn
    djj = (lf - c2) + rt
    dij = 0.25 * (((_shift(x, -1, -1) - _shift(x, -1, 1)) - _shift(x, 1, -1)) + _shift(x, 1, 1))
    return dii, djj, dij, 0.5 * (dn - up), 0.5 * (rt - lf)


def hessian_conv(x: torch.Tensor):
    """The same through F.conv2d with upstream's filters (per channel, zero padding 1)."""
    k = lambda rows: torch.tensor(rows, dtype=x.dtype).view(1, 1, 3, 3)  # noqa: E731
    v = x[:, None]
    f = lambda rows: F.conv2d(v, k(rows), padding=1)[:, 0]  # noqa: E731
    dii = f([[0, 1.0, 0], [0, -2.0, 0], [0, 1.0, 0]])
    djj = f([[0, 0, 0], [1.0, -2.0, 1.0], [0, 0, 0]])
    dij = f([[0.25, 0, -0.25], [0, 0, 0], [-0.25, 0, 0.25]])
    di = f([[0, -0.5, 0], [0, 0, 0], [0, 0.5, 0]])
    dj = f([[0, 0, 0], [-0.5, 0, 0.5], [0, 0, 0]])
    return dii, djj, dij, di, dj


def detect(x: torch.Tensor, form=hessian_explicit):
    """HardDetectionModule + HandcraftedLocalizationModule on x [C,h,w] -> detections [C,h,w] bool, step_i, step_j [C,h,w]."""
    dii, djj, dij, di, dj = form(x)
    depth_max = x.max(dim=0).values
    local_max = F.max_pool2d(x[None], 3, 1, 1)[0]
    a, b = dii * djj, dij * dij
    det = a - b
    tr = dii + djj
    threshold = (EDGE_THRESHOLD + 1) ** 2 / EDGE_THRESHOLD
    detected = (x == depth_max) & (x == local_max) & ((tr * tr) / det <= threshold) & (det > 0)
    h00, h01, h11 = djj / det, (-dij) / det, dii / det
    step_i = -((h00 * di) + (h01 * dj))
    step_j = -((h01 * di) + (h11 * dj))
    return detected, step_i, step_j


def level_candidates(f: torch.Tensor, detected: torch.Tensor, step_i: torch.Tensor, step_j: torch.Tensor, idx: int, rs: float, cs: float):
    """pyramid.py from `fmap_pos = nonzero(detections)` on, f [C,h,w] float32 -> per candidate (after both filters): channel, i, j,
    p (float32 [n,2]), key-point (x, y) float32 [n,2], score, descriptor [n,C]."""
    C, h, w = f.shape
    pos = torch.nonzero(detected)  # (c, i, j) lexicographic
    si, sj = step_i[pos[:, 0], pos[:, 1], pos[:, 2]], step_j[pos[:, 0], pos[:, 1], pos[:, 2]]
    pos = pos[(si.abs() < 0.5) & (sj.abs() < 0.5)]
    si, sj = step_i[pos[:, 0], pos[:, 1], pos[:, 2]], step_j[pos[:, 0], pos[:, 1], pos[:, 2]]
    pi, pj = pos[:, 1].to(f.dtype) + si, pos[:, 2].to(f.dtype) + sj
    it, jl, ib, jr = torch.floor(pi).long(), torch.floor(pj).long(), torch.ceil(pi).long(), torch.ceil(pj).long()
    ok = (it >= 0) & (jl >= 0) & (jr <= w - 1) & (ib <= h - 1)
    pos, pi, pj, it, jl, ib, jr = pos[ok], pi[ok], pj[ok], it[ok], jl[ok], ib[ok], jr[ok]
    di, dj = pi - it.to(f.dtype), pj - jl.to(f.dtype)
    wtl, wtr, wbl, wbr = (1 - di) * (1 - dj), (1 - di) * dj, di * (1 - dj), di * dj
    raw = ((wtl * f[:, it, jl] + wtr * f[:, it, jr]) + wbl * f[:, ib, jl]) + wbr * f[:, ib, jr]
    desc = F.normalize(raw, dim=0).t()
    ui, uj = (pi * 2 + 0.5) * 2 + 0.5, (pj * 2 + 0.5) * 2 + 0.5  # upscale_positions, scaling_steps 2
    ui, uj = ui * rs, uj * cs  # `keypoints[0] *= h_init / h_level`: a Python float times a tensor of f's dtype
    score = f[pos[:, 0], pos[:, 1], pos[:, 2]] / (idx + 1)
    return {"channel": pos[:, 0], "i": pos[:, 1], "j": pos[:, 2], "p": torch.stack([pi, pj], 1), "keypoints": torch.stack([uj, ui], 1),
            "scores": score, "descriptors": desc}  # fmt: skip


def select(maps: list, image_hw, level_hw: list, max_keypoints: int, form=hessian_explicit) -> dict:
    """process_multiscale from the dense features on, for ONE image: maps = per level [C,h,w] AFTER the multi-scale sum; image_hw the
    input size, level_hw the level images' sizes.  -> the wrapper's outputs (ascending score, stable) plus per key-point level,
    channel, i, j, and the per-level `banned` masks."""
    banned = None
    cands, bans = [], []
    for idx, f in enumerate(maps):
        detected, si, sj = detect(f, form)
        h, w = f.shape[1:]
        if banned is not None:
            banned = F.interpolate(banned[None, None].float(), size=[h, w])[0, 0].bool()
            detected = detected & ~banned
            banned = banned | detected.any(dim=0)
        else:
            banned = detected.any(dim=0)
        bans.append(banned)
        c = level_candidates(f, detected, si, sj, idx, image_hw[0] / level_hw[idx][0], image_hw[1] / level_hw[idx][1])
        c["level"] = torch.full_like(c["channel"], idx)
        cands.append(c)
    out = {k: torch.cat([c[k] for c in cands]) for k in cands[0]}
    keep = cut(out["scores"], max_keypoints)
    out = {k: v[keep] for k, v in out.items()}
    out["banned"] = bans
    return out


def cut(scores: torch.Tensor, max_keypoints: int) -> torch.Tensor:
    """d2net.py:51 `scores.argsort()[-max_keypoints or None:]`, ties pinned as a stable argsort (numpy's default leaves them open)."""
    return torch.argsort(scores, stable=True)[-max_keypoints or None :]


def level_sizes(H: int, W: int, scales) -> list:
    return [(int(math.floor(H * s)), int(math.floor(W * s))) for s in scales]


def extract(sd: dict, image: torch.Tensor, conf: dict, dtype=torch.float32, form=hessian_explicit) -> dict:
    """image [1,3,H,W] RGB in [0,1] -> `select`'s outputs plus `dense_features` (per level [h,w,512], after the sum) and `levels`."""
    sd = strip(sd)
    conf = {**DEFAULT_CONF, **conf}
    assert image.shape[0] == 1 and image.shape[1] == 3
    H, W = image.shape[2:]
    img = image.to(dtype).flip(1)
    img = img * 255 - torch.tensor(MEAN_BGR, dtype=dtype, device=img.device).view(1, 3, 1, 1)
    scales = [0.5, 1, 2] if conf["multiscale"] else [1]
    maps, sizes, prev = [], [], None
    for s in scales:
        cur = F.interpolate(img, scale_factor=s, mode="bilinear", align_corners=True)
        sizes.append(tuple(cur.shape[2:]))
        f = trunk(sd, cur, conf["use_relu"])
        if prev is not None:
            f = f + F.interpolate(prev, size=f.shape[2:], mode="bilinear", align_corners=True)
        prev = f
        maps.append(f[0])
    assert sizes == level_sizes(H, W, scales)
    out = select(maps, (H, W), sizes, int(conf["max_keypoints"] or 0), form)
    out["dense_features"] = [m.permute(1, 2, 0) for m in maps]
    out["levels"] = [tuple(m.shape[1:]) for m in maps]
    return out
