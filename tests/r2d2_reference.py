"""Plain-torch restatement of the R2D2 extractor as imcui/hloc/extractors/r2d2.py:49-73 runs it (naver/r2d2: nets/patchnet.py
Quad_L2Net_ConfCFS, extract.py NonMaxSuppression + extract_multiscale), CPU, float32 or float64.

Upstream's sources are not vendored: the NETWORK is restated from its description (layer table below) and its parity with upstream's
code is not pinned ("R2D2: what is pinned").  The wrapper -- normalisation, the scale schedule, the detector, the
float32 coordinate arithmetic, the argsort cut -- is read from the reference and restated literally."""
from __future__ import annotations

import torch
import torch.nn.functional as F

# (cin, cout, kernel, dilation, BatchNorm, ReLU, index of the convolution in the flat `ops` ModuleList); stride 1, pad ((k-1) d) // 2
LAYERS = ((3, 32, 3, 1, True, True, 0), (32, 32, 3, 1, True, True, 3), (32, 64, 3, 1, True, True, 6), (64, 64, 3, 2, True, True, 9),
          (64, 128, 3, 2, True, True, 12), (128, 128, 3, 4, True, True, 15), (128, 128, 2, 4, True, False, 18), (128, 128, 2, 8, True, False, 20),
          (128, 128, 2, 16, False, False, 22))  # fmt: skip
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DEFAULT_CONF = {"max_keypoints": 5000, "scale_factor": 2**0.25, "min_size": 256, "max_size": 1024, "min_scale": 0, "max_scale": 1,
                "reliability_threshold": 0.7, "repetability_threshold": 0.7}  # fmt: skip


def strip(sd: dict) -> dict:
    if "state_dict" in sd:
        sd = sd["state_dict"]
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def network(sd: dict, img: torch.Tensor) -> dict:
    """img [B,3,h,w] (normalised) -> the final map x [B,128,h,w], reliability and repeatability [B,h,w]."""
    dt = img  # (dtype and device of the image)
    x = img
    for cin, cout, k, d, bn, relu, op in LAYERS:
        x = F.conv2d(x, sd[f"ops.{op}.weight"].to(dt), sd[f"ops.{op}.bias"].to(dt), padding=((k - 1) * d) // 2, dilation=d)
        if bn:  # BatchNorm2d(affine=False), eval
            x = F.batch_norm(x, sd[f"ops.{op + 1}.running_mean"].to(dt), sd[f"ops.{op + 1}.running_var"].to(dt), None, None, False, 0.0, 1e-5)
        if relu:
            x = F.relu(x)
    assert x.shape[2:] == img.shape[2:]
    x2 = x * x
    ucl = F.conv2d(x2, sd["clf.weight"].to(dt), sd["clf.bias"].to(dt))
    usa = F.conv2d(x2, sd["sal.weight"].to(dt), sd["sal.bias"].to(dt))
    sp = F.softplus(usa)
    return {"map": x, "reliability": F.softmax(ucl, dim=1)[:, 1], "repeatability": (sp / (1 + sp))[:, 0]}


def schedule(H: int, W: int, scale_f, min_size, max_size, min_scale, max_scale) -> list:
    """The literal loop of extract_multiscale: [(nh, nw, runs)]."""
    assert max_scale <= 1
    out = []
    s = 1.0
    nh, nw = H, W
    while s + 0.001 >= max(min_scale, min_size / max(H, W)):
        out.append((nh, nw, s - 0.001 <= min(max_scale, max_size / max(H, W))))
        s /= scale_f
        nh, nw = round(H * s), round(W * s)
    return out


def detect(rel: torch.Tensor, rep: torch.Tensor, rel_thr: float, rep_thr: float):
    """NonMaxSuppression.forward on one image's maps [h,w] -> (y, x) in row-major order."""
    maxima = rep == F.max_pool2d(rep[None, None], 3, 1, 1)[0, 0]
    maxima = maxima & (rep >= rep_thr) & (rel >= rel_thr)
    yx = maxima.nonzero()
    return yx[:, 0], yx[:, 1]


def candidates(levels, H: int, W: int, rel_thr: float, rep_thr: float):
    """levels = [(rel [h,w], rep [h,w])] of ONE image, float32 -> candidate lists, level-major: x, y (float32, (x * W) / nw), score
    = rel * rep (float32), level, flat index."""
    X, Y, S, L, I = [], [], [], [], []
    for l, (rel, rep) in enumerate(levels):
        nh, nw = rep.shape
        y, x = detect(rel, rep, rel_thr, rep_thr)
        X.append(x.float() * W / nw)
        Y.append(y.float() * H / nh)
        S.append(rel[y, x] * rep[y, x])
        L.append(torch.full_like(y, l))
        I.append(y * nw + x)
    return torch.cat(X), torch.cat(Y), torch.cat(S), torch.cat(L), torch.cat(I)


def cut(scores: torch.Tensor, max_keypoints: int) -> torch.Tensor:
    """r2d2.py:63 `scores.argsort()[-max_keypoints or None:]`, ties pinned as torch.argsort(stable=True)."""
    return torch.argsort(scores, stable=True)[-max_keypoints or None :]


def extract(sd: dict, image: torch.Tensor, conf: dict, dtype=torch.float32) -> dict:
    """image [1,3,H,W] RGB in [0,1] -> keypoints [N,2], scores [N], descriptors [N,128] in the wrapper's order, plus the per-level maps
    (`levels`: (nh, nw); `reliability`, `repeatability` [nh,nw]; `final_map` [nh,nw,128]) and the candidates' level / flat index."""
    sd = strip(sd)
    conf = {**DEFAULT_CONF, **conf}
    assert image.shape[0] == 1 and image.shape[1] == 3
    H, W = image.shape[2:]
    img = image.to(dtype)
    img = (img - torch.tensor(MEAN, dtype=dtype, device=img.device)[None, :, None, None]) / torch.tensor(STD, dtype=dtype, device=img.device)[None, :, None, None]
    sched = schedule(H, W, conf["scale_factor"], conf["min_size"], conf["max_size"], conf["min_scale"], conf["max_scale"])
    out = {"levels": [], "reliability": [], "repeatability": [], "final_map": []}
    maps, D = [], []
    for i, (nh, nw, runs) in enumerate(sched):
        if i > 0:
            img = F.interpolate(img, (nh, nw), mode="bilinear", align_corners=False)
        if not runs:
            continue
        r = network(sd, img)
        out["levels"].append((nh, nw))
        out["reliability"].append(r["reliability"][0])
        out["repeatability"].append(r["repeatability"][0])
        out["final_map"].append(r["map"][0].permute(1, 2, 0))
        maps.append((r["reliability"][0].float(), r["repeatability"][0].float()))
        D.append(F.normalize(r["map"], p=2, dim=1)[0].permute(1, 2, 0).reshape(-1, 128))
    if not maps:
        z = torch.zeros(0)
        return {**out, "keypoints": torch.zeros(0, 2), "scores": z, "descriptors": torch.zeros(0, 128), "level": z.long(), "index": z.long()}
    x, y, s, lev, idx = candidates(maps, H, W, conf["reliability_threshold"], conf["repetability_threshold"])
    keep = cut(s, int(conf["max_keypoints"] or 0))
    first = torch.tensor([0] + [d.shape[0] for d in D[:-1]], device=lev.device).cumsum(0)  # first row of each level in cat(D)
    desc = torch.cat(D)[(first[lev] + idx)[keep]]
    return {**out, "keypoints": torch.stack([x[keep], y[keep]], 1), "scores": s[keep], "descriptors": desc, "level": lev[keep], "index": idx[keep]}
