"""NetVLAD in plain torch, float64-capable: imcui/hloc/extractors/netvlad.py:17-38 (NetVLADLayer) and :122-146 (`_forward`) restated on a
state dict under the reference module's names (+ `preprocess.mean`).  tests/test_netvlad_cpu.py pins it to the reference's own output
(tests/golden/netvlad_*.npz, written by make_netvlad_golden.py from the reference checkout); the GPU tests use it as the float64 yardstick
at shapes the golden files do not hold."""
from __future__ import annotations

import torch
import torch.nn.functional as F

# (cin, cout, index in vgg16().features, a MaxPool2d(2, 2) follows the ReLU): the reference drops the last ReLU and the last pool (:68)
LAYERS = ((3, 64, 0, False), (64, 64, 2, True), (64, 128, 5, False), (128, 128, 7, True), (128, 256, 10, False), (256, 256, 12, False),
          (256, 256, 14, True), (256, 512, 17, False), (512, 512, 19, False), (512, 512, 21, True), (512, 512, 24, False), (512, 512, 26, False),
          (512, 512, 28, False))  # fmt: skip


def preprocess(sd: dict, image: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """:126-129 (std is 1): clamp(image * 255, 0, 255) - mean."""
    image = image.to(dtype)
    image = torch.clamp(image * 255, 0.0, 255.0)
    return image - sd["preprocess.mean"].to(dtype).view(1, -1, 1, 1)


def backbone(sd: dict, x: torch.Tensor, dtype=torch.float32, upto: int | None = None) -> torch.Tensor:
    """vgg16().features[:-2] on the preprocessed image; upto = number of convolutions to run (each with its ReLU / pool, None: all 13)."""
    n = len(LAYERS) if upto is None else upto
    for i, (_, _, op, pool) in enumerate(LAYERS[:n]):
        x = F.conv2d(x, sd[f"backbone.{op}.weight"].to(dtype), sd[f"backbone.{op}.bias"].to(dtype), padding=1)
        if i < len(LAYERS) - 1:
            x = F.relu(x)
        if pool:
            x = F.max_pool2d(x, 2, 2)
    return x


def vlad_layer(sd: dict, descriptors: torch.Tensor, dtype=torch.float32, return_assignment: bool = False):
    """:138 + NetVLADLayer.forward: descriptors [b, 512, n] (NOT yet normalised) -> [b, 32768]."""
    x = F.normalize(descriptors.to(dtype), dim=1)
    b = x.size(0)
    scores = F.conv1d(x, sd["netvlad.score_proj.weight"].to(dtype))
    scores = F.softmax(scores, dim=1)
    centers = sd["netvlad.centers"].to(dtype)
    # (scores.unsqueeze(1) * (x.unsqueeze(2) - centers[None, :, :, None])).sum(-1) without the [b, 512, 64, n] tensor, one cluster at a time
    desc = torch.stack([(scores[:, k : k + 1] * (x - centers[None, :, k, None])).sum(dim=-1) for k in range(centers.shape[1])], dim=2)
    desc = F.normalize(desc, dim=1)
    desc = desc.reshape(b, -1)
    desc = F.normalize(desc, dim=1)
    return (desc, scores) if return_assignment else desc


def whiten(sd: dict, desc: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """:143-144."""
    return F.normalize(F.linear(desc.to(dtype), sd["whiten.weight"].to(dtype), sd["whiten.bias"].to(dtype)), dim=1)


def forward(sd: dict, image: torch.Tensor, whiten_: bool, dtype=torch.float32) -> dict:
    """-> {"backbone": [b, 512, h, w], "vlad": [b, 32768], "global_descriptor": [b, 4096] (whiten_) or the vlad vector}."""
    f = backbone(sd, preprocess(sd, image, dtype), dtype)
    b, c = f.shape[:2]
    v = vlad_layer(sd, f.view(b, c, -1), dtype)
    return {"backbone": f, "vlad": v, "global_descriptor": whiten(sd, v, dtype) if whiten_ else v}
