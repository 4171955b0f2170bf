"""CosPlace / EigenPlaces in plain torch, float64-capable: torchvision's ResNet-18 / 50 / 101 / 152 (models/resnet.py: BasicBlock,
Bottleneck with the stride on the 3x3, `downsample` where the stride or the width changes) without avgpool / fc, and the aggregation of
gmberton/CosPlace's cosplace_model/network.py and layers.py (L2Norm, GeM, Flatten, Linear, L2Norm), restated as nn.Modules whose
`state_dict()` carries upstream's key names, under the wrappers' tvf.Normalize (imcui/hloc/extractors/cosplace.py:36-41).

Neither torchvision nor the hub checkpoints are available to the tests, so nothing here is pinned to upstream's output; the one outside
fact that is checked is the parameter count of every backbone (tests/test_places_cpu.py).  The GPU tests use this file as the float64
yardstick and as the float32 comparison."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

DEPTHS = {18: (2, 2, 2, 2), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)  # v1.5: the stride sits on the 3x3
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


def make_backbone(backbone: int) -> nn.Sequential:
    """nn.Sequential(*list(resnetNN().children())[:-2]): conv1, bn1, relu, maxpool, layer1 .. layer4 (children 0 .. 7)."""
    block = BasicBlock if backbone == 18 else Bottleneck
    inplanes = 64
    layers = []
    for L, depth in enumerate(DEPTHS[backbone]):
        planes, blocks = 64 << L, []
        for i in range(depth):
            stride = 2 if (i == 0 and L > 0) else 1
            down = None
            if stride != 1 or inplanes != planes * block.expansion:
                down = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, 1, stride, bias=False), nn.BatchNorm2d(planes * block.expansion))
            blocks.append(block(inplanes, planes, stride, down))
            inplanes = planes * block.expansion
        layers.append(nn.Sequential(*blocks))
    return nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1), *layers)


class L2Norm(nn.Module):
    def forward(self, x):
        return F.normalize(x, p=2.0, dim=1)


class GeM(nn.Module):
    def __init__(self, p=3, eps=1e-6):
        super().__init__()
        self.p = nn.Parameter(torch.ones(1) * p)
        self.eps = eps

    def forward(self, x):
        return F.avg_pool2d(x.clamp(min=self.eps).pow(self.p), (x.size(-2), x.size(-1))).pow(1.0 / self.p)


class Flatten(nn.Module):
    def forward(self, x):
        assert x.shape[2] == x.shape[3] == 1
        return x[:, :, 0, 0]


class GeoLocalizationNet(nn.Module):
    def __init__(self, backbone: int, fc_output_dim: int):
        super().__init__()
        self.backbone = make_backbone(backbone)
        self.features_dim = 512 if backbone == 18 else 2048
        self.aggregation = nn.Sequential(L2Norm(), GeM(), Flatten(), nn.Linear(self.features_dim, fc_output_dim), L2Norm())

    def forward(self, x):
        return self.aggregation(self.backbone(x))


def build(sd: dict, backbone: int, fc_output_dim: int, dtype=torch.float32) -> GeoLocalizationNet:
    """The module in eval mode with `sd` loaded strictly, parameters and buffers in `dtype`."""
    net = GeoLocalizationNet(backbone, fc_output_dim)
    net.load_state_dict(sd, strict=True)
    return net.to(dtype).eval()


def normalize_rgb(image: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """tvf.Normalize(mean, std): (x - mean) / std with the constants rounded to the image's dtype first, as torchvision does."""
    image = image.to(dtype)
    mean = torch.tensor(MEAN, dtype=dtype, device=image.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype, device=image.device).view(1, 3, 1, 1)
    return (image - mean) / std


@torch.no_grad()
def forward(net: GeoLocalizationNet, image: torch.Tensor) -> dict:
    """image [b, 3, h, w] RGB in [0, 1] -> {"stem": the pooled stem map [b, 64, hp, wp], "blocks": {(layer, block): output}, "backbone":
    the layer4 map [b, F, h4, w4], "gem": [b, F], "global_descriptor": [b, D]} in the dtype of `net`."""
    dtype = next(net.parameters()).dtype
    x = normalize_rgb(image, dtype)
    for i in range(4):
        x = net.backbone[i](x)
    out = {"stem": x, "blocks": {}}
    for L in range(4):
        for i, blk in enumerate(net.backbone[4 + L]):
            x = blk(x)
            out["blocks"][(L + 1, i)] = x
    out["backbone"] = x
    g = net.aggregation[2](net.aggregation[1](net.aggregation[0](x)))
    out["gem"] = g
    out["global_descriptor"] = net.aggregation[4](net.aggregation[3](g))
    return out


def gem(x: torch.Tensor, p: float, dtype=torch.float32) -> torch.Tensor:
    """aggregation[0:3] on a map x [b, F, h, w] -> [b, F]; p is rounded to float32 first (it is a float32 parameter)."""
    m = GeM(p).to(dtype)
    return Flatten()(m(L2Norm()(x.to(dtype))))


def head(w: torch.Tensor, b: torch.Tensor, g: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """aggregation[3:5]: normalize(g W^T + b)."""
    return F.normalize(F.linear(g.to(dtype), w.to(dtype), b.to(dtype)), dim=1)
