"""CPU restatement of kornia's DISK (kornia.feature.DISK, copied from cvlab-epfl/disk) for the DISK parity tests.

kornia is not a dependency of this project, so the network and the detection are restated here from the published source, built
from `torch.nn` modules: the U-Net `Unet(in_features=3, size=5, down=[16, 32, 64, 64, 64], up=[64, 64, 64, 129])` with
`Conv = Sequential(InstanceNorm2d, PReLU, dropout (no-op), Conv2d 5x5)` whose norm and gate act on the convolution's input (the
first block has neither), avg-pool down, bilinear x2 up (align_corners=False) then `cat([upsampled, skip])`; the heatmap is output
channel 128, the dense descriptors channels 0..127; `heatmap_to_keypoints` (max_pool2d NMS, strict threshold, the `n + 1`-th
value cut-off, row-major order) and `merge_with_descriptors` (integer-pixel read, F.normalize).  State-dict keys are kornia's
(`unet.path_down.*`, `unet.path_up.*`), so a real `depth-save.pth` ["extractor"] loads unchanged.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


class _Down(nn.Module):  # TrivialDownsample
    def forward(self, x):
        return F.avg_pool2d(x, 2)


def _conv(cin: int, cout: int, first: bool = False) -> nn.Sequential:
    if first:
        return nn.Sequential(nn.Identity(), nn.Identity(), nn.Identity(), nn.Conv2d(cin, cout, 5, padding=2, bias=True))
    return nn.Sequential(nn.InstanceNorm2d(cin), nn.PReLU(cin), nn.Identity(), nn.Conv2d(cin, cout, 5, padding=2, bias=True))


class _Up(nn.Module):  # ThinUpBlock
    def __init__(self, bottom: int, horizontal: int, out: int):
        super().__init__()
        self.conv = _conv(bottom + horizontal, out)

    def forward(self, bot, hor):
        big = F.interpolate(bot, scale_factor=2, mode="bilinear", align_corners=False)
        return self.conv(torch.cat([big, hor], dim=1))


class Unet(nn.Module):
    def __init__(self, in_features=3, down=(16, 32, 64, 64, 64), up=(64, 64, 64, 129)):
        super().__init__()
        self.in_features = in_features
        dd = [in_features, *down]
        self.path_down = nn.ModuleList(
            nn.Sequential(nn.Identity() if i == 0 else _Down(), _conv(a, b, first=i == 0)) for i, (a, b) in enumerate(zip(dd[:-1], dd[1:])))
        bot = [down[-1], *up]
        hor = dd[-2::-1]
        self.path_up = nn.ModuleList(_Up(b, h, o) for b, h, o in zip(bot, hor, up))
        self.divisor = 2 ** (len(down) - 1)

    def forward(self, x):
        if x.shape[1] != self.in_features:
            raise ValueError(f"Expected {self.in_features} input channels, got {x.shape[1]}")
        if x.shape[2] % self.divisor or x.shape[3] % self.divisor:
            raise ValueError(f"Input image shape must be divisible by {self.divisor} (got {tuple(x.shape)}).")
        feats = [x]
        for layer in self.path_down:
            feats.append(layer(feats[-1]))
        f = feats[-1]
        for layer, h in zip(self.path_up, feats[-2::-1]):
            f = layer(f, h)
        return f


def nms(signal: torch.Tensor, window_size: int = 5, cutoff: float | None = 0.0) -> torch.Tensor:
    if window_size % 2 != 1:
        raise ValueError(f"window_size has to be odd, got {window_size}")
    _, ixs = F.max_pool2d(signal, kernel_size=window_size, stride=1, padding=window_size // 2, return_indices=True)
    h, w = signal.shape[1:]
    coords = torch.arange(h * w, device=signal.device).reshape(1, h, w)
    keep = ixs == coords
    return keep if cutoff is None else keep & (signal > cutoff)


def heatmap_to_keypoints(heatmap: torch.Tensor, n=None, window_size=5, score_threshold=0.0):
    """heatmap [B,1,H,W] -> list of (xy [N,2] long, logp [N]) per image, kornia's rule (raises on zero candidates with n given)."""
    heatmap = heatmap.squeeze(1)
    kept = nms(heatmap, window_size=window_size, cutoff=score_threshold)
    out = []
    for b in range(heatmap.shape[0]):
        yx = kept[b].nonzero(as_tuple=False)
        logp = heatmap[b][kept[b]]
        xy = yx.flip((1,))
        if n is not None:
            n_ = min(n + 1, logp.numel())
            minus_threshold, _ = torch.kthvalue(-logp, n_)
            mask = logp > -minus_threshold
            xy, logp = xy[mask][:n], logp[mask][:n]
        out.append((xy, logp))
    return out


class DISKReference(nn.Module):
    desc_dim = 128

    def __init__(self, state_dict: dict | None = None):
        super().__init__()
        self.unet = Unet()
        if state_dict is not None:
            self.load_state_dict(state_dict)
        self.eval()

    @torch.no_grad()
    def heatmap_and_dense_descriptors(self, images: torch.Tensor, pad_if_not_divisible: bool = True):
        """-> (heatmaps [B,1,h,w], descriptors [B,128,h,w]) cropped to the input size."""
        h, w = images.shape[2:]
        if pad_if_not_divisible:
            images = F.pad(images, (0, (16 - w % 16) % 16, 0, (16 - h % 16) % 16), value=0.0)
        o = self.unet(images)
        return o[:, 128:, :h, :w], o[:, :128, :h, :w]

    @torch.no_grad()
    def forward(self, images, n=None, window_size=5, score_threshold=0.0, pad_if_not_divisible=True, return_heatmap=False):
        heat, desc = self.heatmap_and_dense_descriptors(images, pad_if_not_divisible)
        kps = heatmap_to_keypoints(heat, n=n, window_size=window_size, score_threshold=score_threshold)
        feats = []
        for i, (xy, logp) in enumerate(kps):
            d = F.normalize(desc[i][:, xy[:, 1], xy[:, 0]].T, dim=-1)
            feats.append({"keypoints": xy.float(), "scores": logp, "descriptors": d})
        return (feats, heat) if return_heatmap else feats


def descriptors_at(desc_dense: torch.Tensor, xy: torch.Tensor) -> torch.Tensor:
    """merge_with_descriptors for one image: desc_dense [128,h,w], xy [N,2] -> [N,128] unit rows."""
    xy = xy.long()
    return F.normalize(desc_dense[:, xy[:, 1], xy[:, 0]].T, dim=-1)
