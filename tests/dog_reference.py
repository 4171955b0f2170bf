"""The descriptor half of imcui/hloc/extractors/dog.py:87-105 restated in plain torch, for the tests of csrc/dog.hip.

kornia is not installed here and the reference's requirements do not pin it, so this file restates the rules of ONE release,
kornia 0.7.0 (kornia/feature/laf.py, kornia/geometry/transform/pyramid.py, kornia/feature/hardnet.py, kornia/feature/sosnet.py), as
recalled from its sources; the stage is parity-unpinned ("DoG + HardNet / SOSNet: what is pinned").  The two choices that
differ between releases are written down where they are made: `pyrdown` is the 5x5 binomial blur followed by a BILINEAR halving (older
releases averaged 2x2 blocks), and LAFs and sampling grids are normalised by `w - 1` / `h - 1` (older releases divided by `w` / `h`).

Everything runs in float32 or float64 (`dtype`): the float64 run is the truth of the layer tests, the float32 run gives the error that
the same operations have on the CPU."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

PS = 32


# ------------------------------------------------------------------ the networks (state-dict key names as in kornia)
def _block(cin, cout, stride=1):
    return [nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False), nn.BatchNorm2d(cout, affine=False), nn.ReLU()]


class HardNet(nn.Module):
    """kornia.feature.HardNet: `features` and the per-patch input normalisation."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(*_block(1, 32), *_block(32, 32), *_block(32, 64, 2), *_block(64, 64), *_block(64, 128, 2), *_block(128, 128),
                                      nn.Dropout(0.3), nn.Conv2d(128, 128, kernel_size=8, bias=False), nn.BatchNorm2d(128, affine=False))  # fmt: skip

    @staticmethod
    def normalize_input(x, eps=1e-6):
        sp, mp = torch.std_mean(x, dim=(-3, -2, -1), keepdim=True)  # unbiased std
        return (x - mp) / (sp + eps)

    def raw(self, x):
        """[N,1,32,32] -> [N,128], before the output normalisation."""
        return self.features(self.normalize_input(x)).view(x.size(0), -1)

    def forward(self, x):
        return F.normalize(self.raw(x), dim=1)


class SOSNet(nn.Module):
    """kornia.feature.SOSNet: `layers` (InstanceNorm2d first) and `desc_norm`."""

    def __init__(self):
        super().__init__()
        self.layers = nn.Sequential(nn.InstanceNorm2d(1, affine=False), *_block(1, 32), *_block(32, 32), *_block(32, 64, 2), *_block(64, 64),
                                    *_block(64, 128, 2), *_block(128, 128), nn.Dropout(0.1), nn.Conv2d(128, 128, kernel_size=8, bias=False),
                                    nn.BatchNorm2d(128, affine=False))  # fmt: skip
        self.desc_norm = nn.Sequential(nn.LocalResponseNorm(256, alpha=256.0, beta=0.5, k=0.0))

    @staticmethod
    def normalize_input(x):
        return F.instance_norm(x, eps=1e-5)

    def raw(self, x):
        return self.layers(x).view(x.size(0), -1)

    def forward(self, x, eps=1e-10):
        descr = self.desc_norm(self.layers(x) + eps)
        return descr.view(descr.size(0), -1)


def build(name: str, state_dict: dict, dtype=torch.float32) -> nn.Module:
    """The network with `state_dict` loaded STRICTLY (the key-name test), in eval mode and `dtype`."""
    net = {"hardnet": HardNet, "sosnet": SOSNet}[name]()
    net.load_state_dict(state_dict, strict=True)
    return net.eval().to(dtype)


def layer_modules(net) -> list:
    """The seven (convolution, BatchNorm) pairs of a network, in order."""
    seq = net.features if isinstance(net, HardNet) else net.layers
    mods = list(seq)
    return [(m, mods[i + 1]) for i, m in enumerate(mods) if isinstance(m, nn.Conv2d)]


# ------------------------------------------------------------------ LAFs (kornia/feature/laf.py)
def laf_from_center_scale_ori(xy, scale, ori_deg):
    """xy [N,2], scale [N], ori_deg [N] -> LAF [N,2,3]: scale * [[cos a, sin a], [-sin a, cos a]] | xy (angle_to_rotation_matrix)."""
    rad = ori_deg * math.pi / 180.0
    c, s = torch.cos(rad), torch.sin(rad)
    rot = torch.stack([c, s, -s, c], dim=-1).view(-1, 2, 2) * scale.view(-1, 1, 1)
    return torch.cat([rot, xy.unsqueeze(-1)], dim=-1)


def lafs_from_keypoints(kp, scales, oris_deg, mr_size=12.0, dtype=torch.float32):
    """dog.py:88-95 in float32 (the reference's numpy arrays are float32), then cast: centre xy + 0.5, scale * mr_size / 2, angle -ori."""
    kp, scales, oris_deg = kp.float(), scales.float(), oris_deg.float()
    return laf_from_center_scale_ori((kp + 0.5).to(dtype), (scales * mr_size / 2).to(dtype), (-oris_deg).to(dtype))


def _laf_coef(h, w, like, inverse):
    wf, hf = float(w - 1), float(h - 1)
    ms = min(hf, wf)
    dtype, device = like.dtype, like.device
    coef = torch.ones(1, 2, 3, dtype=dtype, device=device) * ms
    coef[0, 0, 2] = wf
    coef[0, 1, 2] = hf
    if not inverse:
        return coef
    coef = torch.ones(1, 2, 3, dtype=dtype, device=device) / ms
    coef[0, 0, 2] = 1.0 / wf
    coef[0, 1, 2] = 1.0 / hf
    return coef


def normalize_laf(laf, h, w):
    return _laf_coef(h, w, laf, True) * laf


def denormalize_laf(laf, h, w):
    return _laf_coef(h, w, laf, False) * laf


def get_laf_scale(laf, eps=1e-10):
    return (laf[:, 0, 0] * laf[:, 1, 1] - laf[:, 1, 0] * laf[:, 0, 1] + eps).abs().sqrt()


# ------------------------------------------------------------------ pyramid (kornia/geometry/transform/pyramid.py)
def pyrdown(x):
    """[B,1,h,w] -> [B,1,h//2,w//2]: filter2d(5x5 binomial / 256, border "reflect"), then bilinear resize (align_corners=False)."""
    k1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=x.dtype, device=x.device)
    kernel = (k1[:, None] * k1[None, :] / 256.0)[None, None]
    h, w = x.shape[-2:]
    blur = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), kernel)
    return F.interpolate(blur, size=(int(float(h) / 2.0), int(float(w) / 2.0)), mode="bilinear", align_corners=False)


def pyramid(image) -> list:
    """The levels `extract_patches_from_pyramid` walks: level l + 1 exists when min(h, w) of level l is at least PS."""
    levels = [image]
    while min(levels[-1].shape[-2:]) >= PS:
        levels.append(pyrdown(levels[-1]))
    return levels


def patch_levels(lafs, h, w):
    """The pyramid level every LAF samples: floor(log2(2 scale / PS)) clamped to [0, max(0, min(h, w) // PS - 1)]; and log2 itself."""
    nlaf = normalize_laf(lafs, h, w)
    scale = 2.0 * get_laf_scale(denormalize_laf(nlaf, h, w)) / float(PS)
    max_level = min(h, w) // PS
    return scale.log2().clamp(min=0.0, max=max(0, max_level - 1)).long(), scale.log2()


def extract_patches(image, lafs):
    """extract_patches_from_pyramid(image [1,1,H,W], lafs [N,2,3], PS=32) -> [N,1,32,32]; a level the loop never reaches leaves zeros."""
    H, W = image.shape[-2:]
    nlaf = normalize_laf(lafs, H, W)
    idx, _ = patch_levels(lafs, H, W)
    out = torch.zeros(lafs.shape[0], 1, PS, PS, dtype=image.dtype, device=image.device)
    for lev, cur in enumerate(pyramid(image)):
        mask = idx == lev
        n = int(mask.sum())
        if n == 0:
            continue
        h, w = cur.shape[-2:]
        grid = F.affine_grid(denormalize_laf(nlaf[mask], h, w), [n, 1, PS, PS], align_corners=False)
        grid = torch.stack([2.0 * grid[..., 0] / float(w - 1) - 1.0, 2.0 * grid[..., 1] / float(h - 1) - 1.0], dim=-1)
        out[mask] = F.grid_sample(cur.expand(n, 1, h, w), grid, mode="bilinear", padding_mode="border", align_corners=False)
    return out


# ------------------------------------------------------------------ the wrapper stages
def describe(net, patches, max_batch_size=1024):
    """dog.py:99-105."""
    desc = patches.new_zeros((len(patches), 128))
    with torch.no_grad():
        for s in range(0, len(patches), max_batch_size):
            desc[s : s + max_batch_size] = net(patches[s : s + max_batch_size])
    return desc


def forward(name, state_dict, image, kp, scales, oris_deg, mr_size=12.0, dtype=torch.float32, return_patches=False, net=None):
    """image [1,1,H,W] (or [H,W]) in [0,1], kp [N,2], scales [N] (sigma), oris_deg [N] -> descriptors [N,128] in `dtype`, on the image's
    device.  net: the network already built (`build`), else it is built from `state_dict`."""
    image = image.reshape(1, 1, *image.shape[-2:]).to(dtype)
    lafs = lafs_from_keypoints(kp, scales, oris_deg, mr_size, dtype)
    patches = extract_patches(image, lafs)
    desc = describe(net if net is not None else build(name, state_dict, dtype).to(image.device), patches)
    return (desc, patches[:, 0]) if return_patches else desc
