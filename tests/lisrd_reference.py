"""LISRD (Pautrat et al., ECCV 2020) restated in plain PyTorch: the definition csrc/lisrd.hip is tested against.

`third_party/LISRD` is not part of the reference checkout, so nothing here is copied or pinned to upstream's text: the network is written
from its description and the attribute names are restated from memory ("LISRD: what is pinned").  What IS pinned -- the
wrapper's own code, imcui/hloc/matchers/lisrd.py -- is exercised through tests/golden/make_lisrd_golden.py.

  block      conv 3x3 (pad 1, bias) -> ReLU -> BatchNorm2d (running statistics): the BatchNorm sits BEHIND the ReLU
  backbone   3->64, 64->64, AvgPool2d(2, 2) | 64->64, 64->64, pool | 64->128, 128->128, pool | 128->256, 256->256: 256 channels at 1/8
  heads      per variance: descriptor head block 256->256, conv 1x1 256->128 (un-normalised); meta head block 256->256, conv 1x1 256->128
  meta       the meta head's map is cut into 3 x 3 regions of Hc // 3 x Wc // 3 cells (remainder rows / columns dropped); a NetVLAD layer
             with 8 clusters per region -> (1024, 3, 3)
  input      the network divides its input by 255 (the wrapper multiplies by 255)
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

VARIANCES = ["rot_var_illum_var", "rot_invar_illum_var", "rot_var_illum_invar", "rot_invar_illum_invar"]
LISRD_CONFIG = {"name": "lisrd", "desc_size": 128, "tile": 3, "n_clusters": 8, "meta_desc_dim": 128, "compute_meta_desc": True}
BACKBONE = [("1_1", 3, 64, False), ("1_2", 64, 64, True), ("2_1", 64, 64, False), ("2_2", 64, 64, True), ("3_1", 64, 128, False), ("3_2", 128, 128, True),
            ("4_1", 128, 256, False), ("4_2", 256, 256, False)]  # fmt: skip


class VGGLike(nn.Module):
    def __init__(self):
        super().__init__()
        for tag, cin, cout, _ in BACKBONE:
            setattr(self, f"_conv{tag}", nn.Conv2d(cin, cout, 3, padding=1))
            setattr(self, f"_bn{tag}", nn.BatchNorm2d(cout))

    def forward(self, x):
        for tag, _, _, pool in BACKBONE:
            x = getattr(self, f"_bn{tag}")(F.relu(getattr(self, f"_conv{tag}")(x)))
            if pool:
                x = F.avg_pool2d(x, 2, 2)
        return x


class NetVLAD(nn.Module):
    def __init__(self, num_clusters, dim):
        super().__init__()
        self.conv = nn.Conv2d(dim, num_clusters, 1, bias=False)
        self.centroids = nn.Parameter(torch.rand(num_clusters, dim))

    def forward(self, x):
        n, c = x.shape[:2]
        x = F.normalize(x, dim=1)
        a = F.softmax(self.conv(x).view(n, -1, x.shape[2] * x.shape[3]), dim=1)  # [n, k, cells]
        xf = x.view(n, c, -1)
        v = (a[:, :, None, :] * (xf[:, None] - self.centroids[None, :, :, None])).sum(-1)  # [n, k, c]
        v = F.normalize(v, dim=2)
        return F.normalize(v.reshape(n, -1), dim=1)


class LisrdNet(nn.Module):
    def __init__(self, config=LISRD_CONFIG):
        super().__init__()
        self.config = dict(config)
        d, m, k = config["desc_size"], config["meta_desc_dim"], config["n_clusters"]
        self._backbone = VGGLike()
        for v in VARIANCES:
            for pre, width in (("", d), ("_meta", m)):
                setattr(self, f"conv{pre}_{v}_1", nn.Conv2d(256, 256, 3, padding=1))
                setattr(self, f"bn{pre}_{v}_1", nn.BatchNorm2d(256))
                setattr(self, f"conv{pre}_{v}_2", nn.Conv2d(256, width, 1))
            setattr(self, f"vlad_{v}", NetVLAD(k, m))

    def head(self, feat, pre, v):
        x = getattr(self, f"bn{pre}_{v}_1")(F.relu(getattr(self, f"conv{pre}_{v}_1")(feat)))
        return getattr(self, f"conv{pre}_{v}_2")(x)

    def regional_vlad(self, meta, v):
        t = self.config["tile"]
        b, _, hc, wc = meta.shape
        th, tw = hc // t, wc // t
        vlad = getattr(self, f"vlad_{v}")
        rows = [torch.stack([vlad(meta[:, :, ry * th : (ry + 1) * th, rx * tw : (rx + 1) * tw]) for rx in range(t)], dim=2) for ry in range(t)]
        return torch.stack(rows, dim=2)  # [b, k * dim, t, t]

    def forward(self, image255):
        """image255 [B, 3, H, W] in [0, 255] -> descriptors {v: [B, 128, Hc, Wc]}, meta_maps {v: [B, 128, Hc, Wc]}, meta_descriptors {v: [B, 1024, 3, 3]}"""
        if image255.shape[1] != 3:
            raise ValueError(f"LISRD reads 3 channels, got {image255.shape[1]}")
        if min(image255.shape[2:]) < 8 * self.config["tile"]:
            raise ValueError("LISRD: a region of the 1/8-resolution map without cells")
        feat = self._backbone(image255 / 255.0)
        desc = {v: self.head(feat, "", v) for v in VARIANCES}
        maps = {v: self.head(feat, "_meta", v) for v in VARIANCES}
        return {"descriptors": desc, "meta_maps": maps, "meta_descriptors": {v: self.regional_vlad(maps[v], v) for v in VARIANCES}}


# ---- what the wrapper imports from `lisrd.models` and `lisrd.models.base_model` (make_lisrd_golden.py injects this module under those names)
class Mode:
    TRAIN, VAL, TEST, EXPORT = "train", "validation", "test", "export"


class Lisrd:
    """`get_model("lisrd")(dataset, config, device)` as the wrapper drives it: load(path, Mode.EXPORT), _net.eval(), _forward(inputs, mode, config)."""

    def __init__(self, dataset, config, device):
        self._config, self._device = config, device
        self._net = LisrdNet(config).to(device)

    def load(self, path, mode):
        sd = torch.load(path, map_location="cpu")
        self._net.load_state_dict(sd.get("model_state_dict", sd))

    def _forward(self, inputs, mode, config):
        out = self._net(inputs["image0"])
        return {"descriptors": out["descriptors"], "meta_descriptors": out["meta_descriptors"]}


def get_model(name):
    if name != "lisrd":
        raise ValueError(name)
    return Lisrd


# ---- the wrapper's own steps, restated for the tests that cannot import the reference (formulas: imcui/hloc/matchers/lisrd.py:77-149)
def extract_descriptors(keypoints_xy, out, img_size, dtype=torch.float32):
    """keypoints [N, 2] (x, y), `out` of LisrdNet.forward for ONE image -> desc [N, 4, 128], meta [N, 4, 1024]"""
    kp = keypoints_xy[:, [1, 0]].to(dtype)
    grid = (kp * 2.0 / torch.tensor(img_size, dtype=dtype) - 1.0)[..., [1, 0]].view(-1, kp.shape[0], 1, 2)
    pick = lambda maps: torch.stack([F.normalize(F.grid_sample(maps[v].to(dtype), grid, align_corners=False), dim=1)[0, :, :, 0].t() for v in VARIANCES], dim=1)
    return pick(out["descriptors"]), pick(out["meta_descriptors"])
