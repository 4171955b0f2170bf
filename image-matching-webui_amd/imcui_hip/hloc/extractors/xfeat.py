"""XFeat extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/xfeat.py: same module name (`xfeat`), one BaseModel subclass, same `default_conf` (:9-12) and
`required_inputs` (:13), same outputs (:30-34: keypoints [1,N,2], scores [1,N], descriptors [1,64,N]).  The arithmetic of
`self.net.detectAndCompute(data["image"], top_k=max_keypoints)` (:27-29 -> upstream's XFeat: resize to multiples of 32, XFeatModel,
NMS, score sampling, sort, bicubic descriptors) runs in libimcui_hip (imcui_hip_xfeat_forward): no PyTorch convolution, interpolation,
grid_sample or `nonzero` on the path.  Like the reference, `keypoint_threshold` is never handed on: detection runs at upstream's 0.05.
"""
from __future__ import annotations

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import load_checkpoint_file, unwrap_checkpoint

# verlab/accelerated_features hubconf.py / modules/xfeat.py: the weights torch.hub.load(..., "XFeat", pretrained=True) fetches
XFEAT_URL = "https://github.com/verlab/accelerated_features/raw/main/weights/xfeat.pt"


def resolve_xfeat_state_dict(conf: dict) -> dict:
    """conf["state_dict"], conf["weights_path"] (a local file), else upstream's `weights/xfeat.pt` through torch.hub (`weights_only=True`)."""
    sd = conf.get("state_dict")
    if sd is not None:
        return unwrap_checkpoint(sd)
    path = conf.get("weights_path")
    if path:
        return load_checkpoint_file(path)
    return unwrap_checkpoint(torch.hub.load_state_dict_from_url(XFEAT_URL, map_location="cpu", weights_only=True))


class XFeat(BaseModel):
    default_conf = {
        "keypoint_threshold": 0.005,
        "max_keypoints": -1,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `xfeat` conf); [B,1,h,w] runs too

    def _init(self, conf):
        sd = resolve_xfeat_state_dict(conf)
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_xfeat(sd), persistent=False)
        self._impl = backend.XFeatHIP()

    def forward_batched(self, image: torch.Tensor, want_dense: bool = False, kcap: int | None = None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2], scores [B,K], descriptors [B,K,64]
        (row per key-point, descending score), num_keypoints [B] int32, status [1] int32.  `max_keypoints` applies per image."""
        return self._impl.forward(self.packed, image, self.conf, want_dense=want_dense, kcap=kcap)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word; a capacity overflow (status
        bit 1: exactly tied scores, e.g. a constant image) is retried with room for every pixel, any other non-zero status raises.
        -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status & 2:
            out = self.forward_batched(image, kcap=image.shape[-2] * image.shape[-1])
            *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"XFeat key-point selection failed (status {status})")
        return out, counts

    def _forward(self, data):
        # the reference returns image 0 of the batch as [1,N,2] / [1,N] / [1,64,N] tensors
        out, counts = self.forward_checked(data["image"])
        n = counts[0]
        return {
            "keypoints": out["keypoints"][0, :n][None].contiguous(),
            "scores": out["scores"][0, :n][None].contiguous(),
            "descriptors": out["descriptors"][0, :n].t()[None].contiguous(),
        }
