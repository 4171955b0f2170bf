"""ALIKE extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/alike.py: same module name (`alike`), one BaseModel subclass `Alike`, same `default_conf` (:19-27)
and `required_inputs` (:29), same outputs (:57-61: keypoints [1,N,2] in pixels, scores [1,N], descriptors [1,dim,N] of image 0).  The
arithmetic of `self.net(image, sub_pixel=...)` (:50 -> Shiaoming/ALIKE: ALNet, DKD, the descriptor sampling) runs in libimcui_hip
(imcui_hip_alike_forward): no PyTorch convolution, pooling, interpolation, grid_sample or `nonzero` on the path.  `use_relu` and
`multiscale` are accepted and unused, as in the reference (alike.py never reads them).  alike-l is refused by name.
"""
from __future__ import annotations

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import load_checkpoint_file, unwrap_checkpoint

# Shiaoming/ALIKE: the checkpoints the reference mirrors under `alike/{model_name}.pth`
ALIKE_URL = "https://github.com/Shiaoming/ALIKE/raw/main/models/{}.pth"


def resolve_alike_state_dict(conf: dict) -> dict:
    """conf["state_dict"], conf["weights_path"] (a local file), else upstream's URL through torch.hub (`weights_only=True`)."""
    sd = conf.get("state_dict")
    if sd is not None:
        return unwrap_checkpoint(sd)
    path = conf.get("weights_path")
    if path:
        return load_checkpoint_file(path)
    return unwrap_checkpoint(torch.hub.load_state_dict_from_url(ALIKE_URL.format(conf["model_name"]), map_location="cpu", weights_only=True))


class Alike(BaseModel):
    default_conf = {
        "model_name": "alike-t",  # 'alike-t', 'alike-s', 'alike-n' ('alike-l' is refused)
        "use_relu": True,
        "multiscale": False,
        "max_keypoints": 1000,
        "detection_threshold": 0.5,
        "top_k": -1,
        "sub_pixel": False,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `alike` conf); one channel is refused

    def _init(self, conf):
        backend.alike_check_args((1, 3, 32, 32), conf["model_name"])  # alike-l is refused by name, before any download
        sd = resolve_alike_state_dict(conf)
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_alike(sd, conf["model_name"]), persistent=False)
        self._impl = backend.AlikeHIP(conf["model_name"])

    def forward_batched(self, image: torch.Tensor, want_maps: bool = False, kcap: int | None = None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (pixels), scores [B,K], descriptors
        [B,K,dim] (row per key-point), num_keypoints [B] int32, status [1] int32.  The selection applies per image."""
        return self._impl.forward(self.packed, image, self.conf, want_maps=want_maps, kcap=kcap)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word; a capacity overflow (status
        bit 1: exactly tied scores defeat the NMS bound) is retried with room for every pixel, any other non-zero status raises.
        -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status & 2:
            out = self.forward_batched(image, kcap=image.shape[-2] * image.shape[-1])
            *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"ALIKE key-point selection failed (status {status})")
        return out, counts

    def _forward(self, data):
        # the reference squeezes the batch away and returns image 0 as [1,N,2] / [1,N] / [1,dim,N] tensors
        out, counts = self.forward_checked(data["image"])
        n = counts[0]
        return {
            "keypoints": out["keypoints"][0, :n][None].contiguous(),
            "scores": out["scores"][0, :n][None].contiguous(),
            "descriptors": out["descriptors"][0, :n].t()[None].contiguous(),
        }
