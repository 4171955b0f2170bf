"""ALIKED extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/aliked.py: same module name (`aliked`), one BaseModel subclass, same `default_conf` (:13-18) and
`required_inputs` (:19), the same per-image LISTS out of `_forward` (:27-31: keypoints [N,2] in pixels, scores [N], descriptors
[128,N]).  The arithmetic of `self.model(data)` (:25 -> LightGlue's ALIKED.forward: padder, encoder with deformable convolutions,
score head, DKD, SDDH) runs in libimcui_hip (imcui_hip_aliked_forward): no PyTorch convolution, pooling, interpolation or
grid_sample on the path, and no torchvision.
"""
from __future__ import annotations

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import load_checkpoint_file, unwrap_checkpoint

# lightglue/aliked.py: checkpoint_url
ALIKED_URL = "https://github.com/Shiaoming/ALIKED/raw/main/models/{}.pth"


def resolve_aliked_state_dict(conf: dict) -> dict:
    """conf["state_dict"], conf["weights_path"] (a local file), else upstream's URL through torch.hub (`weights_only=True`)."""
    sd = conf.get("state_dict")
    if sd is not None:
        return unwrap_checkpoint(sd)
    path = conf.get("weights_path")
    if path:
        return load_checkpoint_file(path)
    return unwrap_checkpoint(torch.hub.load_state_dict_from_url(ALIKED_URL.format(conf["model_name"]), map_location="cpu", weights_only=True))


class ALIKED(BaseModel):
    default_conf = {
        "model_name": "aliked-n16",
        "max_num_keypoints": -1,
        "detection_threshold": 0.2,
        "nms_radius": 2,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `aliked-n16` confs)

    def _init(self, conf):
        backend.aliked_check_model(conf["model_name"])  # aliked-t16 / aliked-n32 are refused by name, before any download
        for variant in ("mask", "conv2D"):  # SDDH variants no shipped ALIKED model uses
            if conf.get(variant):
                raise backend.ImcuiHipError(f"ALIKED: the descriptor head's `{variant}` variant is not implemented in the HIP backend")
        backend.aliked_check_args((1, 3, 32, 32), conf["nms_radius"])
        sd = resolve_aliked_state_dict(conf)
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_aliked(sd, conf["model_name"]), persistent=False)
        self._impl = backend.AlikedHIP()

    @staticmethod
    def _rgb(image: torch.Tensor) -> torch.Tensor:
        # upstream: `if image.shape[1] == 1: image = grayscale_to_rgb(image)` (the grey value in all three channels)
        return image.expand(-1, 3, -1, -1) if image.shape[1] == 1 else image

    def forward_batched(self, image: torch.Tensor, want_maps: bool = False, kcap: int | None = None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (pixels), scores [B,K], descriptors
        [B,K,128] (row per key-point), num_keypoints [B] int32, status [1] int32."""
        return self._impl.forward(self.packed, self._rgb(image), self.conf, want_maps=want_maps, kcap=kcap)

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
            raise backend.ImcuiHipError(f"ALIKED key-point selection failed (status {status})")
        return out, counts

    def _forward(self, data):
        out, counts = self.forward_checked(data["image"])
        return {
            "keypoints": [out["keypoints"][b, :n].contiguous() for b, n in enumerate(counts)],
            "scores": [out["scores"][b, :n].contiguous() for b, n in enumerate(counts)],
            "descriptors": [out["descriptors"][b, :n].t().contiguous() for b, n in enumerate(counts)],
        }
