"""DISK extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/disk.py: same module name (`disk`), one BaseModel subclass, same `default_conf` (:9-15) and
`required_inputs` (:16); the runtime conf is re-read on every call like the reference's `self.conf[...]` reads (:24-28; the UI
mutates `max_keypoints`).  The arithmetic of `self.model(image, ...)` (:22-29 -> kornia DISK.forward) runs in libimcui_hip
(imcui_hip_disk_forward): no PyTorch convolution on the path.
"""
from __future__ import annotations

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import load_checkpoint_file, unwrap_checkpoint

# kornia.feature.disk: DISK.from_pretrained(checkpoint) downloads these and loads ["extractor"]
DISK_URLS = {
    "depth": "https://raw.githubusercontent.com/cvlab-epfl/disk/master/depth-save.pth",
    "epipolar": "https://raw.githubusercontent.com/cvlab-epfl/disk/master/epipolar-save.pth",
}


def _unwrap_extractor(obj):
    """cvlab-epfl/disk checkpoints hold the network under "extractor"; a bare state dict passes through."""
    if isinstance(obj, dict) and isinstance(obj.get("extractor"), dict):
        obj = obj["extractor"]
    return unwrap_checkpoint(obj)


def resolve_disk_state_dict(conf: dict) -> dict:
    """conf["state_dict"] (bare or {"extractor": ...}), conf["weights_path"] (a local file), else the named weights through kornia
    when it is importable, else kornia's URL through torch.hub (`weights_only=True`)."""
    sd = conf.get("state_dict")
    if sd is not None:
        return _unwrap_extractor(sd)
    path = conf.get("weights_path")
    if path:
        try:
            return load_checkpoint_file(path)
        except TypeError:  # a {"extractor": ...} container
            return _unwrap_extractor(torch.load(str(path), map_location="cpu", weights_only=True))
    name = conf["weights"]
    try:
        import kornia  # noqa: F401
    except ImportError:
        kornia = None
    if kornia is not None:
        return dict(kornia.feature.DISK.from_pretrained(name, device=torch.device("cpu")).state_dict())
    if name not in DISK_URLS:
        raise ValueError(f"unknown DISK weights '{name}' (expected one of {sorted(DISK_URLS)}, or conf['weights_path'])")
    return _unwrap_extractor(torch.hub.load_state_dict_from_url(DISK_URLS[name], map_location="cpu", weights_only=True))


class DISK(BaseModel):
    default_conf = {
        "weights": "depth",
        "max_keypoints": None,
        "nms_window_size": 5,
        "detection_threshold": 0.0,
        "pad_if_not_divisible": True,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `disk` conf)

    def _init(self, conf):
        sd = resolve_disk_state_dict(conf)
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_disk(sd), persistent=False)
        self._impl = backend.DiskHIP()

    def forward_batched(self, image: torch.Tensor, want_heatmap: bool = False, kcap: int | None = None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (row-major order), scores [B,K],
        descriptors [B,K,128] (row per key-point), num_keypoints [B] int32, status [1] int32."""
        return self._impl.forward(self.packed, image, self.conf, want_heatmap=want_heatmap, kcap=kcap)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word; a capacity overflow (status
        bit 1) is retried with room for every pixel, any other non-zero status raises.  -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status & 2:
            out = self.forward_batched(image, kcap=image.shape[-2] * image.shape[-1])
            *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"DISK key-point selection failed (status {status})")
        return out, counts

    def _forward(self, data):
        # the reference returns image 0 of the batch as [1,N,2] / [1,N] / [1,128,N] tensors
        out, counts = self.forward_checked(data["image"])
        n = counts[0]
        return {
            "keypoints": out["keypoints"][0, :n][None].contiguous(),
            "scores": out["scores"][0, :n][None].contiguous(),
            "descriptors": out["descriptors"][0, :n].t()[None].contiguous(),
        }
