"""R2D2 extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/r2d2.py: same module name (`r2d2`), one BaseModel subclass `R2D2`, same `default_conf` (:21-31) and
`required_inputs` (:32), same outputs (:67-72: keypoints [1,N,2] in pixels, descriptors [1,128,N], scores [1,N] of image 0, in ascending
score order).  `norm_rgb`, `extract_multiscale` with `NonMaxSuppression` and the argsort cut (:49-66 -> naver/r2d2 extract.py,
nets/patchnet.py) run in libimcui_hip (imcui_hip_r2d2_forward): no PyTorch convolution, interpolation, max-pooling or `nonzero` on the
path.  The scale schedule is upstream's own float64 loop, evaluated here and handed to the library as a level list.

The network (Quad_L2Net_ConfCFS: r2d2_WASF_N16, r2d2_WASF_N8, r2d2_WAF_N16) is restated from its description, its parity with
upstream's code is not pinned.  Refused by name: faster2d2 checkpoints (their 'net' string builds
Fast_Quad_L2Net_ConfCFS).  Refused by value: max_scale above 1 (upstream's assertion).  One batch holds images of one size.
"""
from __future__ import annotations

import os

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import MODEL_REPO_ID


def resolve_r2d2_checkpoint(conf: dict) -> dict:
    """conf["state_dict"] (a state dict, or upstream's {'net', 'state_dict'} container), conf["weights_path"] (a local file), else the
    reference's hub path `r2d2/{model_name}`.  The container is kept: backend.pack_r2d2 reads its 'net' string."""
    sd = conf.get("state_dict")
    if sd is not None:
        return sd
    path = conf.get("weights_path")
    if not path:
        from huggingface_hub import hf_hub_download

        path = hf_hub_download(repo_type="model", repo_id=MODEL_REPO_ID, filename="r2d2/{}".format(conf["model_name"]))
    if not os.path.isfile(str(path)):
        raise FileNotFoundError(f"checkpoint file not found: {path}")
    return torch.load(str(path), map_location="cpu", weights_only=True)


class R2D2(BaseModel):
    default_conf = {
        "model_name": "r2d2_WASF_N16.pt",
        "max_keypoints": 5000,
        "scale_factor": 2**0.25,
        "min_size": 256,
        "max_size": 1024,
        "min_scale": 0,
        "max_scale": 1,
        "reliability_threshold": 0.7,
        "repetability_threshold": 0.7,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `r2d2` conf); one channel is refused

    def _init(self, conf):
        backend.r2d2_levels(64, 64, conf["scale_factor"], conf["min_size"], conf["max_size"], conf["min_scale"], conf["max_scale"])  # refusals first
        ckpt = resolve_r2d2_checkpoint(conf)
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_r2d2(ckpt), persistent=False)
        self._impl = backend.R2D2HIP()

    def forward_batched(self, image: torch.Tensor, want_maps: bool = False, kcap=None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (pixels), scores [B,K], descriptors
        [B,K,128] (row per key-point), num_keypoints [B] int32, status [1] int32.  The schedule and the cut apply per image."""
        return self._impl.forward(self.packed, image, self.conf, want_maps=want_maps, kcap=kcap)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word; a candidate overflow (status
        bit 1: a flat map makes every pixel of a plateau a 3x3 maximum) is retried with room for every pixel of every level, any
        other non-zero status raises.  -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status & 2:
            out = self.forward_batched(image, kcap="all")
            *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"R2D2 key-point selection failed (status {status})")
        return out, counts

    def _forward(self, data):
        # the reference runs one image and returns [1,N,2] / [1,128,N] / [1,N] tensors
        out, counts = self.forward_checked(data["image"])
        n = counts[0]
        return {
            "keypoints": out["keypoints"][0, :n][None].contiguous(),
            "descriptors": out["descriptors"][0, :n].t()[None].contiguous(),
            "scores": out["scores"][0, :n][None].contiguous(),
        }
