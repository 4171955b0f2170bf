"""LiftFeat extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/liftfeat.py: same module name (`liftfeat`), one BaseModel subclass `Liftfeat`, same `default_conf`
(:13-17) and `required_inputs` (:19), same outputs (:48-52: keypoints [1,N,2], descriptors [1,64,N], scores [1,N]).  The arithmetic of
`self.net.extract(image)` (:37) and the wrapper's own cut (:42-46) run in libimcui_hip (imcui_hip_liftfeat_forward): no PyTorch
convolution, interpolation, grid_sample, `nonzero` or argsort on the path.  Unlike XFeat's wrapper, `keypoint_threshold` IS handed on
(:29).  Equal scores are cut and ordered stably by row-major pixel index, where the reference's `argsort` leaves the order open.

The network (`models.liftfeat_wrapper.LiftFeat`) is not part of the reference checkout: it is restated from its description
(tests/liftfeat_reference.py) and parity with upstream's code is not pinned ("LiftFeat: what is pinned").
"""
from __future__ import annotations

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import resolve_state_dict


class Liftfeat(BaseModel):
    default_conf = {
        "keypoint_threshold": 0.05,
        "max_keypoints": 5000,
        "model_name": "LiftFeat.pth",
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `liftfeat` conf); one channel is refused

    def _init(self, conf):
        sd = resolve_state_dict(conf, "liftfeat")  # liftfeat.py:23-26: `{Path(__file__).stem}/{model_name}`
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        packed, cfg = backend.pack_liftfeat(sd)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", packed, persistent=False)
        self._impl = backend.LiftFeatHIP(cfg)

    def forward_batched(self, image: torch.Tensor, want_dense: bool = False, kcap: int | None = None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2], scores [B,K], descriptors [B,K,64] (row
        per key-point), num_keypoints [B] int32, status [1] int32.  `max_keypoints` and the order it implies apply per image."""
        return self._impl.forward(self.packed, image, self.conf, want_dense=want_dense, kcap=kcap)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word; a capacity overflow (status
        bit 1: exactly tied scores, e.g. a constant image) is retried with room for every pixel, any other non-zero status raises.
        -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status & 2:
            out = self.forward_batched(image, kcap=backend.liftfeat_pad(image.shape[-2]) * backend.liftfeat_pad(image.shape[-1]))
            *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"LiftFeat key-point selection failed (status {status})")
        return out, counts

    def _forward(self, data):
        # the reference runs image 0 and returns [1,N,2] / [1,64,N] / [1,N] tensors
        out, counts = self.forward_checked(data["image"])
        n = counts[0]
        return {
            "keypoints": out["keypoints"][0, :n][None].contiguous(),
            "descriptors": out["descriptors"][0, :n].t()[None].contiguous(),
            "scores": out["scores"][0, :n][None].contiguous(),
        }
