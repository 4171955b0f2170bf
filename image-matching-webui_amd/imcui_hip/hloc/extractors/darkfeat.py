"""DarkFeat extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/darkfeat.py: same module name (`darkfeat`), one BaseModel subclass `DarkFeat`, same `default_conf`
(:14-19) and `required_inputs` (:20), same outputs (:40-44: keypoints [1,N,2] as (x, y) in pixels, scores [1,N], descriptors [1,128,N]
of image 0, in ascending score order).  `self.net({"image": image})` (:32) and the cut (:36: the argsort and `[-max_keypoints or None:]`)
run in libimcui_hip (imcui_hip_darkfeat_forward): no PyTorch convolution, normalisation, interpolation or argsort on the path.
`max_keypoints` is read from `self.conf` on every call.  The reference hands NONE of its conf to the network (:28), so
`detection_threshold` and `sub_pixel` are carried and, as there, read by nobody; upstream's own detector config is accepted as keys of this
backend only -- `score_thld` 0.5, `edge_thld` 10, `nms_size` 3 (or 0), `eof_mask` 5, `kpt_n` 5000 -- and `multi_scale`,
`multi_level: False` and `use_peakiness: False` are refused by name.

The network (`darkfeat.DarkFeat`) is not part of the reference checkout: it is restated from its description
(tests/darkfeat_reference.py) and parity with upstream's code is not pinned ("DarkFeat: what is pinned").  Equal scores
follow a stable order (ascending score, then ascending pixel index; torch's sort leaves them open), a negative `max_keypoints` is refused
(the reference's slice would silently drop the lowest scores), and a flat image (std == 0), NaN upstream, yields zero key-points and
status bit 4 -- the one intended divergence.  One batch holds images of one size; every image of a batch is independent.
"""
from __future__ import annotations

import os

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import MODEL_REPO_ID


def resolve_darkfeat_state_dict(conf: dict) -> dict:
    """conf["state_dict"] (a state dict), conf["weights_path"] (a local file), else the reference's hub path `darkfeat/{model_name}`
    (darkfeat.py:23-26)."""
    sd = conf.get("state_dict")
    if sd is None:
        path = conf.get("weights_path")
        if not path:
            from huggingface_hub import hf_hub_download

            path = hf_hub_download(repo_type="model", repo_id=MODEL_REPO_ID, filename="darkfeat/{}".format(conf["model_name"]))
        if not os.path.isfile(str(path)):
            raise FileNotFoundError(f"checkpoint file not found: {path}")
        sd = torch.load(str(path), map_location="cpu", weights_only=True)
    return sd


class DarkFeat(BaseModel):
    default_conf = {
        "model_name": "DarkFeat.pth",
        "max_keypoints": 1000,
        "detection_threshold": 0.5,
        "sub_pixel": False,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `darkfeat` conf); one channel is refused

    def _init(self, conf):
        backend.darkfeat_check_args((1, 3, backend.DARKFEAT_MIN_SIDE, backend.DARKFEAT_MIN_SIDE), conf["max_keypoints"] or 0)
        backend.darkfeat_det_conf(conf)
        sd = resolve_darkfeat_state_dict(conf)
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_darkfeat(sd), persistent=False)
        self._impl = backend.DarkFeatHIP()

    def forward_batched(self, image: torch.Tensor, want_maps: bool = False, layer: int = -1) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (x, y), scores [B,K], descriptors
        [B,K,128] (row per key-point), num_keypoints [B] int32, status [1] int32.  The selection applies per image."""
        return self._impl.forward(self.packed, image, self.conf, want_maps=want_maps, layer=layer)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word.  Status bit 4 (a flat image: zero
        key-points for it) is a result, not an error; any other bit is a defect (the candidate list holds every pixel) and raises.
        -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status & ~backend.DARKFEAT_STATUS_FLAT:
            raise backend.ImcuiHipError(f"DarkFeat key-point selection failed (status {status})")
        return out, counts

    def _forward(self, data):
        # the reference runs one image and returns [1,N,2] / [1,N] / [1,128,N] tensors
        out, counts = self.forward_checked(data["image"])
        n = counts[0]
        return {
            "keypoints": out["keypoints"][0, :n][None].contiguous(),
            "scores": out["scores"][0, :n][None].contiguous(),
            "descriptors": out["descriptors"][0, :n].t()[None].contiguous(),
        }
