"""LANet extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/lanet.py: same module name (`lanet`), one BaseModel subclass `LANet`, same `default_conf` (:20-24) and
`required_inputs` (:25), same outputs (:59-63: keypoints [1,N,2] as (x, y) in pixels, scores [1,N], descriptors [1,256,N] of image 0, in
ascending score order).  `self.net(image)` and the selection (:41-57: the threshold, the argsort, the `[-max_keypoints or None:]` cut)
run in libimcui_hip (imcui_hip_lanet_forward): no PyTorch convolution, pooling, grid_sample or argsort on the path.
`keypoint_threshold` and `max_keypoints` are read from `self.conf` on every call.  `activation` ("relu", "leaky_relu") is a key of
this backend only.

The network (`lanet.network_v0.model.PointModel`) is not part of the reference checkout: it is restated from its description
(tests/lanet_reference.py) and parity with upstream's code is not pinned ("LANet: what is pinned").  LANET_KEYS below is
the ONE place that names a checkpoint's keys; what the table does not cover is refused, never guessed.  Equal scores follow a stable
order (ascending score, then ascending cell index; torch.argsort leaves them open), and a negative `max_keypoints` is refused (the
reference's slice would silently drop the lowest scores).  One batch holds images of one size; every image of a batch is independent.
"""
from __future__ import annotations

import os

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import MODEL_REPO_ID

# checkpoint key prefix -> the library's layer name (include/imcui_hip.h).  Recalled from upstream's source, not checked against a
# checkpoint: edit HERE when a real file names its layers differently.
LANET_PREFIX = "interestpoint_module."
LANET_KEYS = {
    **{f"{LANET_PREFIX}conv{n}": f"conv{n}" for n in backend.LANET_LAYERS},
    **{f"{LANET_PREFIX}bn{n}": f"bn{n}" for n in backend.LANET_LAYERS},
    f"{LANET_PREFIX}convDb": "convDb",  # score head: three level weights + the score
    f"{LANET_PREFIX}convPb": "convPb",  # location head
    f"{LANET_PREFIX}des_conv2": "des_conv2",
    f"{LANET_PREFIX}des_conv3": "des_conv3",
    f"{LANET_PREFIX}des_bn2": "des_bn2",
    f"{LANET_PREFIX}des_bn3": "des_bn3",
}
LANET_CHECKPOINT_KEY = "model_state"  # lanet.py:36


def map_lanet_keys(sd: dict) -> dict:
    """Checkpoint keys -> the library's names through LANET_KEYS; `num_batches_tracked` counters are dropped, any other key the table
    does not know is refused."""
    out, unknown = {}, []
    for key, t in sd.items():
        if key.endswith("num_batches_tracked"):
            continue
        stem, _, leaf = key.rpartition(".")
        if stem in LANET_KEYS:
            out[f"{LANET_KEYS[stem]}.{leaf}"] = t
        else:
            unknown.append(key)
    if unknown:
        raise backend.ImcuiHipError(f"LANet checkpoint: {len(unknown)} keys are not in the plugin's key table (LANET_KEYS), e.g. {sorted(unknown)[:4]}")
    return out


def resolve_lanet_state_dict(conf: dict) -> dict:
    """conf["state_dict"] (a state dict, or the {'model_state': ...} container), conf["weights_path"] (a local file), else the
    reference's hub path `lanet/{model_name}` (lanet.py:30-33)."""
    sd = conf.get("state_dict")
    if sd is None:
        path = conf.get("weights_path")
        if not path:
            from huggingface_hub import hf_hub_download

            path = hf_hub_download(repo_type="model", repo_id=MODEL_REPO_ID, filename="lanet/{}".format(conf["model_name"]))
        if not os.path.isfile(str(path)):
            raise FileNotFoundError(f"checkpoint file not found: {path}")
        sd = torch.load(str(path), map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and LANET_CHECKPOINT_KEY in sd and isinstance(sd[LANET_CHECKPOINT_KEY], dict):
        sd = sd[LANET_CHECKPOINT_KEY]
    return sd


class LANet(BaseModel):
    default_conf = {
        "model_name": "PointModel_v0.pth",
        "keypoint_threshold": 0.1,
        "max_keypoints": 1024,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `lanet` conf); one channel is refused

    def _init(self, conf):
        backend.lanet_check_args((1, 3, 8, 8), conf["max_keypoints"] or 0)
        sd = map_lanet_keys(resolve_lanet_state_dict(conf))
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        packed, cfg = backend.pack_lanet(sd, conf.get("activation", "relu"))
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", packed, persistent=False)
        self._impl = backend.LanetHIP(cfg)

    def forward_batched(self, image: torch.Tensor, want_maps: bool = False) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (x, y), scores [B,K], descriptors
        [B,K,256] (row per key-point), num_keypoints [B] int32, status [1] int32.  The selection applies per image."""
        return self._impl.forward(self.packed, image, self.conf, want_maps=want_maps)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word (the candidate list holds every
        cell, so a non-zero status is a defect and raises).  -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"LANet key-point selection failed (status {status})")
        return out, counts

    def _forward(self, data):
        # the reference runs one image and returns [1,N,2] / [1,N] / [1,256,N] tensors
        out, counts = self.forward_checked(data["image"])
        n = counts[0]
        return {
            "keypoints": out["keypoints"][0, :n][None].contiguous(),
            "scores": out["scores"][0, :n][None].contiguous(),
            "descriptors": out["descriptors"][0, :n].t()[None].contiguous(),
        }
