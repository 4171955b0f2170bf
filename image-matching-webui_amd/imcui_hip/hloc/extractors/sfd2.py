"""SFD2 extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/sfd2.py: same module name (`sfd2`), one BaseModel subclass `SFD2`, same `default_conf` (:15-19) and
`required_inputs` (:20), same outputs (:39-43: keypoints [1,N,2] as (x, y) in pixels, scores [1,N], descriptors [1,128,N] of image 0).
`self.norm_rgb(data["image"])` (:37) and `self.net.extract_local_global(...)` (:36) run in libimcui_hip (imcui_hip_sfd2_forward): no
PyTorch convolution, normalisation, pooling, top-k or grid_sample on the path.  `max_keypoints` and `conf_th` are read from `self.conf`
on every call; `min_keypoints` (128) and `remove_borders` (4) are keys of this backend only; `multiscale` is refused by name.

The network (`pram.nets.sfd2`) is not part of the reference checkout: it is restated from its description (tests/sfd2_reference.py) and
parity with upstream's code is not pinned ("SFD2: what is pinned").  SFD2_KEYS below is the ONE table of the state-dict
keys the backend admits; widths, bottleneck count, groups, the kernel size of convPb / convDb, BatchNorm and bias are read from the
checkpoint's shapes.  Key-points leave in descending score order, equal scores by ascending pixel index (torch.topk leaves that open);
a negative `max_keypoints` is refused.  One batch holds images of one size; every image of a batch is independent.
"""
from __future__ import annotations

import os
import re

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import MODEL_REPO_ID

# The state-dict keys of ResNet4x the backend admits, as patterns over the key without its last component.  Recalled from upstream's
# source, not checked against a checkpoint: edit HERE when a real file names its layers differently.  `num_batches_tracked` counters are
# dropped; every other key has to match one row.
SFD2_KEYS = (
    r"conv(1a|1b|2a|2b|3a|3b)\.0",       # trunk convolutions (3x3; 1b and 2b stride 2)
    r"conv(1a|1b|2a|2b|3a|3b)\.1",       # their BatchNorm
    r"conv4\.\d+\.conv[123]",            # bottlenecks: 1x1, grouped 3x3, 1x1
    r"conv4\.\d+\.bn[123]",
    r"conv[PD]a\.[01]",                  # hidden layer of the score / descriptor head and its BatchNorm
    r"conv[PD]b",                        # score logits (16) / descriptors (128)
)
SFD2_CHECKPOINT_KEY = "model"  # a checkpoint may hold the state dict under this key
_SFD2_KEY_RE = re.compile("|".join(f"(?:{p})" for p in SFD2_KEYS))


def map_sfd2_keys(sd: dict) -> dict:
    """The state dict without its `num_batches_tracked` counters; a key SFD2_KEYS does not know is refused."""
    out, unknown = {}, []
    for key, t in sd.items():
        if key.endswith("num_batches_tracked"):
            continue
        stem, _, _ = key.rpartition(".")
        if _SFD2_KEY_RE.fullmatch(stem):
            out[key] = t
        else:
            unknown.append(key)
    if unknown:
        raise backend.ImcuiHipError(f"SFD2 checkpoint: {len(unknown)} keys are not in the plugin's key table (SFD2_KEYS), e.g. {sorted(unknown)[:4]}")
    return out


def resolve_sfd2_state_dict(conf: dict) -> dict:
    """conf["state_dict"] (a state dict, or the {'model': ...} container), conf["weights_path"] (a local file), else the reference's hub
    path `pram/{model_name}` (sfd2.py:27-30)."""
    sd = conf.get("state_dict")
    if sd is None:
        path = conf.get("weights_path")
        if not path:
            from huggingface_hub import hf_hub_download

            path = hf_hub_download(repo_type="model", repo_id=MODEL_REPO_ID, filename="pram/{}".format(conf["model_name"]))
        if not os.path.isfile(str(path)):
            raise FileNotFoundError(f"checkpoint file not found: {path}")
        sd = torch.load(str(path), map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and SFD2_CHECKPOINT_KEY in sd and isinstance(sd[SFD2_CHECKPOINT_KEY], dict):
        sd = sd[SFD2_CHECKPOINT_KEY]
    return sd


class SFD2(BaseModel):
    default_conf = {
        "max_keypoints": 4096,
        "model_name": "sfd2_20230511_210205_resnet4x.79.pth",
        "conf_th": 0.001,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `sfd2` conf); one channel is refused

    def _init(self, conf):
        backend.sfd2_select_conf(conf)
        sd = map_sfd2_keys(resolve_sfd2_state_dict(conf))
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        packed, cfg = backend.pack_sfd2(sd)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", packed, persistent=False)
        self._impl = backend.Sfd2HIP(cfg)

    def forward_batched(self, image: torch.Tensor, want_maps: bool = False, layer: int = -1) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (x, y), scores [B,K], descriptors
        [B,K,128] (row per key-point), num_keypoints [B] int32, status [1] int32.  The selection applies per image."""
        return self._impl.forward(self.packed, image, self.conf, want_maps=want_maps, layer=layer)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word (the candidate list holds every
        score-map pixel, so a non-zero status is a defect and raises).  -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"SFD2 key-point selection failed (status {status})")
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
