"""DeDoDe extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/dedode.py: same module name (`dedode`), one BaseModel subclass `DeDoDe`, same `default_conf`
(:21-28) and `required_inputs` (:29-31), same outputs (:82-86: keypoints [1,N,2] as (x, y) in pixels, scores [1,N], descriptors
[1,256,N] of image 0, not normalised -- the Dual-Softmax matcher normalises -- in descending score order).  transforms.Normalize,
`dedode_detector_L.detect(num_keypoints=max_keypoints)`, `dedode_descriptor_B.describe_keypoints` and `to_pixel_coords` (:61-80) run in
libimcui_hip (imcui_hip_dedode_forward): no PyTorch convolution, interpolation, soft-max, top-k or grid_sample on the path.  Both state
dicts go into ONE packed buffer; the ConvRefiner widths and block counts are read from the tensors.

The networks are restated from their description; parity with upstream's code is not pinned ("DeDoDe: what is pinned").
fp32-grade arithmetic where upstream autocasts to float16 on CUDA; equal scores at the cut go to the lower pixel index; max_keypoints
above H * W raises, as topk does; `dense: True`, other detector / descriptor sizes and sides that are not multiples of 8 are refused;
one batch holds images of one size.
"""
from __future__ import annotations

import os

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import MODEL_REPO_ID


def resolve_dedode_checkpoint(conf: dict, which: str, folder: str) -> dict:
    """conf["state_dict_<which>"] (a state dict), conf["weights_path_<which>"] (a local file), else the reference's hub path
    `{folder}/{model_<which>_name}`."""
    sd = conf.get(f"state_dict_{which}")
    if sd is not None:
        return sd
    path = conf.get(f"weights_path_{which}")
    if not path:
        from huggingface_hub import hf_hub_download

        path = hf_hub_download(repo_type="model", repo_id=MODEL_REPO_ID, filename="{}/{}".format(folder, conf[f"model_{which}_name"]))
    if not os.path.isfile(str(path)):
        raise FileNotFoundError(f"checkpoint file not found: {path}")
    return torch.load(str(path), map_location="cpu", weights_only=True)


class DeDoDe(BaseModel):
    default_conf = {
        "name": "dedode",
        "model_detector_name": "dedode_detector_L.pth",
        "model_descriptor_name": "dedode_descriptor_B.pth",
        "max_keypoints": 2000,
        "match_threshold": 0.2,
        "dense": False,  # Now fixed to be false
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the dedode conf)
    hub_folder = "dedode"  # upstream: Path(__file__).stem

    def _init(self, conf):
        if conf["dense"]:
            raise ValueError("DeDoDe: `dense: True` (detect_dense) is not served by the HIP backend; the reference fixes it to False")
        for which in backend.DEDODE_MODELS:
            if conf[f"model_{which}_name"] != backend.DEDODE_MODEL_NAMES[which]:
                raise ValueError(f"DeDoDe: model_{which}_name={conf[f'model_{which}_name']!r} is not served, only "
                                 f"{backend.DEDODE_MODEL_NAMES[which]!r} (detector L with descriptor B)")  # fmt: skip
        sds = [resolve_dedode_checkpoint(conf, which, self.hub_folder) for which in backend.DEDODE_MODELS]
        for which in backend.DEDODE_MODELS:  # keep self.conf small / printable
            conf.pop(f"state_dict_{which}", None)
            self.conf.pop(f"state_dict_{which}", None)
        packed, self.dims = backend.pack_dedode(*sds)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", packed, persistent=False)
        self._impl = backend.DeDoDeHIP()

    def forward_batched(self, image: torch.Tensor, want_maps: bool = False, want_dense: bool = False, kout=None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (x, y), scores [B,K], descriptors
        [B,K,256] (row per key-point), num_keypoints [B] int32, status [1] int32.  Soft-max, density and cut apply per image."""
        return self._impl.forward(self.packed, self.dims, image, self.conf, want_maps=want_maps, want_dense=want_dense, kout=kout)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"DeDoDe key-point selection failed (status {status})")
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
