"""D2-Net extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/d2net.py: same module name (`d2net`), one BaseModel subclass `D2Net`, same `default_conf` (:16-22;
`checkpoint_dir`, a path inside upstream's source tree, has no meaning here and is not carried) and `required_inputs` (:23), same
outputs (:56-60: keypoints [1,N,2] as (x, y) in pixels, scores [1,N], descriptors [1,512,N] of image 0, in ascending score order).  The
flip to BGR, `x * 255 - mean`, `process_multiscale` (scales [1], or [.5, 1, 2] with `multiscale`), the column swap and the argsort cut
(:37-54 -> mihaidusmanu/d2-net lib/model_test.py, lib/pyramid.py) run in libimcui_hip (imcui_hip_d2net_forward): no PyTorch convolution,
pooling, interpolation or `nonzero` on the path.  The level sizes floor(H s) x floor(W s) are evaluated here in float64 and handed to
the library as a level list.

The network, its detector and the pyramid are restated from their description; parity with upstream's code is not pinned
(INTEGRATION.md).  Equal scores across the cut follow a stable argsort of upstream's concatenation order (upstream's numpy argsort
leaves them open).  One batch holds images of one size; upstream asserts a batch of one, here every image of a batch is independent.
"""
from __future__ import annotations

import os

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import MODEL_REPO_ID


def resolve_d2net_checkpoint(conf: dict, folder: str) -> dict:
    """conf["state_dict"] (a state dict, or upstream's {'model': ...} container), conf["weights_path"] (a local file), else the
    reference's hub path `{folder}/{model_name}`."""
    sd = conf.get("state_dict")
    if sd is not None:
        return sd
    path = conf.get("weights_path")
    if not path:
        from huggingface_hub import hf_hub_download

        path = hf_hub_download(repo_type="model", repo_id=MODEL_REPO_ID, filename="{}/{}".format(folder, conf["model_name"]))
    if not os.path.isfile(str(path)):
        raise FileNotFoundError(f"checkpoint file not found: {path}")
    return torch.load(str(path), map_location="cpu", weights_only=True)


class D2Net(BaseModel):
    default_conf = {
        "model_name": "d2_tf.pth",
        "use_relu": True,
        "multiscale": False,
        "max_keypoints": 1024,
    }
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the d2net-ss / d2net-ms / rord confs)
    hub_folder = "d2net"  # upstream: Path(__file__).stem

    def _init(self, conf):
        ckpt = resolve_d2net_checkpoint(conf, self.hub_folder)
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_d2net(ckpt), persistent=False)
        self._impl = backend.D2NetHIP()

    def forward_batched(self, image: torch.Tensor, want_maps: bool = False, kcap=None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (x, y), scores [B,K], descriptors
        [B,K,512] (row per key-point), num_keypoints [B] int32, status [1] int32.  The pyramid and the cut apply per image."""
        return self._impl.forward(self.packed, image, self.conf, want_maps=want_maps, kcap=kcap)

    def forward_checked(self, image: torch.Tensor):
        """`forward_batched` + the ONE device->host copy of the per-image counts and the status word; a candidate overflow (status
        bit 1: channels tied for the maximum gave a pixel more than one candidate) raises.  -> (outputs, counts)."""
        out = self.forward_batched(image)
        *counts, status = torch.cat([out["num_keypoints"], out["status"]]).tolist()
        if status:
            raise backend.ImcuiHipError(f"D2-Net key-point selection failed (status {status}: more candidates than the list holds)")
        return out, counts

    def _forward(self, data):
        # the reference runs one image and returns [1,N,2] / [1,N] / [1,512,N] tensors
        out, counts = self.forward_checked(data["image"])
        n = counts[0]
        return {
            "keypoints": out["keypoints"][0, :n][None].contiguous(),
            "scores": out["scores"][0, :n][None].contiguous(),
            "descriptors": out["descriptors"][0, :n].t()[None].contiguous(),
        }
