"""CosPlace global-descriptor plugin on the MI355X HIP backend (retrieval_zoo entry `cosplace`).

Drop-in for imcui/hloc/extractors/cosplace.py: same module name (`cosplace`), one BaseModel subclass `CosPlace`, same `default_conf` (:24),
`required_inputs` (:25) and output (:43-45: `global_descriptor` [B,fc_output_dim], unit norm).  tvf.Normalize (:36-38, :41), the ResNet
trunk, L2Norm, GeM, the linear layer and the last L2Norm run in libimcui_hip (imcui_hip_places_forward): no PyTorch convolution, pooling
or matrix product on the path.  imcui/hloc/extractors/eigenplaces.py is the same wrapper over the same architecture with other
checkpoints; its plugin (eigenplaces.py here) subclasses this one.

The weights come from conf["state_dict"], else conf["weights_path"], else the file upstream's hubconf leaves in
`torch.hub.get_dir()/checkpoints`, else `torch.hub.load_state_dict_from_url` as upstream does.  The reference calls
torch.hub.load("gmberton/CosPlace", "get_trained_model", ...) (:28-34), which runs upstream's Python from the hub cache; this plugin only
reads the checkpoint.

NOT pinned to the reference: the network is not in the reference checkout, it is restated from torchvision's ResNet and
gmberton/CosPlace's cosplace_model/network.py (tests/places_reference.py).  The checkpoint file names, the release URLs and the
state-dict key names below are as recalled from upstream and have not been checked against a real file ("CosPlace /
EigenPlaces: what is pinned"); `STATE_DICT_KEYS` is the one table to edit if a real checkpoint names its tensors differently.  One batch
holds images of one size.
"""
from __future__ import annotations

from pathlib import Path

import torch

from ... import backend
from ..utils.base_model import BaseModel

# upstream prefix -> the prefix imcui_hip_places_tensor_name uses.  Identity today (unverified against a real checkpoint): a differing
# file is a one-line fix here.
STATE_DICT_KEYS = {
    "backbone.": "backbone.",
    "aggregation.": "aggregation.",
}


def rename_state_dict(sd: dict) -> dict:
    """Unwrap `{"state_dict": ...}` / `{"model_state_dict": ...}`, strip DataParallel's `module.`, apply STATE_DICT_KEYS."""
    for wrapper in ("state_dict", "model_state_dict"):
        if wrapper in sd and isinstance(sd[wrapper], dict):
            sd = sd[wrapper]
    out = {}
    for k, v in sd.items():
        k = k[len("module."):] if k.startswith("module.") else k
        for src, dst in STATE_DICT_KEYS.items():
            if k.startswith(src):
                k = dst + k[len(src):]
                break
        out[k] = v
    return out


class CosPlace(BaseModel):
    default_conf = {"backbone": "ResNet50", "fc_output_dim": 2048}
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `cosplace` / `eigenplaces` confs)
    returns_global_descriptor = True  # ... and writes `global_descriptor` / `image_size` groups without key-points

    variant = "CosPlace"  # the hub repository gmberton/<variant> and the checkpoint suffix
    # as recalled from upstream's hubconf (unverified): <release>/<backbone>_<fc_output_dim>_<suffix>.pth
    release_url = "https://github.com/gmberton/{variant}/releases/download/v1.0/{backbone}_{dim}_{suffix}.pth"

    def checkpoint_name(self, conf) -> str:
        return f"{conf['backbone']}_{conf['fc_output_dim']}_{self.variant.lower()}.pth"

    def _init(self, conf):
        code = backend.places_backbone_code(conf["backbone"])  # refuses VGG16 by name
        dim = int(conf["fc_output_dim"])
        sd = conf.get("state_dict")
        if sd is None:
            path = conf.get("weights_path")
            checkpoint = Path(path) if path else Path(torch.hub.get_dir(), "checkpoints", self.checkpoint_name(conf))
            if checkpoint.exists():
                sd = torch.load(str(checkpoint), map_location="cpu", weights_only=True)
            elif path:
                raise FileNotFoundError(f"checkpoint file not found: {checkpoint}")
            else:
                url = self.release_url.format(variant=self.variant, backbone=conf["backbone"], dim=dim, suffix=self.variant.lower())
                sd = torch.hub.load_state_dict_from_url(url, map_location="cpu")
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_places(rename_state_dict(sd), code, dim), persistent=False)
        self._impl = backend.PlacesHIP(code, dim)

    def forward_batched(self, image: torch.Tensor, want_map: bool = False) -> dict:
        """image [B,3,H,W] in [0,1] -> {"global_descriptor": [B,fc_output_dim]}; no host synchronisation (graph-capturable)."""
        return self._impl.forward_batched(self.packed, image, want_map=want_map)

    def _forward(self, data):
        return {"global_descriptor": self.forward_batched(data["image"])["global_descriptor"]}
