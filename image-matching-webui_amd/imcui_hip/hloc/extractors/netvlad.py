"""NetVLAD global-descriptor plugin on the MI355X HIP backend (retrieval_zoo entry `netvlad`).

Drop-in for imcui/hloc/extractors/netvlad.py: same module name (`netvlad`), one BaseModel subclass `NetVLAD`, same `default_conf` (:42),
`required_inputs` (:43), `dir_models` keys (:47-50) and assertions (:53, :124-125), same output (:146: `global_descriptor` [B,4096], or
[B,32768] with `whiten: False`).  The checkpoint is the same MATLAB file at the same cache path
`torch.hub.get_dir()/netvlad/<model_name>.mat` (or conf["weights_path"]), parsed with scipy.io.loadmat exactly as :76-120 does: the
permutes, the sign flip of the centres and `averageImage[0, 0]`.  The wrapper's `clamp(x * 255, 0, 255) - mean`, VGG-16 to conv5_3, the
per-pixel normalisation, the NetVLAD layer, the whitening and both normalisations (:126-144) run in libimcui_hip
(imcui_hip_netvlad_forward): no PyTorch convolution, soft-max or matrix product on the path.

This network IS pinned to the reference: its whole definition is in the reference checkout, and tests/golden/make_netvlad_golden.py
records the reference's own output ("NetVLAD: what is pinned").  One batch holds images of one size.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from ... import backend
from ..utils.base_model import BaseModel

EPS = 1e-6

VGG16_CONV_OPS = tuple(op for _, _, op in backend.NETVLAD_LAYERS)  # the nn.Conv2d children of vgg16().features[:-2]


def load_netvlad_mat(path, whiten: bool) -> dict:
    """The MATLAB checkpoint -> the state dict of the reference module (+ `preprocess.mean`), following netvlad.py:76-120 line by line."""
    from scipy.io import loadmat

    mat = loadmat(str(path), struct_as_record=False, squeeze_me=True)
    layers = mat["net"].layers
    sd = {}
    for op in VGG16_CONV_OPS:  # :79-90, zip(backbone.children(), layers): child `op` takes layer `op`
        w = layers[op].weights[0]  # S x S x IN x OUT
        b = layers[op].weights[1]  # OUT
        sd[f"backbone.{op}.weight"] = torch.tensor(w).float().permute([3, 2, 0, 1]).contiguous()
        sd[f"backbone.{op}.bias"] = torch.tensor(b).float()
    score_w = layers[30].weights[0]  # D x K
    center_w = -layers[30].weights[1]  # D x K; centers are stored as opposite in the official MATLAB code (:94-95)
    sd["netvlad.score_proj.weight"] = torch.tensor(score_w).float().permute([1, 0]).unsqueeze(-1).contiguous()
    sd["netvlad.centers"] = torch.tensor(center_w).float()
    if whiten:  # :106-114
        w = layers[33].weights[0]  # 1 x 1 x IN x OUT
        b = layers[33].weights[1]  # OUT
        sd["whiten.weight"] = torch.tensor(w).float().squeeze().permute([1, 0]).contiguous()
        sd["whiten.bias"] = torch.tensor(b.squeeze()).float()
    sd["preprocess.mean"] = torch.tensor(np.asarray(mat["net"].meta.normalization.averageImage[0, 0], dtype=np.float32))  # :118
    return sd


class NetVLAD(BaseModel):
    default_conf = {"model_name": "VGG16-NetVLAD-Pitts30K", "whiten": True}
    required_inputs = ["image"]
    takes_rgb = True  # the batch extractor feeds [B,3,h,w] for `grayscale: False` (the `netvlad` conf)
    returns_global_descriptor = True  # ... and writes `global_descriptor` / `image_size` groups without key-points

    # Models exported using https://github.com/uzh-rpg/netvlad_tf_open/blob/master/matlab/net_class2struct.m.
    dir_models = {
        "VGG16-NetVLAD-Pitts30K": "https://cvg-data.inf.ethz.ch/hloc/netvlad/Pitts30K_struct.mat",
        "VGG16-NetVLAD-TokyoTM": "https://cvg-data.inf.ethz.ch/hloc/netvlad/TokyoTM_struct.mat",
    }

    def _init(self, conf):
        assert conf["model_name"] in self.dir_models.keys()
        whiten = bool(conf["whiten"])
        sd = conf.get("state_dict")
        if sd is None:
            path = conf.get("weights_path")
            checkpoint = Path(path) if path else Path(torch.hub.get_dir(), "netvlad", conf["model_name"] + ".mat")
            if not checkpoint.exists():
                if path:
                    raise FileNotFoundError(f"checkpoint file not found: {checkpoint}")
                checkpoint.parent.mkdir(exist_ok=True, parents=True)
                torch.hub.download_url_to_file(self.dir_models[conf["model_name"]], str(checkpoint))  # the reference runs wget (:59-62)
            sd = load_netvlad_mat(checkpoint, whiten)
        elif not whiten:
            sd = {k: v for k, v in sd.items() if not k.startswith("whiten.")}
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        self.whiten = whiten
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_netvlad(sd, whiten), persistent=False)
        self._impl = backend.NetVLADHIP()

    def forward_batched(self, image: torch.Tensor, want_map: bool = False) -> dict:
        """image [B,3,H,W] in [0,1] -> {"global_descriptor": [B,4096] or [B,32768]}; no host synchronisation (graph-capturable)."""
        return self._impl.forward_batched(self.packed, image, self.whiten, want_map=want_map)

    def _forward(self, data):
        image = data["image"]
        assert image.shape[1] == 3
        assert image.min() >= -EPS and image.max() <= 1 + EPS
        return {"global_descriptor": self.forward_batched(image)["global_descriptor"]}
