"""RoRD extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/rord.py, which is imcui/hloc/extractors/d2net.py line for line with its own checkpoint (`rord.pth`,
hub folder `rord`): same module name (`rord`), one BaseModel subclass `RoRD`, same `default_conf` (:17-23, without `checkpoint_dir`)
and `required_inputs` (:24), same outputs.  RoRD's lib/model_test.py and lib/pyramid.py are taken to be D2-Net's (the repository is a
fork that trains other weights for the same network); everything runs in libimcui_hip through the D2-Net plugin (imcui_hip_d2net_forward).
"""
from __future__ import annotations

from .d2net import D2Net


class RoRD(D2Net):
    default_conf = {
        "model_name": "rord.pth",
        "use_relu": True,
        "multiscale": False,
        "max_keypoints": 1024,
    }
    required_inputs = ["image"]
    takes_rgb = True
    hub_folder = "rord"
