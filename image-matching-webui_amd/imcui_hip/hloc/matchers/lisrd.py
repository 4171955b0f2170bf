"""LISRD matcher plugin on the MI355X HIP backend (zoo entries LISRD+SuperPoint, LISRD+ALIKED, LISRD+SIFT).

Drop-in for imcui/hloc/matchers/lisrd.py: same module name (`lisrd`), one BaseModel subclass `Lisrd`, same `default_conf` (:166-171) and
`required_inputs` (:172-175), same outputs (:300-306: keypoints0 / keypoints1 [N,2] as (x, y), mkeypoints0 / mkeypoints1 [P,2], mconf [P],
matches in ascending order of the image-0 index, as the reference's mask yields them).  What runs where:

  detector   this backend's own SuperPoint / ALIKED / SIFT plugin, built with exactly the confs of the reference's `_DETECTOR_BUILDERS`
             (:45-69); an unknown detector raises the reference's ValueError (:194-198)
  describe   `img * 255` (:209-210), the network (:259-268), the (x, y) -> (row, col) flip (:256-257) and `_extract_descriptors` (:90-119)
             are ONE library call per image (imcui_hip_lisrd_describe)
  match      `_lisrd_matcher` (:122-134) and `_compute_confidence` (:137-149) are ONE library call (imcui_hip_lisrd_match); neither
             [N,4,M] tensor exists.  Among exactly equal similarities the first index wins (`torch.max` leaves it open)
  host       the gray conversion for SuperPoint (kornia is not installed: `rgb_to_grayscale` is restated with its weights 0.299 / 0.587 /
             0.114), the zero-key-point guards (:237-245) and ONE read-back of the matched rows for the ragged outputs

The network (`lisrd.models`) is not part of the reference checkout: it is restated from its description (tests/lisrd_reference.py) and
parity with upstream's code is not pinned ("LISRD: what is pinned").  Weights: conf["state_dict"] / conf["weights_path"],
else the reference's hub path `lisrd/<model_name>.pth`; the checkpoint's `model_state_dict` container is unwrapped.  Backend-only conf key:
`detector_weights` (a dict merged into the detector's conf: `state_dict` or `weights_path`).  `compute_meta_desc: False` is not served.
"""
from __future__ import annotations

import torch

from ... import backend
from ..extractors.aliked import ALIKED as ALIKEDExtractor
from ..extractors.sift import SIFT as SIFTExtractor
from ..extractors.superpoint import SuperPoint as SuperPointExtractor
from ..utils.base_model import BaseModel
from ..utils.weights import resolve_state_dict

# lisrd.py:45-69, conf for conf
_DETECTOR_BUILDERS = {
    "superpoint": lambda max_kpts, extra: SuperPointExtractor(
        {"nms_radius": 4, "model_name": "superpoint_v1.pth", "keypoint_threshold": 0.005, "max_keypoints": max_kpts, "remove_borders": 4, **extra}
    ),
    "aliked": lambda max_kpts, extra: ALIKEDExtractor({"name": "aliked", "model_name": "aliked-n16", "max_num_keypoints": max_kpts, "detection_threshold": 0.2, **extra}),
    "sift": lambda max_kpts, extra: SIFTExtractor({"max_keypoints": max_kpts, "backend": "opencv", **extra}),
}


def rgb_to_grayscale(image: torch.Tensor) -> torch.Tensor:
    """kornia.color.rgb_to_grayscale restated (kornia is not installed): 0.299 r + 0.587 g + 0.114 b on [B,3,H,W]."""
    r, g, b = image[:, 0:1], image[:, 1:2], image[:, 2:3]
    return 0.299 * r + 0.587 * g + 0.114 * b


class Lisrd(BaseModel):
    default_conf = {
        "name": "two_view_pipeline",
        "model_name": "lisrd_aachen",
        "max_keypoints": 2048,
        "detector": "superpoint",  # "superpoint", "aliked", or "sift"
    }
    required_inputs = [
        "image0",
        "image1",
    ]

    def _init(self, conf):
        detector_name = conf.get("detector", "superpoint")
        if detector_name not in _DETECTOR_BUILDERS:
            raise ValueError(f"Unknown LISRD detector: {detector_name}. " f"Choose from {list(_DETECTOR_BUILDERS.keys())}.")
        sd = resolve_state_dict({**conf, "model_name": f"{conf['model_name']}.pth"}, "lisrd")
        extra = dict(conf.get("detector_weights") or {})
        for key in ("state_dict", "detector_weights"):  # keep self.conf small / printable
            conf.pop(key, None)
            self.conf.pop(key, None)
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", backend.pack_lisrd(sd), persistent=False)
        self._impl = backend.LisrdHIP()
        self.detector = _DETECTOR_BUILDERS[detector_name](conf["max_keypoints"], extra)

    def detect(self, image: torch.Tensor) -> torch.Tensor:
        """(x, y) key-points [N,2] of ONE image [1,C,H,W] in [0,1] (lisrd.py:219-252)."""
        if self.conf.get("detector", "superpoint") == "superpoint" and image.shape[1] == 3:
            image = rgb_to_grayscale(image)
        kps = self.detector({"image": image})["keypoints"]
        kps = kps[0]  # SuperPoint / ALIKED: a list of per-image tensors; SIFT: [B,N,2] with B = 1
        if kps.numel() == 0:
            kps = torch.zeros(0, 2, device=image.device)
        return kps.view(-1, 2).to(image.device)

    def describe(self, image: torch.Tensor, kps: torch.Tensor) -> dict:
        """desc [1,K,4,128], meta [1,K,4,1024] (K = max(N, 1) rows, the first N live) and the count on the device."""
        n = kps.shape[0]
        rows = torch.zeros((1, max(n, 1), 2), dtype=torch.float32, device=image.device)
        rows[0, :n] = kps
        cnt = torch.tensor([n], dtype=torch.int32, device=image.device)
        out = self._impl.describe(self.packed, image, rows, cnt)
        out["count"] = cnt
        return out

    def _forward(self, data):
        img0, img1 = data["image0"], data["image1"]
        dev = self.packed.device
        img0, img1 = img0.to(dev), img1.to(dev)
        with torch.no_grad():
            kps0, kps1 = self.detect(img0), self.detect(img1)
            d0, d1 = self.describe(img0, kps0), self.describe(img1, kps1)
            m = backend.lisrd_match(d0["desc"], d0["meta"], d1["desc"], d1["meta"], d0["count"], d1["count"])
            matches0 = m["matches0"][0]
            idx0 = torch.nonzero(matches0 > -1).flatten()  # (the one read-back: the number of matches sizes the ragged outputs)
            idx1 = matches0[idx0].long()
        return {
            "keypoints0": kps0,
            "keypoints1": kps1,
            "mkeypoints0": kps0[idx0],
            "mkeypoints1": kps1[idx1],
            "mconf": m["mconf"][0][idx0],
        }
