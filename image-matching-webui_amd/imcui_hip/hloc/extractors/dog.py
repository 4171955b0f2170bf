"""DoG + HardNet / SOSNet extractor plugin on the MI355X HIP backend (extractor confs `hardnet` and `sosnet`).

Drop-in for imcui/hloc/extractors/dog.py with `descriptor: "hardnet"` / `"sosnet"`: same module name (`dog`), one BaseModel subclass
`DoG`, the same `default_conf` (:23-32) and `required_inputs` (:33), the same dict out of `_forward` (:129-135: keypoints [1,N,2], scales,
oris in DEGREES, scores all zero, descriptors [1,128,N]).  Detection is csrc/sift.hip (`backend.SiftHIP`, unchanged); the LAF patches cut
from kornia's image pyramid, the 7-layer patch network and the output normalisation (:87-105) run in libimcui_hip
(imcui_hip_patchdesc_forward): no PyTorch convolution or grid_sample on the path.

Stated divergences ("DoG + HardNet / SOSNet: what is pinned"):
  * the reference detects with pycolmap.Sift (VLFeat, `first_octave: 0`); this plugin detects with the OpenCV-semantics detector of
    csrc/sift.hip: the image is quantised to uint8, the first octave is -1 (the doubled image: more fine-scale key-points), three layers
    per octave, contrastThreshold = 3 * options.peak_threshold (OpenCV's |D| * layers < contrastThreshold set equal to VLFeat's
    |D| < peak_threshold), edge threshold 10, no `filter_dog_point`.  scale = KeyPoint.size / 2 (diameter to sigma), ori = angle.
    `options.first_octave` other than 0 and unknown `options` keys are refused; `first_octave: 0` is accepted and served by that detector;
  * the reference's `max_keypoints` cut is `topk` of an all-zero score vector, an arbitrary subset; this plugin keeps the highest
    |contrast| (the detector's own cut).  `scores` are returned as zeros all the same;
  * `descriptor: "sift"` / `"rootsift"` (the class default) are refused by name: the `sift` plugin serves them;
  * kornia is absent and unpinned by the reference: pyramid, LAF and grid rules are those of kornia 0.7.0 as restated in
    tests/dog_reference.py, and the stage is parity-unpinned.

Weights: conf["state_dict"] (a kornia state dict), else conf["checkpoint"] (a file), else the file kornia's `load_state_dict_from_url`
would use in `torch.hub.get_dir()/checkpoints`, fetched as kornia does only when it is missing.
"""
from __future__ import annotations

from pathlib import Path

import torch

from ... import backend
from ..utils.base_model import BaseModel

EPS = 1e-6

# kornia/feature/hardnet.py `urls["liberty_aug"]` and kornia/feature/sosnet.py `urls["lib"]`
WEIGHT_URLS = {
    "hardnet": "https://github.com/DagnyT/hardnet/raw/master/pretrained/train_liberty_with_aug/checkpoint_liberty_with_aug.pth",
    "sosnet": "https://github.com/yuruntian/SOSNet/raw/master/sosnet-weights/sosnet_32x32_liberty.pth",
}
OPTION_KEYS = ("first_octave", "peak_threshold")


class DoG(BaseModel):
    default_conf = {
        "options": {
            "first_octave": 0,
            "peak_threshold": 0.01,
        },
        "descriptor": "rootsift",
        "max_keypoints": -1,
        "patch_size": 32,
        "mr_size": 12,
    }
    required_inputs = ["image"]
    detection_noise = 1.0
    max_batch_size = 1024

    def _init(self, conf):
        name = conf["descriptor"]
        if name in ("sift", "rootsift"):
            raise backend.ImcuiHipError(f"DoG descriptor '{name}' is not served by the `dog` plugin of the HIP backend: use the `sift` plugin (conf `sift`)")
        if name not in backend.PATCHDESC_MODELS:
            raise ValueError(f"Unknown descriptor: {name}")
        options = {**self.default_conf["options"], **dict(conf.get("options") or {})}
        unknown = sorted(set(options) - set(OPTION_KEYS))
        if unknown:
            raise backend.ImcuiHipError(f"DoG options {unknown} are pycolmap.SiftExtractionOptions fields the HIP detector does not read: only {list(OPTION_KEYS)}")
        if int(options["first_octave"]) != 0:
            raise backend.ImcuiHipError(f"DoG options.first_octave={options['first_octave']}: only 0 is accepted (it is served by the first-octave -1 detector of csrc/sift.hip)")
        if int(conf["patch_size"]) != 32:
            raise backend.ImcuiHipError(f"DoG patch_size={conf['patch_size']}: HardNet and SOSNet take 32 x 32 patches")
        self.descriptor = name
        maxk = conf["max_keypoints"]
        self.sift_conf = {
            "rootsift": False,
            "nms_radius": None,  # no filter_dog_point
            "max_keypoints": int(maxk) if maxk is not None and int(maxk) > 0 else -1,
            "backend": "opencv",
            "detection_threshold": 3.0 * float(options["peak_threshold"]),
            "edge_threshold": 10,
            "first_octave": -1,
            "num_octaves": 3,
        }
        backend.sift_check_args((1, 1, 32, 32), self.sift_conf)
        sd = conf.get("state_dict")
        if sd is None:
            path = conf.get("checkpoint")
            checkpoint = Path(path) if path else Path(torch.hub.get_dir(), "checkpoints", WEIGHT_URLS[name].rsplit("/", 1)[1])
            if not checkpoint.exists():
                if path:
                    raise FileNotFoundError(f"checkpoint file not found: {checkpoint}")
                checkpoint.parent.mkdir(exist_ok=True, parents=True)
                torch.hub.download_url_to_file(WEIGHT_URLS[name], str(checkpoint))
            sd = torch.load(str(checkpoint), map_location="cpu")
        conf.pop("state_dict", None)  # keep self.conf small / printable
        self.conf.pop("state_dict", None)
        pack = backend.pack_hardnet if name == "hardnet" else backend.pack_sosnet
        # registered buffer: counted by the UI model cache and moved by `.to(device)`
        self.register_buffer("packed", pack(sd), persistent=False)
        self._sift = backend.SiftHIP()
        self._impl = backend.PatchDescHIP()

    def forward_batched(self, image: torch.Tensor, kcap: int | None = None, ccap: int | None = None, chunk: int | None = None) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (pixels), scores (zeros), scales (sigma),
        oris (degrees) [B,K], descriptors [B,K,128] (row per key-point; rows past the count are zero), num_keypoints [B] int32, status [1]
        int32 (the detector's: bit 1 `kcap`, bit 2 `ccap` too small), desc_status [1] int32 (bit 2: a non-finite key-point), counts [B,3]."""
        det = self._sift.forward(image, self.sift_conf, kcap=kcap, ccap=ccap)
        scales = det["scales"] * 0.5  # OpenCV's KeyPoint.size is a diameter
        oris = torch.rad2deg(det["oris"])
        res = self._impl.forward(self.packed, image, det["keypoints"], scales, oris, det["num_keypoints"], self.descriptor, mr_size=float(self.conf["mr_size"]),
                                 chunk=int(chunk or self.max_batch_size))  # fmt: skip
        return {"keypoints": det["keypoints"], "scores": torch.zeros_like(det["scores"]), "scales": scales, "oris": oris, "descriptors": res["descriptors"],
                "num_keypoints": det["num_keypoints"], "status": det["status"], "desc_status": res["status"], "counts": det["counts"]}  # fmt: skip

    def forward_checked(self, image: torch.Tensor, kcap: int | None = None, ccap: int | None = None):
        """`forward_batched` + the ONE device->host copy of the counts and the status words; a capacity overflow of the detector is retried
        with the capacities the counts ask for, any other non-zero status raises.  -> (outputs, counts)."""
        for _ in range(4):
            out = self.forward_batched(image, kcap=kcap, ccap=ccap)
            *counts, status, dstatus = torch.cat([out["counts"].flatten(), out["status"], out["desc_status"]]).tolist()
            if not status & 3:
                break
            if status & 2:
                ccap = max(counts[0::3] + counts[1::3])
            if status & 1:
                kcap = max(counts[2::3])
        if status or dstatus:
            raise backend.ImcuiHipError(f"DoG key-point selection failed (detector status {status}, descriptor status {dstatus})")
        return out, counts[2::3]

    def _forward(self, data):
        image = data["image"]
        assert image.shape[1] == 1
        assert image.min() >= -EPS and image.max() <= 1 + EPS
        out, counts = self.forward_checked(image)
        if len(set(counts)) > 1:  # every reference caller passes B = 1
            raise ValueError(f"DoG found {counts} key-points in the images of one batch: unequal counts cannot be stacked; use forward_checked")
        n = counts[0]
        pred = {k: out[k][:, :n].contiguous() for k in ("keypoints", "scales", "oris", "scores")}
        pred["descriptors"] = out["descriptors"][:, :n].permute(0, 2, 1)
        return pred
