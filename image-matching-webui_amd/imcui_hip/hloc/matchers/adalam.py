"""AdaLAM matcher plugin (`adalam` of the zoo: SIFT key-points with scales and orientations) on the MI355X HIP backend.

Drop-in for imcui/hloc/matchers/adalam.py: module name `adalam`, class `AdaLAM`, the same `default_conf` (:10-22, minus `device`:
the plugin runs where its inputs live) and `required_inputs` (:23-34).  The arithmetic (:46-57 `self.adalam.match_and_filter`,
kornia.feature.adalam.AdalamFilter) runs in libimcui_hip (imcui_hip_adalam_forward) for all B pairs of a call at once.  There are no
weights.  kornia is not pinned here: the rule this backend implements and every known difference are in INTEGRATION.md, "AdaLAM:
what is pinned".
"""
from __future__ import annotations

import torch

from ... import backend
from ..utils.base_model import BaseModel


class AdaLAM(BaseModel):
    default_conf = {
        "area_ratio": 100,
        "search_expansion": 4,
        "ransac_iters": 128,
        "min_inliers": 6,
        "min_confidence": 200,
        "orientation_difference_threshold": 30,
        "scale_rate_threshold": 1.5,
        "detected_scale_rate_threshold": 5,
        "refit": True,
        "force_seed_mnn": True,
    }
    required_inputs = [
        "image0",
        "image1",
        "descriptors0",
        "descriptors1",
        "keypoints0",
        "keypoints1",
        "scales0",
        "scales1",
        "oris0",
        "oris1",
    ]
    add_scale_ori = True  # hloc/match_features.py::_call_batched hands scales / oris to `forward_batched(..., scales_oris=)`

    def _init(self, conf):
        backend.adalam_conf_array(conf)  # (a conf the kernels would refuse is refused here)
        self.register_buffer("anchor", torch.zeros(1), persistent=False)  # no weights: `.to(device)` and the drivers' device look-up need one buffer
        self._impl = backend.AdaLAMHIP()

    def _check_scale_ori(self, scales_oris):
        """kornia raises AttributeError when a relative test is on and its key-point attribute is missing (adalam.py: `filter_matches`)."""
        need_o, need_s = backend.adalam_needs(self.conf)
        s0, o0, s1, o1 = (None,) * 4 if scales_oris is None else scales_oris
        if need_o and (o0 is None or o1 is None):
            raise AttributeError("orientation_difference_threshold is set but oris0 / oris1 are missing: give them or set the threshold to None")
        if need_s and (s0 is None or s1 is None):
            raise AttributeError("scale_rate_threshold is set but scales0 / scales1 are missing: give them or set the threshold to None")

    def forward_batched(self, kpts0, kpts1, desc0, desc1, n0, n1, size0, size1, scales_oris=None, probe: bool = False) -> dict:
        """Row-per-point descriptors [B,N,D] (D = 64, 128 or 256); n0 / n1 [B] int32 valid counts; sizes (W, H); scales_oris =
        (scales0, oris0, scales1, oris1) [B,N].  Fixed-stride outputs (matches0 int32, -1 = unmatched; matching_scores0 zeros), no host
        synchronisation."""
        self._check_scale_ori(scales_oris)
        return self._impl.forward(kpts0, kpts1, desc0, desc1, n0, n1, size0, size1, self.conf, scales_oris=scales_oris, probe=probe)

    def _forward(self, data):
        kpts0, kpts1 = data["keypoints0"], data["keypoints1"]
        assert kpts0.size(0) == 1  # adalam.py:40
        m, n = kpts0.shape[1], kpts1.shape[1]
        if m < 2 or n < 2:  # adalam.py:41-44: nothing to match, without a launch
            return {"matches0": kpts0.new_full((1, m), -1, dtype=torch.long), "matching_scores0": kpts0.new_zeros((1, m))}
        dev = kpts0.device
        desc0 = data["descriptors0"].transpose(2, 1).float()  # adalam.py:49-50: [1, D, N] -> [1, N, D]
        desc1 = data["descriptors1"].transpose(2, 1).float()
        size0 = tuple(data["image0"].shape[2:][::-1])  # adalam.py:51-52 pass (H, W)
        size1 = tuple(data["image1"].shape[2:][::-1])
        n0 = torch.full((1,), m, dtype=torch.int32, device=dev)
        n1 = torch.full((1,), n, dtype=torch.int32, device=dev)
        so = (data["scales0"].float(), data["oris0"].float(), data["scales1"].float(), data["oris1"].float())
        out = self.forward_batched(kpts0.float(), kpts1.float(), desc0, desc1, n0, n1, size0, size1, scales_oris=so)
        return {"matches0": out["matches0"][:, :m].long(), "matching_scores0": out["matching_scores0"][:, :m]}
