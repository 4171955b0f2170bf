"""IMP matcher plugin (`sfd2+imp` of the zoo) on the MI355X HIP backend.

Drop-in for imcui/hloc/matchers/imp.py: module name `imp`, class `IMP`, same `default_conf` (:15-20) and `required_inputs`
(:21-30); the checkpoint is `pram/<model_name>` of the model repo (:34-37), its `"model"` container (:42) is unwrapped by
`unwrap_checkpoint`, and it is loaded strictly (:41-44).  The arithmetic (:51 `self.net.produce_matches(data, p=0.2)`,
pram.nets.gml.GML) runs in libimcui_hip (imcui_hip_imp_forward) for all B pairs of the call at once.
"""
from __future__ import annotations

import torch

from ... import backend
from ..utils.base_model import BaseModel
from ..utils.weights import resolve_state_dict

MATCH_P = 0.2  # the literal of imp.py:51; conf["match_threshold"] is never read by the reference


class IMP(BaseModel):
    default_conf = {
        "match_threshold": 0.2,
        "features": "sfd2",
        "model_name": "imp_gml.920.pth",
        "sinkhorn_iterations": 20,
    }
    # imp.py:51 passes p=0.2 whatever conf["match_threshold"] says, and `GML(self.conf)` (:40) reads sinkhorn_iterations once: a later
    # `matcher.conf["match_threshold"] = ...` on a cached model (imcui/ui/utils.py:921-922) changes nothing.  False (default) = exactly
    # that; True = re-read both keys on every call (what the slider intends).  Not a reference key: read with
    # conf.get("runtime_match_threshold", False), default_conf stays the reference's.
    required_inputs = [
        "image0",
        "keypoints0",
        "scores0",
        "descriptors0",
        "image1",
        "keypoints1",
        "scores1",
        "descriptors1",
    ]

    def _init(self, conf):
        self._frozen = (int(conf["sinkhorn_iterations"]), MATCH_P)
        sd = resolve_state_dict(conf, "pram")
        conf.pop("state_dict", None)
        self.conf.pop("state_dict", None)
        self.register_buffer("packed", backend.pack_imp(sd, conf), persistent=False)
        self._impl = backend.IMPHIP()

    def forward_batched(self, kpts0, kpts1, scores0, scores1, desc0, desc1, n0, n1, size0, size1) -> dict:
        """Row-per-point descriptors [B,N,128]; n0/n1 [B] int32 valid counts; sizes (W, H).
        Fixed-stride int32 outputs, no host synchronisation."""
        c = self.conf
        iters, thr = (int(c["sinkhorn_iterations"]), float(c["match_threshold"])) if c.get("runtime_match_threshold", False) else self._frozen
        return self._impl.forward(self.packed, kpts0, kpts1, scores0, scores1, desc0, desc1, n0, n1, size0, size1, iters, thr)

    def _forward(self, data):
        kpts0, kpts1 = data["keypoints0"], data["keypoints1"]
        if kpts0.shape[1] == 0 or kpts1.shape[1] == 0:  # an empty side: all -1 / 0 without a launch
            shape0, shape1 = kpts0.shape[:-1], kpts1.shape[:-1]
            return {
                "matches0": kpts0.new_full(shape0, -1, dtype=torch.long),
                "matches1": kpts1.new_full(shape1, -1, dtype=torch.long),
                "matching_scores0": kpts0.new_zeros(shape0),
                "matching_scores1": kpts1.new_zeros(shape1),
            }
        desc0 = data["descriptors0"].transpose(2, 1).float()  # imp.py:48-49: [B, 128, N] -> [B, N, 128]
        desc1 = data["descriptors1"].transpose(2, 1).float()
        B, m = kpts0.shape[0], kpts0.shape[1]
        n = kpts1.shape[1]
        dev = kpts0.device
        size0 = tuple(data["image0"].shape[-2:][::-1])
        size1 = tuple(data["image1"].shape[-2:][::-1])
        n0 = torch.full((B,), m, dtype=torch.int32, device=dev)
        n1 = torch.full((B,), n, dtype=torch.int32, device=dev)
        out = self.forward_batched(kpts0, kpts1, data["scores0"], data["scores1"], desc0, desc1, n0, n1, size0, size1)
        return {
            "matches0": out["matches0"].long(),  # -1 for an unmatched point
            "matches1": out["matches1"].long(),
            "matching_scores0": out["matching_scores0"],
            "matching_scores1": out["matching_scores1"],
        }
