"""SIFT extractor plugin on the MI355X HIP backend.

Drop-in for imcui/hloc/extractors/sift.py with `backend: "opencv"` (the default, and the only backend the `sift` conf and
`sift-lightglue` use): same module name (`sift`), one BaseModel subclass `SIFT`, the same `default_conf` (:82-91) and
`required_data_keys` (:93), the same dict out of `_forward` (:196-216: keypoints [B,N,2], scales, oris, scores, keypoint_scores [B,N],
descriptors [B,128,N]).  `run_opencv_sift` (:61-78, cv2.SIFT_create(...).detectAndCompute), `filter_dog_point` (:19-52), the score
top-k (:188-193) and `sift_to_rootsift` (:55-58) run in libimcui_hip (imcui_hip_sift_forward); no cv2, kornia or omegaconf.

Differences, all stated: key-points come in detection order (octave, layer, row, column, orientation bin), also after the
`max_keypoints` cut (the reference re-orders by score when it cuts; cv2's own order depends on its thread pool); the `pycolmap*`
backends and a non-default `first_octave` are refused by name; `data["image_size"]` is refused.
"""
from __future__ import annotations

import torch

from ... import backend
from ..utils.base_model import BaseModel


class SIFT(BaseModel):
    default_conf = {
        "rootsift": True,
        "nms_radius": 0,  # None to disable filtering entirely.
        "max_keypoints": 4096,
        "backend": "opencv",  # in {opencv, pycolmap, pycolmap_cpu, pycolmap_cuda}
        "detection_threshold": 0.0066667,  # from COLMAP
        "edge_threshold": 10,
        "first_octave": -1,  # only used by pycolmap, the default of COLMAP
        "num_octaves": 4,
    }

    required_data_keys = ["image"]
    required_inputs = ["image"]

    def _init(self, conf):
        backend.sift_check_args((1, 1, 32, 32), conf)
        # SIFT has no weights; the buffer makes `.to(device)`, the UI model cache and the batch driver's `next(model.buffers())` work
        self.register_buffer("anchor", torch.zeros(1), persistent=False)
        self._impl = backend.SiftHIP()

    def forward_batched(self, image: torch.Tensor, kcap: int | None = None, ccap: int | None = None, debug: bool = False) -> dict:
        """Fixed-stride outputs, no host synchronisation (graph-capturable): keypoints [B,K,2] (pixels), scores, scales, oris [B,K],
        descriptors [B,K,128] (row per key-point), num_keypoints [B] int32, status [1] int32, counts [B,3] int32."""
        return self._impl.forward(image, self.conf, kcap=kcap, ccap=ccap, debug=debug)

    def forward_checked(self, image: torch.Tensor, kcap: int | None = None, ccap: int | None = None):
        """`forward_batched` + the ONE device->host copy of the counts and the status word; a capacity overflow (status bit 1: more
        survivors than `kcap`, bit 2: more extrema than `ccap`) is retried with the capacities the counts ask for, any other non-zero
        status raises.  -> (outputs, counts)."""
        for _ in range(4):  # (a longer candidate list can uncover more survivors: the counts of an overflowed call are lower bounds)
            out = self.forward_batched(image, kcap=kcap, ccap=ccap)
            *counts, status = torch.cat([out["counts"].flatten(), out["status"]]).tolist()
            if not status & 3:
                break
            if status & 2:
                ccap = max(counts[0::3] + counts[1::3])
            if status & 1:
                kcap = max(counts[2::3])
        if status:
            raise backend.ImcuiHipError(f"SIFT key-point selection failed (status {status})")
        return out, counts[2::3]

    def _forward(self, data):
        if "image_size" in data:
            raise backend.ImcuiHipError("SIFT on the HIP backend does not crop by `image_size` (the reference slices padded batches on the host): pass unpadded images")
        out, counts = self.forward_checked(data["image"])
        if len(set(counts)) > 1:  # the reference's torch.stack raises here too; every reference caller passes B = 1
            raise ValueError(f"SIFT found {counts} key-points in the images of one batch: unequal counts cannot be stacked; use forward_checked")
        n = counts[0]
        pred = {k: out[k][:, :n].contiguous() for k in ("keypoints", "scales", "oris", "scores")}
        pred["descriptors"] = out["descriptors"][:, :n].permute(0, 2, 1)
        pred["keypoint_scores"] = pred["scores"].clone()
        return pred
