"""Writes tests/golden/sift_wrapper_*.npz: the half of the SIFT wrapper that IS in the reference, pinned to the reference's own code.

    python tests/golden/make_sift_golden.py <directory that holds the reference's `imcui` package>

Imports imcui.hloc.extractors.sift with `cv2`, `kornia.color` and `omegaconf` stubbed in sys.modules (none of them is needed by the two
functions used here), feeds seeded synthetic detections to its `filter_dog_point` and `sift_to_rootsift`, applies the score top-k of
`extract_single_image` (:188-193), and stores inputs and results.  Only data is written.
"""
import os
import sys
import types

import numpy as np
import torch


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def main(reference_root: str) -> None:
    sys.path.insert(0, reference_root)
    _stub("cv2", Feature2D=object)
    _stub("kornia", color=_stub("kornia.color", rgb_to_grayscale=None))
    _stub("omegaconf", OmegaConf=object)
    from imcui.hloc.extractors import sift as ref

    out_dir = os.path.dirname(os.path.abspath(__file__))
    import json

    with open(os.path.join(out_dir, "sift_conf.json"), "w") as fh:  # the reference class's settings, for the plugin-contract test
        json.dump({"default_conf": ref.SIFT.default_conf, "required_data_keys": ref.SIFT.required_data_keys}, fh, indent=1)
    h, w = 60, 80
    for tag, seed, n, radius, max_keypoints in (("r0", 0, 400, 0, 150), ("r3", 1, 400, 3, 40), ("r0_all", 2, 120, 0, 4096)):
        rng = np.random.default_rng(seed)
        pts = (rng.random((n, 2)) * (w - 6, h - 6) + 3).astype(np.float32)
        pts[n // 4 : n // 2] = pts[: n // 4] + (rng.random((n // 4, 2)) * 0.3 - 0.15).astype(np.float32)  # duplicates at one pixel
        scores = rng.random(n).astype(np.float32) + np.float32(0.01)
        scores[n // 4 : n // 4 + 40] = scores[:40]  # equal scores at one pixel: the lowest |angle| decides
        scales = (rng.random(n) * 8 + 2).astype(np.float32)
        angles = (rng.random(n) * 2 * np.pi).astype(np.float32)
        angles[n // 4 + 40 : n // 4 + 50] = angles[40:50]
        scores[n // 4 + 40 : n // 4 + 50] = scores[40:50]  # equal score AND equal angle: both stay
        keep = ref.filter_dog_point(pts, scales, angles, (h, w), radius, scores=scores)
        kept_scores = torch.from_numpy(scores[keep])
        top = keep[torch.topk(kept_scores, max_keypoints).indices.numpy()] if len(keep) > max_keypoints else keep
        desc = np.rint(rng.random((32, 128)) ** 3 * 255).astype(np.float32)
        desc[0] = 0  # an all-zero row goes through the eps clamps
        root = ref.sift_to_rootsift(torch.from_numpy(desc.copy())).numpy()
        np.savez_compressed(os.path.join(out_dir, f"sift_wrapper_{tag}.npz"), points=pts, scores=scores, scales=scales, angles=angles,
                            image_shape=np.array([h, w]), nms_radius=np.array(radius), max_keypoints=np.array(max_keypoints), keep=keep,
                            topk=np.sort(top), descriptors=desc, rootsift=root)  # fmt: skip
        print(tag, "kept", len(keep), "of", n, "after top-k", len(top))


if __name__ == "__main__":
    main(sys.argv[1])
