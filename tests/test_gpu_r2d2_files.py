"""R2D2 through the file-based batch extractor (the `r2d2` zoo entry: `feature: r2d2` + `matcher: NN-mutual`): RGB files ->
device-side RGB preprocessing (`grayscale: False`, resize_max 1024) -> R2D2 in batches -> feature .h5 with the keys, shapes and
dtypes the reference writes, compared with one image per plugin call (imcui/hloc/configs/extractors.py conf `r2d2`)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import r2d2_state_dict
from test_gpu_disk_files import _host_rgb, _rgb_u8

pytestmark = pytest.mark.gpu


def test_r2d2_extract_from_files(tmp_path):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc.extractors.r2d2 import R2D2
    from imcui_hip.hloc.utils.h5lite import open_h5

    root = tmp_path / "images"
    root.mkdir()
    images = {"a.png": _rgb_u8(96, 128, 400), "b.png": _rgb_u8(96, 128, 401)}  # one size: one batch of two
    for name, arr in images.items():
        Image.fromarray(np.ascontiguousarray(arr)).save(root / name)
    files = list(images)
    conf = {"output": "feats-r2d2-n5000-r1024",
            "model": {"name": "r2d2", "max_keypoints": 5000, "reliability_threshold": 0.7, "repetability_threshold": 0.7},
            "preprocessing": {"grayscale": False, "resize_max": 1024}}  # the reference's `r2d2` conf  # fmt: skip
    # (min_size is a conf key of the extractor: lowered so that the small test images run six levels)
    r2d2 = R2D2({**conf["model"], "min_size": 48, "state_dict": r2d2_state_dict(0)}).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=r2d2, batch_size=2)
    assert feature_path == tmp_path / "out" / "feats-r2d2-n5000-r1024.h5"
    assert sorted(ef.list_h5_names(feature_path)) == sorted(files)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    with open_h5(feature_path, "r") as fd:
        for f in files:
            raw = ef.read_image_u8(root / f)
            image = _host_rgb(raw, pconf).cuda()
            with torch.no_grad():
                pred = r2d2({"image": image})
            h, w = image.shape[-2:]
            scales = (np.array(raw.shape[:2][::-1]) / np.array([w, h])).astype(np.float32)
            kp = ((pred["keypoints"][0].cpu().numpy() + 0.5) * scales[None] - 0.5).astype(np.float16)
            grp = fd[f]
            assert set(grp.keys()) == {"keypoints", "scores", "descriptors", "image_size"}
            n = kp.shape[0]
            assert n > 50
            assert grp["keypoints"].__array__().shape == (n, 2) and grp["keypoints"].__array__().dtype == np.float16
            assert grp["scores"].__array__().shape == (n,) and grp["scores"].__array__().dtype == np.float16
            assert grp["descriptors"].__array__().shape == (128, n) and grp["descriptors"].__array__().dtype == np.float16
            assert np.array_equal(grp["keypoints"].__array__(), kp), f
            assert np.array_equal(grp["scores"].__array__(), pred["scores"][0].cpu().numpy().astype(np.float16))
            assert np.array_equal(grp["descriptors"].__array__(), pred["descriptors"][0].cpu().numpy().astype(np.float16))
            assert tuple(grp["image_size"].__array__()) == tuple(raw.shape[:2][::-1])
