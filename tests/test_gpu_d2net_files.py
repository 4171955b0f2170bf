"""D2-Net and RoRD through the file-based batch extractor (the `d2net` / `rord` zoo entries: `feature: d2net-ss` / `rord` + `matcher:
NN-mutual`): RGB files -> device-side RGB preprocessing (`grayscale: False`, resize_max 1600) -> the extractor in batches -> feature .h5
with the keys, shapes and dtypes the reference writes, compared with one image per plugin call.  The confs are the reference's
(imcui/hloc/configs/extractors.py:76-111), recorded as data in tests/golden/d2net_confs.json; the weights are synthetic."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import d2net_state_dict
from test_gpu_disk_files import _host_rgb, _rgb_u8

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["d2net-ss", "rord"])
def test_d2net_extract_from_files(name, tmp_path, golden_dir):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load
    from imcui_hip.hloc.utils.h5lite import open_h5

    with open(os.path.join(golden_dir, "d2net_confs.json")) as f:
        conf = json.load(f)["extractor_confs"][name]
    root = tmp_path / "images"
    root.mkdir()
    images = {"a.png": _rgb_u8(96, 128, 400), "b.png": _rgb_u8(96, 128, 401)}  # one size: one batch of two
    for fname, arr in images.items():
        Image.fromarray(np.ascontiguousarray(arr)).save(root / fname)
    files = list(images)
    model = dynamic_load(extractors, conf["model"]["name"])({**conf["model"], "state_dict": d2net_state_dict(0)}).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=model, batch_size=2)
    assert feature_path == tmp_path / "out" / (conf["output"] + ".h5")
    assert sorted(ef.list_h5_names(feature_path)) == sorted(files)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    with open_h5(feature_path, "r") as fd:
        for f in files:
            raw = ef.read_image_u8(root / f)
            image = _host_rgb(raw, pconf).cuda()
            with torch.no_grad():
                pred = model({"image": image})
            h, w = image.shape[-2:]
            scales = (np.array(raw.shape[:2][::-1]) / np.array([w, h])).astype(np.float32)
            kp = ((pred["keypoints"][0].cpu().numpy() + 0.5) * scales[None] - 0.5).astype(np.float16)
            grp = fd[f]
            assert set(grp.keys()) == {"keypoints", "scores", "descriptors", "image_size"}
            n = kp.shape[0]
            assert n > 20
            assert grp["keypoints"].__array__().shape == (n, 2) and grp["keypoints"].__array__().dtype == np.float16
            assert grp["scores"].__array__().shape == (n,) and grp["scores"].__array__().dtype == np.float16
            assert grp["descriptors"].__array__().shape == (512, n) and grp["descriptors"].__array__().dtype == np.float16
            assert np.array_equal(grp["keypoints"].__array__(), kp), f
            assert np.array_equal(grp["scores"].__array__(), pred["scores"][0].cpu().numpy().astype(np.float16))
            assert np.array_equal(grp["descriptors"].__array__(), pred["descriptors"][0].cpu().numpy().astype(np.float16))
            assert tuple(grp["image_size"].__array__()) == tuple(raw.shape[:2][::-1])
