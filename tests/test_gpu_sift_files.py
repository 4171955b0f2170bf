"""SIFT through the file-based batch drivers (the `sift` extractor conf and the `sift-lightglue` zoo entry): image files -> device-side
gray preprocessing (`grayscale: True`, `force_resize`, `resize_max: 1600`) -> SIFT in batches -> feature .h5 with `scales` / `oris`
(imcui/hloc/extract_features.py:216-217) -> LightGlue with the (x, y, scale, orientation) encoding in batches (match_features.py:227-234)
-> match .h5, compared with one plugin call per image / pair."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import lightglue_state_dict
from test_gpu_disk_files import _rgb_u8

pytestmark = pytest.mark.gpu


def test_sift_extract_then_match_from_files_equals_the_per_call_plugins(tmp_path):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import match_features as mf
    from imcui_hip.hloc.extractors.sift import SIFT
    from imcui_hip.hloc.matchers.lightglue import LightGlue
    from imcui_hip.hloc.utils.h5lite import open_h5

    root = tmp_path / "images"
    root.mkdir()
    # two files of one size (one batch), a gray PNG, and one larger than resize_max (area resize); the others grow (INTER_LINEAR)
    specs = [("a.png", 240, 320, "RGB"), ("b.jpg", 240, 320, "RGB"), ("c.png", 225, 300, "L"), ("d.jpg", 1210, 1800, "RGB")]
    files = []
    for i, (name, h, w, mode) in enumerate(specs):
        arr = _rgb_u8(h, w, 300 + i)
        Image.fromarray(arr if mode == "RGB" else arr[..., 1]).save(root / name, **({"quality": 92} if name.endswith(".jpg") else {}))
        files.append(name)
    conf = {"output": "feats-sift-n5000-r1600", "model": {"name": "sift", "rootsift": True, "max_keypoints": 5000},
            "preprocessing": {"grayscale": True, "force_resize": True, "resize_max": 1600, "width": 640, "height": 480, "dfactor": 8}}  # configs/extractors.py:128-143  # fmt: skip
    sift = SIFT(dict(conf["model"])).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=sift, batch_size=2)
    assert sorted(ef.list_h5_names(feature_path)) == sorted(files)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    dev = torch.device("cuda:0")
    with open_h5(feature_path, "r") as fd:
        for f in files:
            raw = ef.read_images_device([root / f], True, dev)[0]
            image = ef.preprocess_on_device(raw, pconf, dev)
            assert image.shape[1] == 1 and max(image.shape[-2:]) == 1600
            with torch.no_grad():
                pred = sift({"image": image})
            h, w = image.shape[-2:]
            original = np.array(tuple(raw.shape[:2][::-1]))
            scales = (original / np.array([w, h])).astype(np.float32)
            kp = ((pred["keypoints"][0].cpu().numpy() + 0.5) * scales[None] - 0.5).astype(np.float16)
            grp = fd[f]
            n = kp.shape[0]
            assert 100 < n <= 5000 and grp["descriptors"].__array__().shape == (128, n)
            assert np.array_equal(grp["keypoints"].__array__(), kp), f
            assert np.array_equal(grp["scores"].__array__(), pred["scores"][0].cpu().numpy().astype(np.float16))
            assert np.array_equal(grp["descriptors"].__array__(), pred["descriptors"][0].cpu().numpy().astype(np.float16))
            assert np.array_equal(grp["scales"].__array__(), (pred["scales"][0].cpu().numpy() * scales.mean()).astype(np.float16))
            assert np.array_equal(grp["oris"].__array__(), pred["oris"][0].cpu().numpy().astype(np.float16))
            assert tuple(grp["image_size"].__array__()) == tuple(original)
            assert float(grp["keypoints"].attrs["uncertainty"]) == pytest.approx(1.0 * scales.mean())
    # ---- matching from the files: `sift-lightglue` (128-d descriptors through input_proj, 4-column positional encoding)
    pairs = [("a.png", "b.jpg"), ("c.png", "d.jpg"), ("a.png", "d.jpg")]
    pairs_path = tmp_path / "pairs.txt"
    pairs_path.write_text("".join(f"{q} {r}\n" for q, r in pairs))
    store = mf.H5FeatureStore(feature_path)
    model = LightGlue({"depth_confidence": 0.95, "width_confidence": 0.99, "match_threshold": 0.1, "features": "sift", "add_scale_ori": True,
                       "state_dict": lightglue_state_dict(0, input_dim=128, add_scale_ori=True)}).eval().to("cuda:0")  # fmt: skip
    assert model.add_scale_ori
    match_path = mf.match_from_paths(model, pairs_path, tmp_path / "out" / "matches-sift-lightglue.h5", feature_path, feature_path, batch_size=2)
    with open_h5(match_path, "r") as fd:
        for q, r in pairs:
            f0, f1 = store.get(q), store.get(r)
            data = {"image0": torch.empty((1, 1) + tuple(int(v) for v in f0["image_size"])[::-1]),
                    "image1": torch.empty((1, 1) + tuple(int(v) for v in f1["image_size"])[::-1])}  # fmt: skip
            for side, f in (("0", f0), ("1", f1)):
                for k in ("keypoints", "scores", "descriptors", "scales", "oris"):
                    data[k + side] = torch.from_numpy(f[k].astype(np.float32))[None].cuda()
            with torch.no_grad():
                pred = model(data)
            grp = fd[mf.names_to_pair(q, r)]
            m = grp["matches0"].__array__()
            assert m.dtype == np.int16 and np.array_equal(m, pred["matches0"][0].cpu().numpy().astype(np.int16)), (q, r)
            assert np.array_equal(grp["matching_scores0"].__array__(), pred["matching_scores0"][0].cpu().numpy().astype(np.float16)), (q, r)
            assert m.shape == (f0["keypoints"].shape[0],)
