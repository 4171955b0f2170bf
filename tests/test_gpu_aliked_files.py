"""ALIKED through the file-based batch drivers (the `aliked+lightglue` zoo entry): RGB files -> device-side RGB preprocessing
(`grayscale: False`, `resize_max: 1024`) -> ALIKED in batches -> feature .h5 -> 128-d LightGlue in batches -> match .h5, compared with
the reference flow: one image / one pair per plugin call on host-preprocessed tensors (imcui/hloc/extract_features.py:80-99, 199-243;
match_features.py:172-185)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import aliked_state_dict, lightglue_state_dict
from test_gpu_disk_files import _host_rgb, _rgb_u8

pytestmark = pytest.mark.gpu


def test_aliked_extract_then_match_from_files_equals_the_per_call_plugins(tmp_path):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import match_features as mf
    from imcui_hip.hloc.extractors.aliked import ALIKED
    from imcui_hip.hloc.matchers.lightglue import LightGlue
    from imcui_hip.hloc.utils.h5lite import open_h5

    root = tmp_path / "images"
    root.mkdir()
    # two 480 x 640 files (one batch), a size that needs the padder, and two larger than resize_max (area resize, then the padder)
    specs = [("a.png", 480, 640), ("b.jpg", 480, 640), ("c.png", 472, 632), ("d.jpg", 1000, 1700), ("e.png", 1210, 1800)]
    files = []
    for i, (name, h, w) in enumerate(specs):
        Image.fromarray(_rgb_u8(h, w, 200 + i)).save(root / name, **({"quality": 92} if name.endswith(".jpg") else {}))
        files.append(name)
    conf = {"output": "feats-aliked-n16", "model": {"name": "aliked", "model_name": "aliked-n16", "max_num_keypoints": -1,
                                                     "detection_threshold": 0.2, "nms_radius": 2},
            "preprocessing": {"grayscale": False, "resize_max": 1024}}  # the reference's `aliked-n16` conf (configs/extractors.py:247-261)  # fmt: skip
    aliked = ALIKED({**conf["model"], "state_dict": aliked_state_dict(0)}).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=aliked, batch_size=4)
    assert sorted(ef.list_h5_names(feature_path)) == sorted(files)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    with open_h5(feature_path, "r") as fd:
        for f in files:
            raw = ef.read_image_u8(root / f)
            assert raw.ndim == 3 and raw.shape[2] == 3
            image = _host_rgb(raw, pconf).cuda()
            dev = ef.preprocess_on_device(raw, pconf, torch.device("cuda:0"), rgb=True)
            assert torch.equal(dev, image), f  # the device preprocessing is the host's, bit for bit
            assert max(image.shape[-2:]) <= 1024
            with torch.no_grad():
                pred = aliked({"image": image})
            h, w = image.shape[-2:]
            scales = (np.array(raw.shape[:2][::-1]) / np.array([w, h])).astype(np.float32)
            kp = ((pred["keypoints"][0].cpu().numpy() + 0.5) * scales[None] - 0.5).astype(np.float16)
            grp = fd[f]
            assert grp["descriptors"].__array__().shape == (128, kp.shape[0]) and kp.shape[0] > 100
            assert np.array_equal(grp["keypoints"].__array__(), kp), f
            assert np.array_equal(grp["scores"].__array__(), pred["scores"][0].cpu().numpy().astype(np.float16))
            assert np.array_equal(grp["descriptors"].__array__(), pred["descriptors"][0].cpu().numpy().astype(np.float16))
            assert tuple(grp["image_size"].__array__()) == tuple(raw.shape[:2][::-1])
            assert float(grp["keypoints"].attrs["uncertainty"]) == pytest.approx(1.0 * scales.mean())
    # ---- matching from the files: `aliked-lightglue` (128-d descriptors through input_proj)
    pairs = [("a.png", "b.jpg"), ("c.png", "d.jpg"), ("a.png", "e.png"), ("d.jpg", "e.png")]
    pairs_path = tmp_path / "pairs.txt"
    pairs_path.write_text("".join(f"{q} {r}\n" for q, r in pairs))
    store = mf.H5FeatureStore(feature_path)
    model = LightGlue({"depth_confidence": 0.95, "width_confidence": 0.99, "match_threshold": 0.1, "features": "aliked",
                       "state_dict": lightglue_state_dict(0, input_dim=128)}).eval().to("cuda:0")  # fmt: skip
    match_path = mf.match_from_paths(model, pairs_path, tmp_path / "out" / "matches-aliked-lightglue.h5", feature_path, feature_path, batch_size=3)
    with open_h5(match_path, "r") as fd:
        for q, r in pairs:
            f0, f1 = store.get(q), store.get(r)
            data = {"image0": torch.empty((1, 3) + tuple(int(v) for v in f0["image_size"])[::-1]),
                    "image1": torch.empty((1, 3) + tuple(int(v) for v in f1["image_size"])[::-1])}  # fmt: skip
            for side, f in (("0", f0), ("1", f1)):
                data["keypoints" + side] = torch.from_numpy(f["keypoints"].astype(np.float32))[None].cuda()
                data["scores" + side] = torch.from_numpy(f["scores"].astype(np.float32))[None].cuda()
                data["descriptors" + side] = torch.from_numpy(f["descriptors"].astype(np.float32))[None].cuda()
            with torch.no_grad():
                pred = model(data)
            grp = fd[mf.names_to_pair(q, r)]
            m = grp["matches0"].__array__()
            assert m.dtype == np.int16 and np.array_equal(m, pred["matches0"][0].cpu().numpy().astype(np.int16)), (q, r)
            assert np.array_equal(grp["matching_scores0"].__array__(), pred["matching_scores0"][0].cpu().numpy().astype(np.float16)), (q, r)
            assert m.shape == (f0["keypoints"].shape[0],)
