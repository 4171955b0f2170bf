"""ALIKE through the file-based batch extractor (the `alike` zoo entry: `feature: alike` + `matcher: NN-mutual`): RGB files ->
device-side RGB preprocessing (`grayscale: False`, resize_max 1600) -> ALIKE in batches -> feature .h5, compared with one image per
plugin call; then the mutual-NN matcher plugin on the features file against backend.mutual_nn on the same descriptors, and a
shifted pair whose shift the matches have to recover (imcui/hloc/configs/extractors.py:272-287 conf `alike`, matchers/nearest_neighbor.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import alike_state_dict
from test_gpu_disk_files import _host_rgb, _rgb_u8

pytestmark = pytest.mark.gpu


def test_alike_extract_then_mutual_nn_from_files(tmp_path):
    from PIL import Image

    from imcui_hip import backend
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import match_features as mf
    from imcui_hip.hloc.extractors.alike import Alike
    from imcui_hip.hloc.matchers.nearest_neighbor import NearestNeighbor
    from imcui_hip.hloc.utils.h5lite import open_h5

    root = tmp_path / "images"
    root.mkdir()
    # a.png / b.png: two windows of one 160 x 232 image, 8 pixels apart; c.jpg / d.png: 150 x 200
    # (zero-padded to 160 x 224 inside the extractor, cropped again)
    big = _rgb_u8(160, 232, 300)
    images = {"a.png": big[:, :224], "b.png": big[:, 8:], "c.jpg": _rgb_u8(150, 200, 301), "d.png": _rgb_u8(150, 200, 302)}
    for name, arr in images.items():
        Image.fromarray(np.ascontiguousarray(arr)).save(root / name, **({"quality": 92} if name.endswith(".jpg") else {}))
    files = list(images)
    conf = {"output": "feats-alike-n5000-r1600",
            "model": {"name": "alike", "max_keypoints": 5000, "use_relu": True, "multiscale": False, "detection_threshold": 0.5, "top_k": -1, "sub_pixel": False},
            "preprocessing": {"grayscale": False, "resize_max": 1600}}  # the reference's `alike` conf  # fmt: skip
    alike = Alike({**conf["model"], "state_dict": alike_state_dict("alike-t", 0)}).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=alike, batch_size=4)
    assert sorted(ef.list_h5_names(feature_path)) == sorted(files)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    with open_h5(feature_path, "r") as fd:
        for f in files:
            raw = ef.read_image_u8(root / f)
            image = _host_rgb(raw, pconf).cuda()
            with torch.no_grad():
                pred = alike({"image": image})
            h, w = image.shape[-2:]
            scales = (np.array(raw.shape[:2][::-1]) / np.array([w, h])).astype(np.float32)
            kp = ((pred["keypoints"][0].cpu().numpy() + 0.5) * scales[None] - 0.5).astype(np.float16)
            grp = fd[f]
            assert grp["descriptors"].__array__().shape == (64, kp.shape[0]) and kp.shape[0] > 50
            assert np.array_equal(grp["keypoints"].__array__(), kp), f
            assert np.array_equal(grp["scores"].__array__(), pred["scores"][0].cpu().numpy().astype(np.float16))
            assert np.array_equal(grp["descriptors"].__array__(), pred["descriptors"][0].cpu().numpy().astype(np.float16))
            assert tuple(grp["image_size"].__array__()) == tuple(raw.shape[:2][::-1])
    # ---- NN-mutual on the features file, one pair per plugin call (the reference's flow), against backend.mutual_nn
    store = mf.H5FeatureStore(feature_path)
    nn = NearestNeighbor({"do_mutual_check": True}).eval()
    for q, r in (("a.png", "b.png"), ("c.jpg", "d.png"), ("a.png", "d.png")):
        f0, f1 = store.get(q), store.get(r)
        d0 = torch.from_numpy(f0["descriptors"].astype(np.float32))[None].cuda()  # [1, 64, N]
        d1 = torch.from_numpy(f1["descriptors"].astype(np.float32))[None].cuda()
        with torch.no_grad():
            pred = nn({"descriptors0": d0, "descriptors1": d1})
        m0, s0 = backend.mutual_nn(d0.transpose(1, 2).contiguous(), d1.transpose(1, 2).contiguous())
        assert torch.equal(pred["matches0"], m0.long()) and torch.allclose(pred["matching_scores0"], s0, atol=1e-6), (q, r)
        m = pred["matches0"][0].cpu()
        assert m.shape == (f0["keypoints"].shape[0],) and int((m >= 0).sum()) > 10
        if (q, r) == ("a.png", "b.png"):  # a point at x in b.png is the point at x + 8 in a.png
            k0 = torch.from_numpy(f0["keypoints"].astype(np.float32))[m >= 0]
            k1 = torch.from_numpy(f1["keypoints"].astype(np.float32))[m[m >= 0]]
            hit = ((k0 - k1 - torch.tensor([8.0, 0.0])).abs().max(dim=1).values <= 1.0).sum().item()
            print(f"a.png / b.png: {len(k0)} mutual matches, {hit} recover the 8 px shift within 1 px")
            assert hit >= 0.5 * len(k0), (hit, len(k0))
