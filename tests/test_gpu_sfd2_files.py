"""SFD2 through the file-based batch extractor (the `sfd2+mnn` zoo entry: `feature: sfd2` + `matcher: NN-mutual`): RGB files ->
device-side RGB preprocessing (`grayscale: False`, `force_resize`) -> SFD2 in batches -> feature .h5, compared with one image per plugin
call; then the mutual-NN matcher plugin on two crops of one canvas, in both directions (imcui/hloc/configs/extractors.py:349-365 conf
`sfd2`, matchers/nearest_neighbor.py).

`force_resize` reaches the device-side resize the way the reference's file driver applies it (`ImageDataset.__getitem__` :83-88): the longer
side goes to `resize_max`; `width` / `height` (640 x 480) are read by the UI's `extract` only, which this driver does not restate.  The
conf's own `resize_max` is 1600 (tests/test_sfd2_cpu.py checks the rule on it); here it is set to 640, so that the 1280 x 960 files come
out as the 640 x 480 maps the conf names, through the same forced INTER_AREA resize, at a sixth of the pixels."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import sfd2_synth_state
from test_gpu_disk_files import _host_rgb, _rgb_u8

pytestmark = pytest.mark.gpu


def test_sfd2_extract_then_mutual_nn_from_files(tmp_path):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import match_features as mf
    from imcui_hip.hloc.extractors.sfd2 import SFD2
    from imcui_hip.hloc.matchers.nearest_neighbor import NearestNeighbor
    from imcui_hip.hloc.utils.h5lite import open_h5

    root = tmp_path / "images"
    root.mkdir()
    big = _rgb_u8(960, 1296, 411)  # a.png / b.png: two crops of one canvas, 16 pixels apart
    images = {"a.png": big[:, :1280], "b.png": big[:, 16:]}
    for name, arr in images.items():
        Image.fromarray(np.ascontiguousarray(arr)).save(root / name)
    files = list(images)
    conf = ef.confs["sfd2"]
    assert conf["preprocessing"]["force_resize"] and conf["model"]["max_keypoints"] == 4096
    conf = {**conf, "preprocessing": {**conf["preprocessing"], "resize_max": 640}}
    model = SFD2({**conf["model"], "state_dict": sfd2_synth_state(0)}).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=model, batch_size=2)
    assert sorted(ef.list_h5_names(feature_path)) == sorted(files)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    with open_h5(feature_path, "r") as fd:
        for f in files:
            raw = ef.read_image_u8(root / f)
            image = _host_rgb(raw, pconf).cuda()
            assert tuple(image.shape) == (1, 3, 480, 640), "force_resize gives 640 x 480 maps"
            with torch.no_grad():
                pred = model({"image": image})
            h, w = image.shape[-2:]
            scales = (np.array(raw.shape[:2][::-1]) / np.array([w, h])).astype(np.float32)
            kp = ((pred["keypoints"][0].cpu().numpy() + 0.5) * scales[None] - 0.5).astype(np.float16)
            grp = fd[f]
            assert grp["descriptors"].__array__().shape == (128, kp.shape[0]) and kp.shape[0] > 100
            assert np.array_equal(grp["keypoints"].__array__(), kp), f
            assert np.array_equal(grp["scores"].__array__(), pred["scores"][0].cpu().numpy().astype(np.float16))
            assert np.array_equal(grp["descriptors"].__array__(), pred["descriptors"][0].cpu().numpy().astype(np.float16))
            assert tuple(grp["image_size"].__array__()) == tuple(raw.shape[:2][::-1])
    # ---- NN-mutual on the features file: a -> b and b -> a name the same pairs
    store = mf.H5FeatureStore(feature_path)
    nn = NearestNeighbor({"do_mutual_check": True}).eval()
    fa, fb = store.get("a.png"), store.get("b.png")
    da = torch.from_numpy(fa["descriptors"].astype(np.float32))[None].cuda()
    db = torch.from_numpy(fb["descriptors"].astype(np.float32))[None].cuda()
    with torch.no_grad():
        mab = nn({"descriptors0": da, "descriptors1": db})["matches0"][0].cpu()
        mba = nn({"descriptors0": db, "descriptors1": da})["matches0"][0].cpu()
    pairs_ab = {(i, int(j)) for i, j in enumerate(mab.tolist()) if j >= 0}
    pairs_ba = {(int(i), j) for j, i in enumerate(mba.tolist()) if i >= 0}
    print(f"a.png / b.png: {len(fa['keypoints'])} / {len(fb['keypoints'])} key-points, {len(pairs_ab)} mutual matches a -> b, {len(pairs_ba)} b -> a")
    assert mab.shape == (fa["keypoints"].shape[0],) and len(pairs_ab) > 5
    assert pairs_ab == pairs_ba
