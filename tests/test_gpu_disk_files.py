"""DISK through the file-based batch drivers (the `disk` zoo entries): RGB files -> device-side RGB preprocessing (INTER_AREA per
channel, `grayscale: False`) -> DISK in batches -> feature .h5 -> 128-d LightGlue in batches -> match .h5, compared
with the reference flow: one image / one pair per plugin call on host-preprocessed tensors (imcui/hloc/extract_features.py:80-99,
199-243; match_features.py:172-185)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import disk_state_dict, lightglue_state_dict
from oracle.preprocess import area_resize_f32

pytestmark = pytest.mark.gpu


def _rgb_u8(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros(3, h, w)
    for s, a in ((6, 0.5), (24, 0.3), (96, 0.2)):
        low = torch.rand(1, 3, max(2, h // s), max(2, w // s), generator=g)
        img += a * torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
    return (img.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def _host_rgb(raw: np.ndarray, pconf) -> torch.Tensor:
    """The reference's host preprocessing of an RGB image: astype(float32) -> cv2 INTER_AREA per channel -> CxHxW -> / 255."""
    from imcui_hip.hloc import extract_features as ef

    H, W = raw.shape[:2]
    size = ef.target_size((W, H), pconf)
    chans = [raw[..., c].astype(np.float32) if size is None else area_resize_f32(raw[..., c].astype(np.float32), size) for c in range(3)]
    return torch.from_numpy(np.stack(chans)[None] / np.float32(255.0))


@pytest.mark.parametrize("src_hw,dst_wh", [((750, 1000), (640, 480)), ((673, 1013), (640, 425)), ((960, 1280), (640, 480)), ((48, 64), (64, 48))])
def test_device_rgb_preprocessing_equals_the_host_path(src_hw, dst_wh):
    """RGB mode of the area resize vs oracle/preprocess.py per channel: bit-exact (fractional, integer and unit factors)."""
    from imcui_hip import backend

    g = np.random.default_rng(src_hw[0])
    img = g.integers(0, 256, size=(2, *src_hw, 3), dtype=np.uint8)
    out = backend.preprocess_area_rgb(torch.from_numpy(img).cuda(), dst_wh).cpu().numpy()
    assert out.shape == (2, 3, dst_wh[1], dst_wh[0])
    for b in range(2):
        for c in range(3):
            x = img[b, ..., c].astype(np.float32)
            ref = (x if dst_wh == src_hw[::-1] else area_resize_f32(x, dst_wh)) / np.float32(255.0)
            assert np.array_equal(out[b, c], ref), (b, c, np.abs(out[b, c] - ref).max())


def test_disk_extract_then_match_from_files_equals_the_per_call_plugins(tmp_path):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import match_features as mf
    from imcui_hip.hloc.extractors.disk import DISK
    from imcui_hip.hloc.matchers.lightglue import LightGlue
    from imcui_hip.hloc.utils.h5lite import open_h5

    root = tmp_path / "images"
    root.mkdir()
    # two 480 x 640 files (one batch), a size that needs the padding, and two larger than resize_max (area resize, then padding)
    specs = [("a.png", 480, 640), ("b.jpg", 480, 640), ("c.png", 472, 632), ("d.jpg", 1000, 1700), ("e.png", 1210, 1800)]
    files = []
    for i, (name, h, w) in enumerate(specs):
        Image.fromarray(_rgb_u8(h, w, 100 + i)).save(root / name, **({"quality": 92} if name.endswith(".jpg") else {}))
        files.append(name)
    conf = {"output": "feats-disk-n5000-r1600", "model": {"name": "disk", "max_keypoints": 5000},
            "preprocessing": {"grayscale": False, "resize_max": 1600}}  # the reference's `disk` conf (configs/extractors.py)  # fmt: skip
    disk = DISK({**conf["model"], "state_dict": disk_state_dict(0)}).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=disk, batch_size=4)
    assert sorted(ef.list_h5_names(feature_path)) == sorted(files)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    with open_h5(feature_path, "r") as fd:
        for f in files:
            raw = ef.read_image_u8(root / f)
            assert raw.ndim == 3 and raw.shape[2] == 3
            image = _host_rgb(raw, pconf).cuda()
            dev = ef.preprocess_on_device(raw, pconf, torch.device("cuda:0"), rgb=True)
            assert torch.equal(dev, image), f  # the device preprocessing is the host's, bit for bit
            with torch.no_grad():
                pred = disk({"image": image})
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
    # ---- matching from the files: a 128-d LightGlue (`disk+lightglue`)
    pairs = [("a.png", "b.jpg"), ("c.png", "d.jpg"), ("a.png", "e.png"), ("d.jpg", "e.png")]
    pairs_path = tmp_path / "pairs.txt"
    pairs_path.write_text("".join(f"{q} {r}\n" for q, r in pairs))
    store = mf.H5FeatureStore(feature_path)
    # (the batch match driver takes matchers with a batched entry; NN-mutual of the `disk` entry is matched per pair by its plugin)
    matchers = {
        "disk-lightglue": LightGlue({"depth_confidence": 0.95, "width_confidence": 0.99, "match_threshold": 0.1, "features": "disk",
                                     "state_dict": lightglue_state_dict(0, input_dim=128)}).eval().to("cuda:0"),
    }  # fmt: skip
    for mname, model in matchers.items():
        match_path = mf.match_from_paths(model, pairs_path, tmp_path / "out" / f"matches-{mname}.h5", feature_path, feature_path, batch_size=3)
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
                assert m.dtype == np.int16 and np.array_equal(m, pred["matches0"][0].cpu().numpy().astype(np.int16)), (mname, q, r)
                assert np.array_equal(grp["matching_scores0"].__array__(), pred["matching_scores0"][0].cpu().numpy().astype(np.float16)), (mname, q, r)
                assert m.shape == (f0["keypoints"].shape[0],)
