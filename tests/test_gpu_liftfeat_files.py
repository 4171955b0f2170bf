"""LiftFeat against the golden file written by the reference's own wrapper (tests/golden/make_liftfeat_golden.py: two images at
max_keypoints 5000, 7, 0 and -1), through the plugin's `_forward`; then the file-based batch extractor (the `liftfeat(sparse)` zoo entry:
`feature: liftfeat` + `matcher: NN-mutual`): RGB files -> device-side RGB preprocessing (`grayscale: False`) -> LiftFeat in batches ->
feature .h5, compared with one image per plugin call; then the mutual-NN matcher plugin on two crops of one canvas, in both directions
(imcui/hloc/configs/extractors.py:198-208 conf `liftfeat`, matchers/nearest_neighbor.py).

The golden file holds the float32 CPU restatement behind the reference's wrapper: counts and order must be equal, positions equal (the
restatement's own float32-against-float64 position difference is zero at these seeds, tests/test_gpu_liftfeat.py), scores and descriptors
within 1e-4 of the largest magnitude (the floor of the project's end-to-end bar).

Measured on one MI355X: 59 / 84 key-points at the default, 7, 59 / 84 and 58 / 83 at max_keypoints 7, 0 and -1, equal positions and order,
scores within 8.2e-07, descriptors within 7.0e-07; the file driver: 1287 / 1292 key-points, 825 mutual matches in both directions."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import liftfeat_synth_state
from test_gpu_disk_files import _host_rgb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "liftfeat_golden.npz")
SETTINGS = (("default", None), ("top7", 7), ("zero", 0), ("minus1", -1))


def _rel(a, ref):
    return float(np.abs(a.astype(np.float64) - ref.astype(np.float64)).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("tag", ["40x56", "50x70"])
def test_golden_through_the_plugin(tag):
    from imcui_hip.hloc.extractors.liftfeat import Liftfeat

    g = np.load(GOLDEN)
    img = (torch.from_numpy(g[f"image_u8_{tag}"]).float() / 255.0).cuda()
    full = g[f"descriptors_default_{tag}"]
    for name, k in SETTINGS:
        m = Liftfeat({"state_dict": liftfeat_synth_state(int(g["seed"])), **({} if k is None else {"max_keypoints": k})}).eval().to("cuda:0")
        with torch.no_grad():
            pred = m({"image": img})
        kp, sc, de = pred["keypoints"][0].cpu().numpy(), pred["scores"][0].cpu().numpy(), pred["descriptors"][0].cpu().numpy().T
        want_kp, want_sc = g[f"keypoints_{name}_{tag}"], g[f"scores_{name}_{tag}"]
        want_de = full if name == "default" else full[g[f"desc_rows_{name}_{tag}"]]
        assert tuple(pred["keypoints"].shape) == (1, len(want_sc), 2) and tuple(pred["descriptors"].shape) == (1, 64, len(want_sc))
        assert np.array_equal(kp, want_kp), f"{tag} {name}: the same key-points in the same order"
        e_sc, e_de = _rel(sc, want_sc), _rel(de, want_de)
        print(f"golden {tag} {name}: {len(sc)} key-points, scores {e_sc:.2e}, descriptors {e_de:.2e} (bar 1e-4)")
        assert e_sc <= 1e-4 and e_de <= 1e-4


def _noise_u8(h, w, seed):
    return torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).numpy()


def test_liftfeat_extract_then_mutual_nn_from_files(tmp_path):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import match_features as mf
    from imcui_hip.hloc.extractors.liftfeat import Liftfeat
    from imcui_hip.hloc.matchers.nearest_neighbor import NearestNeighbor
    from imcui_hip.hloc.utils.h5lite import open_h5

    root = tmp_path / "images"
    root.mkdir()
    big = _noise_u8(240, 352, 511)  # a.png / b.png: two crops of one canvas, 32 pixels apart
    images = {"a.png": big[:, :320], "b.png": big[:, 32:]}
    for name, arr in images.items():
        Image.fromarray(np.ascontiguousarray(arr)).save(root / name)
    files = list(images)
    conf = ef.confs["liftfeat"]
    model = Liftfeat({**conf["model"], "state_dict": liftfeat_synth_state(0)}).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=model, batch_size=2)
    assert sorted(ef.list_h5_names(feature_path)) == sorted(files)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    with open_h5(feature_path, "r") as fd:
        for f in files:
            raw = ef.read_image_u8(root / f)
            image = _host_rgb(raw, pconf).cuda()
            assert tuple(image.shape) == (1, 3, 240, 320)
            with torch.no_grad():
                pred = model({"image": image})
            h, w = image.shape[-2:]
            scales = (np.array(raw.shape[:2][::-1]) / np.array([w, h])).astype(np.float32)
            kp = ((pred["keypoints"][0].cpu().numpy() + 0.5) * scales[None] - 0.5).astype(np.float16)
            grp = fd[f]
            assert grp["descriptors"].__array__().shape == (64, kp.shape[0]) and kp.shape[0] > 100
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
