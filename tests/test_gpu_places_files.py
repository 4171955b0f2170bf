"""CosPlace / EigenPlaces through the file-based drivers.

Files on disk -> device-side RGB preprocessing (the `cosplace` / `eigenplaces` confs: resize_max 1024) -> `global-feats-cosplace.h5` /
`global-feats-eigenplaces.h5` with the keys and dtypes the reference writes (`global_descriptor` float16, `image_size`; no key-points, no
`uncertainty`) -> pairs_from_retrieval, unchanged, on descriptors that are 2048 and 256 wide -> the pairs file, equal to what one image
per plugin call and a float64 numpy ranking give; a disagreement must be a near-tie (the two float64 scores within 2e-6, the audit of
tests/test_gpu_netvlad_files.py).  The tree holds no image files, so the PNGs are synthesised into the test's directory as the NetVLAD
file test does.  `cosplace` runs its default ResNet-50 / 2048, `eigenplaces` ResNet-18 / 256 to stay small."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_disk_files import _host_rgb, _rgb_u8
from test_places_cpu import state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.mark.parametrize("name,model_conf,dim", [("cosplace", {}, 2048), ("eigenplaces", {"backbone": "ResNet18", "fc_output_dim": 256}, 256)],
                         ids=["cosplace-resnet50-2048", "eigenplaces-resnet18-256"])  # fmt: skip
def test_extract_and_pair_from_files(tmp_path, name, model_conf, dim):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors, pairs_from_retrieval as pr
    from imcui_hip.hloc.utils.base_model import dynamic_load
    from imcui_hip.hloc.utils.h5lite import open_h5

    conf = ef.confs[name]
    root = tmp_path / "images"
    (root / "db").mkdir(parents=True)
    (root / "query").mkdir()
    images = {"db/a.png": _rgb_u8(96, 128, 600), "db/b.png": _rgb_u8(96, 128, 601), "db/c.png": _rgb_u8(80, 112, 602), "query/d.png": _rgb_u8(96, 128, 603),
              "query/e.png": _rgb_u8(80, 112, 604)}  # fmt: skip  (two sizes: a batch of three, a batch of two)
    for fname, arr in images.items():
        Image.fromarray(np.ascontiguousarray(arr)).save(root / fname)
    backbone = 18 if model_conf else 50
    model = dynamic_load(extractors, conf["model"]["name"])({**conf["model"], **model_conf, "state_dict": state(backbone, dim)}).eval().to(DEV)
    feature_path = ef.main(conf, root, tmp_path / "out", model=model, batch_size=4)
    assert feature_path == tmp_path / "out" / f"global-feats-{name}.h5"
    assert sorted(ef.list_h5_names(feature_path)) == sorted(images)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    desc = {}
    with open_h5(feature_path, "r") as fd:
        for fname in images:
            raw = ef.read_image_u8(root / fname)
            with torch.no_grad():
                pred = model({"image": _host_rgb(raw, pconf).to(DEV)})
            grp = fd[fname]
            assert set(grp.keys()) == {"global_descriptor", "image_size"}
            got = grp["global_descriptor"].__array__()
            assert got.shape == (dim,) and got.dtype == np.float16
            assert np.array_equal(got, pred["global_descriptor"][0].cpu().numpy().astype(np.float16)), fname  # (batch-independent bits)
            assert tuple(grp["image_size"].__array__()) == tuple(raw.shape[:2][::-1])
            assert "uncertainty" not in grp["global_descriptor"].attrs
            desc[fname] = got.astype(np.float64)
    out = tmp_path / "pairs.txt"
    pairs = pr.main(feature_path, out, 2, query_prefix="query", db_prefix="db")
    text = out.read_text()
    assert text == "\n".join(f"{q} {d}" for q, d in pairs) and not text.endswith("\n")
    db = [n for n in images if n.startswith("db")]
    near_ties = 0
    for q in ("query/d.png", "query/e.png"):
        sims = {d: float(desc[q] @ desc[d]) for d in db}
        want = [d for d in sorted(db, key=lambda d: (-sims[d], db.index(d)))[:2] if sims[d] >= 0]  # (main passes min_score = 0, as the reference)
        got = [d for qq, d in pairs if qq == q]
        assert len(got) == len(want) and len(set(got)) == len(got)
        for g, w in zip(got, want):
            if g != w:  # only a near-tie may differ from the float64 ranking
                assert abs(sims[g] - sims[w]) < 2e-6, (q, g, w, sims)
                near_ties += 1
    assert near_ties <= 1, near_ties
    # every image against every image: the self-pair is masked
    allp = pr.main(feature_path, tmp_path / "all.txt", 10)
    assert len(allp) <= 5 * 4 and all(q != d for q, d in allp) and {q for q, _ in allp} == set(images)
