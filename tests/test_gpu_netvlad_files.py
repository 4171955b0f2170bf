"""NetVLAD through the file-based drivers, and the retrieval top-k on the device.

Files on disk -> device-side RGB preprocessing (the `netvlad` conf: resize_max 1024) -> `global-feats-netvlad.h5` with the keys and dtypes
the reference writes (`global_descriptor` float16, `image_size`; no key-points, no `uncertainty`) -> pairs_from_retrieval -> the pairs
file, equal to what one image per plugin call and a float64 ranking give.

imcui_hip_retrieval_topk against a float64 numpy evaluation: Q = 1, 5, 130 queries x N = 1, 7, 300 database rows, `num_select` above N,
rows that are entirely invalid, duplicated database rows (which resolve to the lower index); any other disagreement must be a near-tie
(the two scores within 2e-6 in float64), as test_nn_argmax_vs_float64 audits."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_disk_files import _host_rgb, _rgb_u8
from test_netvlad_cpu import state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def test_extract_and_pair_from_files(tmp_path, golden_dir):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors, pairs_from_retrieval as pr
    from imcui_hip.hloc.utils.base_model import dynamic_load
    from imcui_hip.hloc.utils.h5lite import open_h5

    with open(os.path.join(golden_dir, "netvlad_conf.json")) as f:
        conf = json.load(f)["extractor_conf"]
    assert conf == ef.confs["netvlad"]
    root = tmp_path / "images"
    (root / "db").mkdir(parents=True)
    (root / "query").mkdir()
    images = {"db/a.png": _rgb_u8(96, 128, 500), "db/b.png": _rgb_u8(96, 128, 501), "db/c.png": _rgb_u8(80, 112, 502), "query/d.png": _rgb_u8(96, 128, 503),
              "query/e.png": _rgb_u8(80, 112, 504)}  # fmt: skip  (two sizes: a batch of three, a batch of two)
    for fname, arr in images.items():
        Image.fromarray(np.ascontiguousarray(arr)).save(root / fname)
    model = dynamic_load(extractors, conf["model"]["name"])({**conf["model"], "state_dict": state(False), "whiten": False}).eval().to(DEV)
    feature_path = ef.main(conf, root, tmp_path / "out", model=model, batch_size=4)
    assert feature_path == tmp_path / "out" / "global-feats-netvlad.h5"
    assert sorted(ef.list_h5_names(feature_path)) == sorted(images)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    desc = {}
    with open_h5(feature_path, "r") as fd:
        for name in images:
            raw = ef.read_image_u8(root / name)
            with torch.no_grad():
                pred = model({"image": _host_rgb(raw, pconf).to(DEV)})
            grp = fd[name]
            assert set(grp.keys()) == {"global_descriptor", "image_size"}
            got = grp["global_descriptor"].__array__()
            assert got.shape == (32768,) and got.dtype == np.float16
            assert np.array_equal(got, pred["global_descriptor"][0].cpu().numpy().astype(np.float16)), name  # (batch-independent bits)
            assert tuple(grp["image_size"].__array__()) == tuple(raw.shape[:2][::-1])
            assert "uncertainty" not in grp["global_descriptor"].attrs
            desc[name] = got.astype(np.float64)
    out = tmp_path / "pairs.txt"
    pairs = pr.main(feature_path, out, 2, query_prefix="query", db_prefix="db")
    text = out.read_text()
    assert text == "\n".join(f"{q} {d}" for q, d in pairs) and not text.endswith("\n")
    db = [n for n in images if n.startswith("db")]
    for q in ("query/d.png", "query/e.png"):
        sims = sorted(((float(desc[q] @ desc[d]), d) for d in db), key=lambda t: -t[0])
        assert [d for qq, d in pairs if qq == q] == [d for s, d in sims[:2] if s >= 0]
    # every image against every image: the self-pair is masked
    allp = pr.main(feature_path, tmp_path / "all.txt", 10)
    assert len(allp) <= 5 * 4 and all(q != d for q, d in allp) and {q for q, _ in allp} == set(images)


@pytest.mark.parametrize("N", [1, 7, 300])
@pytest.mark.parametrize("Q", [1, 5, 130])
def test_retrieval_topk_against_float64(Q, N):
    from imcui_hip import backend

    D, num_select = 256, 12  # above N = 1 and 7
    g = torch.Generator().manual_seed(1000 * Q + N)
    db = F.normalize(torch.randn(N, D, generator=g), dim=1)
    if N >= 7:
        db[N - 3 :] = db[:3]  # duplicated rows behind the originals
    q = F.normalize(db[torch.randint(0, N, (Q,), generator=g)] + 0.5 * torch.randn(Q, D, generator=g), dim=1)
    invalid = torch.rand(Q, N, generator=g) < 0.2
    if Q >= 5:
        invalid[1] = True  # a row that is entirely invalid
    idx, val = backend.retrieval_topk(q.to(DEV), db.to(DEV), num_select, invalid, min_score=0)
    torch.cuda.synchronize()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    sim = (q.double() @ db.double().T).numpy()
    if N >= 7:
        sim[:, N - 3 :] = sim[:, :3]  # (a BLAS may sum two equal columns in different orders: a duplicate's float64 score IS its original's)
    masked = np.where(invalid.numpy() | (sim < 0), -np.inf, sim)
    near_ties = 0
    for i in range(Q):
        order = sorted(range(N), key=lambda j: (-masked[i, j], j))  # descending score, equal scores by ascending index
        nfin = int(np.isfinite(masked[i]).sum())
        k = min(num_select, N)
        assert (idx[i, k:] == -1).all() and np.isneginf(val[i, k:]).all()
        assert np.isfinite(val[i, : min(k, nfin)]).all() and np.isneginf(val[i, min(k, nfin) : k]).all(), i
        for r in range(min(k, nfin)):
            j, want = int(idx[i, r]), order[r]
            assert abs(val[i, r] - masked[i, j]) < 1e-5
            if j != want:  # only a near-tie may differ from the float64 ranking
                assert abs(masked[i, j] - masked[i, want]) < 2e-6, (i, r, j, want)
                near_ties += 1
            if r > 0:
                assert val[i, r] < val[i, r - 1] or (val[i, r] == val[i, r - 1] and idx[i, r] > idx[i, r - 1]), "descending, ties by ascending index"
        got = idx[i, : min(k, nfin)].tolist()
        assert len(set(got)) == len(got)
        if N >= 7:  # of a duplicated pair both valid, the lower index ranks first
            for a in range(3):
                b = N - 3 + a
                if a in got and b in got:
                    assert got.index(a) < got.index(b)
    assert near_ties <= max(2, Q * min(num_select, N) // 100), near_ties
    if Q >= 5:
        assert np.isneginf(val[1]).all()
