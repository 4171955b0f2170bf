"""NetVLAD without a GPU: the restatement (tests/netvlad_reference.py) against the reference's own output (tests/golden/netvlad_*.npz,
written by make_netvlad_golden.py from the reference checkout), the packed format's digest, the strict packer, the plugin's contract
against values recorded from the reference class (tests/golden/netvlad_conf.json), the .mat round trip through the plugin's loader, and the
host logic of pairs_from_retrieval (name parsing, self-masking, the walk over the ranks, the file format).

The golden maker printed, for both sizes: reference float32 spread (1 against 8 torch threads) 0, reference against the float64
restatement 1.9e-06 / 2.8e-06 (32768-d) and 5.8e-07 / 7.0e-07 (whitened), relative to the largest magnitude; the float32 restatement
reproduced the reference bit for bit.  The end-to-end bar of the project, max(1e-4, 3 x spread), is therefore 1e-4."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import netvlad_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import netvlad_synth_state, netvlad_write_mat

SIZES = ((32, 48), (50, 70))
BAR = 1e-4  # max(1e-4, 3 x the reference's own float32 spread (0))


@functools.lru_cache(maxsize=None)
def state(whiten: bool = True) -> dict:
    """The seeded weights shared by every NetVLAD test; read-only.  The whitened dict holds the other one's tensors (one stream)."""
    return netvlad_synth_state(0, whiten=whiten)


@functools.lru_cache(maxsize=None)
def golden(h: int, w: int) -> dict:
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"netvlad_{h}x{w}.npz")
    with np.load(path) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def rel(out, ref) -> float:
    return (out.double().cpu() - ref.double()).abs().max().item() / ref.double().abs().max().item()


def test_synthetic_state_is_one_stream():
    a, b = state(False), state(True)
    assert set(b) - set(a) == {"whiten.weight", "whiten.bias"}
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert b["whiten.weight"].shape == (4096, 32768) and b["whiten.weight"].dtype == torch.float32


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_matches_the_reference_output(hw):
    g = golden(*hw)
    for dtype in (torch.float32, torch.float64):
        out = R.forward(state(True), g["image"], True, dtype)
        errs = rel(out["backbone"], g["backbone"]), rel(out["vlad"], g["vlad"]), rel(out["global_descriptor"], g["whitened"])
        print(f"[netvlad-cpu] {hw} {dtype}: backbone {errs[0]:.2e}, vlad {errs[1]:.2e}, whitened {errs[2]:.2e}")
        assert max(errs) < BAR, errs
    assert g["backbone"].shape[2:] == (hw[0] // 16, hw[1] // 16)
    assert torch.allclose(g["vlad"].norm(dim=1), torch.ones(2), atol=1e-5) and torch.allclose(g["whitened"].norm(dim=1), torch.ones(2), atol=1e-5)


def test_assignments_are_sharp_but_not_one_hot():
    """The synthetic score scale: median top probability in 0.5 .. 0.9, so that the soft-max matters and no cluster map is trivial."""
    g = golden(50, 70)
    f = R.backbone(state(False), R.preprocess(state(False), g["image"]))
    _, a = R.vlad_layer(state(False), f.flatten(2), return_assignment=True)
    top = a.amax(dim=1).median().item()
    assert 0.5 <= top <= 0.9, top


def test_packed_buffer_is_byte_identical(lib, golden_dir):
    with open(os.path.join(golden_dir, "netvlad_packed_digest.json")) as f:
        gold = json.load(f)
    buf = backend.pack_netvlad(state(False)).numpy()
    assert buf.size == gold["floats"] == lib.imcui_hip_netvlad_packed_floats(0)
    assert hashlib.sha256(buf.tobytes()).hexdigest() == gold["sha256"]
    # layer 0 is [9 taps][3 input channels (RGB)][64], the mean follows the bias
    w = torch.from_numpy(buf[: 27 * 64]).reshape(3, 3, 3, 64).permute(3, 2, 0, 1)
    assert torch.equal(w, state(False)["backbone.0.weight"])
    assert torch.equal(torch.from_numpy(buf[27 * 64 + 64 : 27 * 64 + 67]), state(False)["preprocess.mean"])


def test_whitened_buffer_appends_the_matrix_as_float32(lib):
    plain = backend.pack_netvlad(state(False))
    full = backend.pack_netvlad(state(True))
    n, nw = plain.numel(), 4096 * 32768
    assert full.numel() == lib.imcui_hip_netvlad_packed_floats(1) == n + nw + 4096
    assert torch.equal(full[:n], plain)
    assert torch.equal(full[n : n + nw].view(4096, 32768), state(True)["whiten.weight"])
    assert torch.equal(full[n + nw :], state(True)["whiten.bias"])


def test_packer_is_strict(lib):
    names = backend.netvlad_tensor_names(False)
    assert names[0] == "backbone.0.weight" and names[-1] == "preprocess.mean" and len(names) == 29
    assert backend.netvlad_tensor_names(True)[-2:] == ["whiten.weight", "whiten.bias"]
    sd = dict(state(False))
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_netvlad({k: v for k, v in sd.items() if k != "netvlad.centers"})
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_netvlad({**sd, "backbone.30.weight": torch.zeros(1)})
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_netvlad({**sd, "netvlad.centers": sd["netvlad.centers"].t().contiguous()})
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_netvlad(sd, whiten=True)  # the whitening pair is asked for and absent


def test_plugin_contract(lib, golden_dir):
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import BaseModel, dynamic_load

    with open(os.path.join(golden_dir, "netvlad_conf.json")) as f:
        ref = json.load(f)
    cls = dynamic_load(extractors, "netvlad")
    assert cls.__name__ == "NetVLAD" and issubclass(cls, BaseModel)
    assert cls.default_conf == ref["default_conf"] and list(cls.required_inputs) == ref["required_inputs"]
    assert sorted(cls.dir_models) == ref["model_names"]
    assert ef.confs["netvlad"] == ref["extractor_conf"]
    with pytest.raises(AssertionError):
        cls({"model_name": "VGG16-NetVLAD-Nowhere", "state_dict": state(False), "whiten": False})
    m = cls({"state_dict": state(False), "whiten": False})
    assert torch.equal(m.packed, backend.pack_netvlad(state(False))) and "state_dict" not in m.conf
    with pytest.raises(AssertionError):
        m({"image": torch.zeros(1, 1, 32, 32)})  # the reference's `assert image.shape[1] == 3`
    with pytest.raises(AssertionError):
        m({"image": torch.full((1, 3, 32, 32), 1.5)})  # ... and its range assertion
    with pytest.raises(FileNotFoundError):
        cls({"weights_path": "/nonexistent/netvlad.mat", "whiten": False})
    with pytest.raises(ValueError, match="16"):
        backend.netvlad_check_args((1, 3, 15, 64))
    with pytest.raises(ValueError, match="RGB"):
        backend.netvlad_check_args((1, 1, 64, 64))


def test_mat_round_trip_through_the_plugin_loader(lib, tmp_path, monkeypatch):
    """The synthetic checkpoint as a MATLAB file -> the plugin's loader (the reference's permutes, the centres' sign flip, averageImage[0, 0])
    -> the tensors it was written from; by `weights_path` and at the reference's cache path."""
    from imcui_hip.hloc.extractors import netvlad as P

    path = tmp_path / "hub" / "netvlad" / "VGG16-NetVLAD-TokyoTM.mat"
    path.parent.mkdir(parents=True)
    netvlad_write_mat(path, state(False))
    sd = P.load_netvlad_mat(path, whiten=False)
    assert set(sd) == set(state(False))
    for k, v in state(False).items():
        assert sd[k].dtype == torch.float32 and torch.equal(sd[k], v), k
    want = backend.pack_netvlad(state(False))
    assert torch.equal(P.NetVLAD({"weights_path": str(path), "whiten": False}).packed, want)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    assert torch.equal(P.NetVLAD({"model_name": "VGG16-NetVLAD-TokyoTM", "whiten": False}).packed, want)
    # a small whitening pair goes through the same cell layout ([1, 1, IN, OUT] -> [OUT, IN])
    tiny = {**state(False), "whiten.weight": torch.arange(12.0).view(3, 4), "whiten.bias": torch.tensor([1.0, 2.0, 3.0])}
    netvlad_write_mat(tmp_path / "tiny.mat", tiny)
    got = P.load_netvlad_mat(tmp_path / "tiny.mat", whiten=True)
    assert torch.equal(got["whiten.weight"], tiny["whiten.weight"]) and torch.equal(got["whiten.bias"], tiny["whiten.bias"])


def test_pairs_from_retrieval_host_logic(tmp_path):
    from imcui_hip.hloc import pairs_from_retrieval as pr

    names = ["db/a.jpg", "db/b.jpg", "query/c.jpg", "query/d.jpg"]
    assert pr.parse_names("db", None, names) == names[:2]
    assert pr.parse_names(["query", "db/b"], None, names) == names[1:]
    assert pr.parse_names(None, ["x", "y"], names) == ["x", "y"]
    assert pr.parse_names(None, None, names) is names
    with pytest.raises(ValueError, match="prefix"):
        pr.parse_names("nowhere", None, names)
    with pytest.raises(ValueError, match="Unknown type"):
        pr.parse_names(None, 3, names)
    lst = tmp_path / "list.txt"
    lst.write_text("# comment\nquery/c.jpg\n\nquery/d.jpg PINHOLE 1 1\n")
    assert pr.parse_names(None, lst, names) == ["query/c.jpg", "query/d.jpg"]
    # the reference's walk: row-major over the ranks, non-finite ranks skipped
    idx = np.array([[2, 0, 1], [1, -1, -1]], dtype=np.int32)
    val = np.array([[0.9, 0.5, -np.inf], [0.3, -np.inf, -np.inf]], dtype=np.float32)
    assert pr.pairs_from_topk(idx, val) == [(0, 2), (0, 0), (1, 1)]
    with pytest.raises(NotImplementedError, match="db_model"):
        pr.main(tmp_path / "none.h5", tmp_path / "pairs.txt", 2, db_model=tmp_path, db_descriptors=[])
