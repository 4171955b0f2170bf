"""The `sfd2+imp` zoo entry through the file-based drivers: two crops of one seeded canvas -> `extract_features` with the `sfd2` plugin ->
feature .h5 -> `match_features` with the `imp` plugin, in both pair orders -> match .h5 in the reference's layout (`matches0` int16,
`matching_scores0` float16 under `name0/name1`), compared with ONE `forward_batched` call on the features read back from the file."""
import numpy as np
import pytest
import torch

from imcui_hip.synth_weights import imp_synth_state, sfd2_synth_state
from test_gpu_disk_files import _rgb_u8

pytestmark = pytest.mark.gpu


def test_sfd2_extract_then_imp_match_from_files(tmp_path):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import match_features as mf
    from imcui_hip.hloc.extractors.sfd2 import SFD2
    from imcui_hip.hloc.matchers.imp import IMP
    from imcui_hip.hloc.utils.h5lite import open_h5

    root = tmp_path / "images"
    root.mkdir()
    canvas = _rgb_u8(272, 352, 77)
    Image.fromarray(canvas[:240, :320].copy()).save(root / "a.png")
    Image.fromarray(canvas[32:, 32:].copy()).save(root / "b.png")  # the same 240 x 320 window, 32 pixels down and right
    conf = {**ef.confs["sfd2"], "preprocessing": {**ef.confs["sfd2"]["preprocessing"], "resize_max": 320}}  # (no resize: keeps the test small)
    sfd2 = SFD2({**conf["model"], "state_dict": sfd2_synth_state(0)}).eval().to("cuda:0")
    feature_path = ef.main(conf, root, tmp_path / "out", model=sfd2, batch_size=2)
    assert sorted(ef.list_h5_names(feature_path)) == ["a.png", "b.png"]
    store = mf.H5FeatureStore(feature_path)
    fa, fb = store.get("a.png"), store.get("b.png")
    assert fa["descriptors"].shape[0] == 128 and fa["keypoints"].shape[0] > 50 and fb["keypoints"].shape[0] > 50

    # descriptors of the seeded SFD2 weights are crowded (mean cosine 0.94 between the two crops): final_proj.8 doubled makes the scores,
    # and with them the dust-bin score, four times as sharp, and the restatement then matches 806 of the 1071 points (681 of the 696
    # true correspondences); at the calibration of imp_synth_state it matches 4
    sd = imp_synth_state(0)
    sd["final_proj.8.weight"], sd["final_proj.8.bias"], sd["bin_score"] = sd["final_proj.8.weight"] * 2, sd["final_proj.8.bias"] * 2, sd["bin_score"] * 4
    model = IMP({"state_dict": sd}).eval().to("cuda:0")
    files = {}
    for tag, (q, r) in (("ab", ("a.png", "b.png")), ("ba", ("b.png", "a.png"))):
        pairs_path = tmp_path / f"pairs-{tag}.txt"
        pairs_path.write_text(f"{q} {r}\n")
        files[(q, r)] = mf.match_from_paths(model, pairs_path, tmp_path / "out" / f"matches-sfd2-imp-{tag}.h5", feature_path, feature_path, batch_size=2)

    # one forward_batched call on the same features: pair 0 = (a, b), pair 1 = (b, a)
    ncap = max(fa["keypoints"].shape[0], fb["keypoints"].shape[0])
    t = {k: torch.zeros((2, ncap) + s) for k, s in (("keypoints0", (2,)), ("keypoints1", (2,)), ("scores0", ()), ("scores1", ()),
                                                     ("descriptors0", (128,)), ("descriptors1", (128,)))}  # fmt: skip
    counts = torch.zeros(2, 2, dtype=torch.int32)
    for b, (f0, f1) in enumerate(((fa, fb), (fb, fa))):
        for side, f in (("0", f0), ("1", f1)):
            n = f["keypoints"].shape[0]
            t["keypoints" + side][b, :n] = torch.from_numpy(f["keypoints"].astype(np.float32))
            t["scores" + side][b, :n] = torch.from_numpy(f["scores"].astype(np.float32))
            t["descriptors" + side][b, :n] = torch.from_numpy(f["descriptors"].astype(np.float32)).t()
            counts[b, int(side)] = n
    size = tuple(int(v) for v in fa["image_size"])
    assert size == (320, 240) and tuple(int(v) for v in fb["image_size"]) == size
    out = model.forward_batched(*(t[k].cuda() for k in ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1")),
                                counts[:, 0].cuda(), counts[:, 1].cuda(), size, size)  # fmt: skip
    torch.cuda.synchronize()
    for b, (q, r) in enumerate((("a.png", "b.png"), ("b.png", "a.png"))):
        n = int(counts[b, 0])
        with open_h5(files[(q, r)], "r") as fd:
            grp = fd[mf.names_to_pair(q, r)]
            m, s = grp["matches0"].__array__(), grp["matching_scores0"].__array__()
        assert m.dtype == np.int16 and s.dtype == np.float16 and m.shape == (n,) and s.shape == (n,)
        assert (m > -1).sum() > 10, (q, r, int((m > -1).sum()))
        assert np.array_equal(m, out["matches0"][b, :n].cpu().numpy().astype(np.int16)), (q, r)
        assert np.array_equal(s, out["matching_scores0"][b, :n].cpu().numpy().astype(np.float16)), (q, r)
