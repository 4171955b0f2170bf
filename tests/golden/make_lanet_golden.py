"""Writes tests/golden/lanet_golden.npz from the REFERENCE's own wrapper (imcui/hloc/extractors/lanet.py), on the CPU.

    python tests/golden/make_lanet_golden.py <reference root>

Run by hand, never by a test; it writes data only and copies no reference code: the wrapper is imported.  The network the wrapper imports
(`lanet.network_v0.model.PointModel`) is not in the reference checkout, so the restatement tests/lanet_reference.py is injected under
that module name; `_download_model` is pointed at a synthetic checkpoint (imcui_hip.synth_weights.lanet_synth_state(0), saved under
the wrapper's `model_state` key), which the wrapper loads with its own code.  What the file pins is therefore the WRAPPER: which output
of the network is the score, the view / transpose of :45-46, the strict threshold, the argsort cut and the output layout.

Two images (uint8 values / 255, seeded; 40x56 = 5x7 cells and 50x70 = 6x8 cells), each at (keypoint_threshold, max_keypoints) = (0.1, 0),
(the median of the interior scores, placed midway between the two middle ones, 0) and (0.1, 7).  Descriptors are stored once per image, for (0.1, 0); the other two settings store the row of
that array each of their descriptors equals bit for bit (asserted here), which keeps the file small.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "image-matching-webui_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = ((40, 56), (50, 70))
SEED = 0


def image_u8(h, w):
    return torch.randint(0, 256, (1, 3, h, w), generator=torch.Generator().manual_seed(2000 + h), dtype=torch.uint8)


def main(reference_root):
    from imcui_hip.synth_weights import lanet_synth_state

    import lanet_reference as R

    try:
        import huggingface_hub  # noqa: F401
    except ImportError:  # the reference's BaseModel imports hf_hub_download at module level; nothing is downloaded here
        hub = types.ModuleType("huggingface_hub")
        hub.hf_hub_download = None
        sys.modules["huggingface_hub"] = hub
    pkg, v0, model = types.ModuleType("lanet"), types.ModuleType("lanet.network_v0"), types.ModuleType("lanet.network_v0.model")
    model.PointModel = R.PointModel
    pkg.network_v0, v0.model = v0, model
    sys.modules.update({"lanet": pkg, "lanet.network_v0": v0, "lanet.network_v0.model": model})
    sys.path.insert(0, os.path.abspath(reference_root))
    out = {"seed": np.int64(SEED)}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)  # (the reference package opens log.txt in the working directory)
        ckpt = os.path.join(tmp, "PointModel_v0.pth")
        torch.save({"model_state": lanet_synth_state(SEED)}, ckpt)
        from imcui.hloc.extractors.lanet import LANet

        LANet._download_model = lambda self, repo_id=None, filename=None, **kw: ckpt
        with torch.no_grad():
            for h, w in SIZES:
                u8 = image_u8(h, w)
                img = u8.float() / 255.0
                probe = LANet({"keypoint_threshold": 0.1, "max_keypoints": 0}).eval()
                median = R.median_threshold(probe.net(img)[0])  # midway between the two middle scores: no cell sits on it
                tag = f"{h}x{w}"
                out[f"image_u8_{tag}"] = u8.numpy()
                out[f"median_{tag}"] = np.float32(median)
                full = None
                for name, thr, k in (("all", 0.1, 0), ("median", median, 0), ("top7", 0.1, 7)):
                    r = LANet({"keypoint_threshold": thr, "max_keypoints": k}).eval()({"image": img})
                    kp, sc, de = r["keypoints"][0].numpy(), r["scores"][0].numpy(), r["descriptors"][0].numpy().T
                    out[f"keypoints_{name}_{tag}"], out[f"scores_{name}_{tag}"] = kp, sc
                    if full is None:
                        full = de
                        out[f"descriptors_all_{tag}"] = de
                    else:
                        rows = np.array([int(np.flatnonzero((full == d).all(axis=1))[0]) for d in de], dtype=np.int64)
                        assert (full[rows] == de).all()
                        out[f"desc_rows_{name}_{tag}"] = rows
                    print(f"[lanet golden] {tag} {name}: threshold {thr:.6f}, max_keypoints {k}: {len(sc)} key-points, scores {sc.min() if len(sc) else 0:.4f} .. "
                          f"{sc.max() if len(sc) else 0:.4f}")  # fmt: skip
        os.chdir(ROOT)
    path = os.path.join(HERE, "lanet_golden.npz")
    np.savez_compressed(path, **out)
    print(f"[lanet golden] {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
