"""Writes tests/golden/liftfeat_golden.npz from the REFERENCE's own wrapper (imcui/hloc/extractors/liftfeat.py), on the CPU.

    python tests/golden/make_liftfeat_golden.py <reference root>

Run by hand, never by a test; it writes data only and copies no reference code: the wrapper is imported.  The class the wrapper imports
(`models.liftfeat_wrapper.LiftFeat`, from the empty third_party directory) is not in the reference checkout, so the restatement
tests/liftfeat_reference.py is injected under that module name; `_download_model` is pointed at a synthetic checkpoint
(imcui_hip.synth_weights.liftfeat_synth_state(0)), which the injected class reads from the path the wrapper hands it.  What the file pins
is therefore the WRAPPER: the `* 255` and the HWC transpose, that `keypoint_threshold` and `max_keypoints` reach the class, the cut
`scores.argsort()[-max_keypoints or None:]` with its ascending order, 0 and -1, and the output layout.

Two images (uint8 values / 255, seeded; 40x56 and 50x70), each at max_keypoints 5000 (the default, above the count: row-major), 7, 0 and
-1.  Descriptors are stored once per image, for the default; the other settings store the row of that array each of their descriptors
equals bit for bit (asserted here), which keeps the file small.
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
SETTINGS = (("default", None), ("top7", 7), ("zero", 0), ("minus1", -1))


def image_u8(h, w):
    return torch.randint(0, 256, (1, 3, h, w), generator=torch.Generator().manual_seed(2200 + h), dtype=torch.uint8)


def main(reference_root):
    from imcui_hip.synth_weights import liftfeat_synth_state

    import liftfeat_reference as R

    try:
        import huggingface_hub  # noqa: F401
    except ImportError:  # the reference's BaseModel imports hf_hub_download at module level; nothing is downloaded here
        hub = types.ModuleType("huggingface_hub")
        hub.hf_hub_download = None
        sys.modules["huggingface_hub"] = hub
    models, mod = types.ModuleType("models"), types.ModuleType("models.liftfeat_wrapper")
    mod.LiftFeat = R.LiftFeat
    models.liftfeat_wrapper = mod
    sys.modules["models"], sys.modules["models.liftfeat_wrapper"] = models, mod
    sys.path.insert(0, os.path.abspath(reference_root))
    out = {"seed": np.int64(SEED)}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)  # (the reference package opens log.txt in the working directory)
        ckpt = os.path.join(tmp, "LiftFeat.pth")
        torch.save(liftfeat_synth_state(SEED), ckpt)
        from imcui.hloc.extractors.liftfeat import Liftfeat

        Liftfeat._download_model = lambda self, repo_id=None, filename=None, **kw: ckpt
        with torch.no_grad():
            for h, w in SIZES:
                u8 = image_u8(h, w)
                img = u8.float() / 255.0
                tag = f"{h}x{w}"
                out[f"image_u8_{tag}"] = u8.numpy()
                full = None
                for name, k in SETTINGS:
                    r = Liftfeat({} if k is None else {"max_keypoints": k}).eval()({"image": img})
                    kp, sc, de = r["keypoints"][0].numpy(), r["scores"][0].numpy(), r["descriptors"][0].numpy().T
                    out[f"keypoints_{name}_{tag}"], out[f"scores_{name}_{tag}"] = kp.astype(np.float32), sc
                    assert len(np.unique(sc)) == len(sc), "equal scores: the reference's argsort would leave their order open"
                    if full is None:
                        full = de
                        out[f"descriptors_default_{tag}"] = de
                    else:
                        rows = np.array([int(np.flatnonzero((full == d).all(axis=1))[0]) for d in de], dtype=np.int64)
                        assert (full[rows] == de).all()
                        out[f"desc_rows_{name}_{tag}"] = rows
                    print(f"[liftfeat golden] {tag} {name}: max_keypoints {k}: {len(sc)} key-points, scores {sc.min() if len(sc) else 0:.4f} .. "
                          f"{sc.max() if len(sc) else 0:.4f}")  # fmt: skip
        os.chdir(ROOT)
    path = os.path.join(HERE, "liftfeat_golden.npz")
    np.savez_compressed(path, **out)
    print(f"[liftfeat golden] {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
