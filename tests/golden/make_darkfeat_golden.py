"""Writes tests/golden/darkfeat_golden.npz from the REFERENCE's own wrapper (imcui/hloc/extractors/darkfeat.py), on the CPU.

    python tests/golden/make_darkfeat_golden.py <reference root>

Run by hand, never by a test; it writes data only and copies no reference code: the wrapper is imported.  The network the wrapper imports
(`darkfeat.DarkFeat`, from the empty submodule third_party/DarkFeat) is not in the reference checkout, so the restatement
tests/darkfeat_reference.py is injected under that module name; `_download_model` is pointed at a synthetic checkpoint
(imcui_hip.synth_weights.darkfeat_synth_state(0)), which the injected class loads from the path the wrapper hands it.  What the file
pins is therefore the WRAPPER: that none of its conf reaches the network, the `{"image": ...}` call, the ascending argsort, the
`[-max_keypoints or None:]` cut and the output layout.

Two images (uint8 values / 255, seeded; 40x56 and 50x70), each at max_keypoints 0 (all), 7 and 1000 (above the count).  Descriptors are
stored once per image, for max_keypoints 0; the other settings store the row of that array each of their descriptors equals bit for bit
(asserted here), which keeps the file small.
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
SETTINGS = (("all", 0), ("top7", 7), ("above", 1000))


def image_u8(h, w):
    return torch.randint(0, 256, (1, 3, h, w), generator=torch.Generator().manual_seed(2000 + h), dtype=torch.uint8)


def main(reference_root):
    from imcui_hip.synth_weights import darkfeat_synth_state

    import darkfeat_reference as R

    try:
        import huggingface_hub  # noqa: F401
    except ImportError:  # the reference's BaseModel imports hf_hub_download at module level; nothing is downloaded here
        hub = types.ModuleType("huggingface_hub")
        hub.hf_hub_download = None
        sys.modules["huggingface_hub"] = hub
    mod = types.ModuleType("darkfeat")
    mod.DarkFeat = R.DarkFeat
    sys.modules["darkfeat"] = mod
    sys.path.insert(0, os.path.abspath(reference_root))
    out = {"seed": np.int64(SEED)}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)  # (the reference package opens log.txt in the working directory)
        ckpt = os.path.join(tmp, "DarkFeat.pth")
        torch.save(darkfeat_synth_state(SEED), ckpt)
        from imcui.hloc.extractors.darkfeat import DarkFeat

        DarkFeat._download_model = lambda self, repo_id=None, filename=None, **kw: ckpt
        with torch.no_grad():
            for h, w in SIZES:
                u8 = image_u8(h, w)
                img = u8.float() / 255.0
                tag = f"{h}x{w}"
                out[f"image_u8_{tag}"] = u8.numpy()
                full = None
                for name, k in SETTINGS:
                    r = DarkFeat({"max_keypoints": k}).eval()({"image": img})
                    kp, sc, de = r["keypoints"][0].numpy(), r["scores"][0].numpy(), r["descriptors"][0].numpy().T
                    out[f"keypoints_{name}_{tag}"], out[f"scores_{name}_{tag}"] = kp, sc
                    if full is None:
                        full = de
                        out[f"descriptors_all_{tag}"] = de
                    else:
                        rows = np.array([int(np.flatnonzero((full == d).all(axis=1))[0]) for d in de], dtype=np.int64)
                        assert (full[rows] == de).all()
                        out[f"desc_rows_{name}_{tag}"] = rows
                    print(f"[darkfeat golden] {tag} {name}: max_keypoints {k}: {len(sc)} key-points, scores {sc.min() if len(sc) else 0:.4f} .. "
                          f"{sc.max() if len(sc) else 0:.4f}")  # fmt: skip
        os.chdir(ROOT)
    path = os.path.join(HERE, "darkfeat_golden.npz")
    np.savez_compressed(path, **out)
    print(f"[darkfeat golden] {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
