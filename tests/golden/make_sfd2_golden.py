"""Writes tests/golden/sfd2_golden.npz from the REFERENCE's own wrapper (imcui/hloc/extractors/sfd2.py), on the CPU.

    python tests/golden/make_sfd2_golden.py <reference root>

Run by hand, never by a test; it writes data only and copies no reference code: the wrapper is imported.  The network the wrapper imports
(`pram.nets.sfd2.load_sfd2`, from the empty third_party directory) is not in the reference checkout, so the restatement
tests/sfd2_reference.py is injected under that module name; `torchvision.transforms.Normalize` is stubbed with its two operations
((x - mean) / std per channel, float32) where torchvision is missing; `_download_model` is pointed at a synthetic checkpoint
(imcui_hip.synth_weights.sfd2_synth_state(0)), which the injected loader reads from the path the wrapper hands it.  What the file pins is
therefore the WRAPPER: the Normalize constants, that the whole conf reaches `extract_local_global` as `config`, the `{"image": ...}`
call and the `pred[...][0][None]` output layout.

Two images (uint8 values / 255, seeded; 40x56 and 50x70), each at the default max_keypoints (4096, above the count), 7, and 1000 (above
the count as well).  Descriptors are stored once per image, for the default; the other settings store the row of that array each of
their descriptors equals bit for bit (asserted here), which keeps the file small.
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
SETTINGS = (("default", None), ("top7", 7), ("above", 1000))


def image_u8(h, w):
    return torch.randint(0, 256, (1, 3, h, w), generator=torch.Generator().manual_seed(2100 + h), dtype=torch.uint8)


def _stub_missing_modules():
    try:
        import huggingface_hub  # noqa: F401
    except ImportError:  # the reference's BaseModel imports hf_hub_download at module level; nothing is downloaded here
        hub = types.ModuleType("huggingface_hub")
        hub.hf_hub_download = None
        sys.modules["huggingface_hub"] = hub
    try:
        import torchvision.transforms  # noqa: F401
    except ImportError:

        class Normalize:  # torchvision.transforms.Normalize on a float tensor [..., C, H, W]: (x - mean) / std
            def __init__(self, mean, std):
                self.mean, self.std = torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1), torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)

            def __call__(self, x):
                return (x - self.mean) / self.std

        tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
        tvt.Normalize = Normalize
        tv.transforms = tvt
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tvt


def main(reference_root):
    from imcui_hip.synth_weights import sfd2_synth_state

    import sfd2_reference as R

    _stub_missing_modules()
    pram, nets, mod = types.ModuleType("pram"), types.ModuleType("pram.nets"), types.ModuleType("pram.nets.sfd2")
    mod.load_sfd2 = R.load_sfd2
    pram.nets, nets.sfd2 = nets, mod
    sys.modules["pram"], sys.modules["pram.nets"], sys.modules["pram.nets.sfd2"] = pram, nets, mod
    sys.path.insert(0, os.path.abspath(reference_root))
    out = {"seed": np.int64(SEED)}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)  # (the reference package opens log.txt in the working directory)
        ckpt = os.path.join(tmp, "sfd2.pth")
        torch.save(sfd2_synth_state(SEED), ckpt)
        from imcui.hloc.extractors.sfd2 import SFD2

        SFD2._download_model = lambda self, repo_id=None, filename=None, **kw: ckpt
        with torch.no_grad():
            for h, w in SIZES:
                u8 = image_u8(h, w)
                img = u8.float() / 255.0
                tag = f"{h}x{w}"
                out[f"image_u8_{tag}"] = u8.numpy()
                full = None
                for name, k in SETTINGS:
                    r = SFD2({} if k is None else {"max_keypoints": k}).eval()({"image": img})
                    kp, sc, de = r["keypoints"][0].numpy(), r["scores"][0].numpy(), r["descriptors"][0].numpy().T
                    out[f"keypoints_{name}_{tag}"], out[f"scores_{name}_{tag}"] = kp, sc
                    if full is None:
                        full = de
                        out[f"descriptors_default_{tag}"] = de
                    else:
                        rows = np.array([int(np.flatnonzero((full == d).all(axis=1))[0]) for d in de], dtype=np.int64)
                        assert (full[rows] == de).all()
                        out[f"desc_rows_{name}_{tag}"] = rows
                    print(f"[sfd2 golden] {tag} {name}: max_keypoints {k}: {len(sc)} key-points, scores {sc.min() if len(sc) else 0:.4f} .. "
                          f"{sc.max() if len(sc) else 0:.4f}")  # fmt: skip
        os.chdir(ROOT)
    path = os.path.join(HERE, "sfd2_golden.npz")
    np.savez_compressed(path, **out)
    print(f"[sfd2 golden] {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
