"""Writes tests/golden/lisrd_golden.npz from the REFERENCE's own wrapper (imcui/hloc/matchers/lisrd.py), on the CPU.

    python tests/golden/make_lisrd_golden.py <reference root>

Run by hand, never by a test; it writes data only and copies no reference code: the wrapper is imported.  What the wrapper imports and the
checkout (or this machine) does not have is injected into sys.modules before the import: the restatement tests/lisrd_reference.py as
`lisrd.models` and `lisrd.models.base_model` (`get_model`, `Mode`), a `kornia.color` stand-in (rgb_to_grayscale with kornia's weights) and
stand-ins for the three reference extractor modules, whose one detector class returns STORED key-points.  `_download_model` is pointed at
a synthetic checkpoint (imcui_hip.synth_weights.lisrd_synth_state(0) under the `model_state_dict` key), which the restated `load` reads.
What the file pins is therefore the WRAPPER: the `* 255`, the (x, y) -> (row, col) flip, `_keypoints_to_grid`, grid_sample + normalize,
`_lisrd_matcher`, `_compute_confidence` and the output dictionary.

Two pairs, each a 40x56 image against a 50x70 image (uint8 values / 255, seeded), about 60 key-points per image: (0, 0), (W - 1, H - 1),
integer and sub-pixel positions.  Seeds are tried until the smallest top-2 gap of the similarity matrix over rows and columns is at least
1e-4, so that no arg-max of the pair hangs on float32 round-off.  Stored as float32: the sampled descriptors of every key-point, the
sampled meta descriptors of the first META_ROWS key-points (the file has to stay below 1 MiB), matches, mconf and the margin.
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

PAIRS = (((40, 56), (50, 70)), ((50, 70), (40, 56)))
NKPTS = (60, 55)
META_ROWS = 6
MIN_MARGIN = 1e-4
QUEUE = []  # key-points the stand-in detector hands out, in call order


def image_u8(h, w, seed):
    return torch.randint(0, 256, (1, 3, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def keypoints(h, w, n, seed):
    """(x, y): the two image corners, integer positions, sub-pixel positions"""
    g = torch.Generator().manual_seed(seed)
    third = (n - 2) // 3
    ints = torch.stack([torch.randint(0, w, (third,), generator=g), torch.randint(0, h, (third,), generator=g)], 1).float()
    sub = torch.rand(n - 2 - third, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    return torch.cat([torch.tensor([[0.0, 0.0], [w - 1.0, h - 1.0]]), ints, sub])


class StoredDetector:
    def __init__(self, conf):
        self.conf = conf

    def to(self, device):
        return self

    def __call__(self, data):
        return {"keypoints": [QUEUE.pop(0)]}


def inject(reference_root):
    import lisrd_reference as R

    try:
        import huggingface_hub  # noqa: F401
    except ImportError:  # the reference's BaseModel imports hf_hub_download at module level; nothing is downloaded here
        hub = types.ModuleType("huggingface_hub")
        hub.hf_hub_download = None
        sys.modules["huggingface_hub"] = hub
    pkg, models, base = types.ModuleType("lisrd"), types.ModuleType("lisrd.models"), types.ModuleType("lisrd.models.base_model")
    models.get_model, base.Mode, base.get_model = R.get_model, R.Mode, R.get_model
    pkg.models, models.base_model = models, base
    sys.modules.update({"lisrd": pkg, "lisrd.models": models, "lisrd.models.base_model": base})
    if "kornia" not in sys.modules:
        kornia, color = types.ModuleType("kornia"), types.ModuleType("kornia.color")
        color.rgb_to_grayscale = lambda im: 0.299 * im[:, 0:1] + 0.587 * im[:, 1:2] + 0.114 * im[:, 2:3]
        kornia.color = color
        sys.modules.update({"kornia": kornia, "kornia.color": color})
    sys.path.insert(0, os.path.abspath(reference_root))
    import imcui.hloc.extractors  # noqa: F401  (the package itself is the reference's)

    for mod, cls in (("aliked", "ALIKED"), ("sift", "SIFT"), ("superpoint", "SuperPoint")):
        m = types.ModuleType(f"imcui.hloc.extractors.{mod}")
        setattr(m, cls, StoredDetector)
        sys.modules[m.__name__] = m


def main(reference_root):
    from imcui_hip.synth_weights import lisrd_synth_state

    out = {"meta_rows": np.int64(META_ROWS)}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)  # (the reference package opens log.txt in the working directory)
        inject(reference_root)
        ckpt = os.path.join(tmp, "lisrd_aachen.pth")
        torch.save({"model_state_dict": lisrd_synth_state(0)}, ckpt)
        import imcui.hloc.matchers.lisrd as W

        W.Lisrd._download_model = lambda self, repo_id=None, filename=None, **kw: ckpt
        seen = {}
        inner = W._lisrd_matcher

        def spy(desc1, desc2, meta1, meta2):
            seen.update(desc0=desc1, desc1=desc2, meta0=meta1, meta1=meta2)
            return inner(desc1, desc2, meta1, meta2)

        W._lisrd_matcher = spy
        model = W.Lisrd({"detector": "superpoint"}).eval()
        for p, ((h0, w0), (h1, w1)) in enumerate(PAIRS):
            for seed in range(100 * p, 100 * p + 40):
                u0, u1 = image_u8(h0, w0, 3000 + seed), image_u8(h1, w1, 4000 + seed)
                k0, k1 = keypoints(h0, w0, NKPTS[0], 5000 + seed), keypoints(h1, w1, NKPTS[1], 6000 + seed)
                QUEUE[:] = [k0.clone(), k1.clone()]
                with torch.no_grad():
                    r = model({"image0": u0.float() / 255.0, "image1": u1.float() / 255.0})
                sim = (torch.einsum("nid,mid->nim", seen["desc0"].double(), seen["desc1"].double())
                       * torch.softmax(torch.einsum("nid,mid->nim", seen["meta0"].double(), seen["meta1"].double()), dim=1)).sum(1)  # fmt: skip
                tr, tc = sim.topk(2, dim=1).values, sim.topk(2, dim=0).values
                margin = min(float((tr[:, 0] - tr[:, 1]).min()), float((tc[0] - tc[1]).min()))
                print(f"[lisrd golden] pair {p} seed {seed}: {len(r['mconf'])} matches, margin {margin:.3g}")
                if margin >= MIN_MARGIN:
                    break
            else:
                raise SystemExit("no seed reached the margin")
            assert torch.equal(r["keypoints0"], k0) and torch.equal(r["keypoints1"], k1)
            f32 = lambda t: t.detach().float().numpy()
            out.update({f"seed_{p}": np.int64(seed), f"margin_{p}": np.float64(margin), f"image0_u8_{p}": u0.numpy(), f"image1_u8_{p}": u1.numpy(),
                        f"keypoints0_{p}": f32(k0), f"keypoints1_{p}": f32(k1), f"desc0_{p}": f32(seen["desc0"]), f"desc1_{p}": f32(seen["desc1"]),
                        f"meta0_{p}": f32(seen["meta0"][:META_ROWS]), f"meta1_{p}": f32(seen["meta1"][:META_ROWS]), f"mkeypoints0_{p}": f32(r["mkeypoints0"]),
                        f"mkeypoints1_{p}": f32(r["mkeypoints1"]), f"mconf_{p}": f32(r["mconf"])})  # fmt: skip
        os.chdir(ROOT)
    path = os.path.join(HERE, "lisrd_golden.npz")
    np.savez_compressed(path, **out)
    print(f"[lisrd golden] {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
