"""Writes tests/golden/netvlad_*.npz and netvlad_conf.json from the REFERENCE's own NetVLAD (imcui/hloc/extractors/netvlad.py), on the CPU.

    python tests/golden/make_netvlad_golden.py <reference root>

Run by hand, never by a test; it writes data only.  The reference imports `torchvision.models` for the VGG-16 layer SEQUENCE alone (every
weight comes from the MATLAB checkpoint), so where torchvision is missing a stub `vgg16()` with the standard sequence stands in.  The
checkpoint is the synthetic one of imcui_hip.synth_weights.netvlad_synth_state(0) written as a .mat into a temporary TORCH_HOME, so the
reference parses it with its own code (the permutes, the sign flip of the centres, averageImage[0, 0]).

Stored per image size (batch 2, seeded uniform images): the images, the backbone output, the 32768-d descriptor (`whiten: False`) and the
4096-d descriptor (`whiten: True`); float16 would lose the point, so the backbone map is kept only for the small sizes used here.
Printed: the reference's own float32 spread (1 against 8 torch threads) and its distance from the float64 restatement -- the numbers the
end-to-end bar max(1e-4, 3 x spread) of tests/test_gpu_netvlad.py rests on.
"""
import json
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

SIZES = ((32, 48), (50, 70))
SEED = 0


def images(h, w):
    return torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(1000 + h))


def stub_torchvision():
    try:
        import torchvision.models  # noqa: F401

        return
    except ImportError:
        pass
    from torch import nn

    def vgg16():
        cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
        layers, cin = [], 3
        for v in cfg:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        return nn.Sequential(nn.Sequential(*layers), nn.AdaptiveAvgPool2d(7), nn.Sequential(nn.Linear(512 * 49, 8)))

    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    models.vgg16 = vgg16
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models


def main(reference_root):
    from imcui_hip.synth_weights import NETVLAD_MODEL_NAMES, netvlad_synth_state, netvlad_write_mat

    import netvlad_reference as R

    stub_torchvision()
    sys.path.insert(0, os.path.abspath(reference_root))
    with tempfile.TemporaryDirectory() as tmp:
        os.environ["TORCH_HOME"] = tmp
        os.chdir(tmp)  # (the reference package opens log.txt in the working directory)
        state = netvlad_synth_state(SEED, whiten=True)
        os.makedirs(os.path.join(torch.hub.get_dir(), "netvlad"), exist_ok=True)
        netvlad_write_mat(os.path.join(torch.hub.get_dir(), "netvlad", NETVLAD_MODEL_NAMES[0] + ".mat"), state)
        from imcui.hloc.extractors.netvlad import NetVLAD

        with torch.no_grad():
            plain, white = NetVLAD({"whiten": False}).eval(), NetVLAD({"whiten": True}).eval()
            for h, w in SIZES:
                img = images(h, w)
                feat = plain.backbone(torch.clamp(img * 255, 0.0, 255.0) - img.new_tensor(plain.preprocess["mean"]).view(1, -1, 1, 1))
                torch.set_num_threads(8)
                v8, d8 = plain({"image": img})["global_descriptor"], white({"image": img})["global_descriptor"]
                torch.set_num_threads(1)
                v1, d1 = plain({"image": img})["global_descriptor"], white({"image": img})["global_descriptor"]
                r64 = R.forward(state, img, True, torch.float64)
                r32 = R.forward(state, img, True, torch.float32)
                top = torch.softmax(torch.nn.functional.conv1d(torch.nn.functional.normalize(r64["backbone"].flatten(2), dim=1),
                                                                state["netvlad.score_proj.weight"].double()), dim=1).amax(1)  # fmt: skip

                def rel(a, b):
                    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()

                print(f"[netvlad golden] {h}x{w}: map {tuple(feat.shape[2:])}, median top assignment {top.median().item():.2f}; reference float32 spread 1 vs 8 threads: "
                      f"vlad {rel(v1, v8):.2e}, whitened {rel(d1, d8):.2e}; reference vs float64 restatement: vlad {rel(v1, r64['vlad']):.2e}, whitened "
                      f"{rel(d1, r64['global_descriptor']):.2e}; float32 restatement vs reference: vlad {rel(r32['vlad'], v1):.2e}, whitened "
                      f"{rel(r32['global_descriptor'], d1):.2e}")  # fmt: skip
                np.savez_compressed(os.path.join(HERE, f"netvlad_{h}x{w}.npz"), image=img.numpy(), backbone=feat.numpy(), vlad=v1.numpy(), whitened=d1.numpy())
        conf = {"default_conf": NetVLAD.default_conf, "required_inputs": NetVLAD.required_inputs, "model_names": sorted(NetVLAD.dir_models),
                "extractor_conf": {"output": "global-feats-netvlad", "model": {"name": "netvlad"}, "preprocessing": {"resize_max": 1024}}}  # fmt: skip
        try:
            from imcui.hloc import extract_features as ref_ef

            conf["extractor_conf"] = ref_ef.confs["netvlad"]
        except Exception as e:  # noqa: BLE001 -- the driver module needs h5py / cv2; the conf then stays as transcribed from configs/extractors.py:372-376
            print(f"[netvlad golden] extract_features.confs not importable ({type(e).__name__}): conf transcribed")
        with open(os.path.join(HERE, "netvlad_conf.json"), "w") as f:
            json.dump(conf, f, indent=1, sort_keys=True)
        # the packed format (needs the built library; no GPU)
        import hashlib

        from imcui_hip import backend

        buf = backend.pack_netvlad(netvlad_synth_state(SEED, whiten=False)).numpy()
        with open(os.path.join(HERE, "netvlad_packed_digest.json"), "w") as f:
            json.dump({"comment": "sha256 of backend.pack_netvlad(synth_weights.netvlad_synth_state(0, whiten=False)): the packed NetVLAD weight format "
                                  "(with whitening the float32 matrix and its bias follow, tests/test_netvlad_cpu.py)",
                       "floats": int(buf.size), "sha256": hashlib.sha256(buf.tobytes()).hexdigest()}, f, indent=1)  # fmt: skip
        os.chdir(ROOT)


if __name__ == "__main__":
    main(sys.argv[1])
