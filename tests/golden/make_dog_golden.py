"""Writes tests/golden/dog_packed_digest.json: size and SHA-256 of the packed HardNet and SOSNet buffers of the seeded weights
(imcui_hip.synth_weights.hardnet_synth_state(0) / sosnet_synth_state(0)).  Needs the built library, no GPU:

    python tests/golden/make_dog_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "image-matching-webui_amd"))

from imcui_hip import backend, build  # noqa: E402
from imcui_hip.synth_weights import hardnet_synth_state, sosnet_synth_state  # noqa: E402


def main():
    build.build()
    out = {}
    for name, pack, state in (("hardnet", backend.pack_hardnet, hardnet_synth_state), ("sosnet", backend.pack_sosnet, sosnet_synth_state)):
        buf = pack(state(0)).numpy()
        out[name] = {"floats": int(buf.size), "sha256": hashlib.sha256(buf.tobytes()).hexdigest()}
    with open(os.path.join(HERE, "dog_packed_digest.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
