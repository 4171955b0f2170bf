"""SHA-256 of the packed weight buffers of the extractors (seeded weights, seed 0), their sizes in floats and the workspace sizes at
B = 2, 72 x 104, as the library named by IMCUI_HIP_LIB (default: the in-tree build) produces them -> packed_digests.json.

The committed file was recorded from the library of the commit BEFORE the extractors' host code was shared (csrc/netpack.h); it pins the
packed format.  Run it against that library only, never to make tests/test_pack_golden_cpu.py pass:

    IMCUI_HIP_LIB=/path/to/old/libimcui_hip.so python tests/golden/make_packed_digests.py
"""
import hashlib
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, os.path.join(ROOT, "image-matching-webui_amd"))

ALIKE_VARIANTS = ("alike-t", "alike-s", "alike-n")
SHAPE = (2, 72, 104)  # B, H, W of the workspace sizes
SP_NMS_RADIUS = 4


def packers():
    """name -> function returning the packed buffer of the seeded weights"""
    from imcui_hip import backend
    from imcui_hip import synth_weights as sw

    def superpoint():
        # The seeded convDb.bias is the mean of a CPU forward pass over a noise image: its last bits follow the thread count of the
        # machine.  It is replaced by seeded noise of the same size; every other tensor is the default one.
        import torch

        sd = sw.superpoint_state_dict(seed=0)
        sd["convDb.bias"] = torch.randn(256, generator=torch.Generator().manual_seed(1)) * 0.05
        return backend.pack_superpoint(sd)

    p = {
        "superpoint": superpoint,
        "disk": lambda: backend.pack_disk(sw.disk_state_dict(seed=0)),
        "xfeat": lambda: backend.pack_xfeat(sw.xfeat_state_dict(seed=0)),
        "aliked": lambda: backend.pack_aliked(sw.aliked_state_dict(seed=0)),
    }
    for v in ALIKE_VARIANTS:
        p[v] = lambda v=v: backend.pack_alike(sw.alike_state_dict(v, seed=0), v)
    return p


def sizes(lib):
    """name -> (packed floats, workspace bytes at SHAPE) from the library's own size functions"""
    B, H, W = SHAPE
    s = {
        "superpoint": (lib.imcui_hip_superpoint_packed_floats(), lib.imcui_hip_superpoint_workspace_bytes(B, H, W, SP_NMS_RADIUS)),
        "disk": (lib.imcui_hip_disk_packed_floats(), lib.imcui_hip_disk_workspace_bytes(B, H, W)),
        "xfeat": (lib.imcui_hip_xfeat_packed_floats(), lib.imcui_hip_xfeat_workspace_bytes(B, H, W)),
        "aliked": (lib.imcui_hip_aliked_packed_floats(), lib.imcui_hip_aliked_workspace_bytes(B, H, W)),
    }
    for i, v in enumerate(ALIKE_VARIANTS):
        s[v] = (lib.imcui_hip_alike_packed_floats(i), lib.imcui_hip_alike_workspace_bytes(i, B, H, W))
    return s


def record():
    from imcui_hip import load_library

    sz = sizes(load_library())
    out = {}
    for name, pack in packers().items():
        buf = pack().numpy()
        out[name] = {"sha256": hashlib.sha256(buf.tobytes()).hexdigest(), "packed_floats": int(sz[name][0]), "workspace_bytes": int(sz[name][1])}
        assert buf.size == sz[name][0], name
    return out


if __name__ == "__main__":
    import torch

    torch.set_num_threads(1)
    with open(os.path.join(OUT, "packed_digests.json"), "w") as f:
        json.dump({"shape": list(SHAPE), "superpoint_nms_radius": SP_NMS_RADIUS, "nets": record()}, f, indent=1, sort_keys=True)
        f.write("\n")
