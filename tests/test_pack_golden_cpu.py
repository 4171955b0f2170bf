"""The packed weight format of the extractors is pinned: tests/golden/packed_digests.json holds the SHA-256 of every packed buffer
(seeded weights, seed 0), its size and the workspace size at B = 2, 72 x 104, recorded from the library as it was BEFORE the
extractors' host code moved into csrc/netpack.h.  A digest that moves means a layout or a BatchNorm fold changed: fix the code, the
file is not regenerated."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_packed_digests as gen  # noqa: E402

NETS = ("superpoint", "disk", "xfeat", "aliked") + gen.ALIKE_VARIANTS


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "packed_digests.json")) as f:
        g = json.load(f)
    assert tuple(g["shape"]) == gen.SHAPE and g["superpoint_nms_radius"] == gen.SP_NMS_RADIUS and set(g["nets"]) == set(NETS)
    return g["nets"]


@pytest.mark.parametrize("net", NETS)
def test_sizes_match_the_recorded_ones(lib, golden, net):
    packed_floats, workspace_bytes = gen.sizes(lib)[net]
    assert packed_floats == golden[net]["packed_floats"]
    assert workspace_bytes == golden[net]["workspace_bytes"]


@pytest.mark.parametrize("net", NETS)
def test_packed_buffer_is_byte_identical(lib, golden, net):
    buf = gen.packers()[net]().numpy()
    assert buf.size == golden[net]["packed_floats"]
    assert hashlib.sha256(buf.tobytes()).hexdigest() == golden[net]["sha256"]
