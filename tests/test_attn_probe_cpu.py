"""CPU side of the attention variant tests (tests/test_gpu_attention_variants.py): the descriptor mirror and the route numbering shared
with csrc/attention.h."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN_H = os.path.join(ROOT, "image-matching-webui_amd", "csrc", "attention.h")


def test_descriptor_mirror_matches_the_library(lib):
    from imcui_hip import backend

    assert ctypes.sizeof(backend.AttnDesc) == lib.imcui_hip_attn_desc_bytes()


def test_scratch_sizes(lib):
    # attention.h: ATTN_MAX_CHUNKS(R) * nseq * heads * R * 66 floats; 6400 bytes per (sequence, head, 64-key tile)
    assert lib.imcui_hip_attention_part_floats(2, 4, 2048) == 4 * 2 * 4 * 2048 * 66
    assert lib.imcui_hip_attention_part_floats(2, 12, 768) == 2 * 2 * 12 * 768 * 66
    assert lib.imcui_hip_attention_part_floats(0, 4, 128) == 0
    assert lib.imcui_hip_attention_mx_scratch_bytes(2, 4, 1024) == 2 * 4 * 16 * 6400


def test_route_numbering_matches_attention_h():
    from imcui_hip import backend

    src = open(ATTN_H).read()
    body = re.search(r"enum AttnRouteKind\s*\{(.*?)\};", src, re.S).group(1)
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b([A-Z][A-Z0-9_]+)\s*=\s*(\d+)", body)}
    nkind = enum.pop("AR_NKIND")
    kinds = {k[3:].lower(): v for k, v in enum.items()}
    assert kinds == backend.ATTN_ROUTE_KINDS
    assert nkind == max(kinds.values()) + 1
    assert re.search(r"#define ATTN_ROUTE\(kind, split\) \(\(kind\) \* 2 \+ \(split\)\)", src)
    assert backend.attn_route("l2d_v7", True) == 4 * 2 + 1
    assert backend.attn_route_name(backend.attn_route("mx")) == "mx" and backend.attn_route_name(7) == "l2d_v8/split"


def test_case_table_routes_are_well_formed():
    """Every mode of the GPU case table names a route that exists, every case only modes its geometry allows."""
    import test_gpu_attention_variants as t

    from imcui_hip import backend

    cov = t.covered_routes()
    assert all(0 < r < 16 for r in cov)
    names = {backend.attn_route_name(r) for r in cov}
    assert names == {"exact", "natlog", "l2d_v8", "l2d_v8/split", "l2d_v7", "l2d_v7/split", "l2d_single", "l2d_single/split", "mx"}
    assert len({c["id"] for c in t.CASES}) == len(t.CASES)
    for c, m in t.PARAMS:
        assert m in t.MODES, (c["id"], m)
        assert c["R"] > 512 or not t.MODES[m][4], f"{c['id']}: a key-split launch needs more than one chunk"
        assert c["refusal"] if c["run"] is t.run_refusal else (c["R"] % 128 == 0 and (c["S"] * c["H"]) % 8 == 0), c["id"]
