"""NetVLAD on the GPU, end to end, in both arithmetic modes, with and without the whitening.

Against the REFERENCE's own float32 CPU output (tests/golden/netvlad_*.npz, imcui/hloc/extractors/netvlad.py run by
make_netvlad_golden.py): 32 x 48 (a 2 x 3 map: 6 pixels, fewer than the 64 clusters and than any tile) and 50 x 70 (odd at every pool:
25/12/6/3 x 35/17/8/4).  272 x 336 (17 x 21 = 357 pixels: crosses the 256-pixel chunk of the aggregation) against the float32 restatement,
which reproduces the reference bit for bit at the golden sizes (tests/test_netvlad_cpu.py).

Bar: the project's end-to-end rule max(1e-4, 3 x the reference's own float32 spread) relative to the descriptor's largest magnitude; the
golden maker measured a spread of 0 (1 against 8 threads), so 1e-4.  Then: an image alone against inside a batch of 3, bitwise; HIP-graph
replay, bitwise; the refusals.

Measured on one MI355X, both modes: conv5_3 map 1.1e-06 .. 1.3e-06 (1.8e-06 at 272 x 336), 32768-d descriptor 2.6e-06 .. 8.3e-06
(1.4e-06 .. 1.8e-06 at 272 x 336), whitened descriptor 9.0e-07 .. 1.3e-06."""
import functools

import pytest
import torch

import netvlad_reference as R
from test_netvlad_cpu import BAR, SIZES, golden, rel, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def packed(whiten: bool) -> torch.Tensor:
    from imcui_hip import backend

    return backend.pack_netvlad(state(whiten)).to(DEV)


@functools.lru_cache(maxsize=None)
def impl():
    from imcui_hip import backend

    return backend.NetVLADHIP()


@functools.lru_cache(maxsize=None)
def large_case():
    """One 272 x 336 image and the float32 restatement's outputs (computed once, read-only)."""
    img = torch.rand(1, 3, 272, 336, generator=torch.Generator().manual_seed(272))
    with torch.no_grad():
        return img, R.forward(state(True), img, True, torch.float32)


@pytest.mark.parametrize("whiten", [False, True], ids=["vlad32768", "whitened4096"])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_the_reference_output(hw, whiten, precision):
    g = golden(*hw)
    out = impl().forward_batched(packed(whiten), g["image"].to(DEV), whiten, want_map=True)
    torch.cuda.synchronize()
    desc, want = out["global_descriptor"], g["whitened" if whiten else "vlad"]
    assert desc.shape == want.shape == (2, 4096 if whiten else 32768)
    e_map, e_desc = rel(out["backbone"].permute(0, 3, 1, 2), g["backbone"]), rel(desc, want)
    print(f"[netvlad] {hw} whiten={whiten} mode {precision}: conv5_3 map {e_map:.2e}, descriptor {e_desc:.2e} of its largest magnitude (bar {BAR:.0e})")
    assert e_map < BAR and e_desc < BAR
    assert torch.allclose(desc.norm(dim=1).cpu(), torch.ones(2), atol=1e-5)


@pytest.mark.parametrize("whiten", [False, True], ids=["vlad32768", "whitened4096"])
def test_map_that_crosses_a_pixel_chunk(whiten, precision):
    img, ref = large_case()
    assert ref["backbone"].shape[2:] == (17, 21)
    out = impl().forward_batched(packed(whiten), img.to(DEV), whiten, want_map=True)
    torch.cuda.synchronize()
    e_map, e_desc = rel(out["backbone"].permute(0, 3, 1, 2), ref["backbone"]), rel(out["global_descriptor"], ref["global_descriptor" if whiten else "vlad"])
    print(f"[netvlad] 272x336 (357 pixels) whiten={whiten} mode {precision}: conv5_3 map {e_map:.2e}, descriptor {e_desc:.2e} (bar {BAR:.0e})")
    assert e_map < BAR and e_desc < BAR


@pytest.mark.parametrize("whiten", [False, True], ids=["vlad32768", "whitened4096"])
def test_batch_independence_and_graph_replay_bitwise(whiten, precision):
    from imcui_hip import backend

    batch = torch.rand(3, 3, 50, 70, generator=torch.Generator().manual_seed(7)).to(DEV)
    trio = impl().forward_batched(packed(whiten), batch, whiten)["global_descriptor"]
    for i in range(3):
        solo = impl().forward_batched(packed(whiten), batch[i : i + 1], whiten)["global_descriptor"]
        assert torch.equal(solo[0], trio[i]), i
    table = {}
    with backend.workspace_owner(table):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            impl().forward_batched(packed(whiten), batch, whiten)  # warm-up: allocates the graph-owned workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = impl().forward_batched(packed(whiten), batch, whiten)["global_descriptor"]
    for _ in range(2):
        cap.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, trio)


def test_plugin_returns_the_reference_dict():
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load

    g = golden(32, 48)
    m = dynamic_load(extractors, "netvlad")({"state_dict": state(False), "whiten": False}).eval().to(DEV)
    with torch.no_grad():
        out = m({"image": g["image"].to(DEV)})
    assert set(out) == {"global_descriptor"} and out["global_descriptor"].shape == (2, 32768)
    assert rel(out["global_descriptor"], g["vlad"]) < BAR


def test_refusals():
    from imcui_hip import backend
    from imcui_hip.backend import get_handle, _ptr

    with pytest.raises(ValueError, match="at least 16"):
        impl().forward_batched(packed(False), torch.zeros(1, 3, 15, 64, device=DEV), False)
    with pytest.raises(ValueError, match="RGB"):
        impl().forward_batched(packed(False), torch.zeros(1, 1, 64, 64, device=DEV), False)
    with pytest.raises(backend.ImcuiHipError, match="packed buffer"):
        impl().forward_batched(packed(False), torch.zeros(1, 3, 32, 32, device=DEV), True)  # whitening asked of a buffer without the matrix
    # the library refuses the same with a message of its own
    hd = get_handle(DEV)
    img, out, ws = torch.zeros(1, 3, 15, 64, device=DEV), torch.empty(1, 32768, device=DEV), torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    with pytest.raises(backend.ImcuiHipError, match="at least 16"):
        hd.launch(hd.lib.imcui_hip_netvlad_forward, _ptr(packed(False)), _ptr(img), 1, 3, 15, 64, 0, _ptr(out), None, _ptr(ws), ws.numel())
    with pytest.raises(backend.ImcuiHipError, match="3 \\(RGB\\)"):
        hd.launch(hd.lib.imcui_hip_netvlad_forward, _ptr(packed(False)), _ptr(img), 1, 1, 64, 64, 0, _ptr(out), None, _ptr(ws), ws.numel())
    with pytest.raises(backend.ImcuiHipError, match="workspace too small"):
        hd.launch(hd.lib.imcui_hip_netvlad_forward, _ptr(packed(False)), _ptr(img), 1, 3, 64, 64, 0, _ptr(out), None, _ptr(ws), 1024)
