"""CosPlace / EigenPlaces on the GPU, end to end, in both arithmetic modes, against the float32 restatement (tests/places_reference.py) run
by torch on the CPU with the synthetic weights of seed 0 on uniform-random images, all at B = 2:

  ResNet-18 / 512 and ResNet-50 / 2048 at 32 x 48 (layer4 map 1 x 2: fewer pixels than any tile), 50 x 70 (odd at every stage:
  25x35 -> 13x18 -> 7x9 -> 4x5 -> 2x3) and 272 x 336 (9 x 11 = 99 pixels: crosses the 64-pixel chunk of the GeM sum);
  ResNet-101 / 2048 (the `eigenplaces` default) and ResNet-152 / 512 at 32 x 48.

Bar: the project's end-to-end rule max(1e-4, 3 x the restatement's float32-vs-float64 spread), relative to the largest magnitude of the
layer4 map and of the descriptor; tests/test_places_cpu.py measures the spread (below 1e-6 everywhere), so 1e-4.  Then: descriptor norms
1 within 1e-5; an image alone against inside a batch of 3, bitwise; HIP-graph replay, bitwise; the refusals.

Measured on one MI355X, of the largest magnitude: layer4 map 4.4e-07 .. 1.0e-06 (split) / 5.2e-07 .. 1.7e-06 (exact), descriptor 3.7e-07 ..
9.6e-07 / 4.2e-07 .. 1.0e-06; the largest are ResNet-152 / 512 (split: 1.0e-06 / 9.6e-07) and ResNet-50 / 2048 at 50 x 70 (exact map 1.7e-06)."""
import functools

import pytest
import torch

from test_places_cpu import BAR, SPREAD, image, reference32, rel, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)  # (1.2 GB on the device over the four backbones)
def packed(backbone: int, dim: int) -> torch.Tensor:
    from imcui_hip import backend

    return backend.pack_places(state(backbone, dim), backbone, dim).to(DEV)


@functools.lru_cache(maxsize=None)
def impl(backbone: int, dim: int):
    from imcui_hip import backend

    return backend.PlacesHIP(backbone, dim)


@pytest.mark.parametrize("cfg", list(SPREAD), ids=lambda c: f"resnet{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}")
def test_against_the_float32_restatement(cfg, precision):
    from imcui_hip import backend

    backbone, dim, hw = cfg
    ref = reference32(backbone, dim, hw)
    out = impl(backbone, dim).forward_batched(packed(backbone, dim), image(hw).to(DEV), want_map=True)
    torch.cuda.synchronize()
    desc, fmap = out["global_descriptor"], out["backbone"]
    assert desc.shape == ref["global_descriptor"].shape == (2, dim)
    assert fmap.shape == (2, *backend.places_map_size(*hw)[-1], 512 if backbone == 18 else 2048)
    e_map, e_desc = rel(fmap.permute(0, 3, 1, 2), ref["backbone"]), rel(desc, ref["global_descriptor"])
    print(f"[places] ResNet-{backbone}/{dim} {hw} mode {precision}: layer4 map {e_map:.2e}, descriptor {e_desc:.2e} of its largest magnitude (bar {BAR:.0e})")
    assert not torch.isnan(desc).any().item() and e_map < BAR and e_desc < BAR
    assert torch.allclose(desc.norm(dim=1).cpu(), torch.ones(2), atol=1e-5)


@pytest.mark.parametrize("cfg", [(18, 512), (50, 2048)], ids=["resnet18-512", "resnet50-2048"])
def test_batch_independence_and_graph_replay_bitwise(cfg, precision):
    from imcui_hip import backend

    m, pk = impl(*cfg), packed(*cfg)
    batch = torch.rand(3, 3, 50, 70, generator=torch.Generator().manual_seed(7)).to(DEV)
    trio = m.forward_batched(pk, batch)["global_descriptor"]
    for i in range(3):
        solo = m.forward_batched(pk, batch[i : i + 1])["global_descriptor"]
        assert torch.equal(solo[0], trio[i]), i
    table = {}
    with backend.workspace_owner(table):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.forward_batched(pk, batch)  # warm-up: allocates the graph-owned workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = m.forward_batched(pk, batch)["global_descriptor"]
    for _ in range(2):
        cap.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, trio)


def test_plugins_return_the_reference_dict():
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load

    hw = (32, 48)
    for name, conf in (("cosplace", {"backbone": "ResNet18", "fc_output_dim": 512}), ("eigenplaces", {"backbone": "ResNet18", "fc_output_dim": 512})):
        m = dynamic_load(extractors, name)({**conf, "state_dict": state(18, 512)}).eval().to(DEV)
        with torch.no_grad():
            out = m({"image": image(hw).to(DEV)})
        assert set(out) == {"global_descriptor"} and out["global_descriptor"].shape == (2, 512)
        assert rel(out["global_descriptor"], reference32(18, 512, hw)["global_descriptor"]) < BAR


def test_refusals():
    from imcui_hip import backend
    from imcui_hip.backend import _ptr, get_handle

    m, pk = impl(18, 512), packed(18, 512)
    with pytest.raises(ValueError, match="RGB"):
        m.forward_batched(pk, torch.zeros(1, 1, 64, 64, device=DEV))
    with pytest.raises(backend.ImcuiHipError, match="packed buffer"):
        impl(18, 256).forward_batched(pk, torch.zeros(1, 3, 32, 32, device=DEV))  # another head's buffer
    with pytest.raises(ValueError, match="VGG16"):
        backend.PlacesHIP("VGG16", 512)
    # the library refuses the same with a message of its own
    hd = get_handle(DEV)
    img, out, ws = torch.zeros(1, 3, 64, 64, device=DEV), torch.empty(1, 512, device=DEV), torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    with pytest.raises(backend.ImcuiHipError, match="3 \\(RGB\\)"):
        hd.launch(hd.lib.imcui_hip_places_forward, _ptr(pk), _ptr(img), 1, 1, 64, 64, 18, 512, _ptr(out), None, _ptr(ws), ws.numel())
    with pytest.raises(backend.ImcuiHipError, match="unknown backbone 34"):
        hd.launch(hd.lib.imcui_hip_places_forward, _ptr(pk), _ptr(img), 1, 3, 64, 64, 34, 512, _ptr(out), None, _ptr(ws), ws.numel())
    with pytest.raises(backend.ImcuiHipError, match="workspace too small"):
        hd.launch(hd.lib.imcui_hip_places_forward, _ptr(pk), _ptr(img), 1, 3, 64, 64, 18, 512, _ptr(out), None, _ptr(ws), 1024)
    # a 1 x 1 image is valid: no map can become empty
    one = m.forward_batched(pk, torch.rand(1, 3, 1, 1, device=DEV), want_map=True)
    torch.cuda.synchronize()
    assert one["backbone"].shape == (1, 1, 1, 512) and abs(one["global_descriptor"].norm().item() - 1) < 1e-5
