"""DoG + HardNet / SOSNet end to end on the GPU (imcui_hip_patchdesc_forward, the `dog` plugin).

On synthetic key-points of a 96 x 130 seeded texture (n = 0, 1, 33, 257, a ragged batch of three images, both networks, both arithmetic
modes) the descriptors are within 1e-4 of the float32 restatement (tests/dog_reference.py) and have unit norm; rows past the count are not
written.  Two exclusions are conditions, not tolerances: scales are drawn with |log2(12 sigma / 32) - nearest integer| > 1e-3, so no pyramid
level is in doubt, and value comparison leaves out patches whose float64 std is below 1e-3 (the normalisation amplifies sampling rounding
without bound there) -- the test asserts that only the one deliberately constant patch falls under that cap, and checks that one for finite
output and unit norm.  Bitwise: chunk = 32 against the default at n = 70, B = 1 against B = 3, eager against graph replay.

Through the plugin: a 96 x 96 seeded image and its torch.rot90.  Key-points that correspond (position within 1 px after mapping, scale
within 5 %) must have matching descriptors.  On the CPU, from the restatements (tests/sift_reference.py for the key-points), the median
cosine of corresponding descriptors is 0.9198 with the wrapper's sign (LAF angle = -ori) and 0.7126 with the orientation negated (seed 10,
31 pairs; both networks); the test recomputes both, requires them to be at least 0.1 apart, and asserts the device within 0.02 of the
former and at least 0.1 above the latter.  The plugin's own key-points, fed to the restatement, give its descriptors within 1e-4;
key-points within 1e-4 of a level boundary are left out, capped at 1 % (on the CPU the chosen image has none)."""
import functools
import math

import numpy as np
import pytest
import torch

import dog_reference as R
import sift_reference as S
from test_dog_cpu import NETS, pack, state
from test_gpu_dog_layers import texture

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 1e-4  # the standing descriptor bar (NetVLAD, R2D2)
STD_CAP = 1e-3
H, W, FLAT = 96, 130, 40
ROT_SEED = 10


@functools.lru_cache(maxsize=None)
def impl():
    from imcui_hip import backend

    return backend.PatchDescHIP()


@functools.lru_cache(maxsize=None)
def packed(name):
    return pack(name).to(DEV)


@functools.lru_cache(maxsize=None)
def image(seed=0):
    """The seeded texture with a constant 40 x 40 block in its top-left corner."""
    img = texture(H, W, 100 + seed).clone()
    img[:FLAT, :FLAT] = 0.5
    return img


@functools.lru_cache(maxsize=None)
def keypoints(n, seed=0):
    """n synthetic key-points right of the flat block; scales log-uniform in [1.2, 12] and away from the level boundaries; key-point 0
    (when n >= 33) sits in the middle of the flat block with a patch that stays inside it."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    kp = torch.rand(n, 2, generator=g) * torch.tensor([W - 1.0 - 45.0, H - 1.0]) + torch.tensor([45.0, 0.0])
    sc = torch.empty(n)
    for i in range(n):
        while True:
            s = 1.2 * 10.0 ** torch.rand(1, generator=g).item()
            l2 = math.log2(12.0 * s / 32.0)
            if abs(l2 - round(l2)) > 1e-3:
                break
        sc[i] = s
    od = torch.rand(n, generator=g) * 360.0 - 180.0
    if n >= 33:
        kp[0], sc[0] = torch.tensor([19.5, 19.5]), 1.5
    return kp, sc, od


@functools.lru_cache(maxsize=None)
def reference(name, n, seed=0):
    """float32 descriptors of the restatement and the float64 std of every patch (computed once, read-only)."""
    kp, sc, od = keypoints(n, seed)
    d32 = R.forward(name, state(name), image(seed), kp, sc, od)
    p64 = R.extract_patches(image(seed)[None, None].double(), R.lafs_from_keypoints(kp, sc, od, dtype=torch.float64))
    return d32, p64.flatten(1).std(dim=1)


def run(name, n_list, K, chunk=1024, out=None):
    """One call on len(n_list) images (image b = image(b), its first n_list[b] key-points of keypoints(max n, b))."""
    B = len(n_list)
    img = torch.stack([image(b) for b in range(B)])[:, None]
    kp, sc, od = torch.zeros(B, K, 2), torch.ones(B, K), torch.zeros(B, K)
    for b, n in enumerate(n_list):
        if n:
            k, s, o = keypoints(n, b)
            kp[b, :n], sc[b, :n], od[b, :n] = k, s, o
    cnt = torch.tensor(n_list, dtype=torch.int32)
    return impl().forward(packed(name), img.to(DEV), kp.to(DEV), sc.to(DEV), od.to(DEV), cnt.to(DEV), name, chunk=chunk, out=out)


def check_rows(name, got, n, seed=0):
    d32, std = reference(name, n, seed)
    flat = std < STD_CAP
    assert flat.nonzero().flatten().tolist() == ([0] if n >= 33 else []), "a seeded-texture patch fell under the std cap"
    err = (got.cpu()[~flat] - d32[~flat]).abs().max().item() if (~flat).any() else 0.0
    assert torch.isfinite(got).all().item() and torch.allclose(got.norm(dim=1).cpu(), torch.ones(n), atol=1e-5)
    return err


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("n", [0, 1, 33, 257])
def test_descriptors_match_the_restatement(name, n, precision):
    K = max(n, 4)
    out = torch.full((1, K, 128), 7.0, device=DEV)
    res = run(name, [n], K, out=out)
    torch.cuda.synchronize()
    assert res["status"].item() == 0 and res["descriptors"] is out
    assert torch.all(out[0, n:] == 7.0).item(), "a row past the count was written"
    if n:
        err = check_rows(name, out[0, :n], n)
        print(f"[dog] {name} n={n} mode {precision}: descriptors {err:.2e} (bar {BAR:.0e})")
        assert err < BAR


@pytest.mark.parametrize("name", NETS)
def test_ragged_batch_is_bitwise_the_single_images(name, precision):
    counts, K = [257, 0, 33], 257
    trio = run(name, counts, K)["descriptors"]
    torch.cuda.synchronize()
    for b, n in enumerate(counts):
        assert torch.all(trio[b, n:] == 0).item()
        if n == 0:
            continue
        err = check_rows(name, trio[b, :n], n, seed=b)
        print(f"[dog] {name} ragged image {b} (n={n}) mode {precision}: {err:.2e}")
        assert err < BAR
    # image 2 alone (B = 1, K = 33) and image 0 alone: the same bits as inside the batch of three
    for b, n in ((0, 257), (2, 33)):
        k, s, o = keypoints(n, b)
        solo = impl().forward(packed(name), image(b)[None, None].to(DEV), k[None].to(DEV), s[None].to(DEV), o[None].to(DEV),
                              torch.tensor([n], dtype=torch.int32, device=DEV), name)["descriptors"]  # fmt: skip
        assert torch.equal(solo[0], trio[b, :n]), f"image {b}: the descriptors depend on the batch"


def test_chunk_size_does_not_change_a_bit(precision):
    a = run("hardnet", [70], 70)["descriptors"]
    b = run("hardnet", [70], 70, chunk=32)["descriptors"]
    c = run("sosnet", [70], 70, chunk=32)["descriptors"]
    d = run("sosnet", [70], 70)["descriptors"]
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(c, d)
    assert a.norm(dim=2).min().item() > 0.99


def test_graph_replay_is_bitwise_the_eager_call(precision):
    from imcui_hip import backend

    counts, K = [33, 70, 0], 70
    eager = run("sosnet", counts, K, chunk=32)["descriptors"].clone()
    B = len(counts)
    img = torch.stack([image(b) for b in range(B)])[:, None].to(DEV)
    kp, sc, od = torch.zeros(B, K, 2), torch.ones(B, K), torch.zeros(B, K)
    for b, n in enumerate(counts):
        if n:
            kp[b, :n], sc[b, :n], od[b, :n] = keypoints(n, b)
    kp, sc, od, cnt = kp.to(DEV), sc.to(DEV), od.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)
    call = lambda: impl().forward(packed("sosnet"), img, kp, sc, od, cnt, "sosnet", chunk=32)  # noqa: E731
    table = {}
    with backend.workspace_owner(table):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()  # warm-up: allocates the graph-owned workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = call()
    for _ in range(2):
        cap["descriptors"].fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        for b, n in enumerate(counts):
            assert torch.equal(cap["descriptors"][b, :n], eager[b, :n])
        assert cap["status"].item() == 0


def test_status_bits():
    """A count above the capacity sets bit 1 (and is clipped); a non-finite orientation sets bit 2 and leaves a zero row."""
    k, s, o = keypoints(33)
    o = o.clone()
    o[5] = float("inf")
    res = impl().forward(packed("hardnet"), image()[None, None].to(DEV), k[None].to(DEV), s[None].to(DEV), o[None].to(DEV),
                         torch.tensor([40], dtype=torch.int32, device=DEV), "hardnet")  # fmt: skip
    torch.cuda.synchronize()
    assert res["status"].item() == 3
    d = res["descriptors"][0]
    assert d[5].abs().max().item() == 0 and torch.allclose(d[[1, 2, 3, 4, 6, 32]].norm(dim=1).cpu(), torch.ones(6), atol=1e-5)


# ------------------------------------------------------------------ through the plugin
def plugin(name, **conf):
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load

    return dynamic_load(extractors, "dog")({**ef.confs[name]["model"], "state_dict": state(name), **conf}).eval().to(DEV)


def corresponding(ka, sa, kb, sb, width):
    """Index pairs (i, j): key-point i of the image and j of its torch.rot90 (k = 1: pixel (x, y) -> (y, width - 1 - x)) within 1 px and 5 % of scale."""
    mapped = np.stack([ka[:, 1], width - 1 - ka[:, 0]], 1)
    d = np.linalg.norm(mapped[:, None] - kb[None], axis=2)
    return np.argwhere((d < 1.0) & (np.abs(sa[:, None] / sb[None] - 1.0) < 0.05))


@functools.lru_cache(maxsize=None)
def rotation_case():
    """The image, its rotation, and the restatement's median cosines with the wrapper's sign and with the orientation negated."""
    img = S.seeded_image(96, 96, seed=ROT_SEED)
    rot = np.ascontiguousarray(np.rot90(img, 1))
    conf = {"rootsift": False, "nms_radius": None, "max_keypoints": 0, "detection_threshold": 0.03, "edge_threshold": 10, "num_octaves": 3}
    a, b = S.extract(img[None], conf, dtype=np.float32), S.extract(rot[None], conf, dtype=np.float32)
    pairs = corresponding(a["keypoints"], a["scales"], b["keypoints"], b["scales"], 96)
    med = {}
    for name in NETS:
        for sign in (1.0, -1.0):
            f = lambda im, k: R.forward(name, state(name), torch.from_numpy(im.copy()), torch.from_numpy(k["keypoints"]), torch.from_numpy(k["scales"] * 0.5),  # noqa: E731
                                        torch.from_numpy(np.rad2deg(k["oris"])) * sign)  # fmt: skip
            da, db = f(img, a), f(rot, b)
            med[name, sign] = (da[pairs[:, 0]] * db[pairs[:, 1]]).sum(1).median().item()
    lafs = R.lafs_from_keypoints(torch.from_numpy(a["keypoints"]), torch.from_numpy(a["scales"] * 0.5), torch.from_numpy(np.rad2deg(a["oris"])))
    _, l2 = R.patch_levels(lafs, 96, 96)
    near = int(((l2 - l2.round()).abs() < 1e-4).sum())
    return img, rot, med, len(pairs), near, len(l2)


@pytest.mark.parametrize("name", NETS)
def test_rotated_image_gives_matching_descriptors(name):
    img, rot, med, npairs, near, nkp = rotation_case()
    good, wrong = med[name, 1.0], med[name, -1.0]
    assert npairs >= 16 and good - wrong > 0.1, (npairs, good, wrong)  # the two signs separate on the CPU
    assert near <= 0.01 * nkp  # the image stays under the level-boundary cap
    m = plugin(name, max_keypoints=-1)
    with torch.no_grad():
        a = m({"image": torch.from_numpy(img)[None, None].to(DEV)})
        b = m({"image": torch.from_numpy(rot)[None, None].to(DEV)})
    ka, kb = a["keypoints"][0].cpu().numpy(), b["keypoints"][0].cpu().numpy()
    pairs = corresponding(ka, a["scales"][0].cpu().numpy(), kb, b["scales"][0].cpu().numpy(), 96)
    da, db = a["descriptors"][0].t().cpu(), b["descriptors"][0].t().cpu()
    dev = (da[pairs[:, 0]] * db[pairs[:, 1]]).sum(1).median().item()
    print(f"[dog] {name} rot90: {len(pairs)} corresponding key-points, median cosine {dev:.4f}; restatement {good:.4f}, orientation negated {wrong:.4f}")
    assert len(pairs) >= 16 and abs(dev - good) < 0.02 and dev - wrong > 0.1


@pytest.mark.parametrize("name", NETS)
def test_plugin_output_and_its_own_keypoints_through_the_restatement(name, precision):
    img = torch.from_numpy(S.seeded_image(96, 96, seed=ROT_SEED))
    m = plugin(name, max_keypoints=-1)
    with torch.no_grad():
        out = m({"image": img[None, None].to(DEV)})
    n = out["keypoints"].shape[1]
    assert set(out) == {"keypoints", "scales", "oris", "scores", "descriptors"} and n >= 16
    assert out["keypoints"].shape == (1, n, 2) and out["descriptors"].shape == (1, 128, n) and out["scales"].shape == out["oris"].shape == out["scores"].shape == (1, n)
    assert torch.all(out["scores"] == 0).item() and out["oris"].abs().max().item() > 2 * math.pi  # degrees
    kp, sc, od = out["keypoints"][0].cpu(), out["scales"][0].cpu(), out["oris"][0].cpu()
    _, l2 = R.patch_levels(R.lafs_from_keypoints(kp, sc, od, dtype=torch.float64), 96, 96)
    keep = (l2 - l2.round()).abs() >= 1e-4
    assert (~keep).sum().item() <= 0.01 * n
    ref = R.forward(name, state(name), img, kp, sc, od)
    err = (out["descriptors"][0].t().cpu()[keep] - ref[keep]).abs().max().item()
    print(f"[dog] {name} plugin on 96x96 mode {precision}: {n} key-points, descriptors against the restatement {err:.2e} (bar {BAR:.0e})")
    assert err < BAR


def test_confs_run_a_pair_through_the_mutual_nn_matcher():
    """`extract_features.confs["hardnet"]` on two overlapping crops of one canvas, then the NN-mutual matcher on the device."""
    from imcui_hip import backend

    a, b = S.shift_pair(160, 192)
    m = plugin("hardnet")
    with torch.no_grad():
        fa, fb = m({"image": torch.from_numpy(a)[None].to(DEV)}), m({"image": torch.from_numpy(b)[None].to(DEV)})
    m0, _ = backend.mutual_nn_dn(fa["descriptors"], fb["descriptors"])
    torch.cuda.synchronize()
    m0 = m0[0].cpu()
    ok = m0 >= 0
    assert ok.sum().item() >= 10
    # a match of a shifted crop lies SHIFT away
    d = fa["keypoints"][0].cpu()[ok] - fb["keypoints"][0].cpu()[m0[ok].long()]
    right = ((d - torch.tensor([float(S.SHIFT[1]), float(S.SHIFT[0])])).norm(dim=1) < 1.5).float().mean().item()
    print(f"[dog] hardnet + mutual NN on a shifted pair: {int(ok.sum())} matches, {right:.0%} at the true offset")
    assert right > 0.5
