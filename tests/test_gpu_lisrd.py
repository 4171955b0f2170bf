"""LISRD end to end on the GPU: the network against the float32 CPU restatement (tests/lisrd_reference.py), the plugin against the golden
file the REFERENCE's wrapper wrote (tests/golden/make_lisrd_golden.py), the three real detectors, the refusals (GPU box only).

Bars.  Dense maps: 1e-4 of each map's largest magnitude against the float32 restatement (the issue's figure; the restatement's own
float32 error against float64 is 3e-6 on that scale).  A component of a sampled unit vector: E = max(3 x the float32 reference's own
error against float64, 1.8e-07) + NLAUNCH x (2e-6 exact / 4e-6 split) x amp.  NLAUNCH = 9: every value went through nine chained
launches of the shared GEMM (conv1_2 .. conv4_2, the fused head launch, a 1x1 layer), each with the project's per-launch bar on values
of the scale of its map, and the calibrated BatchNorms keep that scale (unit variance in, unit variance out), so the bars add.  amp =
the largest magnitude of the dense map over the smallest length of a sampled vector before it is normalised (v / |v| multiplies an
error of v by 1 / |v|), at least 1, worked out from the float64 restatement per case and printed.  mconf: max(3 x the wrapper's own
float32 error against float64, 1.8e-07) + NLAUNCH x (2e-6 / 4e-6), the same additive per-launch figure on a value in [-1, 1].
Every test prints its figures before it asserts."""
import functools
import os

import numpy as np
import pytest
import torch

import lisrd_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1.8e-07
NLAUNCH = 9
SIZES = {"24x32": (24, 32, 1), "50x70": (50, 70, 2), "96x128": (96, 128, 3)}


@functools.lru_cache(maxsize=None)
def _sd():
    from imcui_hip.synth_weights import lisrd_synth_state

    return lisrd_synth_state(0)


@functools.lru_cache(maxsize=None)
def _net():
    net = R.LisrdNet().eval()
    net.load_state_dict(_sd())
    return net


@functools.lru_cache(maxsize=None)
def _packed():
    from imcui_hip import backend

    return backend.pack_lisrd(_sd()).to(DEV)


def image(h, w, seed):
    return torch.randint(0, 256, (1, 3, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).float() / 255.0


def keypoints(h, w, n, seed):
    g = torch.Generator().manual_seed(seed)
    sub = torch.rand(n - 4, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    return torch.cat([torch.tensor([[0.0, 0.0], [w - 1.0, h - 1.0], [7.0, 3.0], [3.5, 3.5]]), sub])


def component_bar(precision, out64, kp, hw, r32, r64):
    """(E_desc, E_meta) of the module docstring for key-points kp (x, y) of an image of size hw; r32 / r64 = (desc, meta) of the float32 reference and of float64"""
    import torch.nn.functional as F

    g = (kp[:, [1, 0]].double() * 2.0 / torch.tensor(hw, dtype=torch.float64) - 1.0)[..., [1, 0]].view(1, -1, 1, 2)
    bars = []
    for key, a, b in (("descriptors", r32[0], r64[0]), ("meta_descriptors", r32[1], r64[1])):
        amp = max(float(out64[key][v].abs().max()) / float(F.grid_sample(out64[key][v], g, align_corners=False)[0, :, :, 0].norm(dim=0).min()) for v in R.VARIANCES)
        own = float((a.double() - b).abs().max())
        bars.append(max(3.0 * own, FLOOR) + NLAUNCH * (4e-6 if precision == 1 else 2e-6) * max(amp, 1.0))
        print(f"  {key}: reference's own error {own:.3g}, amp {amp:.3g}, component bar {bars[-1]:.3g}")
    return bars


@functools.lru_cache(maxsize=None)
def _oracle(size):
    """(image, float32 outputs of the restatement, float64 outputs)"""
    h, w, seed = SIZES[size]
    img = image(h, w, seed)
    with torch.no_grad():
        o32 = _net()(img * 255.0)
        o64 = R.LisrdNet().double().eval()
        o64.load_state_dict(_sd())
        o64 = o64(img.double() * 255.0)
    return img, o32, o64


@pytest.mark.parametrize("size", list(SIZES))
def test_end_to_end(precision, size):
    from imcui_hip import backend

    img, o32, o64 = _oracle(size)
    h, w, seed = SIZES[size]
    impl = backend.LisrdHIP()
    dense = impl.dense(_packed(), img.to(DEV))
    for name, key, got in (("descriptors", "descriptors", dense["descriptors"]), ("meta maps", "meta_maps", dense["meta_maps"])):
        for i, v in enumerate(R.VARIANCES):
            ref = o32[key][v][0].permute(1, 2, 0)
            err = float((got[i, 0].cpu() - ref).abs().max()) / float(ref.abs().max())
            own = float((ref.double() - o64[key][v][0].permute(1, 2, 0)).abs().max()) / float(ref.abs().max())
            print(f"{size} {name} {v}: relative error {err:.3g} (the restatement's own float32 error {own:.3g}), bar 1e-4")
            assert err <= 1e-4
    for i, v in enumerate(R.VARIANCES):
        ref = o32["meta_descriptors"][v][0].permute(1, 2, 0)  # [3, 3, 1024], unit vectors
        err = float((dense["meta_descriptors"][0, i].cpu() - ref).abs().max()) / float(ref.abs().max())
        print(f"{size} meta descriptors {v}: relative error {err:.3g}, bar 1e-4")
        assert err <= 1e-4
    # sampled vectors at common key-points
    n = 37
    kp = keypoints(h, w, n, seed)
    rows = torch.zeros(1, n + 3, 2)
    rows[0, :n] = kp
    out = impl.describe(_packed(), img.to(DEV), rows.to(DEV), torch.tensor([n], dtype=torch.int32))
    d32, m32 = R.extract_descriptors(kp, {k: {v: t for v, t in o32[k].items()} for k in ("descriptors", "meta_descriptors")}, (h, w))
    d64, m64 = R.extract_descriptors(kp.double(), {k: {v: t for v, t in o64[k].items()} for k in ("descriptors", "meta_descriptors")}, (h, w), torch.float64)
    bars = component_bar(precision, o64, kp, (h, w), (d32, m32), (d64, m64))
    for name, got, r64, bar in (("desc", out["desc"], d64, bars[0]), ("meta", out["meta"], m64, bars[1])):
        err = float((got[0, :n].cpu().double() - r64).abs().max())
        print(f"{size} sampled {name}: error {err:.3g} against float64, bar {bar:.3g}")
        assert err <= bar
        assert bool((got[0, n:] == 0).all())
        assert float((got[0, :n].norm(dim=-1) - 1).abs().max()) < 1e-6


def _stored(golden_dir):
    return np.load(os.path.join(golden_dir, "lisrd_golden.npz"))


class StoredDetector(torch.nn.Module):
    """stands where the plugin's detector stands and returns the golden file's key-points, in call order"""

    def __init__(self, queue):
        super().__init__()
        self.queue = list(queue)

    def forward(self, data):
        return {"keypoints": [self.queue.pop(0).to(data["image"].device)]}


def _plugin(detector="superpoint", detector_weights=None):
    from imcui_hip.hloc.matchers.lisrd import Lisrd

    return Lisrd({"detector": detector, "state_dict": {"model_state_dict": _sd()}, "detector_weights": detector_weights, "max_keypoints": 256}).eval().to(DEV)


def test_golden_through_the_plugin(precision, golden_dir):
    """fails without the feature: the plugin module, the library entries and the golden file are all new"""
    from imcui_hip.synth_weights import superpoint_state_dict

    g = _stored(golden_dir)
    m = _plugin("superpoint", {"state_dict": superpoint_state_dict(0)})
    for p in range(2):
        assert float(g[f"margin_{p}"]) >= 1e-4
        k0, k1 = torch.from_numpy(g[f"keypoints0_{p}"]), torch.from_numpy(g[f"keypoints1_{p}"])
        m.detector = StoredDetector([k0, k1])
        img0, img1 = (torch.from_numpy(g[f"image{i}_u8_{p}"]).float() / 255.0 for i in (0, 1))
        out = m({"image0": img0.to(DEV), "image1": img1.to(DEV)})
        assert torch.equal(out["keypoints0"].cpu(), k0) and torch.equal(out["keypoints1"].cpu(), k1)
        print(f"pair {p}: {len(out['mconf'])} matches (golden {len(g[f'mconf_{p}'])}), margin of the golden pair {float(g[f'margin_{p}']):.3g}")
        assert np.array_equal(out["mkeypoints0"].cpu().numpy(), g[f"mkeypoints0_{p}"])  # the matches AND their order
        assert np.array_equal(out["mkeypoints1"].cpu().numpy(), g[f"mkeypoints1_{p}"])
        # the float64 restatement on the same pair: what the wrapper's float32 is off by, and the amplification of the normalisation
        with torch.no_grad():
            n64 = R.LisrdNet().double().eval()
            n64.load_state_dict(_sd())
            o0, o1 = n64(img0.double() * 255.0), n64(img1.double() * 255.0)
        s0 = R.extract_descriptors(k0.double(), o0, tuple(img0.shape[2:]), torch.float64)
        s1 = R.extract_descriptors(k1.double(), o1, tuple(img1.shape[2:]), torch.float64)
        rows = int(g["meta_rows"])
        w0 = (torch.from_numpy(g[f"desc0_{p}"]), torch.from_numpy(g[f"meta0_{p}"]))
        w1 = (torch.from_numpy(g[f"desc1_{p}"]), torch.from_numpy(g[f"meta1_{p}"]))
        e0 = component_bar(precision, o0, k0, tuple(img0.shape[2:]), w0, (s0[0], s0[1][:rows]))
        e1 = component_bar(precision, o1, k1, tuple(img1.shape[2:]), w1, (s1[0], s1[1][:rows]))
        # the sampled vectors the wrapper's own code produced
        for side, img, k, w, e in ((0, img0, k0, w0, e0), (1, img1, k1, w1, e1)):
            d = m.describe(img.to(DEV), k.to(DEV))
            derr = float((d["desc"][0].cpu() - w[0]).abs().max())
            merr = float((d["meta"][0, :rows].cpu() - w[1]).abs().max())
            print(f"pair {p}: sampled desc / meta of image {side} off by {derr:.3g} / {merr:.3g} from the wrapper's, bars {e[0]:.3g} / {e[1]:.3g}")
            assert derr <= e[0] and merr <= e[1]
        i0 = [int((k0 == torch.from_numpy(q)).all(1).float().argmax()) for q in g[f"mkeypoints0_{p}"]]
        i1 = [int((k1 == torch.from_numpy(q)).all(1).float().argmax()) for q in g[f"mkeypoints1_{p}"]]
        c64 = ((s0[0][i0] * s1[0][i1]).sum(2) * torch.softmax((s0[1][i0] * s1[1][i1]).sum(2), dim=1)).sum(1)
        own = float((torch.from_numpy(g[f"mconf_{p}"]).double() - c64).abs().max())
        bar = max(3.0 * own, FLOOR) + NLAUNCH * (4e-6 if precision == 1 else 2e-6)
        err = float(np.abs(out["mconf"].cpu().numpy() - g[f"mconf_{p}"]).max())
        print(f"pair {p}: mconf error {err:.3g} against the wrapper's (its own float32 error {own:.3g}), bar {bar:.3g}")
        assert err <= bar


@pytest.mark.parametrize("detector", ["superpoint", "aliked", "sift"])
def test_real_detectors(precision, detector):
    from imcui_hip.synth import make_shifted_pair
    from imcui_hip.synth_weights import aliked_state_dict, superpoint_state_dict

    weights = {"superpoint": {"state_dict": superpoint_state_dict(0)}, "aliked": {"state_dict": aliked_state_dict(0)}, "sift": None}[detector]
    m = _plugin(detector, weights)
    a, b, _ = make_shifted_pair(5, 128, 160, shift=(24, 16), n_blobs=150)  # two crops of one canvas
    a, b = a.expand(-1, 3, -1, -1).contiguous(), b.expand(-1, 3, -1, -1).contiguous()
    fwd = m({"image0": a.to(DEV), "image1": b.to(DEV)})
    bwd = m({"image0": b.to(DEV), "image1": a.to(DEV)})
    for out, n0 in ((fwd, "a"), (bwd, "b")):
        k0, k1, m0, m1, c = (out[k] for k in ("keypoints0", "keypoints1", "mkeypoints0", "mkeypoints1", "mconf"))
        assert k0.dim() == 2 and k0.shape[1] == 2 and k1.shape[1] == 2 and m0.shape == m1.shape and c.shape == (m0.shape[0],)
        assert bool(torch.isfinite(c).all()) and float(c.abs().max()) <= 1.0 + 1e-5
        print(f"{detector} from {n0}: {k0.shape[0]} / {k1.shape[0]} key-points, {m0.shape[0]} mutual matches")
        assert k0.shape[0] > 0 and k1.shape[0] > 0 and m0.shape[0] > 0
        # every matched key-point is one of the image's key-points, image-0 indices ascend
        idx = [(k0[:, None] == m0[None]).all(-1).float().argmax(0)]
        assert bool((idx[0][1:] >= idx[0][:-1]).all())
    # the mutual rule is symmetric: the pairs of a -> b are the pairs of b -> a
    pairs_f = {(tuple(p.tolist()), tuple(q.tolist())) for p, q in zip(fwd["mkeypoints0"].cpu(), fwd["mkeypoints1"].cpu())}
    pairs_b = {(tuple(q.tolist()), tuple(p.tolist())) for p, q in zip(bwd["mkeypoints0"].cpu(), bwd["mkeypoints1"].cpu())}
    print(f"{detector}: {len(pairs_f & pairs_b)} of {len(pairs_f)} pairs found in both directions")
    assert len(pairs_f & pairs_b) >= 0.9 * len(pairs_f)


def test_refusals(precision):
    from imcui_hip import backend
    from imcui_hip.hloc.matchers.lisrd import Lisrd

    with pytest.raises(ValueError, match="Unknown LISRD detector: orb"):
        Lisrd({"detector": "orb", "state_dict": _sd()})
    impl = backend.LisrdHIP()
    kp, cnt = torch.zeros(1, 1, 2, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="at least 24"):
        impl.describe(_packed(), torch.rand(1, 3, 23, 40, device=DEV), kp, cnt)
    with pytest.raises(ValueError, match="at least 24"):
        impl.describe(_packed(), torch.rand(1, 3, 40, 23, device=DEV), kp, cnt)
    with pytest.raises(ValueError, match="3-channel"):
        impl.describe(_packed(), torch.rand(1, 1, 40, 40, device=DEV), kp, cnt)
    # the library's own message, behind the binding's check
    hd = backend.get_handle(torch.device(DEV))
    for shape, word in (((1, 1, 32, 32), "channels"), ((1, 3, 23, 32), "at least 24")):
        rc = hd.launch(hd.lib.imcui_hip_lisrd_describe, _packed().data_ptr(), None, shape[0], shape[1], shape[2], shape[3], None, None, 1, None, None, None, None, 0,
                       check=False)  # fmt: skip
        assert rc == -1 and word in hd.lib.imcui_hip_last_error(hd.h).decode()
